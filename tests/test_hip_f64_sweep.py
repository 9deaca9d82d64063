"""The float64 forward kernels (precision = 64, mvx_f64.hip) swept the way the float32 ones are.

The float64 kernels share the slab body of the float32 ones (mvx_slab_body.inc) but bring their own walks (OpsF64 on the vector
ALU, OpsMx64 on v_mfma_f64_16x16x4_f64), their own exp and their own write-out tile - and no other route gives the same bits, so
nothing cross-checks them for free. Here:

* test_row / test_row_in_a_batch: every instantiation the dispatch can reach (tests/f64_rows.py; tests/test_f64_rows_host.py proves
  on the host that each row reaches its kernel and its line form: one round, extension line, x-list, x-list beyond 1024 entries,
  rows cut along z, misaligned odd grids), alone and as molecule 1 of a ragged batch, device and host staging;
* test_nine_waves_per_slab: a row of nine z sub-tiles in one slab (the "nw" knob), bit for bit the 8 + 1 cut of the plan;
* the fuzz draws of tests/test_hip_fuzz.py at precision 64: 64 configurations, 16 with the in-call random transform, 24 batches;
* exp_nonpos64 and the library's exp against exact values, down to subnormal results and underflow.

The reference everywhere is oracle/numpy_port.voxelize(..., precision=64), pinned to the imported reference by the precision-64
goldens. Bars (tests/tolerance.py): membership identical; binary types / single bit-exact; otherwise per voxel
|out - ref| <= P64_TOL * max(1, |ref|). The two float64 routes add the same non-negative terms in the same order and differ
only by their exp (about 3 * 2^-53 relative): per voxel |mx - dense| <= 1e-13 * max(1, |mx|).
Every test prints its figures ("f64-sweep ..."; pytest -s shows them); DESIGN.md section 10 records the worst ones.
"""
import decimal
import math

import numpy as np
import pytest

from tests import f64_rows as R
from tests.test_hip_fuzz import _draw, _reference
from tests.tolerance import P64_TOL, assert_membership, gaussian_excess

pytestmark = pytest.mark.gpu

ROUTE_TOL = 1e-13


def _voxelizer(D, radii_type, density, sigma, blockdim, output, res=R.RES):
    import molvoxel_amd as mv

    extra = {} if blockdim is None else {"blockdim": blockdim}
    return mv.create_voxelizer(res, D, radii_type, density, "hip", sigma=sigma, precision=64, output=output, **extra)


def _host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)


def _ref(D, blockdim, xyz, chan, radii, radii_type, density, nch, sigma=R.SIGMA, res=R.RES):
    from oracle import numpy_port

    if xyz.shape[0] == 0:
        return np.zeros((nch, D, D, D), np.float64)
    return numpy_port.voxelize(numpy_port.GridSpec(res, D, blockdim), xyz, chan, radii, radii_type=radii_type, density=density,
                               sigma=sigma, precision=64, num_channels=nch)


def _assert_bars(out, ref, exact, what):
    """The project's bars; returns |out - ref| / (P64_TOL * max(1, |ref|)) at its worst voxel."""
    assert out.shape == ref.shape and out.dtype == ref.dtype == np.float64, what
    assert_membership(out, ref)
    if exact:
        assert np.array_equal(out, ref), what
        return 0.0
    ex = gaussian_excess(out, ref, P64_TOL)
    print(f"f64-sweep excess {what} {ex:.3g}")
    assert ex <= 1.0, f"{what}: |out-ref| exceeds {P64_TOL} * max(1,|ref|) by a factor {ex:.3g}"
    return ex


def _assert_routes_agree(mx, dense, what):
    assert np.array_equal(mx != 0, dense != 0), what
    d = float((np.abs(mx - dense) / np.maximum(1.0, np.abs(mx))).max()) if mx.size else 0.0
    print(f"f64-sweep route-diff {what} {d:.3g}")
    assert d <= ROUTE_TOL, f"{what}: matrix-core and vector kernels differ by {d:.3g} relative"


def _device_inputs(v, mol, mode):
    chan = None if mol["chan"] is None else v.asarray(mol["chan"], mode)
    radii = mol["radii"] if np.isscalar(mol["radii"]) else v.asarray(mol["radii"], "radii")
    return v.asarray(mol["xyz"], "coords"), chan, radii


def _plan_of(v, keys):
    p = v.last_plan()
    return {k: p[k] for k in keys}


# ---- a. every row, one molecule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_row(row):
    import torch

    g, mol = row.g, R.make_molecule(row)
    v = _voxelizer(g.D, row.radii, row.density, R.SIGMA, row.blockdim, "torch")
    coords, chan, radii = _device_inputs(v, mol, row.mode)
    if row.geom == "E":  # slice 1 of a batch grid of odd slices: 8 bytes off 16-byte alignment
        whole = v.get_empty_grid(row.nch, batch_size=2)
        grid = whole[1]
        assert grid.data_ptr() % 16 == 8
    else:
        whole = grid = v.get_empty_grid(row.nch)
    whole.fill_(7.0)  # stale content must be overwritten
    out = v.forward(coords, None, chan, radii, out_grid=grid)
    assert out is grid
    assert _plan_of(v, row.plan) == row.plan, v.last_plan()
    first = out.clone()
    if row.geom == "E":
        assert bool((whole[0] == 7.0).all()), "the call wrote outside its grid"
    ref = _ref(g.D, row.blockdim, mol["xyz"], mol["chan"], mol["radii"], row.radii, row.density, row.nch)
    exact = row.density == "binary" and row.mode != "features"
    _assert_bars(first.cpu().numpy(), ref, exact, row.id)
    grid.fill_(3.0)
    assert torch.equal(v.forward(coords, None, chan, radii, out_grid=grid), first), "two runs of the same call differ"
    if row.route == R.F64_MX:  # the same call through the vector kernels: 16 channels per chunk, the library's exp
        v.debug_option("max_ct64", 16)
        grid.fill_(5.0)
        dense = v.forward(coords, None, chan, radii, out_grid=grid)
        assert _plan_of(v, ("route", "ct", "ncc")) == dict(route=R.F64_DENSE, ct=16, ncc=row.ncc16), v.last_plan()
        dense = dense.cpu().numpy()
        _assert_bars(dense, ref, exact, row.id + "/ct16")
        _assert_routes_agree(first.cpu().numpy(), dense, row.id)


# ---- b. the row as molecule 1 of [small, row, empty, small] --------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", R.BATCH_ROWS, ids=R.BATCH_IDS)
def test_row_in_a_batch(row):
    import torch

    g, batch = row.g, R.make_batch(row)
    mols, sizes = batch["mols"], batch["sizes"]
    xyz = np.concatenate([m["xyz"] for m in mols])
    chan = None if row.mode == "single" else np.concatenate([m["chan"] for m in mols])
    radii = np.concatenate([m["radii"] for m in mols]) if row.radii == "atom-wise" else mols[1]["radii"]
    exact = row.density == "binary" and row.mode != "features"

    v = _voxelizer(g.D, row.radii, row.density, R.SIGMA, row.blockdim, "torch")
    d_xyz = v.asarray(xyz, "coords")
    d_chan = None if chan is None else v.asarray(chan, row.mode)
    d_radii = radii if np.isscalar(radii) else v.asarray(radii, "radii")
    d_cen = v.asarray(batch["centers"], "center")
    grid = v.get_empty_grid(row.nch, batch_size=4)
    grid.fill_(7.0)
    out = v.forward_batch(d_xyz, batch["offsets"], d_cen, d_chan, d_radii, num_channels=row.nch, out_grid=grid)
    assert out is grid and _plan_of(v, ("route", "ct", "ncc", "nw", "nzc")) == {k: row.plan[k] for k in ("route", "ct", "ncc", "nw", "nzc")}
    for b, n in enumerate(sizes):
        if n == 0:
            assert not bool(out[b].any())
            continue
        lo, hi = int(batch["offsets"][b]), int(batch["offsets"][b + 1])
        one = v.forward(d_xyz[lo:hi], d_cen[b], None if d_chan is None else d_chan[lo:hi],
                        d_radii[lo:hi] if row.radii == "atom-wise" else d_radii, out_grid=v.get_empty_grid(row.nch).fill_(2.0))
        assert torch.equal(out[b], one), (row.id, b)
        ref = _ref(g.D, row.blockdim, mols[b]["moved"], mols[b]["chan"], mols[b]["radii"], row.radii, row.density, row.nch)
        _assert_bars(out[b].cpu().numpy(), ref, exact, f"{row.id}/batch{b}")
    # numpy inputs and outputs: host staging must give the bits of the device call
    vh = _voxelizer(g.D, row.radii, row.density, R.SIGMA, row.blockdim, "numpy")
    hgrid = vh.get_empty_grid(row.nch, batch_size=4)
    hgrid.fill(7.0)
    hout = vh.forward_batch(xyz, batch["offsets"], batch["centers"], chan, radii, num_channels=row.nch, out_grid=hgrid)
    assert hout is hgrid and np.array_equal(hout, out.cpu().numpy()), row.id


# ---- b2. slabs of more than 8 waves: the rows of a round are staged by waves 0 ... 7 alone ---------------------------------------------------
@pytest.mark.parametrize("C_, radii_type, density, blockdim", [(4, "scalar", "gaussian", None), (16, "channel-wise", "binary", 12)],
                         ids=["C4-scalar-gaussian", "C16-channel-wise-binary-bd12"])
def test_nine_waves_per_slab(C_, radii_type, density, blockdim):
    """D = 72 is nine z sub-tiles: the plan cuts a row 8 + 1; debug_option("nw", 9) keeps it in one slab of nine waves, which the
    rows above (nw <= 8) never launch. Geometry B's blob (600 atoms, radius 2.0) puts more than 63 candidates on its central slabs,
    so they take several rounds, each staged by eight of the nine waves. Same candidates in the same order either way: the two
    cuts must give the same bits."""
    import torch

    D, radius = 72, R.GEOMS["B"].radius
    xyz = R.positions("B")
    n = xyz.shape[0]
    rng = np.random.default_rng(72_009 + C_)
    chan = rng.random((n, C_))
    radii = radius
    if radii_type == "channel-wise":
        radii = radius * rng.uniform(0.8, 1.0, C_)
        radii[C_ // 2] = radius
    lower = R.slab_counts(xyz, np.full(n, radius), D, 9, blockdim)[0]
    assert lower.max() > R.ONE_ROUND, int(lower.max())
    v = _voxelizer(D, radii_type, density, R.SIGMA, blockdim, "torch")
    coords, d_chan = v.asarray(xyz, "coords"), v.asarray(chan, "features")
    d_radii = radii if np.isscalar(radii) else v.asarray(radii, "radii")
    cut = v.forward(coords, None, d_chan, d_radii, out_grid=v.get_empty_grid(C_).fill_(7.0)).clone()
    assert _plan_of(v, ("route", "ct", "nw", "nzc")) == dict(route=R.F64_DENSE, ct=C_, nw=8, nzc=2), v.last_plan()
    v.debug_option("nw", 9)
    whole = v.forward(coords, None, d_chan, d_radii, out_grid=v.get_empty_grid(C_).fill_(3.0))
    assert _plan_of(v, ("route", "ct", "nw", "nzc")) == dict(route=R.F64_DENSE, ct=C_, nw=9, nzc=1), v.last_plan()
    assert torch.equal(whole, cut), "nine waves per slab and the 8 + 1 cut differ"
    ref = _ref(D, blockdim, xyz, chan, radii, radii_type, density, C_)
    _assert_bars(whole.cpu().numpy(), ref, False, f"nw9-C{C_}-{radii_type}-{density}")


# ---- c. the fuzz draws at precision 64 --------------------------------------------------------------------------------------------------------------
def _case_inputs(v, case):
    coords, center, chan, radii = case["xyz"], case["center"], case["chan"], case["radii"]
    if not case["device"]:
        return coords, center, chan, radii
    return (v.asarray(coords, "coords"), None if center is None else v.asarray(center, "center"),
            None if chan is None else v.asarray(chan, case["mode"]), radii if np.isscalar(radii) else v.asarray(radii, "radii"))


def _fill(grid, value):
    if hasattr(grid, "fill_"):
        grid.fill_(value)
    else:
        grid.fill(value)
    return grid


def _summary(case):
    return {k: v for k, v in case.items() if k not in ("xyz", "chan", "radii")}


@pytest.mark.parametrize("seed", range(64))
def test_random_configuration_f64(seed):
    case = _draw(3000 + seed)
    if case["N"] == 0 and case["mode"] == "types":
        pytest.skip("max(types) of an empty array: the reference raises as well (numpy/voxelizer.py:278)")
    v = _voxelizer(case["D"], case["radii_type"], case["density"], case["sigma"], case["blockdim"],
                   "torch" if case["device"] else "numpy", res=case["res"])
    coords, center, chan, radii = _case_inputs(v, case)
    nch = 1 if case["mode"] == "single" else case["C"]
    moved = case["xyz"] - case["center"] if case["center"] is not None else case["xyz"]
    ref = _reference(case, moved, 64)
    exact = case["density"] == "binary" and case["mode"] != "features"
    outs = {}
    for ct64 in (32, 16):
        v.debug_option("max_ct64", ct64)
        grid = _fill(v.get_empty_grid(nch), 7.0)
        out = v.forward(coords, center, chan, radii, out_grid=grid)
        assert out is grid
        outs[ct64] = _host(out).copy()
        plan = v.last_plan()
        assert plan["route"] in (R.F64_DENSE, R.F64_MX) and (ct64 == 32 or plan["route"] == R.F64_DENSE), plan
        _assert_bars(outs[ct64], ref, exact, f"fuzz{seed}/ct{ct64} {_summary(case)}")
    _assert_routes_agree(outs[32], outs[16], f"fuzz{seed}")


# ---- d. ... with the in-call random transform ---------------------------------------------------------------------------------------------------------
TRANSFORM_BASE = 3500


def test_transform_draws_cover_every_radii_type_and_both_routes():
    cases = [_draw(TRANSFORM_BASE + s) for s in range(16)]
    live = [c for c in cases if c["N"] > 0]
    assert {c["radii_type"] for c in live} == {"scalar", "atom-wise", "channel-wise"}
    assert any(c["C"] > 16 and c["mode"] != "single" and not (c["mode"] == "features" and c["radii_type"] == "channel-wise") for c in live)
    assert {c["device"] for c in live} == {True, False}


@pytest.mark.parametrize("seed", range(16))
def test_random_transform_f64(seed):
    """The reference's in-call random transform at precision 64: the host draws (quaternion, translation) from the global numpy
    RNG in the reference's order; the numpy port gets the coordinates do_transform produces from the same RNG state."""
    from molvoxel_amd.voxelizer.hip.transform import do_transform, draw_forward_transform

    case = _draw(TRANSFORM_BASE + seed)
    if case["N"] == 0 and case["mode"] == "types":
        pytest.skip("max(types) of an empty array: the reference raises as well (numpy/voxelizer.py:278)")
    v = _voxelizer(case["D"], case["radii_type"], case["density"], case["sigma"], case["blockdim"],
                   "torch" if case["device"] else "numpy", res=case["res"])
    coords, center, chan, radii = _case_inputs(v, case)
    nch = 1 if case["mode"] == "single" else case["C"]
    np.random.seed(seed)
    out = v.forward(coords, center, chan, radii, 0.7, True, out_grid=_fill(v.get_empty_grid(nch), 7.0))
    np.random.seed(seed)  # replay: same RNG state -> same draw -> the reference's transform arithmetic on the host (float64)
    translation, quaternion = draw_forward_transform(0.7, True)
    moved = case["xyz"] - case["center"] if case["center"] is not None else case["xyz"]
    moved = do_transform(moved, None, translation, quaternion)
    ref = _reference(case, moved, 64)
    _assert_bars(_host(out), ref, case["density"] == "binary" and case["mode"] != "features", f"xform{seed} {_summary(case)}")


# ---- e. ragged batches ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(24))
def test_random_batches_f64(seed):
    """forward_batch over ragged molecules (empty ones included) with per-molecule centres, every operator: each molecule's grid
    within the bars of the numpy port for that molecule alone, and the bits of its own one-molecule call."""
    rng = np.random.default_rng(64_000 + seed)
    D = int(rng.choice([16, 24, 33, 48, 72]))
    res = float(rng.choice([0.4, 0.5, 1.0]))
    B = int(rng.choice([1, 2, 5, 9])) if D < 72 else int(rng.choice([1, 2, 3]))
    mode = str(rng.choice(["features", "types", "single"]))
    radii_type = str(rng.choice(["scalar", "atom-wise"] + ([] if mode == "single" else ["channel-wise"])))
    density = str(rng.choice(["gaussian", "binary"]))
    C_ = 1 if mode == "single" else int(rng.choice([1, 4, 6, 16, 17, 32, 35, 40]))
    if D == 72:
        C_ = min(C_, 17)
    W = res * (D - 1)
    sizes = [int(rng.choice([0, 1, 40, 300, 2000])) for _ in range(B)]
    centers = rng.uniform(-2, 2, (B, 3))
    coords = [rng.uniform(-W / 2 - 1, W / 2 + 1, (n, 3)) + centers[b] for b, n in enumerate(sizes)]
    feats = [rng.random((n, C_)) for n in sizes]
    types = [rng.integers(0, C_, n).astype(np.int16) for n in sizes]
    for t in types:
        t[:1] = C_ - 1  # (a one-molecule call takes its channel count from the largest type)
    r_atom = [rng.uniform(0.8, 2.0, n) * res / 0.5 for n in sizes]
    r_chan = rng.uniform(0.8, 2.0, C_) * res / 0.5
    chan = None if mode == "single" else np.concatenate(feats if mode == "features" else types)
    radii = {"scalar": 1.3 * res / 0.5, "atom-wise": np.concatenate(r_atom), "channel-wise": r_chan}[radii_type]
    offsets = np.cumsum([0] + sizes)
    exact = density == "binary" and mode != "features"
    v = _voxelizer(D, radii_type, density, 0.6, None, "numpy", res=res)
    out = v.forward_batch(np.concatenate(coords), offsets, centers, chan, radii, num_channels=C_,
                          out_grid=_fill(v.get_empty_grid(C_, batch_size=B), 7.0)).copy()
    assert out.shape == (B, C_, D, D, D) and out.dtype == np.float64
    for b, n in enumerate(sizes):
        if n == 0:
            assert not out[b].any()
            continue
        ch = None if mode == "single" else (feats[b] if mode == "features" else types[b])
        rad = {"scalar": radii, "atom-wise": r_atom[b], "channel-wise": r_chan}[radii_type]
        ref = _ref(D, None, coords[b] - centers[b], ch, rad, radii_type, density, C_, sigma=0.6, res=res)
        _assert_bars(out[b], ref, exact, f"batch{seed}/{b} D{D} C{C_} {mode} {radii_type} {density} n{n}")
        one = v.forward(coords[b], centers[b], ch, rad, out_grid=_fill(v.get_empty_grid(C_), 2.0))
        assert np.array_equal(out[b], one), (seed, b)


# ---- f. the two exp implementations against exact values ---------------------------------------------------------------------------------------------
EXP_SIGMAS = (1.0, 0.5, 0.3, 0.1, 0.05, 0.03, 0.026, 0.02)
EXP_ATOMS = ((0.13, -0.21, 0.07), (1.37, 0.52, -0.88), (-2.9, 3.1, 0.3))  # off the grid nodes; the last one near a corner of the box
MIN_NORMAL = decimal.Decimal(2) ** -1022
SPACING = decimal.Decimal(2) ** -1074


def _ulp(e: decimal.Decimal) -> decimal.Decimal:
    """Spacing of float64 at the exact normal value e."""
    k = math.frexp(float(e))[1] - 1  # 2^k <= e < 2^(k + 1), but for the rounding of float(e)
    while decimal.Decimal(2) ** (k + 1) <= e:
        k += 1
    while decimal.Decimal(2) ** k > e:
        k -= 1
    return decimal.Decimal(2) ** (k - 52)


def test_exp_of_the_matrix_core_walk_against_exact_values():
    """One atom, weight 1 in channel 0 of 32: an admitted voxel holds exp(c * d2) and nothing else, d2 in cdist order and
    c = -0.5 / ((r sigma) (r sigma)) as the pre-pass forms them (restated here bit for bit), exp by exp_nonpos64 (matrix-core
    route) or the library's (max_ct64 = 16). Exact values: decimal exp of the float64 product at 50 digits. Arguments span
    0 ... -1250: normal results within 2 ulp (0.5 the correctly rounded table value, 0.5 the final fma, < 0.1 reduction and series),
    subnormal results within one spacing of the exactly rounded value, exact zero wherever the exact value rounds to zero.
    Measured worst error over the 5364 normal results of each route: exp_nonpos64 0.975 ulp, the library's exp 0.825 ulp
    (DESIGN.md section 10)."""
    D, C_, r = 16, 32, 2.0
    half = R.RES * (D - 1) / 2.0
    g = np.arange(D, dtype=np.float64) * R.RES - half
    feats = np.zeros((1, C_))
    feats[0, 0] = 1.0
    ctx = decimal.Context(prec=50)
    worst = {32: 0.0, 16: 0.0}
    kinds = {"normal": 0, "subnormal": 0, "zero": 0}
    for sigma in EXP_SIGMAS:
        v = _voxelizer(D, "scalar", "gaussian", sigma, None, "numpy")
        c = -0.5 / ((r * sigma) * (r * sigma))
        for atom in EXP_ATOMS:
            xyz = np.array([atom], np.float64)
            dx, dy, dz = xyz[0, 0] - g, xyz[0, 1] - g, xyz[0, 2] - g
            d2 = ((dx * dx)[:, None, None] + (dy * dy)[None, :, None]) + (dz * dz)[None, None, :]
            arg = c * d2
            inside = d2 < r * r * (1 - 1e-12)
            assert not (np.abs(d2 - r * r) <= 1e-12 * r * r).any() and inside.sum() > 100
            ref = _ref(D, None, xyz, feats, r, "scalar", "gaussian", C_, sigma=sigma)
            for ct64 in (32, 16):
                v.debug_option("max_ct64", ct64)
                out = v.forward(xyz, None, feats, r, out_grid=_fill(v.get_empty_grid(C_), 7.0))
                assert v.last_plan()["route"] == (R.F64_MX if ct64 == 32 else R.F64_DENSE)
                assert not out[1:].any() and not out[0][~inside].any()
                assert_membership(out, ref)  # the reference agrees on which voxels are non-zero
                for idx in zip(*np.nonzero(inside)):
                    exact = ctx.exp(decimal.Decimal(float(arg[idx])))
                    got = decimal.Decimal(float(out[0][idx]))
                    if exact >= MIN_NORMAL:
                        err = float(abs(got - exact) / _ulp(exact))
                        worst[ct64] = max(worst[ct64], err)
                        kinds["normal"] += 1
                        assert err <= 2.0, (sigma, atom, ct64, idx, float(arg[idx]), err)
                    else:
                        q = (exact / SPACING).to_integral_value(rounding=decimal.ROUND_HALF_EVEN, context=ctx)
                        if q == 0:
                            kinds["zero"] += 1
                            assert got == 0, (sigma, atom, ct64, idx, float(arg[idx]), float(got))
                        else:
                            kinds["subnormal"] += 1
                            assert abs(got / SPACING - q) <= 1, (sigma, atom, ct64, idx, float(arg[idx]), float(got))
    print(f"f64-sweep exp worst-ulp matrix-core {worst[32]:.3f} library {worst[16]:.3f} voxels {kinds}")
    assert kinds["normal"] > 1000 and kinds["subnormal"] >= 4 and kinds["zero"] > 100
