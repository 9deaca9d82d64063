"""forward_batch calls that mvx_capi.hip cuts into several launches, through every kernel family that decodes the cut.

One call is cut along molecules (`plan.nchunk > 1`, `VoxParams::b0`: gridDim.y limit, Infinity Cache budget, the "chunks" side
stream) and along channels (channel chunks, the remainder launch with `c0`, the grouped launch). A wrong `b0`, `c0` or `ncc` in
one family writes a plausible grid of the wrong molecule or leaves channels stale. Every case here has three checks:

1. each checked molecule's grid against the oracle for that molecule alone (oracle.c_oracle, float32; oracle.numpy_port at
   precision 64), at the bars of tests/tolerance.py: membership identical, binary types / single bit-exact, GAUSS_TOL, P64_TOL.
   A bfloat16 grid must have the bits of the float32 grid rounded by torch (the bar of tests/test_hip_bf16.py), and that float32
   grid is held to the oracle;
2. the cut call bit for bit against the same call in one launch;
3. the call really was cut: last_plan() (mvx_debug_last_plan: the plan the call took, debug options applied) has the expected
   nchunk >= 2 and the row's family fields, and with profiling on read_kernel_times_ms() has one entry per voxelize launch -
   nchunk * (1 + remainder launch) on the float32 binned route, which must exceed the uncut run's. A float64 call times ONE
   bracket whatever its cut (both float64 kernels launch behind all pre-passes, 65535 // ncc molecules per launch, and the bracket
   rides on the first launch only), so the profile hook cannot count float64 cuts: there the test asserts the one entry and the
   plan's nchunk.

Before every cut call the same handle voxelizes a mirrored copy of the batch, so the workspace holds another batch's candidate
lines of the same shape: a pre-pass that fills the wrong molecules' lines leaves wrong, never uninitialised, data behind.

Sections: A forced cuts at small shapes (tests/batch_cut_rows.py ROWS; its plan fields are asserted on the host by
tests/test_batch_cuts_host.py and again here), B the gridDim.y limit for real (BIG; grids of 8^3 voxels for up to four channels,
16^3 where the narrow multi-sub-tile kernel has to be reached, 4^3 above four channels, so that 65 536+ molecules stay under 2 GB), C the production Infinity Cache cut beyond 2^32 grid elements.
"""
import dataclasses
import time

import numpy as np
import pytest

from tests import batch_cut_rows as R
from tests.abi import MVX_ERR_ALLOC
from tests.tolerance import GAUSS_TOL, P64_TOL, assert_gaussian

pytestmark = pytest.mark.gpu

TRANSLATION = 0.7


def _voxelizer(case, options=True):
    import molvoxel_amd as mv

    kw = {}
    if getattr(case, "blockdim", None) is not None:
        kw["blockdim"] = case.blockdim
    if case.bf16:
        kw["grid_dtype"] = "bfloat16"
    if case.cl:
        kw["grid_layout"] = "channels_last"
    v = mv.create_voxelizer(R.RES, case.D, case.radii, case.density, "hip", sigma=R.SIGMA, precision=case.precision, output="torch", **kw)
    if options:
        v.debug_option("direct", 0)
        if getattr(case, "narrow_sub", 0):
            v.debug_option("narrow_sub", case.narrow_sub)
    return v


def _bits(t):
    import torch

    return t.view({torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}[t.dtype])


def _same_bits(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _host(grid):
    return grid.contiguous().cpu().numpy()


def _oracle(case, coords, chan, radii):
    from oracle import c_oracle, numpy_port

    nch = 1 if case.mode == "single" else case.C
    blockdim = getattr(case, "blockdim", None)
    kw = dict(radii_type=case.radii, density=case.density, sigma=R.SIGMA, num_channels=nch)
    if case.precision == 32:
        return c_oracle.voxelize(coords, chan, radii, resolution=R.RES, dimension=case.D, blockdim=blockdim, **kw)
    return numpy_port.voxelize(numpy_port.GridSpec(R.RES, case.D, blockdim), coords, chan, radii, precision=64, **kw)


def _compare(case, got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, what
    bad = int(np.not_equal(got != 0, ref != 0).sum())
    assert bad == 0, f"{what}: membership differs in {bad} voxels"
    if case.density == "binary" and case.mode != "features":
        assert np.array_equal(got, ref), what
    else:
        assert_gaussian(got, ref, GAUSS_TOL if case.precision == 32 else P64_TOL)


# ---- A. forced molecule cuts through every kernel family ---------------------------------------------------------------------------
def _inputs(v, row, batch, mirror=False):
    """forward_batch arguments of the row's batch (device tensors or numpy arrays); mirror: the decoy with every molecule reflected."""
    sign = -1.0 if mirror else 1.0
    coords = np.concatenate([sign * c + batch["centers"][b] for b, c in enumerate(batch["coords"])])
    chan = {"features": np.concatenate(batch["feats"]), "types": np.concatenate(batch["types"]), "single": None}[row.mode]
    radii = {"scalar": R.SCALAR_RADIUS, "atom-wise": np.concatenate(batch["r_atom"]), "channel-wise": batch["r_chan"]}[row.radii]
    centers = batch["centers"]
    if row.device:
        coords, centers = v.asarray(coords, "coords"), v.asarray(centers, "center")
        chan = None if chan is None else v.asarray(chan, row.mode)
        radii = radii if np.isscalar(radii) else v.asarray(radii, "radii")
    return coords, centers, chan, radii


def _call(v, row, batch, inputs, seed=None):
    """One profiled forward_batch into a grid full of stale content; returns (grid, timed voxelize launches, the plan the call took)."""
    import torch

    B, nch = len(batch["sizes"]), (1 if row.mode == "single" else row.C)
    if row.misaligned:  # a view 4 bytes off 16-byte alignment: the run-wise write-out on an aligned dimension
        n = B * nch * row.D**3
        out = torch.empty(n + 4, dtype=torch.float32, device=v.device)[1:1 + n].view(B, nch, row.D, row.D, row.D)
        assert out.data_ptr() % 16 == 4
    else:
        out = v.get_empty_grid(nch, batch_size=B)
    out.fill_(7.0)
    coords, centers, chan, radii = inputs
    if seed is not None:
        np.random.seed(seed)
    v.set_profiling(True)
    got = v.forward_batch(coords, batch["offsets"], centers, chan, radii, num_channels=nch, out_grid=out,
                          random_translation=TRANSLATION if row.transform else 0.0, random_rotation=row.transform)
    assert got is out
    launches = len(v.read_kernel_times_ms())
    v.set_profiling(False)
    return got, launches, v.last_plan()


def _run(row, batch, budget_kb=0, chunks=0, seed=None):
    v = _voxelizer(row)
    if budget_kb or chunks:
        _call(v, row, batch, _inputs(v, row, batch, mirror=True), seed)  # the workspace now holds the decoy's lines, uncut
    if budget_kb:
        v.debug_option("mall_budget_kb", budget_kb)
    if chunks:
        v.debug_option("chunks", chunks)
    return _call(v, row, batch, _inputs(v, row, batch), seed)


def _moved(row, batch, seed):
    """Coordinates the oracle gets: centred, and with the call's random transforms replayed from the same RNG state (one draw per
    molecule in molecule order, empty molecules included), as tests/test_hip_fuzz.py does."""
    if not row.transform:
        return batch["coords"]
    from molvoxel_amd.voxelizer.hip.transform import do_transform, draw_forward_transform

    np.random.seed(seed)
    out = []
    for c in batch["coords"]:
        translation, quaternion = draw_forward_transform(TRANSLATION, True)
        out.append(do_transform(c, None, translation, quaternion) if c.shape[0] else c)
    return out


@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_forced_molecule_cuts(row):
    batch = R.make_batch(row)
    sizes = batch["sizes"]
    B, total = len(sizes), int(sum(sizes))
    p = R.host_plan(row, sizes)
    assert {k: p[k] for k in row.plan} == row.plan, p  # the row is the family it names
    seed = 1000 + R.ROW_IDS.index(row.id) if row.transform else None

    uncut, n0, took = _run(row, batch, seed=seed)
    assert n0 == R.expected_launches(p, 1), (n0, p)
    assert took == p, (took, p)  # (no option of the uncut run changes this batch's plan)
    f64 = row.precision == 64
    cuts = [(0, c) for c in row.chunks]
    if not f64:  # budgets for 2-3 chunks and for one molecule per chunk (empty chunks included); the latter is checked last
        cuts += [(R.budget_for(p, B, row.C, total, 3 if B >= 6 else 2), 0), (1, 0)]
    for budget_kb, chunks in cuts:
        nchunk = R.expected_nchunk(p, B, row.C, total, row.precision, budget_kb, chunks)
        assert nchunk >= 2, (budget_kb, chunks)
        got, n, took = _run(row, batch, budget_kb, chunks, seed)
        assert took["nchunk"] == nchunk and {k: took[k] for k in row.plan} == row.plan, (budget_kb, chunks, nchunk, took)
        assert n == R.expected_launches(p, nchunk), (budget_kb, chunks, nchunk, n)
        assert f64 or n > n0
        assert _same_bits(got, uncut), f"cut into {nchunk} (budget {budget_kb} KB, chunks {chunks}) differs from one launch"
    if not f64:
        assert nchunk == B

    grid = got  # the most finely cut run, bit-identical to all others
    if row.bf16:  # float32 grid of the same (uncut) call: the bfloat16 grid is its rounding, and it is held to the oracle
        import torch

        grid = _run(dataclasses.replace(row, bf16=False), batch, seed=seed)[0]
        assert _same_bits(got, grid.to(torch.bfloat16))
    moved = _moved(row, batch, seed)
    for b, n_atoms in enumerate(sizes):
        g = _host(grid[b])
        if n_atoms == 0:
            assert not g.any(), b
            continue
        chan = {"features": batch["feats"][b], "types": batch["types"][b], "single": None}[row.mode]
        rad = {"scalar": R.SCALAR_RADIUS, "atom-wise": batch["r_atom"][b], "channel-wise": batch["r_chan"]}[row.radii]
        _compare(row, g, _oracle(row, moved[b], chan, rad), f"molecule {b}")


# ---- B. the gridDim.y limit for real ----------------------------------------------------------------------------------------------
def _big_data(case):
    """1 ... 5 atoms per molecule (a sixth of the molecules empty) inside and just outside the box; features carry the molecule
    index, types and coordinates are random per molecule: no two molecules share a grid."""
    rng = np.random.default_rng(R.BIG_IDS.index(case.id))
    sizes = R.big_sizes(case)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    total = int(offsets[-1])
    mol = np.repeat(np.arange(case.B), sizes)
    W = R.RES * (case.D - 1)
    coords = rng.uniform(-W / 2 - 0.5, W / 2 + 0.5, (total, 3))
    feats = (0.25 + 0.5 * rng.random((total, case.C)) + ((mol[:, None] * 37 + np.arange(case.C)[None, :] * 11) % 101) / 404.0).astype(np.float32)
    types = rng.integers(0, case.C, total).astype(np.int16)
    r_atom = rng.uniform(0.8, 1.6, total).astype(np.float32)
    r_chan = rng.uniform(0.8, 1.6, case.C).astype(np.float32)
    return dict(sizes=sizes, offsets=offsets, coords=coords, feats=feats, types=types, r_atom=r_atom, r_chan=r_chan)


def _big_call(v, case, d, lo=0, hi=None, mirror=False):
    """forward_batch of molecules [lo, hi) from device-resident inputs."""
    hi = case.B if hi is None else hi
    o0, o1 = int(d["offsets"][lo]), int(d["offsets"][hi])
    sl = slice(o0, o1)
    coords = v.asarray((-d["coords"][sl]) if mirror else d["coords"][sl], "coords")
    chan = {"features": lambda: v.asarray(d["feats"][sl], "features"), "types": lambda: v.asarray(d["types"][sl], "types"),
            "single": lambda: None}[case.mode]()
    radii = {"scalar": lambda: R.SCALAR_RADIUS, "atom-wise": lambda: v.asarray(d["r_atom"][sl], "radii"),
             "channel-wise": lambda: v.asarray(d["r_chan"], "radii")}[case.radii]()
    nch = 1 if case.mode == "single" else case.C
    return v.forward_batch(coords, d["offsets"][lo:hi + 1] - o0, None, chan, radii, num_channels=nch)


@pytest.mark.parametrize("case", R.BIG, ids=R.BIG_IDS)
def test_grid_y_limit(case):
    import torch

    assert R.big_output_bytes(case) < R.MAX_OUTPUT_BYTES
    p = R.big_host_plan(case)
    assert {k: p[k] for k in case.plan} == case.plan, p
    per = R.GRID_Y_MAX // p["ncc"]
    edge = case.B * p["ncc"] <= R.GRID_Y_MAX  # the largest batch the limit leaves in one launch
    assert edge == case.id.endswith(("-65535", "-32767")) and (edge or case.B > per)
    cuts = R.big_cut_points(case, p)
    assert edge or cuts
    d = _big_data(case)

    v = _voxelizer(case, options=False)  # no debug option: the production plan
    _big_call(v, case, d, mirror=True)  # (the workspace holds another batch's lines)
    v.set_profiling(True)
    big = _big_call(v, case, d)
    launches = len(v.read_kernel_times_ms())
    assert v.last_plan() == p, (v.last_plan(), p)
    assert launches == R.expected_launches(p, p["nchunk"]), (launches, p)
    if case.narrow >= 0:
        assert R.narrow_sub_tiles(p, 0, case.cl) == case.narrow
    if case.precision == 32 and not edge:
        assert p["nchunk"] >= 2 and launches >= 2
    assert big.numel() * big.element_size() == R.big_output_bytes(case)

    # every molecule, bit for bit, against calls of at most SUB_BATCH molecules
    ref_v = _voxelizer(case, options=False)
    covered = 0
    for lo in range(0, case.B, R.SUB_BATCH):
        hi = min(lo + R.SUB_BATCH, case.B)
        sub = _big_call(ref_v, case, d, lo, hi)
        assert _same_bits(big[lo:hi], sub), f"molecules [{lo}, {hi}) differ from their own call"
        covered += hi - lo
        del sub
    assert covered == case.B

    grid = big
    if case.bf16:
        grid = _big_call(_voxelizer(dataclasses.replace(case, bf16=False), options=False), case, d)
        assert _same_bits(big, grid.to(torch.bfloat16))
    rng = np.random.default_rng(99)
    picks = {0, case.B - 1} | {c - 1 for c in cuts} | set(cuts) | {int(b) for b in rng.integers(0, case.B, 50)}
    assert all(0 <= b < case.B for b in picks)
    for b in sorted(picks):
        g = _host(grid[b])
        o0, o1 = int(d["offsets"][b]), int(d["offsets"][b + 1])
        if o0 == o1:
            assert not g.any(), b
            continue
        chan = {"features": d["feats"][o0:o1], "types": d["types"][o0:o1], "single": None}[case.mode]
        rad = {"scalar": R.SCALAR_RADIUS, "atom-wise": d["r_atom"][o0:o1], "channel-wise": d["r_chan"]}[case.radii]
        _compare(case, g, _oracle(case, d["coords"][o0:o1], chan, rad), f"molecule {b}")
    del big, grid
    torch.cuda.empty_cache()


# ---- C. beyond 2^32 elements: the production Infinity Cache cut, no knobs ----------------------------------------------------------
@pytest.mark.parametrize("bf16_cl", [False, True], ids=["float32-ncdhw", "bfloat16-channels-last"])
def test_production_cut_beyond_2_pow_32_elements(bf16_cl):
    """513 cfg-2 molecules (C = 32, 64^3, 4 000 atoms each) in one call: 4.3e9 grid elements (17.2 GB of float32, 8.6 GB of
    bfloat16), element offsets cross 2^32 at molecule 512 and the production budget cuts the call in two at molecule 256.
    The grid stays on the device; molecule pairs {0, 1}, both sides of the cut and {511, 512} are compared bit for bit with
    their own two-molecule calls, three of those molecules with the C oracle. Skips only when the allocation fails."""
    import torch

    from molvoxel_amd import workloads
    from molvoxel_amd.voxelizer.hip import _lib
    from oracle import c_oracle

    B, C_, D, N = 513, 32, 64, 4000
    case = R.Big("cfg2x513", D, C_, B, bf16=bf16_cl, cl=bf16_cl)
    grid_type, layout = R.grid_codes(case)
    p = _lib.plan_call(D, C_, B, total_atoms=B * N, max_atoms=N, grid_type=grid_type, layout=layout)
    assert p["route"] == R.BINNED and p["nchunk"] >= 2 and p["ct_rem"] == 0
    assert B * C_ * D**3 > 1 << 32 and 512 * C_ * D**3 == 1 << 32
    cut = [R.chunk_begin(B, p["nchunk"], k) for k in range(1, p["nchunk"])]
    pairs = [(0, 1)] + [(c - 1, c) for c in cut] + [(511, 512)]

    wl = workloads.cfg2(batch=B)
    offsets = np.arange(B + 1, dtype=np.int64) * N
    import molvoxel_amd as mv

    kw = dict(grid_dtype="bfloat16", grid_layout="channels_last") if bf16_cl else {}
    v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", sigma=0.5, output="torch", **kw)
    coords = v.asarray(np.concatenate(wl.coords), "coords")
    feats = v.asarray(np.concatenate(wl.channels), "features")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    free0 = torch.cuda.mem_get_info()[0]
    v.set_profiling(True)
    t0 = time.perf_counter()
    try:
        big = v.forward_batch(coords, offsets, None, feats, 1.0)
    except torch.cuda.OutOfMemoryError as e:  # the grid (torch's allocator)
        pytest.skip(f"not enough device memory for {B} cfg-2 grids: {e}")
    except RuntimeError as e:  # the library's workspace: MVX_ERR_ALLOC, "hipMalloc: ..." (anything else is an error)
        if not str(e).startswith(f"libmvx_hip error {MVX_ERR_ALLOC}: hipMalloc"):
            raise
        pytest.skip(f"not enough device memory for the workspace of {B} cfg-2 molecules: {e}")
    torch.cuda.synchronize()
    seconds = time.perf_counter() - t0
    used = free0 - torch.cuda.mem_get_info()[0]  # the grid and the library's own workspace (hipMalloc, outside torch's allocator)
    kernel_ms = v.read_kernel_times_ms()
    launches = len(kernel_ms)
    print(f"\n[batch cuts C] {'bfloat16 channels-last' if bf16_cl else 'float32 NCDHW'}: grid {big.numel() * big.element_size() / 1e9:.2f} GB, "
          f"device memory taken by the call {used / 1e9:.2f} GB (torch allocator peak {torch.cuda.max_memory_allocated() / 1e9:.2f} GB), "
          f"wall time of the first call {1e3 * seconds:.1f} ms, voxelize launches {[round(t, 2) for t in kernel_ms]} ms")
    assert v.last_plan() == p, (v.last_plan(), p)
    assert launches == p["nchunk"] and launches >= 2

    ref_v = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", sigma=0.5, output="torch", **kw)
    v32 = mv.create_voxelizer(0.5, D, "scalar", "gaussian", "hip", sigma=0.5, output="torch", **({"grid_layout": "channels_last"} if bf16_cl else {}))
    checked = 0
    for a, b in pairs:
        sl = slice(a * N, (b + 1) * N)
        assert b == a + 1
        sub = ref_v.forward_batch(coords[sl], offsets[:3], None, feats[sl], 1.0)
        assert _same_bits(big[a:b + 1], sub), (a, b)
        if checked < 3:  # three molecules against the oracle: 0, the first of the second chunk, 512
            m = b if checked else a
            g = sub[m - a]
            if bf16_cl:
                g32 = v32.forward_batch(coords[m * N:(m + 1) * N], offsets[:2], None, feats[m * N:(m + 1) * N], 1.0)[0]
                assert _same_bits(g, g32.to(torch.bfloat16))
                g = g32
            assert_gaussian(_host(g), c_oracle.voxelize(wl.coords[m], wl.channels[m], 1.0, dimension=D, sigma=0.5))
            checked += 1
    assert checked == 3
    del big, sub
    torch.cuda.empty_cache()
