"""The differentiable entries and the device-pose path of the forward on batches of many molecules (tests/many_molecules_rows.py;
its conditions are asserted on the host by tests/test_many_molecules_host.py).

A the ladder batch, B = 203 = 3 x 64 + 11 molecules of 0 ... 513 atoms with runs of empty molecules: every row against the float64
  references on a sample, the whole call bit for bit against the same batch in six separate calls (the kernels promise "the same
  bits in any batch", which is what makes the sample hide nothing), exact zeros from outputs that start as NaN, both processing
  orders; the call-wide sums on a thin ladder the reference reads completely; a mixed record array through the C ABI.
B tiny totals (1 ... 33 atoms) under the spatial order, where most of its 8 x span workgroups are empty.
C B = 70 001: 70 001 records through find_molecule and through pose_resolve_kernel (1 094 workgroups), mvx_pose_grad_batch.
D dL/dgrid and per-molecule fields past 2^31 and 2^32 elements.
E posed forward calls cut into several launches.

Bars: tests/tolerance.py as the existing tests use them, with the references' own bounds: GRAD_REL / GRAD_ABS for float32 and
bfloat16 grids, GRAD64_REL / GRAD64_ABS for float64 grids and for the scores of binary types / single (exact terms summed in
float64 in another order), assert_gaussian for grids."""
import time

import numpy as np
import pytest

from tests import batch_cut_rows as R
from tests import many_molecules_rows as M
from tests import pose_reference as pr
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL, assert_gaussian

pytestmark = pytest.mark.gpu


def _vox(D, radii_type="scalar", density="gaussian", kind="f32", **kw):
    import molvoxel_amd as mv

    if kind == "bf16":
        kw["grid_dtype"] = "bfloat16"
    return mv.create_voxelizer(0.5, D, radii_type, density, library="hip", precision=64 if kind == "f64" else 32, **kw)


def _gdt(kind):
    import torch

    return {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[kind]


def _device(d):
    """The batch's arrays on the device as the C ABI reads them, and the packed (B, 10) poses [c | q | t]."""
    import torch

    fdt = torch.float64 if d["kind"] == "f64" else torch.float32
    dev = dict(c=torch.tensor(d["xyz"], device="cuda"), ch=None, r=None,
               pose=torch.tensor(np.concatenate([d["cen"], d["q"], d["t"]], axis=1), device="cuda"))
    if d["mode"] == "features":
        dev["ch"] = torch.tensor(d["chan"], device="cuda").to(fdt)
    elif d["mode"] == "types":
        dev["ch"] = torch.tensor(d["chan"], device="cuda").to(torch.int32)
    if not np.isscalar(d["radii"]):
        dev["r"] = torch.tensor(d["radii"], device="cuda").to(fdt)
    return dev


def _generator(d):
    """A device generator seeded from the batch: buffers filled on the device hold the same values in every run."""
    import torch

    g = torch.Generator(device="cuda")
    g.manual_seed(int(d["seed"]))
    return g


def _how(d):
    return {"pose": "pose", "rotation": "rotation", "none": None}[d["transform"]]


def _abi(vox, d, dev, G, entry, lo=0, hi=None, how="default", plain_every=0):
    """One call of the C ABI on molecules [lo, hi) of the batch (offsets rebased; the slices of the atoms' arrays, of the
    per-molecule upstream or field and of the records). Outputs start as NaN: whatever is not overwritten fails every comparison.
    entry: backward | backward_radii | density | score. Returns the outputs (None where the call has none, or no atoms)."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    hi = d["B"] if hi is None else hi
    how = _how(d) if how == "default" else how
    a0, a1 = int(d["off"][lo]), int(d["off"][hi])
    n, Bn, C_, mode = a1 - a0, hi - lo, d["C"], d["mode"]
    fdt = torch.float64 if d["kind"] == "f64" else torch.float32
    nan = lambda shape, dt=torch.float64: torch.full(shape, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    ptr = lambda x: None if (x is None or x.numel() == 0) else x.data_ptr()  # noqa: E731
    chanwise = d["radii_type"] == "channel-wise"
    out = dict(gc=nan((n, 3)), gf=nan((n, C_), fdt) if mode == "features" else None, gr=None, gsig=None, grs=None, scores=None,
               atoms=None)
    if entry in ("backward_radii", "density") and d["radii_type"] != "scalar":
        out["gr"] = nan((C_,) if chanwise else (n,))
    if entry == "density":
        out["gsig"] = nan((1,))
        out["grs"] = nan((1,)) if d["radii_type"] == "scalar" else None
    if entry == "score":
        out["scores"], out["atoms"] = nan((Bn,)), nan((n,))
    if n == 0 and entry != "score":  # (no atoms: the entries return before they look at the outputs; there are no rows)
        return out
    off = np.ascontiguousarray(d["off"][lo:hi + 1] - a0)
    xf = None if how is None else M.records(d, lo, hi, how, dev["pose"].data_ptr(), plain_every)
    r = dev["r"] if (dev["r"] is None or chanwise) else dev["r"][a0:a1]
    ch = None if dev["ch"] is None else dev["ch"][a0:a1]
    g = G if G.dim() == 4 else G[lo:hi]
    assert g.is_contiguous() and g.dtype == _gdt(d["kind"])
    rs = float(d["radii"]) if np.isscalar(d["radii"]) else 0.0
    args = (vox._handle, _lib.MODES[mode], ptr(dev["c"][a0:a1]), ptr(ch), ptr(r), rs, vox._radii_type_code(), off.ctypes.data,
            None if xf is None else xf.ctypes.data, Bn, C_)
    s = vox._stream()
    if entry == "score":
        rc = vox._lib.mvx_score_batch(*args, ptr(g), 0 if G.dim() == 4 else C_ * d["D"] ** 3, ptr(out["scores"]), ptr(out["atoms"]),
                                      ptr(out["gc"]), ptr(out["gf"]), s)
    elif entry == "backward":
        rc = vox._lib.mvx_backward_batch(*args, ptr(g), ptr(out["gc"]), ptr(out["gf"]), s)
    elif entry == "backward_radii":
        rc = vox._lib.mvx_backward_radii_batch(*args, ptr(g), ptr(out["gc"]), ptr(out["gf"]), ptr(out["gr"]), s)
    else:
        rc = vox._lib.mvx_backward_density_batch(*args, ptr(g), ptr(out["gc"]), ptr(out["gf"]), ptr(out["gr"]), ptr(out["gsig"]),
                                                 ptr(out["grs"]), s)
    _lib.check(rc)
    torch.cuda.synchronize()
    return out


def _bits(t):
    import torch

    return t.contiguous().view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def _same(a, b):
    import torch

    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


PER_ATOM = ("gc", "gf", "atoms")
CALL_WIDE = ("gsig", "grs")


def _assert_pieces(d, whole, piece, cuts):
    """`whole` (the outputs of one call on the batch, or on molecules [cuts[0], cuts[-1]) of it) against piece(lo, hi) for every
    piece of `cuts`, bit for bit, on every output row; call-wide sums do not split and are not compared."""
    base_b, base_a = cuts[0], int(d["off"][cuts[0]])
    rows = 0
    for lo, hi in zip(cuts, cuts[1:]):
        got = piece(lo, hi)
        a0, a1 = int(d["off"][lo]) - base_a, int(d["off"][hi]) - base_a
        for k, v in got.items():
            if v is None or k in CALL_WIDE or (k == "gr" and v.shape[0] != a1 - a0):
                continue
            ref = whole[k][lo - base_b:hi - base_b] if k in ("scores", "pose", "grid") else whole[k][a0:a1]
            assert _same(v, ref), f"{k} of molecules [{lo}, {hi}) differs from their own call"
        rows += a1 - a0
    assert rows == int(d["off"][cuts[-1]]) - base_a


def _assert_same_outputs(a, b, what):
    for k in a:
        assert (a[k] is None) == (b[k] is None), (what, k)
        if a[k] is not None:
            assert _same(a[k], b[k]), f"{k}: {what}"


def _bars(d, density, what):
    exact_terms = density == "binary" and d["mode"] != "features" and what == "score"
    return (GRAD64_REL, GRAD64_ABS) if (d["kind"] == "f64" or exact_terms) else (GRAD_REL, GRAD_ABS)


class _Worst:
    """|got - ref| <= rel * bound + abs elementwise, keeping the worst |got - ref| / bound of everything compared."""

    def __init__(self):
        self.ratio = 0.0

    def check(self, got, ref, bound, rel, abs_, what):
        got, ref, bound = (np.asarray(x, np.float64) for x in (got, ref, bound))
        err = np.abs(got - ref)
        if np.any(bound > 0):
            self.ratio = max(self.ratio, float((err[bound > 0] / bound[bound > 0]).max()))
        bad = err > rel * bound + abs_
        assert not bad.any(), f"{what}: {int(bad.sum())} off, worst {float(err[bad].max())} (bound {float(bound[bad].max())})"
        assert np.all(got[bound == 0.0] == 0.0), f"{what}: a value the reference admits nowhere is not an exact zero"


def _check_grad_sample(d, out, b, sel, o, density, worst):
    """The rows of molecule b's atoms `sel` against the grad_reference dict o."""
    rows = int(d["off"][b]) + sel
    rel, abs_ = _bars(d, density, "grad")
    worst.check(out["gc"][rows].cpu().numpy(), *o["coords"], rel, abs_, f"molecule {b} dL/dcoords")
    if d["mode"] == "features":
        worst.check(out["gf"][rows].double().cpu().numpy(), *o["features"], rel, abs_, f"molecule {b} dL/dfeatures")
    if out.get("gr") is not None and out["gr"].shape[0] == d["N"]:
        g, bnd = o["radii"]
        worst.check(out["gr"][rows].cpu().numpy(), g if density == "gaussian" else np.zeros_like(g), bnd, rel, abs_, f"molecule {b} dL/dradii")


def _check_zeros(d, out, C_):
    """Nothing stays NaN; atoms outside the box, types past the channels and molecules without atoms give exact zeros (+0.0 for
    an empty molecule's score)."""
    import torch

    for k, v in out.items():
        assert v is None or not bool(torch.isnan(v).any()), f"{k} holds NaN"
    outside = torch.as_tensor(d["outside"], device="cuda")
    assert len(d["outside"]) >= 1
    dead = [outside]
    if d["mode"] == "types" and np.any(d["chan"] >= C_):
        dead.append(torch.as_tensor(np.flatnonzero(d["chan"] >= C_), device="cuda"))
    for rows in dead:
        for k in PER_ATOM + ("gr",):
            v = out.get(k)
            if v is not None and v.shape[0] == d["N"]:
                assert not bool(v[rows].any()), k
    empty = torch.as_tensor(np.flatnonzero(d["sizes"] == 0), device="cuda")
    assert len(empty) >= 2
    for k in ("scores", "pose"):
        if out.get(k) is not None:
            z = out[k][empty]
            assert not bool(z.any()) and not bool(torch.signbit(z).any()), k


# ---- A. the ladder batch ------------------------------------------------------------------------------------------------------------
def _upstream(d, shared=False):
    import torch

    return torch.tensor(M.all_fields(d, shared), device="cuda").to(_gdt(d["kind"])).contiguous()


ABI_ROWS = [r for r in M.GRAD_ROWS if r.entry != "pose"]


@pytest.mark.parametrize("row", ABI_ROWS, ids=[r.id for r in ABI_ROWS])
def test_ladder_backward_and_score_rows(row):
    import torch

    d = M.row_batch(row)
    dev = _device(d)
    G = _upstream(d, row.entry == "score" and not row.per_mol)
    vox = _vox(M.D_LADDER, row.radii, row.density, row.kind)
    out = _abi(vox, d, dev, G, row.entry)
    # 1. the reference on the sample
    ref = M.row_reference(row)
    worst = _Worst()
    assert len(ref["atoms"]) >= 40
    for b, (sel, o) in ref["atoms"].items():
        if row.entry == "score":
            rel, abs_ = _bars(d, row.density, "score")
            worst.check(out["atoms"][int(d["off"][b]) + sel].cpu().numpy(), o[0], o[1], rel, abs_, f"molecule {b} atom scores")
        else:
            _check_grad_sample(d, out, b, sel, o, row.density, worst)
    if row.entry == "score":
        assert sorted(int(d["sizes"][b]) for b in ref["whole"]) == sorted(set(int(n) for n in d["sizes"]) - {0})
        for b, (_, _, S, Sb) in ref["whole"].items():
            worst.check(out["scores"][b].cpu().numpy(), S, Sb, rel, abs_, f"molecule {b} score")
        # (the gradient rows of a score call are mvx_backward_batch's bits for the field laid out per molecule)
        back = _abi(vox, d, dev, G if G.dim() == 5 else G.expand((d["B"],) + tuple(G.shape)).contiguous(), "backward")
        assert _same(out["gc"], back["gc"]) and (out["gf"] is None or _same(out["gf"], back["gf"]))
    print(f"MANY_WORST {row.entry} {row.kind} {row.mode} {row.radii} {row.density}: |got - ref| / bound = {worst.ratio:.3g}")
    # 2. bits on every row: the same batch as six separate calls
    _assert_pieces(d, out, lambda lo, hi: _abi(vox, d, dev, G, row.entry, lo, hi), M.CUTS)
    # 3. exact zeros
    _check_zeros(d, out, row.C)
    if row.density == "binary":
        assert not bool(out["gc"].any())
    else:
        assert float(out["gc"].abs().sum()) > 0
    # 4. both orders
    vox.debug_option("grad_order", 1)
    _assert_same_outputs(out, _abi(vox, d, dev, G, row.entry), "grad_order 1 differs from grad_order 0")
    del G
    torch.cuda.empty_cache()


def _pose_call(vox, d, G, lo=0, hi=None):
    """forward_posed_batch(...).backward on molecules [lo, hi) with every leaf requiring grad: dL/dcoords, dL/dfeatures and
    the pose rows [dL/dc | dL/dq | dL/dt]."""
    import torch

    hi = d["B"] if hi is None else hi
    a0, a1 = int(d["off"][lo]), int(d["off"][hi])
    leaf = lambda x: torch.tensor(x, device="cuda", requires_grad=True)  # noqa: E731
    xyz, chan = leaf(d["xyz"][a0:a1]), leaf(d["chan"][a0:a1])
    cen, q, t = leaf(d["cen"][lo:hi]), leaf(d["q"][lo:hi]), leaf(d["t"][lo:hi])
    grid = vox.forward_posed_batch(xyz, d["off"][lo:hi + 1] - a0, cen, q, t, chan, d["radii"])
    (grid.double() * G[lo:hi]).sum().backward()
    return dict(gc=xyz.grad, gf=chan.grad, pose=torch.cat([cen.grad, q.grad, t.grad], dim=1))


POSE_ROWS = [r for r in M.ROWS if r.entry == "pose"]


@pytest.mark.parametrize("row", POSE_ROWS, ids=[r.id for r in POSE_ROWS])
def test_ladder_pose_gradients(row):
    import torch

    d = M.row_batch(row)
    G = torch.tensor(M.all_fields(d), device="cuda")  # (float64 holding the grid type's values)
    vox = _vox(M.D_LADDER, row.radii, row.density, row.kind, differentiable=True)
    out = _pose_call(vox, d, G)
    assert tuple(out["pose"].shape) == (d["B"], 10) and out["pose"].dtype == torch.float64
    ref = M.row_reference(row)["whole"]
    assert sorted(int(d["sizes"][b]) for b in ref) == sorted(set(int(n) for n in d["sizes"]) - {0})
    rel, abs_ = _bars(d, row.density, "grad")
    worst = _Worst()
    got = out["pose"].cpu().numpy()
    for b, o in ref.items():
        for name, cols in (("center", slice(0, 3)), ("quaternion", slice(3, 7)), ("translation", slice(7, 10))):
            worst.check(got[b, cols], *o[name], rel, abs_, f"molecule {b} dL/d{name}")
    print(f"MANY_WORST pose {row.kind} {row.mode} {row.radii} {row.density}: |got - ref| / bound = {worst.ratio:.3g}")

    def piece(lo, hi):
        if d["off"][lo] == d["off"][hi]:  # (no atoms: the whole call's rows of these molecules are held to exact zeros below)
            return {}
        return _pose_call(vox, d, G, lo, hi)

    _assert_pieces(d, out, piece, M.CUTS)
    _check_zeros(d, out, row.C)
    full = torch.as_tensor(np.flatnonzero(d["sizes"] > 2), device="cuda")
    assert bool(out["pose"][full].abs().sum(1).all())
    vox.debug_option("grad_order", 1)
    _assert_same_outputs(out, _pose_call(vox, d, G), "grad_order 1 differs from grad_order 0")


def _forward(vox, d, row, lo=0, hi=None, xyz=None):
    import torch

    hi = d["B"] if hi is None else hi
    a0, a1 = int(d["off"][lo]), int(d["off"][hi])
    conv = (lambda x: torch.tensor(x, device="cuda")) if row.device_pose else (lambda x: x)
    xyz = d["xyz"] if xyz is None else xyz
    return vox.forward_posed_batch(torch.tensor(xyz[a0:a1], device="cuda"), d["off"][lo:hi + 1] - a0, conv(d["cen"][lo:hi]),
                                   conv(d["q"][lo:hi]), conv(d["t"][lo:hi]), torch.tensor(d["chan"][a0:a1], device="cuda"), d["radii"],
                                   num_channels=d["C"] if d["mode"] == "types" else None)


def _oracle(d, b, D, **kw):
    from oracle import c_oracle

    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    p = pr.batch_positions(d["xyz"][lo:hi], np.array([0, hi - lo]), d["cen"][b:b + 1], d["q"][b:b + 1], d["t"][b:b + 1])
    return c_oracle.voxelize(p, d["chan"][lo:hi], d["radii"], dimension=D, radii_type="scalar", density="gaussian",
                             num_channels=d["C"] if d["mode"] == "types" else None, **kw)


@pytest.mark.parametrize("row", M.FORWARD_ROWS, ids=M.FORWARD_IDS)
def test_ladder_posed_forward_grid(row):
    import torch

    d = M.row_batch(row)
    vox = _vox(M.D_LADDER)
    grid = _forward(vox, d, row)
    assert tuple(grid.shape) == (d["B"], row.C) + (M.D_LADDER,) * 3 and grid.dtype == torch.float32
    mols = M.sample_molecules(d["sizes"])
    assert len(mols) >= 40
    for b in mols:
        ref = _oracle(d, b, M.D_LADDER)
        assert d["sizes"][b] < 5 or np.count_nonzero(ref) > 0
        assert_gaussian(grid[b].cpu().numpy(), ref)
    _assert_pieces(d, dict(grid=grid), lambda lo, hi: dict(grid=_forward(vox, d, row, lo, hi)), M.CUTS)
    empty = torch.as_tensor(np.flatnonzero(d["sizes"] == 0), device="cuda")
    assert not bool(grid[empty].any()) and not bool(torch.isnan(grid).any())


@pytest.mark.parametrize("row", M.SUM_ROWS, ids=M.SUM_IDS)
def test_thin_ladder_call_wide_sums(row):
    """dL/dsigma, dL/d(scalar radius) and channel-wise dL/dradii sum over every atom of the call: the reference reads them all."""
    d = M.row_batch(row)
    dev = _device(d)
    G = _upstream(d)
    vox = _vox(M.D_LADDER, row.radii, row.density, row.kind)
    out = _abi(vox, d, dev, G, row.entry)
    ref = M.sum_reference(row)
    rel, abs_ = _bars(d, row.density, "grad")
    worst = _Worst()
    for k, name in (("gsig", "sigma"), ("grs", "radius"), ("gr", "radii")):
        assert (out[k] is not None) == (name in ref), (k, name)
        if out[k] is not None:
            got = out[k].cpu().numpy()
            worst.check(got if name == "radii" else got[0], *ref[name], rel, abs_, f"dL/d{name}")
    print(f"MANY_WORST sums {row.kind} {row.mode} {row.radii} {row.density}: |got - ref| / bound = {worst.ratio:.3g}")
    _check_zeros(d, out, row.C)
    plain = _abi(vox, d, dev, G, "backward")  # (the per-atom rows are mvx_backward_batch's bits, whatever else the walk forms)
    assert _same(out["gc"], plain["gc"]) and (out["gf"] is None or _same(out["gf"], plain["gf"]))
    _assert_pieces(d, plain, lambda lo, hi: _abi(vox, d, dev, G, "backward", lo, hi), M.CUTS)
    vox.debug_option("grad_order", 1)
    _assert_same_outputs(out, _abi(vox, d, dev, G, row.entry), "grad_order 1 differs from grad_order 0")


@pytest.mark.parametrize("entry", ["backward", "score"])
def test_mixed_records_resolve_next_to_plain_neighbours(entry):
    """Every third record a plain MVX_XF_CENTER | ROTATE one, the others MVX_XF_POSE_PTR: the early return of pose_resolve_kernel
    next to resolved neighbours. The same bits as the call with every pose resolved on the host into plain records."""
    row = M.ROWS[0]
    d = M.row_batch(row)
    dev = _device(d)
    G = _upstream(d)
    vox = _vox(M.D_LADDER)
    mixed = M.records(d, 0, d["B"], "pose", dev["pose"].data_ptr(), 3)
    assert np.count_nonzero(mixed["flags"] == M.XF_POSE_PTR) == d["B"] - d["B"] // 3 and np.count_nonzero(mixed["flags"] == 3) == d["B"] // 3
    got = _abi(vox, d, dev, G, entry, how="pose", plain_every=3)
    ref = _abi(vox, d, dev, G, entry, how="resolved", plain_every=3)
    _assert_same_outputs(got, ref, "device-resolved poses differ from the poses resolved on the host")
    _check_zeros(d, got, row.C)
    assert float(got["gc"].abs().sum()) > 0
    every = _abi(vox, d, dev, G, entry)  # (all poses: the plain records' molecules differ, their translation is gone)
    assert not _same(every["gc"], got["gc"])


# ---- B. tiny totals under the spatial order --------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", M.TINY_TOTALS)
def test_tiny_totals_under_the_spatial_order(total):
    d = M.tiny_batch(total)
    dev = _device(d)
    G = _upstream(d)
    worst = _Worst()
    for entry in ("backward", "score"):
        vox = _vox(M.D_LADDER)
        out = _abi(vox, d, dev, G, entry)
        vox.debug_option("grad_order", 1)
        _assert_same_outputs(out, _abi(vox, d, dev, G, entry), f"{entry}: grad_order 1 differs from grad_order 0")
        rel, abs_ = _bars(d, "gaussian", entry)
        for b in range(d["B"]):
            n = int(d["sizes"][b])
            if n == 0:
                assert entry != "score" or (float(out["scores"][b]) == 0.0 and not np.signbit(float(out["scores"][b])))
                continue
            Gb = M.field_of(d, b)
            _check_grad_sample(d, out, b, np.arange(n), M.grad_rows(d, b, Gb, "gaussian"), "gaussian", worst)
            if entry == "score":
                s, sb, S, Sb = M.score_rows(d, b, Gb, "gaussian")
                lo = int(d["off"][b])
                worst.check(out["atoms"][lo:lo + n].cpu().numpy(), s, sb, rel, abs_, f"molecule {b} atom scores")
                worst.check(out["scores"][b].cpu().numpy(), S, Sb, rel, abs_, f"molecule {b} score")
        for k, v in out.items():
            assert v is None or not bool(v.isnan().any()), k
    print(f"MANY_WORST tiny-{total} f32 features scalar gaussian: |got - ref| / bound = {worst.ratio:.3g}")


# ---- C. past the block-count edges: B = 70 001 -------------------------------------------------------------------------------------
def _window_cuts(d, out, piece):
    for lo, hi in M.HUGE_WINDOWS:
        a0, a1 = int(d["off"][lo]), int(d["off"][hi])
        window = {k: (None if v is None else (v[lo:hi] if k in ("scores", "pose") else v[a0:a1])) for k, v in out.items()}
        _assert_pieces(d, window, piece, (lo, hi))


def test_70001_molecules_backward():
    """Types mode, C = 4, float32, one rotation per molecule: 70 001 records go through find_molecule."""
    import torch

    d = M.huge_batch("rotation")
    dev = _device(d)
    G = torch.empty((M.HUGE_B, M.HUGE_C) + (M.HUGE_D,) * 3, dtype=torch.float32, device="cuda").normal_(generator=_generator(d))
    assert G.numel() * 4 == M.huge_bytes()["upstream"] < R.MAX_OUTPUT_BYTES
    vox = _vox(M.HUGE_D)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _abi(vox, d, dev, G, "backward")
    print(f"\n[many molecules C] backward, B = {M.HUGE_B}: wall time of the first call {1e3 * (time.perf_counter() - t0):.1f} ms")
    worst = _Worst()
    for b in M.huge_molecules(d["sizes"]):
        n = int(d["sizes"][b])
        if n:
            _check_grad_sample(d, out, b, np.arange(n), M.grad_rows(d, b, G[b].double().cpu().numpy(), "gaussian"), "gaussian", worst)
    print(f"MANY_WORST backward-70001 f32 types scalar gaussian: |got - ref| / bound = {worst.ratio:.3g}")
    _window_cuts(d, out, lambda lo, hi: _abi(vox, d, dev, G, "backward", lo, hi))
    _check_zeros(d, out, M.HUGE_C)
    assert float(out["gc"].abs().sum()) > 0
    del G
    torch.cuda.empty_cache()


def _pose_grad(vox, d, dev, gc, lo=0, hi=None):
    """mvx_pose_grad_batch on the rows gc of molecules [lo, hi); the (hi - lo, 10) output starts as NaN."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    hi = d["B"] if hi is None else hi
    a0, a1 = int(d["off"][lo]), int(d["off"][hi])
    gp = torch.full((hi - lo, 10), float("nan"), dtype=torch.float64, device="cuda")
    off = np.ascontiguousarray(d["off"][lo:hi + 1] - a0)
    xf = M.records(d, lo, hi, "pose", dev["pose"].data_ptr())
    g = gc.contiguous()
    _lib.check(vox._lib.mvx_pose_grad_batch(vox._handle, dev["c"][a0:a1].data_ptr(), g.data_ptr(), off.ctypes.data, xf.ctypes.data,
                                            hi - lo, gp.data_ptr(), vox._stream()))
    torch.cuda.synchronize()
    return gp


def test_70001_molecules_score_and_pose_gradients():
    """One shared field under explicit poses: 70 001 pose records are resolved in 1 094 workgroups; mvx_pose_grad_batch reduces
    that call's dL/dcoords in 70 001 workgroups."""
    import torch

    d = M.huge_batch("pose")
    dev = _device(d)
    F64 = M.field_of(d, 0, True)
    F = torch.tensor(F64, device="cuda").to(torch.float32)
    vox = _vox(M.HUGE_D)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = _abi(vox, d, dev, F, "score")
    t1 = time.perf_counter()
    out["pose"] = _pose_grad(vox, d, dev, out["gc"])
    print(f"\n[many molecules C] score, B = {M.HUGE_B}: wall time of the first call {1e3 * (t1 - t0):.1f} ms, "
          f"mvx_pose_grad_batch {1e3 * (time.perf_counter() - t1):.1f} ms")
    worst = _Worst()
    rel, abs_ = _bars(d, "gaussian", "score")
    got_pose = out["pose"].cpu().numpy()
    for b in M.huge_molecules(d["sizes"]):
        n, lo = int(d["sizes"][b]), int(d["off"][b])
        if n == 0:
            continue
        s, sb, S, Sb = M.score_rows(d, b, F64, "gaussian")
        worst.check(out["atoms"][lo:lo + n].cpu().numpy(), s, sb, rel, abs_, f"molecule {b} atom scores")
        worst.check(out["scores"][b].cpu().numpy(), S, Sb, rel, abs_, f"molecule {b} score")
        _check_grad_sample(d, out, b, np.arange(n), M.grad_rows(d, b, F64, "gaussian"), "gaussian", worst)
        o = M.pose_rows(d, b, F64)
        for name, cols in (("center", slice(0, 3)), ("quaternion", slice(3, 7)), ("translation", slice(7, 10))):
            worst.check(got_pose[b, cols], *o[name], rel, abs_, f"molecule {b} dL/d{name}")
    print(f"MANY_WORST score-70001 f32 types scalar gaussian: |got - ref| / bound = {worst.ratio:.3g}")

    def piece(lo, hi):
        got = _abi(vox, d, dev, F, "score", lo, hi)
        got["pose"] = _pose_grad(vox, d, dev, got["gc"], lo, hi)
        return got

    _window_cuts(d, out, piece)
    _check_zeros(d, out, M.HUGE_C)
    assert float(out["scores"].abs().sum()) > 0


# ---- D. dL/dgrid and per-molecule fields past 2^31 and 2^32 elements ---------------------------------------------------------------
@pytest.mark.parametrize("case", M.WIDE, ids=M.WIDE_IDS)
def test_upstream_and_field_beyond_2_pow_31_and_2_pow_32_elements(case):
    """One 8.6 GB buffer, filled on the device, as dL/dgrid of mvx_backward_batch and as the per-molecule field of
    mvx_score_batch: molecule m's slice starts m * C * D^3 elements in (2^31 at molecule 256, 2^32 at 512; float32: byte offsets
    2^32 at 128 and 2^33 at 256). The checked molecules are bit for bit their own one-molecule calls on their own slice and match
    the float64 reference on the downloaded slice. Skips only when the allocation fails."""
    import torch

    d = M.wide_batch(case)
    per = case.C * case.D**3
    assert case.B * per > max(case.picks) * per >= 1 << 31
    try:
        buf = torch.empty((case.B, case.C) + (case.D,) * 3, dtype=_gdt(case.kind), device="cuda").normal_(generator=_generator(d))
    except torch.cuda.OutOfMemoryError as e:
        pytest.skip(f"not enough device memory for a buffer of {case.B * per} elements: {e}")
    dev = _device(d)
    vox = _vox(case.D, kind=case.kind)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    back = _abi(vox, d, dev, buf, "backward")
    t1 = time.perf_counter()
    score = _abi(vox, d, dev, buf, "score")
    t2 = time.perf_counter()
    print(f"\n[many molecules D] {case.id}: buffer {buf.numel() * buf.element_size() / 1e9:.2f} GB, wall time of the backward call "
          f"{1e3 * (t1 - t0):.1f} ms, of the score call {1e3 * (t2 - t1):.1f} ms")
    assert _same(back["gc"], score["gc"]) and _same(back["gf"], score["gf"])
    worst = _Worst()
    rel, abs_ = _bars(d, "gaussian", "score")
    for m in case.picks:
        lo, hi = int(d["off"][m]), int(d["off"][m + 1])
        for entry, whole in (("backward", back), ("score", score)):
            _assert_pieces(d, {k: (None if v is None else (v[m:m + 1] if k == "scores" else v[lo:hi])) for k, v in whole.items()},
                           lambda a, b: _abi(vox, d, dev, buf, entry, a, b), (m, m + 1))
        G64 = buf[m].to(torch.float64).cpu().numpy()
        o = M.grad_rows(d, m, G64, "gaussian")
        assert np.count_nonzero(np.abs(o["coords"][0]).sum(1)) == case.atoms - 1, m  # (all but the atom outside)
        _check_grad_sample(d, back, m, np.arange(hi - lo), o, "gaussian", worst)
        s, sb, S, Sb = M.score_rows(d, m, G64, "gaussian")
        worst.check(score["atoms"][lo:hi].cpu().numpy(), s, sb, rel, abs_, f"molecule {m} atom scores")
        worst.check(score["scores"][m].cpu().numpy(), S, Sb, rel, abs_, f"molecule {m} score")
        del G64
    print(f"MANY_WORST wide-{case.id} {case.kind} features scalar gaussian: |got - ref| / bound = {worst.ratio:.3g}")
    for out in (back, score):
        for k, v in out.items():
            assert v is None or not bool(torch.isnan(v).any()), k
    del buf
    torch.cuda.empty_cache()


# ---- E. posed forward calls cut into several launches -------------------------------------------------------------------------------
def _cut_vox(D):
    import molvoxel_amd as mv

    v = mv.create_voxelizer(R.RES, D, "scalar", "gaussian", "hip", sigma=R.SIGMA, output="torch")
    v.debug_option("direct", 0)
    return v


@pytest.mark.parametrize("device_pose", [True, False], ids=["device-block", "numpy-poses"])
@pytest.mark.parametrize("row", M.CUT_ROWS, ids=M.CUT_IDS)
def test_posed_forward_calls_cut_into_several_launches(row, device_pose):
    d = M.cut_batch(row.id)
    how = M.Row("cut", "forward", row.mode, row.C, "scalar", device_pose=device_pose)
    p = R.host_plan(row, R.RAGGED_SIZES)
    v = _cut_vox(row.D)
    uncut = _forward(v, d, how)
    assert v.last_plan() == p and p["nchunk"] == 1, (v.last_plan(), p)
    for b in M.CUT_ORACLE_MOLECULES:
        ref = _oracle(d, b, row.D, resolution=R.RES, sigma=R.SIGMA)
        assert np.count_nonzero(ref) > 0
        assert_gaussian(uncut[b].cpu().numpy(), ref)
    cuts = [(kb, 0, n) for n, kb in M.cut_budgets(row).items()] + [(0, c, c) for c in row.chunks]
    assert [n for _, _, n in cuts] == [2, 3, 16, 3]
    for budget_kb, chunks, nchunk in cuts:
        v = _cut_vox(row.D)
        _forward(v, d, how, xyz=d["mirror"])  # (the workspace now holds the mirrored batch's lines, uncut)
        if budget_kb:
            v.debug_option("mall_budget_kb", budget_kb)
        if chunks:
            v.debug_option("chunks", chunks)
        got = _forward(v, d, how)
        took = v.last_plan()
        assert took["nchunk"] == nchunk and {k: took[k] for k in row.plan} == row.plan, (budget_kb, chunks, took)
        assert _same(got, uncut), f"cut into {nchunk} (budget {budget_kb} KB, chunks {chunks}) differs from one launch"


def test_posed_views_cut_into_several_launches():
    import torch

    c = M.views_cloud()
    dev = {k: torch.tensor(c[k], device="cuda") for k in ("xyz", "cen", "q", "t", "chan")}
    mirror = torch.tensor(2.0 * M.CEN - c["xyz"], device="cuda")

    def call(v, xyz):
        return v.forward_posed_views(xyz, dev["cen"], dev["q"], dev["t"], dev["chan"], R.SCALAR_RADIUS)

    v = _cut_vox(c["D"])
    uncut = call(v, dev["xyz"])
    p = v.last_plan()  # (the plan of the compact batch of the selected atoms)
    assert p["nchunk"] == 1 and p["route"] == R.BINNED and float(uncut.abs().sum()) > 0
    _, offsets = v.select_posed_views(dev["xyz"], dev["cen"], dev["q"], dev["t"], dev["chan"], R.SCALAR_RADIUS)
    counts = np.diff(np.asarray(offsets))
    total = int(counts.sum())
    assert 0 < total < c["B"] * c["N"] and counts.min() > 0
    for nchunk in M.VIEWS_NCHUNKS:
        kb = R.budget_for(p, c["B"], c["C"], total, nchunk)
        assert R.expected_nchunk(p, c["B"], c["C"], total, 32, kb) == nchunk
        v = _cut_vox(c["D"])
        call(v, mirror)
        v.debug_option("mall_budget_kb", kb)
        got = call(v, dev["xyz"])
        assert v.last_plan()["nchunk"] == nchunk, v.last_plan()
        assert _same(got, uncut), f"views cut into {nchunk} differ from one launch"
