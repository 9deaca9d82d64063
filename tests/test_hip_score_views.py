"""Scores of many views of one shared cloud on the GPU (score_views / score_posed_views, mvx_score_views) and the reduction of
their per-(view, atom) rows onto the shared atoms (views_reduce, mvx_views_reduce).

The reduction's bookkeeping is pinned with small-integer rows (every order of addition is exact) against the numpy restatement
(tests/views_reduce_reference.py); its rounding with random rows under the float64 bar of tests/tolerance.py. The scores are
held bit for bit to score_batch / score_posed_batch on the gathered rows, to the repeated cloud where the contract says so, and
to the float64 reference (tests/score_reference.py). Shapes: a cloud of 150 atoms in a blob of 20 A around (30, -20, 12),
D = 16 at 0.5 A (a view keeps a few dozen atoms), five views of which one keeps nothing; atom 0 lies outside every view."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import pose_reference as pr
from tests import score_reference as sr
from tests import views_reduce_reference as vr
from tests import views_reference as vw
from tests import hip_support as hip
from tests.abi import MVX_ERR_INVALID
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

CEN = np.array([30.0, -20.0, 12.0])
NORMS = np.array([1.0, 0.8, 1.25])
D, RES = 16, 0.5


def _vox(radii_type="scalar", density="gaussian", kind="f32", **kw):
    import molvoxel_amd as mv

    if kind == "bf16":
        kw["grid_dtype"] = "bfloat16"
    return mv.create_voxelizer(RES, D, radii_type, density, library="hip", precision=64 if kind == "f64" else 32, **kw)


# ---- 1. the reduction: slot lookup and coverage, exactly --------------------------------------------------------------------
def _selection(seed, B, N, keep=0.5, full=True):
    """A selection with the edges of the kernel in it: the last but one view keeps nothing; with `full` the first view keeps the
    whole cloud (no search) and atom N - 1 is in no other view, without it atom N - 1 is in no view at all."""
    rng = np.random.default_rng(seed)
    index, offsets = vr.random_selection(rng, B, N, keep, full=(0,) if full else (), empty=(B - 2,) if B > 3 else (),
                                         never=(N - 1,) if N > 2 else ())
    return rng, index, offsets


def _device_index(index, shift=False):
    """The index on the device; shift: its base 8 bytes past the (at least 16-byte aligned) allocation."""
    import torch

    if not shift:
        return torch.tensor(index, device="cuda")
    buf = torch.empty(len(index) + 1, dtype=torch.int64, device="cuda")
    buf[1:] = torch.tensor(index, device="cuda")
    out = buf[1:]
    assert out.data_ptr() % 16 == 8 or len(index) == 0
    return out


BOOK_CASES = [
    # B, N, width, keep probability, index 8 bytes off, the first view keeps the whole cloud
    (1, 1, 1, 1.0, False, True),
    (1, 65, 3, 0.5, False, False),
    (63, 64, 3, 0.5, True, True),
    (64, 65, 32, 0.3, False, False),
    (65, 64, 33, 0.7, True, True),
    (129, 150, 3, 0.2, False, False),
    (129, 1100, 1, 0.05, True, True),
    (5, 1100, 32, 0.4, False, True),
    (321, 7, 33, 0.6, False, False),  # (a lane of the first wave sees a second view: 256 views per round)
    (64, 1, 32, 0.5, False, False),
]


@pytest.mark.parametrize("B, N, W, keep, shift, full", BOOK_CASES)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_integer_rows_reduce_exactly(B, N, W, keep, shift, full, dtype):
    import torch

    rng, index, offsets = _selection(B * 1000 + N, B, N, keep, full)
    total = len(index)
    rows = rng.integers(-8, 9, (total, W)).astype(dtype)
    ref, _ = vr.reduce_reference(index, offsets, N, rows)
    vox = _vox()
    idx = _device_index(index, shift)
    got = vox.views_reduce(torch.tensor(rows, device="cuda"), idx, offsets, N)
    assert got.dtype == getattr(torch, dtype) and tuple(got.shape) == (N, W)
    assert torch.equal(got.cpu().to(torch.float64), torch.tensor(ref))
    held = np.zeros(N, bool)
    held[index] = True
    if full and B > 1 and N > 2:
        assert np.diff(offsets)[0] == N and np.any(np.diff(offsets)[1:] < N)  # the fast path and the search
    if not full and N > 2:
        assert not held[N - 1]
    assert not got[torch.tensor(~held, device="cuda")].any()  # an atom no view holds: an exact-zero row
    flat = vox.views_reduce(torch.tensor(rows[:, 0].copy(), device="cuda"), idx, offsets, N)  # (total,) rows: (N,) sums
    assert tuple(flat.shape) == (N,) and torch.equal(flat, got[:, 0])


def test_a_cloud_no_view_looks_at_and_a_call_without_views_give_zero_rows():
    import torch

    vox = _vox()
    for B in (0, 3):
        out = torch.full((4, 3), 7.0, dtype=torch.float64, device="cuda")
        off = np.zeros(B + 1, np.int64)
        rc = vox._lib.mvx_views_reduce(vox._handle, None, off.ctypes.data, B, 4, None, 3, 1, out.data_ptr(), vox._stream())
        assert rc == 0 and not out.any() and not torch.signbit(out).any()
    got = vox.views_reduce(torch.zeros((0, 5), device="cuda"), torch.zeros(0, dtype=torch.int64, device="cuda"), np.zeros(3, np.int64), 6)
    assert tuple(got.shape) == (6, 5) and got.dtype == torch.float32 and not got.any()


@pytest.mark.parametrize("B, N, W", [(129, 150, 3), (65, 150, 33), (321, 40, 32)])
def test_random_rows_reduce_within_the_float64_bar_and_reproducibly(B, N, W):
    """float64 sums taken in another order than the reference's: GRAD64_REL * sum |terms| + GRAD64_ABS; float rows are
    accumulated in double as well and rounded once: 2^-24 |ref| more."""
    import torch

    rng, index, offsets = _selection(7 * B + N, B, N, 0.5)
    rows = rng.standard_normal((len(index), W)) * np.exp(rng.uniform(-6, 6, (len(index), 1)))
    vox = _vox()
    idx = _device_index(index)
    for dtype, extra in ((np.float64, 0.0), (np.float32, 2.0 ** -24)):
        r = rows.astype(dtype)
        ref, bound = vr.reduce_reference(index, offsets, N, r)
        rd = torch.tensor(r, device="cuda")
        got = vox.views_reduce(rd, idx, offsets, N)
        again = vox.views_reduce(rd.clone(), idx.clone(), offsets, N)
        assert torch.equal(got, again)  # (the same bytes)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        tol = GRAD64_REL * bound + GRAD64_ABS + extra * np.abs(ref)
        print(f"REDUCE_WORST {np.dtype(dtype).name} B {B} N {N} W {W}: max (|got - ref| - 2^-24 |ref|) / bound = "
              f"{float(((err - extra * np.abs(ref)) / np.maximum(bound, 1e-300)).max()):.3g}")
        assert np.all(err <= tol), float((err - tol).max())


# ---- 2. scores ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _data(seed, N, B, C_, mode, radii_type, kind="f32", tight=False, hole=True):
    """One cloud and B views of it (host arrays; never modified). tight: the blob is small enough for every view to keep it
    whole; hole: view 1 looks at empty space."""
    rng = np.random.default_rng(seed)
    fp = np.float64 if kind == "f64" else np.float32
    half = 0.7 if tight else 10.0
    xyz = CEN + rng.uniform(-half, half, (N, 3))
    outside = np.zeros(0, np.int64)
    if N >= 2 and not tight:
        xyz[0] += [100.0, -80.0, 90.0]  # (outside every view under every pose)
        outside = np.array([0], np.int64)
    if tight:
        cen = CEN + rng.normal(0.0, 0.1, (B, 3))
    else:
        cen = xyz[rng.integers(1 if N > 1 else 0, N, B)] + rng.normal(0.0, 0.5, (B, 3))
        if hole and B >= 3:
            cen[1] = CEN + 60.0
    q = rng.standard_normal((B, 4))
    q *= (NORMS[np.arange(B) % 3] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.3, 0.3, (B, 3))
    types = rng.integers(0, C_, N)
    chan = {"features": rng.standard_normal((N, C_)).astype(fp), "types": types, "single": None}[mode]
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(fp), "channel-wise": rng.uniform(1.0, 1.5, C_).astype(fp)}[radii_type]
    return dict(cen=cen, xyz=xyz, q=q, t=t, chan=chan, radii=radii, B=B, N=N, outside=outside, mode=mode, C=C_, radii_type=radii_type,
                kind=kind)


def _field(d, per_view, seed=9):
    """(device field in the grid type of `kind`, the float64 array the kernel reads)."""
    import torch

    rng = np.random.default_rng(seed)
    F = rng.standard_normal(((d["B"],) if per_view else ()) + (d["C"],) + (D,) * 3)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[d["kind"]]
    Fd = torch.tensor(F, device="cuda").to(dt)
    return Fd, Fd.to(torch.float64).cpu().numpy()


def _views(vox, d, F, transform, per_atom=True, **over):
    """score_posed_views, or score_views under the random rotations of np.random.seed(transform)."""
    a = {k: over.get(k, hip.dev(d[k])) for k in ("xyz", "cen", "q", "t", "chan", "radii")}
    if transform == "posed":
        return vox.score_posed_views(a["xyz"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], F, num_channels=hip.nc(d), per_atom=per_atom)
    np.random.seed(transform)
    return vox.score_views(a["xyz"], a["cen"], a["chan"], a["radii"], F, num_channels=hip.nc(d), random_rotation=True, per_atom=per_atom)


def _take(x, index):
    return x if (x is None or np.isscalar(x)) else x[index]


def _batch(vox, d, F, transform, index, offsets, per_atom=True, **over):
    """The same records on the gathered rows: score_posed_batch / score_batch on coords[index], channels[index] and offsets."""
    a = {k: over.get(k, hip.dev(d[k])) for k in ("xyz", "cen", "q", "t", "chan", "radii")}
    r = _take(a["radii"], index) if d["radii_type"] == "atom-wise" else a["radii"]
    xyz = over["rows"] if "rows" in over else a["xyz"][index]
    chan = over["chan_rows"] if "chan_rows" in over else _take(a["chan"], index)
    if transform == "posed":
        return vox.score_posed_batch(xyz, offsets, a["cen"], a["q"], a["t"], chan, r, F, num_channels=hip.nc(d), per_atom=per_atom)
    np.random.seed(transform)
    return vox.score_batch(xyz, offsets, a["cen"], chan, r, F, num_channels=hip.nc(d), random_rotation=True, per_atom=per_atom)


def _quats(B, seed):
    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform

    np.random.seed(seed)
    return np.array([draw_forward_transform(0.0, True)[1] for _ in range(B)]).reshape(B, 4)


def _positions(d, transform):
    """(B, N, 3): the cloud as each view sees it."""
    if transform == "posed":
        return pr.view_positions(d["xyz"], d["cen"], d["q"], d["t"])
    return vw.view_positions(d["xyz"], d["cen"], seed=transform, random_rotation=True)


def _cull_source(d):
    if d["radii_type"] == "scalar":
        return "scalar"
    if d["radii_type"] == "atom-wise":
        return "atom-wise"
    return "by-type" if d["mode"] == "types" else "channel-features"


def _abi_records(vox, d, transform):
    """(records, what they point at) of the call: explicit device poses, or centres by value with the seed's rotations."""
    from molvoxel_amd.voxelizer.hip import _lib

    B = d["B"]
    if transform == "posed":
        pose = vox._pack_pose(B, hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), True)
        return vox._pose_xforms(pose, B), pose
    xfs = (_lib.MvxXform * B)()
    for b, qb in enumerate(_quats(B, transform)):
        xfs[b].center[:] = d["cen"][b].tolist()
        xfs[b].quat[:] = [float(v) for v in qb]
        xfs[b].flags = _lib.MVX_XF_CENTER | _lib.MVX_XF_ROTATE
    return xfs, None


def _abi(vox, d, F, per_view, xfs, index=None, offsets=None, gathered=False, rows=True):
    """mvx_score_views on the cloud (index / offsets: a selection, or None) or, gathered, mvx_score_batch on coords[index] ...:
    (rc, scores, atom_scores, grad_coords, grad_features)."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    kind = None if d["mode"] == "single" else d["mode"]
    xyz, chan, radii = hip.dev(d["xyz"]), hip.dev(d["chan"]), hip.dev(d["radii"])
    if gathered:
        xyz, chan = xyz[index], _take(chan, index)
        radii = _take(radii, index) if d["radii_type"] == "atom-wise" else radii
    c, ch, r, _, _ = vox._views_inputs(xyz, chan, kind, radii, d["C"])
    B, C_ = d["B"], d["C"]
    total = 0 if index is None else int(offsets[-1])
    rows = rows and index is not None
    scores = torch.full((B,), np.nan, dtype=torch.float64, device="cuda")
    atoms = torch.full((total,), np.nan, dtype=torch.float64, device="cuda") if rows else None
    gc = torch.full((total, 3), np.nan, dtype=torch.float64, device="cuda") if rows else None
    gf = torch.full((total, C_), np.nan, dtype=vox._tfp, device="cuda") if (rows and d["mode"] == "features") else None
    rs = float(d["radii"]) if np.isscalar(d["radii"]) else 0.0
    stride = per_view if isinstance(per_view, int) and not isinstance(per_view, bool) else (C_ * D ** 3 if per_view else 0)
    p = vox._ptr
    if gathered:
        rc = vox._lib.mvx_score_batch(vox._handle, _lib.MODES[d["mode"]], p(c), p(ch), p(r), rs, vox._radii_type_code(),
                                      offsets.ctypes.data, C.addressof(xfs), B, C_, p(F), stride, p(scores), p(atoms), p(gc), p(gf),
                                      vox._stream())
    else:
        rc = vox._lib.mvx_score_views(vox._handle, _lib.MODES[d["mode"]], p(c), p(ch), p(r), rs, vox._radii_type_code(), d["N"], C_,
                                      C.addressof(xfs), B, None if index is None else index.data_ptr(),
                                      None if index is None else offsets.ctypes.data, p(F), stride, p(scores), p(atoms), p(gc),
                                      p(gf), vox._stream())
    torch.cuda.synchronize()
    return rc, scores, atoms, gc, gf


SCORE_CASES = [
    # mode, C, radii type, density, grid, one field per view, transform ("posed" or the seed of the random rotations)
    ("features", 32, "scalar", "gaussian", "f32", False, "posed"),
    ("features", 33, "channel-wise", "gaussian", "f32", True, 11),
    ("features", 5, "atom-wise", "binary", "bf16", False, "posed"),
    ("features", 5, "scalar", "gaussian", "f64", True, "posed"),
    ("features", 1, "scalar", "gaussian", "f32", False, 12),
    ("types", 5, "channel-wise", "gaussian", "f32", False, 13),
    ("types", 33, "atom-wise", "binary", "f64", True, "posed"),
    ("single", 1, "atom-wise", "gaussian", "f32", False, "posed"),
    ("single", 1, "scalar", "binary", "bf16", True, 14),
]


@pytest.mark.parametrize("mode, C_, radii_type, density, kind, per_view, transform", SCORE_CASES)
def test_scores_are_the_batch_entrys_bits_and_match_the_reference(mode, C_, radii_type, density, kind, per_view, transform):
    import torch

    d = _data(31, 150, 5, C_, mode, radii_type, kind)
    B, N = d["B"], d["N"]
    Fd, Fref = _field(d, per_view)
    vox = _vox(radii_type, density, kind)
    scores, atoms, index, offsets = _views(vox, d, Fd, transform)
    assert scores.dtype == torch.float64 and atoms.dtype == torch.float64 and scores.is_cuda and atoms.is_cuda
    assert tuple(scores.shape) == (B,) and tuple(atoms.shape) == (int(offsets[-1]),) == tuple(index.shape)
    counts = np.diff(offsets)
    assert counts[1] == 0 and counts.max() < N and np.count_nonzero(counts) == B - 1 and counts.sum() > 40

    # the selection is the forward's (no (view, atom) pair near a cull bound, so the restatement decides as the kernel does)
    p = _positions(d, transform)
    types = d["chan"] if mode == "types" else None
    cull = (p, RES, D, _cull_source(d), d["radii"], 64 if kind == "f64" else 32, types, C_ if mode == "types" else None)
    assert float(vw.margin(*cull).min()) > 1e-9
    assert vw.selection_mismatch(index.cpu().numpy(), offsets, *vw.select_exact(*cull)) is None

    # 1. bit for bit the batched entry on the gathered rows, from Python and through the C ABI; index = NULL against the index form
    s_b, a_b = _batch(vox, d, Fd, transform, index, offsets)
    assert torch.equal(scores, s_b) and torch.equal(atoms, a_b)
    assert torch.equal(_views(vox, d, Fd, transform, per_atom=False), scores)
    xfs, _keep = _abi_records(vox, d, transform)
    rc, s1, a1, gc1, gf1 = _abi(vox, d, Fd, per_view, xfs, index, offsets)
    rc2, s2, a2, gc2, gf2 = _abi(vox, d, Fd, per_view, xfs, index, offsets, gathered=True)
    rc3, s3, _, _, _ = _abi(vox, d, Fd, per_view, xfs)
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert torch.equal(s1, scores) and torch.equal(a1, atoms) and torch.equal(s2, scores) and torch.equal(a2, atoms)
    assert torch.equal(s3, scores)
    assert torch.equal(gc1, gc2) and not torch.isnan(gc1).any()
    if mode == "features":
        assert torch.equal(gf1, gf2) and not torch.isnan(gf1).any() and bool(gf1.any())
    if density == "gaussian":
        assert bool(gc1.any())
    assert scores[1] == 0.0 and not torch.signbit(scores[1])  # a view that keeps no atom scores exactly 0

    # 2. the float64 reference on every (view, atom) pair: atoms a view does not keep reach none of its voxels
    w = d["chan"].astype(np.float64) if mode == "features" else None
    rep = lambda x: x if (x is None or np.isscalar(x) or len(x) != N) else np.tile(x, (B,) + (1,) * (x.ndim - 1))  # noqa: E731
    s_ref, b_ref, S_ref, Sb_ref = sr.batch_reference(p.reshape(B * N, 3), np.arange(B + 1) * N, Fref, rep(d["radii"]), radii_type,
                                                     w=rep(w), mode=mode, types=rep(types), density=density,
                                                     precision=64 if kind == "f64" else 32)
    slot = np.repeat(np.arange(B), counts) * N + index.cpu().numpy()
    kept = np.zeros(B * N, bool)
    kept[slot] = True
    assert not s_ref[~kept].any() and not b_ref[~kept].any()
    assert np.count_nonzero(s_ref) > 30
    exact_terms = density == "binary" and mode != "features"
    rel, abs_ = (GRAD64_REL, GRAD64_ABS) if (kind == "f64" or exact_terms) else (GRAD_REL, GRAD_ABS)
    S, s = scores.cpu().numpy(), atoms.cpu().numpy()
    err, ERR = np.abs(s - s_ref[slot]), np.abs(S - S_ref)
    b_sel = b_ref[slot]
    worst = max(float((err[b_sel > 0] / b_sel[b_sel > 0]).max()), float((ERR[Sb_ref > 0] / Sb_ref[Sb_ref > 0]).max()))
    print(f"VIEWS_SCORE_WORST grid {kind} {mode} {radii_type} {density}: |got - ref| / bound = {worst:.3g}")
    assert np.all(err <= rel * b_sel + abs_), float(err.max())
    assert np.all(ERR <= rel * Sb_ref + abs_), (ERR, Sb_ref)
    assert np.all(s[b_sel == 0.0] == 0.0)


@pytest.mark.parametrize("mode, C_, radii_type, kind, tight", [
    ("features", 32, "scalar", "f32", False), ("features", 5, "atom-wise", "f64", True), ("types", 5, "channel-wise", "f32", True),
    ("single", 1, "scalar", "bf16", False)])
def test_against_the_repeated_cloud(mode, C_, radii_type, kind, tight):
    """Per-atom scores and rows of kept atoms: the repeated cloud's bits. Scores: the same bits where every view keeps the
    whole cloud; elsewhere score_reduce_kernel groups a molecule's atoms by position, so dropping the zero rows regroups a
    float64 sum: GRAD64_REL * sum |s_n| + GRAD64_ABS."""
    import torch

    d = _data(32, 150, 5, C_, mode, radii_type, kind, tight=tight)
    B, N = d["B"], d["N"]
    Fd, _ = _field(d, True)
    vox = _vox(radii_type, "gaussian", kind)
    scores, atoms, index, offsets = _views(vox, d, Fd, "posed")
    counts = np.diff(offsets)
    assert np.all(counts == N) if tight else (counts.max() < N and counts[1] == 0)
    xfs, _keep = _abi_records(vox, d, "posed")
    _, _, _, gc, gf = _abi(vox, d, Fd, True, xfs, index, offsets)
    whole = torch.arange(N, device="cuda").repeat(B)
    rc, S_rep, a_rep, gc_rep, gf_rep = _abi(vox, d, Fd, True, xfs, whole, np.arange(B + 1, dtype=np.int64) * N, gathered=True)
    assert rc == 0
    slot = torch.tensor(np.repeat(np.arange(B), counts) * N, device="cuda") + index
    assert torch.equal(atoms, a_rep[slot]) and torch.equal(gc, gc_rep[slot])
    if mode == "features":
        assert torch.equal(gf, gf_rep[slot])
    dropped = torch.ones(B * N, dtype=torch.bool, device="cuda")
    dropped[slot] = False
    assert not a_rep[dropped].any() and not gc_rep[dropped].any()  # what the selection drops are exact zeros there
    if tight:
        assert torch.equal(scores, S_rep)
    else:
        bound = torch.segment_reduce(a_rep.abs(), "sum", lengths=torch.full((B,), N, device="cuda"))
        assert bool(((scores - S_rep).abs() <= GRAD64_REL * bound + GRAD64_ABS).all())


def test_views_that_keep_nothing_and_a_cloud_without_atoms():
    import torch

    d = _data(33, 150, 4, 5, "features", "scalar")
    Fd, _ = _field(d, False)
    vox = _vox(differentiable=True)
    far = hip.dev(d["cen"] + 500.0)
    xyz, chan = hip.dev(d["xyz"], True), hip.dev(d["chan"], True)
    scores, atoms, index, offsets = vox.score_posed_views(xyz, far, hip.dev(d["q"]), hip.dev(d["t"]), chan, 1.25, Fd, per_atom=True)
    assert not offsets.any() and index.numel() == 0 and atoms.numel() == 0
    assert not scores.any() and not torch.signbit(scores).any()
    (scores * torch.arange(1.0, 5.0, device="cuda")).sum().backward()
    assert tuple(xyz.grad.shape) == (150, 3) and not xyz.grad.any() and tuple(chan.grad.shape) == (150, 5) and not chan.grad.any()
    only = vox.score_posed_views(xyz.detach(), far, hip.dev(d["q"]), hip.dev(d["t"]), chan.detach(), 1.25, Fd)
    assert tuple(only.shape) == (4,) and not only.any()
    none = vox.score_posed_views(xyz.detach()[:0], far, hip.dev(d["q"]), hip.dev(d["t"]), chan.detach()[:0], 1.25, Fd)
    assert tuple(none.shape) == (4,) and not none.any() and not torch.signbit(none).any()


def test_a_bad_stride_is_rejected_with_a_real_handle():
    d = _data(31, 150, 5, 5, "features", "scalar")
    Fd, _ = _field(d, False)
    vox = _vox()
    xfs, _keep = _abi_records(vox, d, "posed")
    rc, _, _, _, _ = _abi(vox, d, Fd, 7, xfs)
    assert rc == MVX_ERR_INVALID and "field_view_stride" in vox._lib.mvx_last_error().decode()


# ---- 3. gradients --------------------------------------------------------------------------------------------------------------
def _leaves(d, posed, features):
    import torch

    out = dict(xyz=hip.dev(d["xyz"], True), cen=hip.dev(d["cen"], True))
    if features:
        out["chan"] = hip.dev(d["chan"], True)
    if posed:
        out.update(q=hip.dev(d["q"], True), t=hip.dev(d["t"], True))
    torch.cuda.synchronize()
    return out


GRAD_CASES = [
    # mode, C, radii type, density, grid, one field per view, transform, per-atom upstream
    ("features", 32, "scalar", "gaussian", "f32", False, "posed", False),
    ("features", 33, "channel-wise", "gaussian", "f64", True, 21, True),
    ("features", 5, "atom-wise", "binary", "bf16", True, "posed", True),
    ("types", 5, "atom-wise", "gaussian", "f32", False, "posed", True),
    ("single", 1, "scalar", "gaussian", "f64", True, 22, False),
]


@pytest.mark.parametrize("mode, C_, radii_type, density, kind, per_view, transform, per_atom", GRAD_CASES)
def test_shared_gradients_are_the_reduction_of_the_compact_batchs(mode, C_, radii_type, density, kind, per_view, transform, per_atom):
    """(scores * w).sum() (+ (atom_scores * wa).sum()): coords.grad and features.grad are the compact batch's own gradient rows -
    score_batch on the gathered leaves - summed per atom (numpy, ascending views) within the bar of a float64 sum in another
    order (float rows: one rounding more); centre and pose gradients are the compact batch's bits; two runs give the same bits."""
    import torch

    d = _data(34, 150, 5, C_, mode, radii_type, kind)
    B, N = d["B"], d["N"]
    Fd, _ = _field(d, per_view)
    vox = _vox(radii_type, density, kind, differentiable=True)
    rng = np.random.default_rng(5)
    w = hip.dev(rng.uniform(0.5, 2.0, B) * rng.choice([-1.0, 1.0], B))
    posed, features = transform == "posed", mode == "features"

    def run():
        a = _leaves(d, posed, features)
        scores, atoms, index, offsets = _views(vox, d, Fd, transform, **a)
        wa = hip.dev(np.random.default_rng(6).standard_normal(int(offsets[-1])))
        L = (scores * w).sum() + ((atoms * wa).sum() if per_atom else 0.0)
        L.backward()
        return a, index, offsets, wa

    a, index, offsets, wa = run()
    again, _, _, _ = run()
    for k in a:
        assert a[k].grad is not None and torch.equal(a[k].grad, again[k].grad), k  # deterministic
    # the compact batch with leaves of its own
    b = _leaves(d, posed, features)
    rows = b.pop("xyz").detach()[index].requires_grad_()
    chan_rows = b.pop("chan").detach()[index].requires_grad_() if features else _take(hip.dev(d["chan"]), index)
    s_b, a_b = _batch(vox, d, Fd, transform, index, offsets, rows=rows, chan_rows=chan_rows, **b)
    ((s_b * w).sum() + ((a_b * wa).sum() if per_atom else 0.0)).backward()
    idx = index.cpu().numpy()
    ref, bound = vr.reduce_reference(idx, offsets, N, rows.grad.cpu().numpy())
    err = np.abs(a["xyz"].grad.cpu().numpy() - ref)
    assert tuple(a["xyz"].grad.shape) == (N, 3) and a["xyz"].grad.dtype == torch.float64
    assert np.all(err <= GRAD64_REL * bound + GRAD64_ABS), float(err.max())
    if density == "gaussian":
        assert np.count_nonzero(ref) > 30
    assert not a["xyz"].grad[0].any()  # (atom 0 is in no view)
    if features:
        gf = chan_rows.grad.cpu().numpy().astype(np.float64)
        ref, bound = vr.reduce_reference(idx, offsets, N, gf)
        got = a["chan"].grad
        assert tuple(got.shape) == (N, C_) and got.dtype == (torch.float64 if kind == "f64" else torch.float32)
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
        extra = 0.0 if kind == "f64" else 2.0 ** -24
        assert np.all(err <= GRAD64_REL * bound + GRAD64_ABS + extra * np.abs(ref)), float(err.max())
        assert np.count_nonzero(ref) > 30 * C_
    for k in b:
        assert torch.equal(a[k].grad, b[k].grad), k
        assert bool(a[k].grad.any()) or density == "binary"


def test_finite_differences_at_precision_64():
    """Central differences of (score_posed_views * w).sum() in q, t and one atom's coordinates, h = 2^-20 (about 1e-6):
    truncation of order h^2 and rounding of order 1e-16 |L| / h, both far below the bar 1e-6 max(1, |g|) (the bar of
    tests/test_hip_grad.py). The library rounds t to float32 and differentiates straight through: the test's t are float32
    values, and below 0.5 these are multiples of 2^-25, so t +- h is read exactly. The derivative is the one almost everywhere:
    a component whose step moves a voxel across an atom's truncation radius is skipped (the supports are read from binary
    grids with one channel per atom)."""
    import torch

    N, B, C_ = 12, 3, 3
    d = dict(_data(35, N, B, C_, "features", "scalar", "f64", tight=True))
    d["t"] = d["t"].astype(np.float32).astype(np.float64)
    Fd, _ = _field(d, True)
    vox = _vox("scalar", "gaussian", "f64", differentiable=True)
    mask = _vox("scalar", "binary", "f64")
    w = hip.dev(np.array([1.5, -0.7, 1.1]))
    chan = hip.dev(d["chan"])
    ids = torch.arange(N, device="cuda")

    def loss(xyz, q, t):
        with torch.no_grad():
            return float((vox.score_posed_views(hip.dev(xyz), hip.dev(d["cen"]), hip.dev(q), hip.dev(t), chan, 1.25, Fd) * w).sum())

    def support(xyz, q, t):
        return mask.forward_posed_views(hip.dev(xyz), hip.dev(d["cen"]), hip.dev(q), hip.dev(t), ids, 1.25, num_channels=N) != 0

    a = dict(xyz=hip.dev(d["xyz"], True), q=hip.dev(d["q"], True), t=hip.dev(d["t"], True))
    (vox.score_posed_views(a["xyz"], hip.dev(d["cen"]), a["q"], a["t"], chan, 1.25, Fd) * w).sum().backward()
    base = support(d["xyz"], d["q"], d["t"])
    assert bool(base.any(dim=(2, 3, 4)).all())  # every view keeps every atom
    h, checked = 2.0 ** -20, 0
    for name, where in (("q", [(b, k) for b in range(B) for k in range(4)]), ("t", [(b, k) for b in range(B) for k in range(3)]),
                        ("xyz", [(5, k) for k in range(3)])):
        g = a[name].grad.cpu().numpy()
        for at in where:
            vals, moved = [], False
            for sgn in (1.0, -1.0):
                x = {k: d[k].copy() for k in ("xyz", "q", "t")}
                x[name][at] += sgn * h
                moved = moved or not torch.equal(support(x["xyz"], x["q"], x["t"]), base)
                vals.append(loss(x["xyz"], x["q"], x["t"]))
            if moved:
                continue
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[at]) <= 1e-6 * max(abs(g[at]), 1.0), (name, at, fd, g[at])
            checked += 1
    assert checked >= 15


def test_a_step_with_device_poses_does_not_synchronise_outside_the_selection():
    """score_posed_views + backward() under torch's sync debug mode: the one synchronisation of the step is the selection's,
    inside the library (torch does not see it); nothing in the Python layer or in backward() waits for the device."""
    import torch

    d = _data(36, 150, 5, 32, "features", "scalar")
    Fd, _ = _field(d, False)
    vox = _vox(differentiable=True)
    w = hip.dev(np.array([1.0, -2.0, 0.5, 1.5, -1.0]))

    def step():
        a = _leaves(d, True, True)
        return a

    def run(a):
        scores = vox.score_posed_views(a["xyz"], a["cen"], a["q"], a["t"], a["chan"], 1.25, Fd)
        (scores * w).sum().backward()

    ref = step()
    run(ref)  # (first call: allocations)
    got = step()
    canary = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            canary.item()  # the mode is implemented: a synchronising read is an error
        run(got)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for k in ref:
        assert got[k].grad is not None and torch.equal(got[k].grad, ref[k].grad), k


def test_a_step_allocates_less_than_the_repeated_features():
    """256 views of a cloud of 1100 atoms with 32 channels: the whole step (scores, rows, reduction) stays below the bytes of
    the B feature copies the repeated-cloud form needs before it computes anything."""
    import torch

    d = _data(37, 1100, 256, 32, "features", "scalar", hole=False)
    Fd, _ = _field(d, False)
    vox = _vox(differentiable=True)
    a = _leaves(d, True, True)
    w = torch.ones(256, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    scores = vox.score_posed_views(a["xyz"], a["cen"], a["q"], a["t"], a["chan"], 1.25, Fd)
    (scores * w).sum().backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    copies = 256 * 1100 * 32 * 4
    print(f"VIEWS_MEMORY peak {peak} bytes against {copies} bytes of repeated features")
    assert 0 < peak < copies
    assert bool(a["xyz"].grad.any()) and bool(a["chan"].grad.any()) and bool(a["q"].grad.any())
