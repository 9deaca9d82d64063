"""Scores against a field grid on the GPU (score_batch / score_posed_batch, mvx_score_batch): scores and per-atom scores
against the float64 reference (tests/score_reference.py), the gradient rows against mvx_backward_batch bit for bit, autograd
against the unfused path (forward_batch, (grid * field).sum()), determinism and batch independence, layouts, and the memory a call
takes. Shapes as in tests/test_hip_pose.py: D = 16 and 24 at resolution 0.5, three molecules of {0, 1, 300} or {37, 150, 300}
atoms (300 is more than 4 waves x 64: a lane of the reduction sees a second chunk), centres around (30, -20, 12), |q| in
{1, 0.8, 1.25}; the first atom of every molecule of two or more atoms lies far outside the box."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import grad_reference as gr
from tests import pose_reference as pr
from tests import score_reference as sr
from tests import hip_support as hip
from tests.abi import MVX_ERR_INVALID, last_error
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

CEN = np.array([30.0, -20.0, 12.0])
NORMS = np.array([1.0, 0.8, 1.25])
FULL, SPARSE = (37, 150, 300), (0, 1, 300)


def _vox(D, radii_type="scalar", density="gaussian", kind="f32", **kw):
    import molvoxel_amd as mv

    if kind == "bf16":
        kw["grid_dtype"] = "bfloat16"
    return mv.create_voxelizer(0.5, D, radii_type, density, library="hip", precision=64 if kind == "f64" else 32, **kw)


@functools.lru_cache(maxsize=None)
def _data(seed, sizes, D, C_, mode, radii_type, kind="f32", beyond=False):
    """One batch: offsets, centres, coordinates around them, poses, channels and radii (host arrays; never modified)."""
    rng = np.random.default_rng(seed)
    fp = np.float64 if kind == "f64" else np.float32
    B, N = len(sizes), int(sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    W = 0.5 * (D - 1)
    cen = CEN + rng.normal(0.0, 0.4, (B, 3))
    xyz = np.concatenate([cen[b] + rng.uniform(-0.4 * W, 0.4 * W, (n, 3)) for b, n in enumerate(sizes)]).reshape(N, 3)
    outside = np.array([int(off[b]) for b, n in enumerate(sizes) if n >= 2], np.int64)
    for a in outside:
        xyz[a] += [100.0, -80.0, 90.0]  # (far outside under every pose: |q|^2 >= 0.64)
    q = rng.standard_normal((B, 4))
    q *= (NORMS[np.arange(B) % 3] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    types = rng.integers(0, C_ + (1 if beyond else 0), N)  # (beyond: type C_ lies past the channels of the call)
    chan = {"features": rng.standard_normal((N, C_)).astype(fp), "types": types, "single": None}[mode]
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(fp), "channel-wise": rng.uniform(1.0, 1.5, C_).astype(fp)}[radii_type]
    return dict(off=off, cen=cen, xyz=xyz, q=q, t=t, chan=chan, radii=radii, B=B, N=N, outside=outside, mode=mode, C=C_, D=D,
                radii_type=radii_type, kind=kind)


def _field(d, per_mol, seed=9):
    """(device field in the grid type of `kind`, the float64 array the kernel reads)."""
    import torch

    rng = np.random.default_rng(seed)
    shape = ((d["B"],) if per_mol else ()) + (d["C"],) + (d["D"],) * 3
    F = rng.standard_normal(shape)
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[d["kind"]]
    Fd = torch.tensor(F, device="cuda").to(dt)
    return Fd, Fd.to(torch.float64).cpu().numpy()


def _quats(d, seed):
    """The quaternions score_batch / forward_batch draw with random_rotation under np.random.seed(seed), molecule by molecule."""
    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform

    np.random.seed(seed)
    return np.array([draw_forward_transform(0.0, True)[1] for _ in range(d["B"])]).reshape(d["B"], 4)


def _call(vox, d, F, transform, per_atom=True, **over):
    a = {k: over.get(k, hip.dev(d[k])) for k in ("xyz", "cen", "q", "t", "chan", "radii")}
    nc = d["C"] if d["mode"] == "types" else None
    if transform == "posed":
        return vox.score_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], F, num_channels=nc,
                                     per_atom=per_atom)
    np.random.seed(transform)
    return vox.score_batch(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], F, num_channels=nc, random_rotation=True,
                           per_atom=per_atom)


def _positions(d, transform):
    if transform == "posed":
        return pr.batch_positions(d["xyz"], d["off"], d["cen"], d["q"], d["t"])
    return pr.batch_positions(d["xyz"], d["off"], d["cen"], _quats(d, transform), np.zeros((d["B"], 3)))


# ---- 1. scores and per-atom scores against the reference -------------------------------------------------------------------
SCORE_CASES = [
    # mode, C, radii type, density, grid, sizes, D, field per molecule, transform ("posed" or the seed of a random rotation)
    ("features", 32, "scalar", "gaussian", "f32", FULL, 16, False, "posed"),
    ("features", 33, "channel-wise", "gaussian", "f32", FULL, 16, True, 11),
    ("features", 5, "atom-wise", "binary", "f32", SPARSE, 24, False, "posed"),
    ("features", 33, "channel-wise", "binary", "bf16", SPARSE, 16, True, "posed"),
    ("features", 32, "atom-wise", "gaussian", "bf16", FULL, 24, False, 12),
    ("features", 5, "scalar", "gaussian", "f64", FULL, 16, True, "posed"),
    ("features", 33, "channel-wise", "gaussian", "f64", SPARSE, 16, False, 13),
    ("features", 1, "scalar", "binary", "f64", FULL, 16, False, "posed"),
    ("types", 5, "scalar", "gaussian", "f32", FULL, 16, False, "posed"),
    ("types", 5, "channel-wise", "gaussian", "f32", SPARSE, 24, True, 14),
    ("types", 33, "atom-wise", "binary", "f32", FULL, 16, False, "posed"),
    ("types", 32, "channel-wise", "binary", "bf16", FULL, 16, True, 15),
    ("types", 5, "atom-wise", "gaussian", "f64", SPARSE, 16, False, "posed"),
    ("types", 1, "scalar", "binary", "f64", FULL, 24, True, 16),
    ("single", 1, "scalar", "gaussian", "f32", FULL, 24, True, "posed"),
    ("single", 1, "atom-wise", "binary", "f32", SPARSE, 16, False, 17),
    ("single", 1, "atom-wise", "gaussian", "bf16", FULL, 16, False, "posed"),
    ("single", 1, "scalar", "binary", "f64", SPARSE, 16, True, "posed"),
]


@pytest.mark.parametrize("mode, C_, radii_type, density, kind, sizes, D, per_mol, transform", SCORE_CASES)
def test_scores_match_the_reference(mode, C_, radii_type, density, kind, sizes, D, per_mol, transform):
    import torch

    beyond = mode == "types" and radii_type != "channel-wise"
    d = _data(21, sizes, D, C_, mode, radii_type, kind, beyond)
    Fd, Fref = _field(d, per_mol)
    vox = _vox(D, radii_type, density, kind)
    scores, atoms = _call(vox, d, Fd, transform)
    assert scores.dtype == torch.float64 and atoms.dtype == torch.float64 and scores.is_cuda and atoms.is_cuda
    assert tuple(scores.shape) == (d["B"],) and tuple(atoms.shape) == (d["N"],)
    only = _call(vox, d, Fd, transform, per_atom=False)
    assert torch.equal(only, scores)  # (the per-atom scores in workspace instead: the same bits)
    S, s = scores.cpu().numpy(), atoms.cpu().numpy()
    p = _positions(d, transform)
    w = d["chan"].astype(np.float64) if mode == "features" else None
    s_ref, b_ref, S_ref, Sb_ref = sr.batch_reference(p, d["off"], Fref, d["radii"], radii_type, w=w, mode=mode,
                                                     types=d["chan"] if mode == "types" else None, density=density,
                                                     precision=64 if kind == "f64" else 32)
    assert np.count_nonzero(s_ref) > 0.3 * d["N"]
    # binary types / single: the terms are field values times 1, summed in float64 in another order than the reference's
    exact_terms = density == "binary" and mode != "features"
    rel, abs_ = (GRAD64_REL, GRAD64_ABS) if (kind == "f64" or exact_terms) else (GRAD_REL, GRAD_ABS)
    err, ERR = np.abs(s - s_ref), np.abs(S - S_ref)
    worst = max(float((err[b_ref > 0] / b_ref[b_ref > 0]).max()), float((ERR[Sb_ref > 0] / Sb_ref[Sb_ref > 0]).max()))
    print(f"SCORE_WORST grid {kind} {mode} {radii_type} {density}{' exact-terms' if exact_terms else ''}: |got - ref| / bound = {worst:.3g}")
    assert np.all(err <= rel * b_ref + abs_), (float(err.max()), int(np.argmax(err - rel * b_ref)))
    assert np.all(ERR <= rel * Sb_ref + abs_), (ERR, Sb_ref)
    # exact zeros: atoms outside the box, atoms the reference admits nowhere, types past the channels, empty molecules
    assert np.all(s[d["outside"]] == 0.0) and len(d["outside"]) >= 1
    assert np.all(s[b_ref == 0.0] == 0.0)
    if beyond:
        assert np.any(d["chan"] >= C_) and np.all(s[d["chan"] >= C_] == 0.0)
    for b, n in enumerate(sizes):
        if n == 0:
            assert S[b] == 0.0 and not np.signbit(S[b])


def test_molecules_without_atoms_score_exact_zeros():
    import torch

    vox = _vox(16)
    off = np.zeros(4, np.int64)
    F = torch.ones((4, 16, 16, 16), device="cuda")
    scores, atoms = vox.score_batch(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), off, None,
                                    torch.zeros((0, 4), device="cuda"), 1.0, F, per_atom=True)
    assert tuple(scores.shape) == (3,) and tuple(atoms.shape) == (0,) and torch.equal(scores, torch.zeros_like(scores))
    none = vox.score_batch(torch.zeros((0, 3), dtype=torch.float64, device="cuda"), np.zeros(1, np.int64), None,
                           torch.zeros((0, 4), device="cuda"), 1.0, F)
    assert tuple(none.shape) == (0,)


def test_host_inputs_are_moved_to_the_device():
    import torch

    d = _data(22, FULL, 16, 5, "features", "atom-wise")
    Fd, _ = _field(d, False)
    vox = _vox(16, "atom-wise")
    ref = _call(vox, d, Fd, "posed")
    got = vox.score_posed_batch(d["xyz"], d["off"], d["cen"], d["q"], d["t"], d["chan"], d["radii"], Fd.cpu().numpy(), per_atom=True)
    assert got[0].is_cuda and torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_a_bad_stride_and_a_channel_of_four_gib_are_rejected_before_the_device():
    from molvoxel_amd.voxelizer.hip import _lib

    P = 16  # (a non-null pointer: nothing behind it is read)
    off = np.array([0, 3], np.int64)

    def entry(vox, C_, stride):
        rc = vox._lib.mvx_score_batch(vox._handle, 0, P, P, None, 1.0, 0, off.ctypes.data, None, 1, C_, P, stride, P, None, None,
                                      None, None)
        return rc, last_error()

    vox = _vox(16)
    for stride in (1, 4 * 16 ** 3 - 1, 4 * 16 ** 3 + 1, 16 ** 3, 5 * 16 ** 3):
        rc, msg = entry(vox, 4, stride)
        assert rc == MVX_ERR_INVALID and "field_mol_stride" in msg, (stride, rc, msg)
    big = _vox(820, kind="f64")  # 820^3 doubles: a channel of more than 4 GiB (the handle owns no grid)
    rc, msg = entry(big, 1, 0)
    assert rc == MVX_ERR_INVALID and "4 GiB" in msg, (rc, msg)
    assert _lib.MODES["features"] == 0


# ---- 2. gradient bits ---------------------------------------------------------------------------------------------------------
def _abi(vox, d, F, entry="score", want=("scores", "atoms", "gc", "gf")):
    """mvx_score_batch (or mvx_backward_batch with grad_out = F laid out per molecule) through ctypes on the posed batch `d`.
    Outputs start as NaN: whatever is not overwritten fails every comparison."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    mode, C_, B, N = d["mode"], d["C"], d["B"], d["N"]
    fdt = torch.float64 if d["kind"] == "f64" else torch.float32
    c = hip.dev(d["xyz"])
    ch = None if mode == "single" else (hip.dev(d["chan"]).to(fdt) if mode == "features" else hip.dev(d["chan"]).to(torch.int32))
    r = None if np.isscalar(d["radii"]) else hip.dev(d["radii"]).to(fdt)
    rs = float(d["radii"]) if np.isscalar(d["radii"]) else 0.0
    pose = vox._pack_pose(B, hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), True)
    xfs = vox._pose_xforms(pose, B)
    nan = lambda shape, dt=torch.float64: torch.full(shape, float("nan"), dtype=dt, device="cuda")  # noqa: E731
    out = dict(scores=nan((B,)), atoms=nan((N,)) if "atoms" in want else None, gc=nan((N, 3)) if "gc" in want else None,
               gf=nan((N, C_), fdt) if ("gf" in want and mode == "features") else None)
    ptr = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    args = (vox._handle, _lib.MODES[mode], ptr(c), ptr(ch), ptr(r), rs, vox._radii_type_code(), d["off"].ctypes.data, C.addressof(xfs),
            B, C_)
    if entry == "score":
        rc = vox._lib.mvx_score_batch(*args, ptr(F), 0 if F.dim() == 4 else C_ * d["D"] ** 3, ptr(out["scores"]), ptr(out["atoms"]),
                                      ptr(out["gc"]), ptr(out["gf"]), vox._stream())
    else:
        G = F.expand((B,) + tuple(F.shape)).contiguous() if F.dim() == 4 else F
        rc = vox._lib.mvx_backward_batch(*args, ptr(G), ptr(out["gc"]), ptr(out["gf"]), vox._stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    return out


BIT_CASES = [
    # mode, C, radii type, density, grid, sizes, per molecule
    ("features", 32, "scalar", "gaussian", "f32", FULL, False),
    ("features", 33, "channel-wise", "gaussian", "f32", FULL, True),
    ("features", 33, "channel-wise", "binary", "bf16", SPARSE, False),
    ("features", 5, "atom-wise", "gaussian", "bf16", (300,), True),   # B = 1
    ("features", 33, "channel-wise", "gaussian", "f64", (150,), False),  # B = 1
    ("features", 5, "scalar", "binary", "f64", FULL, True),
    ("types", 5, "atom-wise", "gaussian", "f32", FULL, True),
    ("types", 33, "channel-wise", "gaussian", "bf16", SPARSE, False),
    ("types", 5, "scalar", "binary", "f32", FULL, False),
    ("single", 1, "atom-wise", "gaussian", "f64", FULL, True),
]


@pytest.mark.parametrize("mode, C_, radii_type, density, kind, sizes, per_mol", BIT_CASES)
def test_gradient_rows_are_the_backward_entrys_bits(mode, C_, radii_type, density, kind, sizes, per_mol):
    import torch

    D = 16
    d = _data(23, sizes, D, C_, mode, radii_type, kind)
    Fd, _ = _field(d, per_mol)
    vox = _vox(D, radii_type, density, kind)
    got = _abi(vox, d, Fd, "score")
    ref = _abi(vox, d, Fd, "backward", want=("gc", "gf"))
    assert torch.equal(got["gc"], ref["gc"])
    if density == "gaussian":
        assert float(got["gc"].abs().sum()) > 0
    else:  # binary density: zero coordinate gradients, but scores (and feature gradients)
        assert torch.equal(got["gc"], torch.zeros_like(got["gc"])) and float(got["scores"].abs().sum()) > 0
    if mode == "features":
        assert torch.equal(got["gf"], ref["gf"]) and float(got["gf"].abs().sum()) > 0
    # the outputs do not depend on which of the optional ones are asked for
    few = _abi(vox, d, Fd, "score", want=())
    assert torch.equal(few["scores"], got["scores"]) and not torch.isnan(got["atoms"]).any()
    only_gc = _abi(vox, d, Fd, "score", want=("gc",))
    assert torch.equal(only_gc["gc"], got["gc"]) and torch.equal(only_gc["scores"], got["scores"])


# ---- 3. autograd --------------------------------------------------------------------------------------------------------------
def _leaves(d, posed):
    names = ("xyz", "cen", "q", "t") if posed else ("xyz", "cen")
    a = {k: hip.dev(d[k], grad=True) for k in names}
    if d["mode"] == "features":
        a["chan"] = hip.dev(d["chan"], grad=True)
    return a


def _unfused(vox, d, F, transform, a):
    nc = d["C"] if d["mode"] == "types" else None
    chan, radii = a.get("chan", hip.dev(d["chan"])), hip.dev(d["radii"])
    if transform == "posed":
        grid = vox.forward_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], chan, radii, num_channels=nc)
    else:
        np.random.seed(transform)
        grid = vox.forward_batch(a["xyz"], d["off"], a["cen"], chan, radii, num_channels=nc, random_rotation=True,
                                 random_translation=0.5)
    return (grid * F).sum(dim=(1, 2, 3, 4))


def _fused(vox, d, F, transform, a, per_atom=False):
    nc = d["C"] if d["mode"] == "types" else None
    chan, radii = a.get("chan", hip.dev(d["chan"])), hip.dev(d["radii"])
    if transform == "posed":
        return vox.score_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], chan, radii, F, num_channels=nc, per_atom=per_atom)
    np.random.seed(transform)
    return vox.score_batch(a["xyz"], d["off"], a["cen"], chan, radii, F, num_channels=nc, random_rotation=True,
                           random_translation=0.5, per_atom=per_atom)


AUTOGRAD_CASES = [
    ("features", 33, "channel-wise", "gaussian", "f32", FULL, "posed", True),
    ("features", 5, "scalar", "gaussian", "bf16", SPARSE, 31, False),
    ("features", 32, "atom-wise", "gaussian", "f64", FULL, 32, True),
    ("features", 5, "atom-wise", "binary", "f32", FULL, "posed", False),
    ("types", 5, "atom-wise", "gaussian", "f32", FULL, "posed", False),
    ("single", 1, "scalar", "gaussian", "f64", SPARSE, "posed", True),
    ("types", 5, "channel-wise", "gaussian", "bf16", FULL, 33, True),
]


@pytest.mark.parametrize("mode, C_, radii_type, density, kind, sizes, transform, per_mol", AUTOGRAD_CASES)
def test_backward_of_the_summed_scores_is_the_unfused_paths_bits(mode, C_, radii_type, density, kind, sizes, transform, per_mol):
    import torch

    D = 16
    d = _data(24, sizes, D, C_, mode, radii_type, kind)
    Fd, _ = _field(d, per_mol)
    vox = _vox(D, radii_type, density, kind, differentiable=True)
    posed = transform == "posed"
    a, b = _leaves(d, posed), _leaves(d, posed)
    scores = _fused(vox, d, Fd, transform, a)
    assert scores.requires_grad and tuple(scores.shape) == (d["B"],)
    scores.sum().backward()
    _unfused(vox, d, Fd, transform, b).sum().backward()
    plain = _fused(_vox(D, radii_type, density, kind), d, Fd, transform, {k: v.detach() for k, v in a.items()})
    assert torch.equal(plain, scores.detach())  # (recording the graph does not change the scores)
    for k in a:
        assert a[k].grad is not None and torch.equal(a[k].grad, b[k].grad), k
    if density == "gaussian":
        assert float(a["xyz"].grad.abs().sum()) > 0 and float(a["cen"].grad.abs().sum()) > 0


def test_only_what_requires_grad_is_recorded():
    import torch

    d = _data(24, FULL, 16, 5, "features", "scalar")
    Fd, _ = _field(d, False)
    vox = _vox(16, differentiable=True)
    assert not _call(vox, d, Fd, "posed", per_atom=False).requires_grad
    f = hip.dev(d["chan"], grad=True)
    s = _call(vox, d, Fd, "posed", per_atom=False, chan=f)
    s.sum().backward()
    g = hip.dev(d["chan"], grad=True)
    _unfused(vox, d, Fd, "posed", dict(xyz=hip.dev(d["xyz"]), cen=hip.dev(d["cen"]), q=hip.dev(d["q"]), t=hip.dev(d["t"]), chan=g)).sum().backward()
    assert torch.equal(f.grad, g.grad)
    with torch.no_grad():
        assert not _call(vox, d, Fd, "posed", per_atom=False, chan=f).requires_grad


def test_a_non_uniform_upstream_matches_the_unfused_path_within_the_gradient_bars():
    """(scores * wts).sum(): the fused path scales the saved rows, the unfused one walks wts[b] * field - other roundings, so
    the bar is the gradient rule with |wts[b]| times the reference's bound."""
    import torch

    D, C_ = 16, 5
    d = _data(25, FULL, D, C_, "features", "atom-wise")
    Fd, Fref = _field(d, True)
    vox = _vox(D, "atom-wise", differentiable=True)
    wts = np.array([0.37, -2.9, 1.7])
    a, b = _leaves(d, True), _leaves(d, True)
    (_fused(vox, d, Fd, "posed", a) * hip.dev(wts)).sum().backward()
    (_unfused(vox, d, Fd, "posed", b) * hip.dev(wts)).sum().backward()
    p = _positions(d, "posed")
    for m in range(d["B"]):
        lo, hi = int(d["off"][m]), int(d["off"][m + 1])
        o = gr.reference(p[lo:hi], Fref[m], d["radii"][lo:hi], "atom-wise", w=d["chan"][lo:hi].astype(np.float64))
        M = pr.rotation(d["q"][m])
        pose = pr.pose_grads(d["xyz"][lo:hi], d["cen"][m], d["q"][m], *o["coords"])
        bounds = {"xyz": (slice(lo, hi), o["coords"][1] @ np.abs(M)), "chan": (slice(lo, hi), o["features"][1]),
                  "cen": (m, pose["center"][1]), "q": (m, pose["quaternion"][1]), "t": (m, pose["translation"][1])}
        for k, (rows, bound) in bounds.items():
            got, ref = a[k].grad[rows].cpu().numpy().astype(np.float64), b[k].grad[rows].cpu().numpy().astype(np.float64)
            assert np.abs(ref).sum() > 0
            assert np.all(np.abs(got - ref) <= GRAD_REL * abs(wts[m]) * bound + GRAD_ABS), (k, m, float(np.abs(got - ref).max()))


def test_a_per_atom_upstream_is_the_sum_of_the_atoms_own_gradients():
    """L = sum_n u_n s_n with u_n in {0.5, -2, 4}: the unfused path is one call per distinct upstream on the atoms that carry it.
    Powers of two scale every product and sum exactly, so rows agree bit for bit; the centres are sums of the rows in another
    order (float64: the GRAD64 rule on the sum of their absolute values)."""
    import torch

    D, C_ = 16, 5
    d = _data(26, FULL, D, C_, "features", "scalar")
    Fd, _ = _field(d, False)
    vox = _vox(D, differentiable=True)
    u = np.array([0.5, -2.0, 4.0])[np.random.default_rng(1).integers(0, 3, d["N"])]
    a = _leaves(d, False)
    scores, atoms = _fused(vox, d, Fd, 41, a, per_atom=True)
    assert torch.equal(scores, _fused(vox, d, Fd, 41, {k: v.detach() for k, v in a.items()}))
    (atoms * hip.dev(u)).sum().backward()
    gx, gf, gc = torch.zeros_like(a["xyz"]), torch.zeros_like(a["chan"]), torch.zeros_like(a["cen"])
    mol = np.repeat(np.arange(d["B"]), np.diff(d["off"]))
    for v in np.unique(u):
        keep = np.flatnonzero(u == v)
        off = np.concatenate([[0], np.cumsum(np.bincount(mol[keep], minlength=d["B"]))]).astype(np.int64)
        x, f, c = hip.dev(d["xyz"][keep], grad=True), hip.dev(d["chan"][keep], grad=True), hip.dev(d["cen"], grad=True)
        np.random.seed(41)
        grid = vox.forward_batch(x, off, c, f, 1.25, random_rotation=True, random_translation=0.5)
        (float(v) * (grid * Fd).sum()).backward()
        rows = torch.as_tensor(keep, device="cuda")
        gx[rows], gf[rows] = x.grad, f.grad
        gc += c.grad
    assert torch.equal(a["xyz"].grad, gx) and torch.equal(a["chan"].grad, gf) and float(gx.abs().sum()) > 0
    lengths = torch.as_tensor(np.diff(d["off"]), device="cuda")
    bound = torch.segment_reduce(a["xyz"].grad.abs(), "sum", lengths=lengths, axis=0)
    assert bool(((a["cen"].grad - gc).abs() <= GRAD64_REL * bound + GRAD64_ABS).all())
    # upstreams on both outputs add up: L = sum_b S_b + sum_n s_n doubles every row
    b = _leaves(d, False)
    S, s = _fused(vox, d, Fd, 41, b, per_atom=True)
    (S.sum() + s.sum()).backward()
    c = _leaves(d, False)
    _fused(vox, d, Fd, 41, c).sum().backward()
    for k in b:
        assert torch.equal(b[k].grad, 2 * c[k].grad), k


# ---- 4. determinism and batch independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode, C_, radii_type, kind", [("features", 33, "channel-wise", "f32"), ("types", 5, "atom-wise", "bf16"),
                                                         ("features", 5, "scalar", "f64")])
def test_a_molecule_scores_the_same_bits_alone_in_any_batch_and_order(mode, C_, radii_type, kind):
    import torch

    D = 16
    d = _data(27, FULL, D, C_, mode, radii_type, kind)
    Fd, _ = _field(d, True)
    vox = _vox(D, radii_type, "gaussian", kind)
    one, two = _abi(vox, d, Fd), _abi(vox, d, Fd)
    keys = [k for k in one if one[k] is not None]
    assert set(keys) >= {"scores", "atoms", "gc"}
    for k in keys:
        assert torch.equal(one[k].view(torch.uint8), two[k].view(torch.uint8)), k  # the same bytes
    for m in range(d["B"]):
        lo, hi = int(d["off"][m]), int(d["off"][m + 1])
        alone = dict(d, off=np.array([0, hi - lo], np.int64), xyz=d["xyz"][lo:hi], cen=d["cen"][m:m + 1], q=d["q"][m:m + 1],
                     t=d["t"][m:m + 1], chan=None if d["chan"] is None else d["chan"][lo:hi],
                     radii=d["radii"][lo:hi] if radii_type == "atom-wise" else d["radii"], B=1, N=hi - lo)
        for F in (Fd[m].contiguous(), Fd[m:m + 1].contiguous()):  # shared by the one molecule, or its own
            got = _abi(vox, alone, F)
            assert torch.equal(got["scores"], one["scores"][m:m + 1]) and torch.equal(got["atoms"], one["atoms"][lo:hi])
            assert torch.equal(got["gc"], one["gc"][lo:hi])
            if mode == "features":
                assert torch.equal(got["gf"], one["gf"][lo:hi])
    vox.debug_option("grad_order", 1)
    ordered = _abi(vox, d, Fd)
    for k in keys:
        assert torch.equal(ordered[k], one[k]), k


# ---- 5. layout ----------------------------------------------------------------------------------------------------------------
def test_a_channels_last_field_is_read_as_the_contiguous_one():
    import torch

    D, C_ = 16, 32
    d = _data(28, FULL, D, C_, "features", "scalar")
    for per_mol in (False, True):
        Fd, _ = _field(d, per_mol)
        ref = _call(_vox(D), d, Fd, "posed")
        if per_mol:
            Fcl = Fd.contiguous(memory_format=torch.channels_last_3d)
        else:
            Fcl = Fd.unsqueeze(0).contiguous(memory_format=torch.channels_last_3d).squeeze(0)
        assert not Fcl.is_contiguous() and torch.equal(Fcl, Fd)
        got = _call(_vox(D, grid_layout="channels_last"), d, Fcl, "posed")
        assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_a_float32_field_on_a_bfloat16_voxelizer_is_rounded_like_the_upstream_gradient():
    import torch

    D, C_ = 16, 5
    d = _data(28, FULL, D, C_, "features", "atom-wise", "bf16")
    vox = _vox(D, "atom-wise", "gaussian", "bf16")
    F32 = torch.tensor(np.random.default_rng(2).standard_normal((C_, D, D, D)), device="cuda", dtype=torch.float32)
    a, b = _call(vox, d, F32, "posed"), _call(vox, d, F32.to(torch.bfloat16), "posed")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    exact = _call(_vox(D, "atom-wise"), dict(d, kind="f32"), F32, "posed")
    assert not torch.equal(exact[0], a[0])  # (the rounding of the field is visible)


# ---- 6. no grid ---------------------------------------------------------------------------------------------------------------
def test_a_score_call_allocates_far_less_than_the_grids():
    """64 posed ligands at D = 24, C = 32: the grids would take 64 x 32 x 24^3 x 4 bytes = 113 MB; the call's tensors are its
    outputs (scores, gradient rows: tens of kilobytes) - a condition on what the call allocates, not a measurement."""
    import torch

    D, C_, B = 24, 32, 64
    rng = np.random.default_rng(5)
    sizes = tuple(int(n) for n in rng.integers(20, 40, B))
    d = _data(29, sizes, D, C_, "features", "scalar")
    Fd, _ = _field(d, False)
    vox = _vox(D, differentiable=True)
    a = _leaves(d, True)
    _fused(vox, d, Fd, "posed", a).sum().backward()  # (warm: the library's workspace and torch's pools)
    for v in a.values():
        v.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    scores = _fused(vox, d, Fd, "posed", a)
    scores.sum().backward()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - base
    grids = B * C_ * D ** 3 * 4
    assert float(scores.detach().abs().sum()) > 0 and a["q"].grad is not None
    assert used < grids, (used, grids)
