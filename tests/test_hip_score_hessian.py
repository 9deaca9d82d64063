"""Second-order scores on the GPU (score_hessian_batch / score_hessian_posed_batch, mvx_score_hessian_batch): the scores and
per-atom gradients against mvx_score_batch bit for bit, the per-atom Hessians and the twist gradient and Hessian against the
float64 reference (tests/hessian_reference.py), determinism and batch independence, pivots, atoms that reach no voxel, and one
undamped Newton step. Every case has D = 16 at resolution 0.5:

    case    mode      C   radii      atoms per molecule  field         pose      grid
    base    features  5   atom-wise  0 / 17 / 70         shared        explicit  f32
    wide    features  33  scalar     40 / 9              per molecule  explicit  f32     (two channel chunks)
    types   types     4   by type    30 / 1 / 65         shared        none      bf16    (one atom of type 4 >= C)
    single  single    1   scalar     64 / 65             shared        explicit  f64
    binary  types     3   atom-wise  20 / 20             shared        explicit  f32     (binary density)
    feat64  features  5   atom-wise  33 / 12             per molecule  explicit  f64

The types case goes through the C entry itself: the Python layer refuses a type beyond radii given by type, the library gives such
an atom no box; it is the last atom of its molecule, so that the live atoms keep their lanes in the call without it.

Worst |got - ref| / bar over the cases, printed with -s (MI355X; bars GRAD_REL * bound + GRAD_ABS, GRAD64_* at precision 64;
DESIGN.md section 25, profiles/r20_score_hessian.txt): atom_hess 0.0078 (base), atom_grad 0.0061 (base), twist_hess 9.7e-4 (wide),
twist_grad 7.6e-4 (types), M^T atom_grad against the first-order dS/dcoords 8.6e-4 (feat64; float32 cases 2e-11), G_omega under a
shifted pivot 1.9e-4 (single), the Hessian about a shifted pivot 7.9e-4 (types). The Newton step on `single`, molecule 0, from a
twist of 0.02 A and 0.5 degrees: score 1566.777 -> 1568.338, |G| 58.6 -> 18.7 (ratio 0.32; the gradient does not vanish at the
identity pose, because the truncation at the radius is held fixed). 21 cases in 3.5 s.
"""
import functools

import numpy as np
import pytest

from tests import hessian_reference as hr
from tests import pose_reference as pr
from tests import hip_support as hip
from tests.abi import last_error
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

D = 16
CEN = np.array([30.0, -20.0, 12.0])
NORMS = np.array([1.0, 0.9, 1.1])
CASES = {
    "base": dict(mode="features", C=5, radii_type="atom-wise", sizes=(0, 17, 70), per_mol=False, posed=True, kind="f32"),
    "wide": dict(mode="features", C=33, radii_type="scalar", sizes=(40, 9), per_mol=True, posed=True, kind="f32"),
    "types": dict(mode="types", C=4, radii_type="channel-wise", sizes=(30, 1, 65), per_mol=False, posed=False, kind="bf16"),
    "single": dict(mode="single", C=1, radii_type="scalar", sizes=(64, 65), per_mol=False, posed=True, kind="f64"),
    "binary": dict(mode="types", C=3, radii_type="atom-wise", sizes=(20, 20), per_mol=False, posed=True, kind="f32", density="binary"),
    "feat64": dict(mode="features", C=5, radii_type="atom-wise", sizes=(33, 12), per_mol=True, posed=True, kind="f64"),
}
WORST = {}


def _bars(kind):
    return (GRAD64_REL, GRAD64_ABS) if kind == "f64" else (GRAD_REL, GRAD_ABS)


@functools.lru_cache(maxsize=None)
def _data(name, seed=31):
    """One batch of a case as host arrays (never modified): offsets, centres, coordinates, poses, channels, radii, field."""
    c = dict(CASES[name])
    c.setdefault("density", "gaussian")
    rng = np.random.default_rng(seed)
    fp = np.float64 if c["kind"] == "f64" else np.float32
    sizes, C_ = c["sizes"], c["C"]
    B, N = len(sizes), int(sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    W = 0.5 * (D - 1)
    if c["posed"]:
        cen = CEN + rng.normal(0.0, 0.4, (B, 3))
        xyz = np.concatenate([cen[b] + rng.uniform(-0.4 * W, 0.4 * W, (n, 3)) for b, n in enumerate(sizes)]).reshape(N, 3)
    else:  # no centres, no pose: the coordinates are grid-frame positions
        cen = None
        xyz = rng.uniform(-0.45 * W, 0.45 * W, (N, 3))
    q = rng.standard_normal((B, 4))
    q *= (NORMS[np.arange(B) % 3] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    chan = None
    if c["mode"] == "features":
        chan = rng.standard_normal((N, C_)).astype(fp)
    elif c["mode"] == "types":
        chan = rng.integers(0, C_, N)
        if name == "types":
            chan[int(off[3]) - 1] = C_  # the last atom: a type beyond the channels of the call, no box (at the tail the live atoms keep their lanes)
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(fp), "channel-wise": rng.uniform(1.0, 1.5, C_).astype(fp)}[c["radii_type"]]
    F = rng.standard_normal(((B,) if c["per_mol"] else ()) + (C_,) + (D,) * 3)
    return dict(c, name=name, off=off, cen=cen, xyz=xyz, q=q, t=t, chan=chan, radii=radii, F=F, B=B, N=N)


def _sub(d, b):
    """Molecule b of a batch as a batch of its own."""
    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    out = dict(d, sizes=(hi - lo,), off=np.array([0, hi - lo], np.int64), xyz=d["xyz"][lo:hi], q=d["q"][b:b + 1], t=d["t"][b:b + 1],
               cen=None if d["cen"] is None else d["cen"][b:b + 1], chan=None if d["chan"] is None else d["chan"][lo:hi], B=1, N=hi - lo)
    if d["radii_type"] == "atom-wise":
        out["radii"] = d["radii"][lo:hi]
    if d["per_mol"]:
        out["F"] = d["F"][b:b + 1]
    return out


def _without(d, drop):
    """The batch without the atoms `drop` (indices into the batch)."""
    keep = np.ones(d["N"], bool)
    keep[drop] = False
    sizes = tuple(int(keep[int(d["off"][b]):int(d["off"][b + 1])].sum()) for b in range(d["B"]))
    out = dict(d, sizes=sizes, off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64), xyz=d["xyz"][keep],
               chan=None if d["chan"] is None else d["chan"][keep], N=int(keep.sum()))
    if d["radii_type"] == "atom-wise":
        out["radii"] = d["radii"][keep]
    return out, keep


def _vox(d, **kw):
    import molvoxel_amd as mv

    if d["kind"] == "bf16":
        kw["grid_dtype"] = "bfloat16"
    return mv.create_voxelizer(0.5, D, d["radii_type"], d["density"], library="hip", precision=64 if d["kind"] == "f64" else 32, **kw)


def _field(d):
    """(device field in the grid type of the case, the float64 array the kernel reads)."""
    import torch

    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[d["kind"]]
    Fd = torch.tensor(d["F"], device="cuda").to(dt)
    return Fd, Fd.to(torch.float64).cpu().numpy()


def _raw(vox, d, Fd, pivots=None, first_order=False):
    """The types case through the C entries: (scores, twist_grad, twist_hess, atom_grad, atom_hess) of mvx_score_hessian_batch, or
    (scores, grad_coords) of mvx_score_batch."""
    import torch

    assert d["mode"] == "types" and d["radii_type"] == "channel-wise" and not d["posed"] and not d["per_mol"]
    xyz = torch.tensor(d["xyz"], device="cuda")
    ty = torch.tensor(d["chan"].astype(np.int32), device="cuda")
    r = torch.tensor(d["radii"], device="cuda")
    B, N = d["B"], d["N"]
    f64 = dict(dtype=torch.float64, device="cuda")
    scores = torch.full((B,), np.nan, **f64)
    head = (vox._handle, 1, xyz.data_ptr(), ty.data_ptr(), r.data_ptr(), 0.0, 2, d["off"].ctypes.data, None, B, d["C"], Fd.data_ptr(), 0)
    stream = torch.cuda.current_stream().cuda_stream
    if first_order:
        gc = torch.full((N, 3), np.nan, **f64)
        rc = vox._lib.mvx_score_batch(*head, scores.data_ptr(), None, gc.data_ptr(), None, stream)
        assert rc == 0, vox._lib.mvx_last_error()
        return scores, gc
    piv = None if pivots is None else torch.tensor(np.asarray(pivots, np.float64), device="cuda")
    tg, th = torch.full((B, 6), np.nan, **f64), torch.full((B, 6, 6), np.nan, **f64)
    ag, ah = torch.full((N, 3), np.nan, **f64), torch.full((N, 6), np.nan, **f64)
    rc = vox._lib.mvx_score_hessian_batch(*head, None if piv is None else piv.data_ptr(), scores.data_ptr(), ag.data_ptr(), ah.data_ptr(),
                                          tg.data_ptr(), th.data_ptr(), stream)
    assert rc == 0, vox._lib.mvx_last_error()
    return scores, tg, th, ag, ah


def _call(vox, d, Fd, pivots=None, per_atom=True, **over):
    """(scores, twist_grad, twist_hess, atom_grad, atom_hess) of the case's batch."""
    if d["name"] == "types":
        return _raw(vox, d, Fd, pivots)
    a = {k: over.get(k, hip.dev(d[k])) for k in ("xyz", "cen", "q", "t", "chan", "radii")}
    nc = d["C"] if d["mode"] == "types" else None
    piv = None if pivots is None else hip.dev(np.asarray(pivots, np.float64))
    if d["posed"]:
        return vox.score_hessian_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], Fd, num_channels=nc,
                                             pivots=piv, per_atom=per_atom)
    return vox.score_hessian_batch(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], Fd, num_channels=nc, pivots=piv, per_atom=per_atom)


def _first_order(d, Fd):
    """(scores, dS/dcoords) of the existing first-order entry for the same batch."""
    if d["name"] == "types":
        return _raw(_vox(d), d, Fd, first_order=True)
    vox = _vox(d, differentiable=True)
    xyz = hip.dev(d["xyz"], grad=True)
    nc = d["C"] if d["mode"] == "types" else None
    if d["posed"]:
        scores = vox.score_posed_batch(xyz, d["off"], hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), hip.dev(d["chan"]), hip.dev(d["radii"]), Fd, num_channels=nc)
    else:
        scores = vox.score_batch(xyz, d["off"], hip.dev(d["cen"]), hip.dev(d["chan"]), hip.dev(d["radii"]), Fd, num_channels=nc)
    scores.sum().backward()
    return scores.detach(), xyz.grad


def _positions(d):
    if not d["posed"]:
        return d["xyz"] if d["cen"] is None else np.concatenate(
            [d["xyz"][int(d["off"][b]):int(d["off"][b + 1])] - d["cen"][b] for b in range(d["B"])]).reshape(-1, 3)
    return pr.batch_positions(d["xyz"], d["off"], d["cen"], d["q"], d["t"])


def _default_pivots(d):
    return d["t"].astype(np.float32).astype(np.float64) if d["posed"] else np.zeros((d["B"], 3))


@functools.lru_cache(maxsize=None)
def _reference(name):
    """The float64 reference of a case, computed once: positions, per-atom (s, g, H) with bounds, and per molecule the twist
    gradient and Hessian about the default pivots with bounds. Read only."""
    import torch  # noqa: F401  (the field as the kernel reads it needs the device's rounding to the grid type)

    d = _data(name)
    _, Fref = _field(d)
    p = _positions(d)
    N, B = d["N"], d["B"]
    out = {k: (np.zeros((N,) + s), np.zeros((N,) + s)) for k, s in (("s", ()), ("g", (3,)), ("H", (6,)))}
    for b in range(B):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            continue
        r = d["radii"][lo:hi] if d["radii_type"] == "atom-wise" else d["radii"]
        ref = hr.reference(p[lo:hi], Fref[b] if d["per_mol"] else Fref, r, d["radii_type"],
                           w=None if d["mode"] != "features" else d["chan"][lo:hi].astype(np.float64), mode=d["mode"],
                           types=d["chan"][lo:hi] if d["mode"] == "types" else None, density=d["density"],
                           precision=64 if d["kind"] == "f64" else 32)
        for k in out:
            out[k][0][lo:hi], out[k][1][lo:hi] = ref[k]
    piv = _default_pivots(d)
    tw = [hr.twist(p[int(d["off"][b]):int(d["off"][b + 1])], out["g"][0][int(d["off"][b]):int(d["off"][b + 1])],
                   out["H"][0][int(d["off"][b]):int(d["off"][b + 1])], piv[b], out["g"][1][int(d["off"][b]):int(d["off"][b + 1])],
                   out["H"][1][int(d["off"][b]):int(d["off"][b + 1])]) for b in range(B)]
    for v in out.values():
        for x in v:
            x.setflags(write=False)
    return dict(out, p=p, piv=piv, G=np.array([t_[0] for t_ in tw]), bG=np.array([t_[1] for t_ in tw]),
                X=np.array([t_[2] for t_ in tw]), bX=np.array([t_[3] for t_ in tw]))


def _close(got, ref, bound, rel, abs_, what, name):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bar = rel * bound + abs_
    ratio = float((err / bar).max()) if err.size else 0.0
    WORST[(what, name)] = ratio
    print(f"HESS_WORST {name} {what}: |got - ref| / bar = {ratio:.3g}")
    assert (err <= bar).all(), (what, name, ratio, np.argwhere(err > bar)[:3].tolist())


def _same(a, b):
    import torch

    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---- 1. identities with the first-order entry and values against the reference -----------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_values_and_identities(name):
    import torch

    d = _data(name)
    Fd, _ = _field(d)
    vox = _vox(d)
    scores, tg, th, ag, ah = _call(vox, d, Fd)
    for x, shape in ((scores, (d["B"],)), (tg, (d["B"], 6)), (th, (d["B"], 6, 6)), (ag, (d["N"], 3)), (ah, (d["N"], 6))):
        assert x.dtype == torch.float64 and x.is_cuda and tuple(x.shape) == shape and not x.requires_grad
    if name != "types":  # without the rows: they live in workspace, the same bits
        assert _same(_call(vox, d, Fd, per_atom=False), (scores, tg, th))
    # the scores are the first-order entry's bits; its dS/dcoords is M^T atom_grad: the same bits without a rotation
    S1, gc = _first_order(d, Fd)
    assert torch.equal(scores, S1)
    ref = _reference(name)
    rel, abs_ = _bars(d["kind"])
    if not d["posed"]:
        assert torch.equal(ag, gc)
    else:
        g = ag.cpu().numpy()
        for b in range(d["B"]):
            lo, hi = int(d["off"][b]), int(d["off"][b + 1])
            M = pr.rotation(d["q"][b])
            _close(g[lo:hi] @ M, gc.cpu().numpy()[lo:hi], ref["g"][1][lo:hi] @ np.abs(M), rel, abs_, f"M^T atom_grad mol {b}", name)
    binary = d["density"] == "binary"
    if binary:
        for x in (ag, ah, tg, th):
            assert torch.equal(x, torch.zeros_like(x))
        assert (scores != 0).all()
        assert not ref["g"][0].any() and not ref["H"][0].any()
    else:
        assert np.count_nonzero(ref["H"][1][:, 0]) > 0.5 * d["N"]
        _close(ag.cpu().numpy(), ref["g"][0], ref["g"][1], rel, abs_, "atom_grad", name)
        _close(ah.cpu().numpy(), ref["H"][0], ref["H"][1], rel, abs_, "atom_hess", name)
        _close(tg.cpu().numpy(), ref["G"], ref["bG"], rel, abs_, "twist_grad", name)
        _close(th.cpu().numpy(), ref["X"], ref["bX"], rel, abs_, "twist_hess", name)
    assert torch.equal(th, th.transpose(1, 2))  # symmetric to the bit
    # atoms the reference admits nowhere, the type beyond the channels, molecules without atoms: exact zeros
    dead = torch.tensor(ref["s"][1] == 0.0, device="cuda")
    assert not ag[dead].any() and not ah[dead].any()
    if name == "types":
        assert int((d["chan"] >= d["C"]).sum()) == 1 and bool(dead[int(np.argmax(d["chan"] >= d["C"]))])
    for b, n in enumerate(d["sizes"]):
        if n == 0:
            assert scores[b] == 0 and not tg[b].any() and not th[b].any()


def test_unrotated_features_rows_are_the_first_order_bits():
    import torch

    d = dict(_data("base"), posed=False)  # (the base case with centres only)
    Fd, _ = _field(d)
    scores, tg, th, ag, ah = _call(_vox(d), d, Fd)
    S1, gc = _first_order(d, Fd)
    assert torch.equal(scores, S1) and torch.equal(ag, gc) and ag.any()


def test_a_call_without_atoms_gives_zeros():
    import torch

    d = _data("base")
    vox = _vox(d)
    Fd, _ = _field(d)
    empty = dict(d, sizes=(0, 0), off=np.zeros(3, np.int64), xyz=d["xyz"][:0], chan=d["chan"][:0], radii=d["radii"][:0], cen=d["cen"][:2],
                 q=d["q"][:2], t=d["t"][:2], B=2, N=0)
    scores, tg, th, ag, ah = _call(vox, empty, Fd)
    assert tuple(scores.shape) == (2,) and tuple(tg.shape) == (2, 6) and tuple(th.shape) == (2, 6, 6)
    assert tuple(ag.shape) == (0, 3) and tuple(ah.shape) == (0, 6)
    for x in (scores, tg, th):
        assert torch.equal(x, torch.zeros_like(x))


# ---- 2. determinism and batch independence -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_two_runs_and_one_molecule_calls_give_the_same_bits(name):
    import torch

    d = _data(name)
    Fd, _ = _field(d)
    vox = _vox(d)
    first = _call(vox, d, Fd)
    assert _same(_call(vox, d, Fd), first)
    scores, tg, th, ag, ah = first
    for b in range(d["B"]):
        one = _sub(d, b)
        s1, tg1, th1, ag1, ah1 = _call(vox, one, _field(one)[0])
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        assert torch.equal(s1[0], scores[b]) and torch.equal(tg1[0], tg[b]) and torch.equal(th1[0], th[b])
        assert torch.equal(ag1, ag[lo:hi]) and torch.equal(ah1, ah[lo:hi])


# ---- 3. pivots -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["base", "types", "single"])
def test_pivots(name):
    d = _data(name)
    Fd, _ = _field(d)
    vox = _vox(d)
    ref = _reference(name)
    default = _call(vox, d, Fd)
    assert _same(_call(vox, d, Fd, pivots=ref["piv"]), default)  # an explicit pivot equal to the default: the same bits
    shift = np.random.default_rng(4).uniform(-1.0, 1.0, (d["B"], 3))
    scores, tg, th, ag, ah = _call(vox, d, Fd, pivots=ref["piv"] + shift)
    G0, G1 = default[1].cpu().numpy(), tg.cpu().numpy()
    rel, abs_ = _bars(d["kind"])
    assert np.array_equal(G1[:, :3], G0[:, :3])  # G_tau does not depend on the pivot
    want = G0[:, 3:] - np.cross(shift, G0[:, :3])
    bound = ref["bG"][:, 3:] + np.abs(shift)[:, [1, 2, 0]] * ref["bG"][:, [2, 0, 1]] + np.abs(shift)[:, [2, 0, 1]] * ref["bG"][:, [1, 2, 0]]
    _close(G1[:, 3:], want, bound, rel, abs_, "G_omega under a shifted pivot", name)
    # ... and the whole Hessian about the shifted pivot against the reference's
    p = ref["p"]
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        G, bG, X, bX = hr.twist(p[lo:hi], ref["g"][0][lo:hi], ref["H"][0][lo:hi], ref["piv"][b] + shift[b], ref["g"][1][lo:hi], ref["H"][1][lo:hi])
        _close(th[b].cpu().numpy(), X, bX, rel, abs_, f"twist_hess under a shifted pivot mol {b}", name)


# ---- 4. atoms that reach no voxel ------------------------------------------------------------------------------------------------
def _with_dead_rows(d):
    """The base case with three rows appended to molecule 1: a NaN coordinate, a radius of 0 and a coordinate of 9999.999."""
    at = int(d["off"][2])
    near = d["cen"][1]
    rows = np.array([[np.nan, near[1], near[2]], near + 0.1, [9999.999, near[1], near[2]]])
    rng = np.random.default_rng(8)
    xyz = np.insert(d["xyz"], [at] * 3, rows, axis=0)
    chan = np.insert(d["chan"], [at] * 3, rng.standard_normal((3, d["C"])).astype(d["chan"].dtype), axis=0)
    radii = np.insert(d["radii"], [at] * 3, np.array([1.2, 0.0, 1.2], d["radii"].dtype))
    sizes = (d["sizes"][0], d["sizes"][1] + 3, d["sizes"][2])
    return dict(d, xyz=xyz, chan=chan, radii=radii, sizes=sizes, off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64),
                N=d["N"] + 3), np.arange(at, at + 3)


def _dead_rows_check(d, dirty, dead):
    import torch

    Fd, _ = _field(d)
    vox = _vox(d)
    clean, keep = _without(dirty, dead)
    s0, tg0, th0, ag0, ah0 = _call(vox, clean, Fd)
    s1, tg1, th1, ag1, ah1 = _call(vox, dirty, Fd)
    live = torch.tensor(keep, device="cuda")
    assert not ag1[~live].any() and not ah1[~live].any() and not torch.signbit(ag1[~live]).any()  # exact zeros
    assert torch.equal(s1, s0) and torch.equal(tg1, tg0) and torch.equal(th1, th0)
    assert torch.equal(ag1[live], ag0) and torch.equal(ah1[live], ah0)
    assert torch.isfinite(tg1).all() and torch.isfinite(th1).all() and tg1.any()
    return vox, Fd, (s1, tg1, th1, ag1, ah1)


def test_dead_rows_are_zero_and_change_no_other_bit():
    d = _data("base")
    dirty, dead = _with_dead_rows(d)
    vox, Fd, got = _dead_rows_check(d, dirty, dead)
    # the same under a non-finite quaternion for the molecule without atoms
    q = dirty["q"].copy()
    q[0] = [np.nan, 1.0, np.inf, 0.0]
    assert dirty["sizes"][0] == 0
    again = _call(vox, dict(dirty, q=q), Fd)
    assert _same(again, got) and not again[1][0].any() and not again[2][0].any() and again[0][0] == 0


def test_a_type_beyond_the_channels_is_a_dead_row():
    d = _data("types")
    _dead_rows_check(d, d, np.flatnonzero(d["chan"] >= d["C"]))


# ---- 5. a Newton step is a step ---------------------------------------------------------------------------------------------------
def test_one_undamped_newton_step_raises_the_score_and_lowers_the_gradient():
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import apply_twist

    d = _sub(_data("single"), 0)
    vox = _vox(d)
    xyz, cen = hip.dev(d["xyz"]), hip.dev(d["cen"])
    q0 = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64, device="cuda")
    t0 = torch.zeros((1, 3), dtype=torch.float64, device="cuda")
    field = vox.forward_posed_batch(xyz, d["off"], cen, q0, t0, None, d["radii"])[0]  # the molecule's own grid at the identity pose
    axis = np.array([1.0, -2.0, 2.0]) / 3.0
    start = torch.tensor(np.concatenate([0.02 * np.array([2.0, 1.0, -2.0]) / 3.0, np.deg2rad(0.5) * axis])[None], device="cuda")

    def at(q, t):
        S, G, H = vox.score_hessian_posed_batch(xyz, d["off"], cen, q, t, None, d["radii"], field)
        return S, G, H

    q1, t1 = apply_twist(q0, t0, start)
    S1, G1, H1 = at(q1, t1)
    xi = torch.linalg.solve(-H1, G1)
    q2, t2 = apply_twist(q1, t1, xi)
    S2, G2, _ = at(q2, t2)
    Sbest = at(q0, t0)[0]
    n1, n2 = float(torch.linalg.vector_norm(G1)), float(torch.linalg.vector_norm(G2))
    print(f"NEWTON_STEP score {float(S1):.9g} -> {float(S2):.9g} (identity pose {float(Sbest):.9g}); |G| {n1:.3g} -> {n2:.3g}: "
          f"ratio {n2 / n1:.3g}")
    assert float(S2) > float(S1)
    assert n2 < n1


# ---- 6. what is judged against the handle ---------------------------------------------------------------------------------------
def test_a_bad_stride_is_rejected_before_the_entrys_own_rules():
    d = _data("base")
    vox = _vox(d)
    P = 16  # (a non-null pointer: nothing behind it is read)
    off = np.array([0, 3], np.int64)

    def entry(stride, radii_type=1, twist_grad=P):
        rc = vox._lib.mvx_score_hessian_batch(vox._handle, 0, P, P, P, 1.0, radii_type, off.ctypes.data, None, 1, 5, P, stride, None, P, None,
                                              None, twist_grad, P, None)
        return rc, last_error()

    rc, msg = entry(7, radii_type=2, twist_grad=None)
    assert rc == -1 and "field_mol_stride" in msg, (rc, msg)
    rc, msg = entry(5 * D ** 3, radii_type=2, twist_grad=None)
    assert rc == -1 and "channel-wise radii in features mode" in msg, (rc, msg)
    rc, msg = entry(0, twist_grad=None)
    assert rc == -1 and "twist_hess needs twist_grad" in msg, (rc, msg)
