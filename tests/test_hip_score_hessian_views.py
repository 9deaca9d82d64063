"""Second-order scores of views on the GPU (score_hessian_views / score_hessian_posed_views, mvx_score_hessian_views) and the
refinement drivers built on them (refine_posed_views / refine_posed_batch). One cloud of 130 atoms at D = 16, resolution 0.5, and
six views of it: view 0 keeps the whole cloud, view 1 none, view 2 at least 65 atoms, views 3 - 5 partial sets under explicit
poses (unit and unnormalised quaternions):

    case    mode      C   radii      field     grid
    feat    features  5   atom-wise  shared    f32
    wide    features  33  scalar     per view  f32     (two channel chunks)
    types   types     4   by type    shared    bf16
    single  single    1   scalar     shared    f64
    binary  types     3   atom-wise  shared    f32     (binary density)

To the bit: every output against score_hessian_posed_batch / score_hessian_batch on coords[index] with the selection's offsets;
the call without an index against the call with the selection; the rows of kept atoms and the whole-cloud view's per-view outputs
against the cloud repeated six times; twist_hess against its transpose; two runs; an explicit pivot equal to the default; the empty
view and a cloud without atoms; dead rows. Within the bars of tests/test_hip_score_hessian.py (GRAD_REL * bound + GRAD_ABS, GRAD64_*
at precision 64): all four outputs against tests/hessian_reference.py per view, and on unrotated views views_reduce of atom_grad
(width 3) and atom_hess (width 6) against the float64 sum of the reference's rows per shared atom. Worst error / bar with -s.
(MI355X, DESIGN.md section 26, profiles/r21_refine.txt: atom_grad 0.033, atom_hess 0.033, twist_grad 9.7e-4, twist_hess 1.0e-3,
views_reduce of atom_grad 3.1e-3 and of atom_hess 2.9e-3; the first trial pose 2.5e-5 of its bar. 18 cases in 4.4 s.)

The refinement: the rows of tests/test_lm_host.py's CPU loop (8 poses, 12 rounds, the molecule of the Newton step of
tests/test_hip_score_hessian.py) through both drivers.
"""
import functools

import numpy as np
import pytest

from tests import hessian_reference as hr
from tests import lm_rows as R
from tests import pose_reference as pr
from tests import hip_support as hip
from tests.abi import last_error
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

D, N, B = 16, 130, 6
CEN = np.array([30.0, -20.0, 12.0])
CASES = {
    "feat": dict(mode="features", C=5, radii_type="atom-wise", per_view=False, kind="f32"),
    "wide": dict(mode="features", C=33, radii_type="scalar", per_view=True, kind="f32"),
    "types": dict(mode="types", C=4, radii_type="channel-wise", per_view=False, kind="bf16"),
    "single": dict(mode="single", C=1, radii_type="scalar", per_view=False, kind="f64"),
    "binary": dict(mode="types", C=3, radii_type="atom-wise", per_view=False, kind="f32", density="binary"),
}


def _bars(kind):
    return (GRAD64_REL, GRAD64_ABS) if kind == "f64" else (GRAD_REL, GRAD_ABS)


@functools.lru_cache(maxsize=None)
def _data(name, seed=41):
    """The cloud and the six views of a case as host arrays (never modified)."""
    c = dict(CASES[name])
    c.setdefault("density", "gaussian")
    rng = np.random.default_rng(seed)
    fp = np.float64 if c["kind"] == "f64" else np.float32
    C_ = c["C"]
    xyz = CEN + rng.uniform(-3.0, 3.0, (N, 3))  # inside the box of the centred view: 3.75 A to each side
    cen = np.tile(CEN, (B, 1))
    cen[1] += 60.0                               # empty space
    cen[2] += [2.5, 0.0, 0.0]
    cen[3:] += rng.choice([-1.0, 1.0], (B - 3, 3)) * rng.uniform(2.5, 4.5, (B - 3, 3))  # partial sets, rotated or not
    q = np.tile([1.0, 0.0, 0.0, 0.0], (B, 1))
    q[3:] = rng.standard_normal((B - 3, 4))
    q[3:] *= (np.array([1.0, 1.1, 0.9]) / np.linalg.norm(q[3:], axis=1))[:, None]
    t = np.zeros((B, 3))
    t[3:] = rng.uniform(-0.5, 0.5, (B - 3, 3))
    chan = {"features": rng.standard_normal((N, C_)).astype(fp), "types": rng.integers(0, C_, N), "single": None}[c["mode"]]
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(fp), "channel-wise": rng.uniform(1.0, 1.5, C_).astype(fp)}[c["radii_type"]]
    F = rng.standard_normal(((B,) if c["per_view"] else ()) + (C_,) + (D,) * 3)
    for x in (xyz, cen, q, t, F):
        x.setflags(write=False)
    return dict(c, name=name, xyz=xyz, cen=cen, q=q, t=t, chan=chan, radii=radii, F=F)


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


def _views(vox, d, Fd, posed=True, per_atom=True, pivots=None):
    a = {k: hip.dev(d[k]) for k in ("xyz", "cen", "q", "t", "chan", "radii")}
    if posed:
        return vox.score_hessian_posed_views(a["xyz"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], Fd, num_channels=hip.nc(d),
                                             pivots=hip.dev(pivots), per_atom=per_atom)
    return vox.score_hessian_views(a["xyz"], a["cen"], a["chan"], a["radii"], Fd, num_channels=hip.nc(d), pivots=hip.dev(pivots), per_atom=per_atom)


def _take(x, index):
    return x if (x is None or np.isscalar(x)) else x[index]


def _batch(vox, d, Fd, index, offsets, posed=True, pivots=None):
    """The same records on the gathered rows: (scores, twist_grad, twist_hess, atom_grad, atom_hess)."""
    a = {k: hip.dev(d[k]) for k in ("xyz", "cen", "q", "t", "chan", "radii")}
    r = _take(a["radii"], index) if d["radii_type"] == "atom-wise" else a["radii"]
    xyz, chan = a["xyz"][index], _take(a["chan"], index)
    if posed:
        return vox.score_hessian_posed_batch(xyz, offsets, a["cen"], a["q"], a["t"], chan, r, Fd, num_channels=hip.nc(d), pivots=hip.dev(pivots),
                                             per_atom=True)
    return vox.score_hessian_batch(xyz, offsets, a["cen"], chan, r, Fd, num_channels=hip.nc(d), pivots=hip.dev(pivots), per_atom=True)


def _repeated(vox, d, Fd, posed=True):
    """The cloud repeated B times through the batch entry."""
    import torch

    index = torch.arange(N, device="cuda").repeat(B)
    return _batch(vox, d, Fd, index, np.arange(B + 1, dtype=np.int64) * N, posed)


def _same(a, b):
    import torch

    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _check_layout(offsets):
    n = np.diff(offsets)
    assert n[0] == N and n[1] == 0 and 65 <= n[2] < N and (n[3:] > 0).all() and (n[3:] < N).all(), n.tolist()
    return n


def _close(got, ref, bound, rel, abs_, what, name):
    err = np.abs(np.asarray(got, np.float64) - ref)
    bar = rel * bound + abs_
    ratio = float((err / bar).max()) if err.size else 0.0
    print(f"HESS_VIEWS_WORST {name} {what}: |got - ref| / bar = {ratio:.3g}")
    assert (err <= bar).all(), (what, name, ratio, np.argwhere(err > bar)[:3].tolist())


def _view_positions(d, b, idx, posed):
    if posed:
        return pr.positions(d["xyz"][idx], d["cen"][b], d["q"][b], d["t"][b])
    return d["xyz"][idx] - d["cen"][b]


def _view_reference(d, Fref, b, idx, posed):
    """tests/hessian_reference.py on the atoms `idx` of view b: ({s, g, H}, positions)."""
    p = _view_positions(d, b, idx, posed)
    r = d["radii"][idx] if d["radii_type"] == "atom-wise" else d["radii"]
    ref = hr.reference(p, Fref[b] if d["per_view"] else Fref, r, d["radii_type"],
                       w=None if d["mode"] != "features" else d["chan"][idx].astype(np.float64), mode=d["mode"],
                       types=d["chan"][idx] if d["mode"] == "types" else None, density=d["density"],
                       precision=64 if d["kind"] == "f64" else 32)
    return ref, p


# ---- 1. the bits of the batch entry, and the values of the reference -------------------------------------------------------------
@pytest.mark.parametrize("posed", [True, False])
@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_batch_entry_and_values_of_the_reference(name, posed):
    import torch

    d = _data(name)
    Fd, Fref = _field(d)
    vox = _vox(d)
    scores, tg, th, ag, ah, index, offsets = _views(vox, d, Fd, posed)
    n = _check_layout(offsets)
    total = int(offsets[-1])
    for x, shape in ((scores, (B,)), (tg, (B, 6)), (th, (B, 6, 6)), (ag, (total, 3)), (ah, (total, 6))):
        assert x.dtype == torch.float64 and x.is_cuda and tuple(x.shape) == shape and not x.requires_grad
    # the batch entry on the gathered rows; the call that selects itself; a second run
    assert _same(_batch(vox, d, Fd, index, offsets, posed), (scores, tg, th, ag, ah))
    assert _same(_views(vox, d, Fd, posed, per_atom=False), (scores, tg, th))
    again = _views(vox, d, Fd, posed)
    assert _same(again[:5], (scores, tg, th, ag, ah)) and torch.equal(again[5], index) and np.array_equal(again[6], offsets)
    assert torch.equal(th, th.transpose(1, 2))  # symmetric to the bit
    # an explicit pivot equal to the default
    piv = d["t"].astype(np.float32).astype(np.float64) if posed else np.zeros((B, 3))
    assert _same(_views(vox, d, Fd, posed, pivots=piv)[:5], (scores, tg, th, ag, ah))
    # the cloud repeated: the rows of kept atoms, and what the whole-cloud view sums
    rs, rtg, rth, rag, rah = _repeated(vox, d, Fd, posed)
    slot = index + torch.tensor(np.repeat(np.arange(B) * N, n), device="cuda")
    assert torch.equal(ag, rag[slot]) and torch.equal(ah, rah[slot])
    assert torch.equal(scores[0], rs[0]) and torch.equal(tg[0], rtg[0]) and torch.equal(th[0], rth[0])
    # the empty view
    assert scores[1] == 0 and not tg[1].any() and not th[1].any()
    # the reference, view by view
    idx = index.cpu().numpy()
    binary = d["density"] == "binary"
    rel, abs_ = _bars(d["kind"])
    g, H = ag.cpu().numpy(), ah.cpu().numpy()
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi == lo:
            continue
        ref, p = _view_reference(d, Fref, b, idx[lo:hi], posed)
        G, bG, X, bX = hr.twist(p, ref["g"][0], ref["H"][0], piv[b], ref["g"][1], ref["H"][1])
        if binary:
            assert not ref["g"][0].any() and not ref["H"][0].any()
            continue
        assert np.count_nonzero(ref["H"][1][:, 0]) > 0
        _close(g[lo:hi], ref["g"][0], ref["g"][1], rel, abs_, f"atom_grad view {b}", name)
        _close(H[lo:hi], ref["H"][0], ref["H"][1], rel, abs_, f"atom_hess view {b}", name)
        _close(tg[b].cpu().numpy(), G, bG, rel, abs_, f"twist_grad view {b}", name)
        _close(th[b].cpu().numpy(), X, bX, rel, abs_, f"twist_hess view {b}", name)
    if binary:
        for x in (ag, ah, tg, th):
            assert torch.equal(x, torch.zeros_like(x))
        assert (scores[[0, 2, 3, 4, 5]] != 0).all()


# ---- 2. the rows summed back onto the shared atoms, on unrotated views -------------------------------------------------------------
@pytest.mark.parametrize("name", ["feat", "types", "single"])
def test_views_reduce_of_the_rows_against_the_reference_per_shared_atom(name):
    d = _data(name)
    Fd, Fref = _field(d)
    vox = _vox(d)
    scores, tg, th, ag, ah, index, offsets = _views(vox, d, Fd, posed=False)
    sum_g, sum_H = vox.views_reduce(ag, index, offsets, N), vox.views_reduce(ah, index, offsets, N)
    assert tuple(sum_g.shape) == (N, 3) and tuple(sum_H.shape) == (N, 6)
    idx = index.cpu().numpy()
    want = {k: (np.zeros((N, w)), np.zeros((N, w))) for k, w in (("g", 3), ("H", 6))}
    held = np.zeros(N, np.int64)
    for b in range(B):
        lo, hi = int(offsets[b]), int(offsets[b + 1])
        if hi == lo:
            continue
        ref, _ = _view_reference(d, Fref, b, idx[lo:hi], posed=False)
        held[idx[lo:hi]] += 1
        for k in want:
            want[k][0][idx[lo:hi]] += ref[k][0]
            want[k][1][idx[lo:hi]] += ref[k][1]
    assert held.max() >= 3 and held.min() >= 1  # (view 0 holds every atom; most atoms lie in several views)
    rel, abs_ = _bars(d["kind"])
    _close(sum_g.cpu().numpy(), want["g"][0], want["g"][1], rel, abs_, "views_reduce(atom_grad)", name)
    _close(sum_H.cpu().numpy(), want["H"][0], want["H"][1], rel, abs_, "views_reduce(atom_hess)", name)


# ---- 3. no atoms, dead rows ---------------------------------------------------------------------------------------------------------
def test_a_cloud_without_atoms_gives_zeros():
    import torch

    d = _data("feat")
    vox = _vox(d)
    Fd, _ = _field(d)
    empty = dict(d, xyz=d["xyz"][:0], chan=d["chan"][:0], radii=d["radii"][:0])
    for posed in (True, False):
        for per_atom in (True, False):
            out = _views(vox, empty, Fd, posed, per_atom=per_atom)
            scores, tg, th = out[:3]
            assert tuple(scores.shape) == (B,) and tuple(tg.shape) == (B, 6) and tuple(th.shape) == (B, 6, 6)
            for x in (scores, tg, th):
                assert torch.equal(x, torch.zeros_like(x))
            if per_atom:
                assert tuple(out[3].shape) == (0, 3) and tuple(out[4].shape) == (0, 6) and out[5].numel() == 0 and not out[6].any()


def test_dead_rows_are_zero_and_change_no_other_bit():
    """Two atoms appended to the cloud, next to the centre of the whole-cloud view: a NaN coordinate and a radius of 0."""
    import torch

    d = _data("feat")
    vox = _vox(d)
    Fd, _ = _field(d)
    rng = np.random.default_rng(8)
    rows = np.array([[np.nan, CEN[1], CEN[2]], CEN + 0.1])
    dirty = dict(d, xyz=np.concatenate([d["xyz"], rows]), chan=np.concatenate([d["chan"], rng.standard_normal((2, d["C"])).astype(np.float32)]),
                 radii=np.concatenate([d["radii"], np.array([1.2, 0.0], np.float32)]))
    s0, tg0, th0, ag0, ah0, i0, o0 = _views(vox, d, Fd)
    s1, tg1, th1, ag1, ah1, i1, o1 = _views(vox, dirty, Fd)
    assert torch.equal(s1, s0) and torch.equal(tg1, tg0) and torch.equal(th1, th0)
    assert torch.isfinite(tg1).all() and torch.isfinite(th1).all() and tg1.any()
    live = i1 < N
    assert torch.equal(i1[live], i0) and torch.equal(ag1[live], ag0) and torch.equal(ah1[live], ah0)
    assert not ag1[~live].any() and not ah1[~live].any() and not torch.signbit(ag1[~live]).any()
    print(f"HESS_VIEWS dead rows selected: {int((~live).sum())}")
    assert _same(_views(vox, dirty, Fd, per_atom=False), (s0, tg0, th0))


# ---- 4. what is judged against the handle ------------------------------------------------------------------------------------------
def test_a_bad_stride_is_rejected_before_the_entrys_own_rules():
    from molvoxel_amd.voxelizer.hip import _lib
    import ctypes as C

    d = _data("feat")
    vox = _vox(d)
    P = 16  # (a non-null pointer: nothing behind it is read)
    xfs = (_lib.MvxXform * 1)()

    def entry(stride, radii_type=1, twist_grad=P):
        rc = vox._lib.mvx_score_hessian_views(vox._handle, 0, P, P, P, 1.0, radii_type, 3, 5, C.addressof(xfs), 1, None, None, P, stride, None, P,
                                              None, None, twist_grad, P, None)
        return rc, last_error()

    rc, msg = entry(7, radii_type=2, twist_grad=None)
    assert rc == -1 and "field_view_stride" in msg, (rc, msg)
    rc, msg = entry(5 * D ** 3, radii_type=2, twist_grad=None)
    assert rc == -1 and "channel-wise radii in features mode" in msg, (rc, msg)
    rc, msg = entry(0, twist_grad=None)
    assert rc == -1 and "twist_hess needs twist_grad" in msg, (rc, msg)


# ---- 5. refinement: the rows of the CPU loop through both drivers ------------------------------------------------------------------
def _refine_setup():
    import molvoxel_amd as mv
    import torch

    xyz, cen, D_ = R.refine_molecule()
    vox = mv.create_voxelizer(0.5, D_, "scalar", "gaussian", library="hip", precision=64)
    q0, t0 = R.refine_starts()
    P_ = R.REFINE_POSES
    xyz_d, cen_d = torch.tensor(xyz, device="cuda"), torch.tensor(cen, device="cuda")
    ident = torch.tensor([[1.0, 0.0, 0.0, 0.0]], dtype=torch.float64, device="cuda")
    zero = torch.zeros((1, 3), dtype=torch.float64, device="cuda")
    off1 = np.array([0, xyz.shape[0]], np.int64)
    own = vox.forward_posed_batch(xyz_d, off1, cen_d, ident, zero, None, R.REFINE_RADIUS)[0]  # the molecule's own grid ...
    field = torch.tensor(R.cpu_field(), device="cuda")  # ... as the CPU loop builds it: both loops read the same field
    assert float((own - field).abs().max()) <= 1e-12
    return vox, xyz_d, cen_d.repeat(P_, 1), torch.tensor(q0, device="cuda"), torch.tensor(t0, device="cuda"), field


def test_refinement_through_both_drivers():
    import torch

    vox, xyz, cen, q0, t0, field = _refine_setup()
    P_, n = R.REFINE_POSES, xyz.shape[0]
    kw = dict(steps=R.REFINE_ROUNDS, lam_down=R.LAM_DOWN, lam_up=R.LAM_UP, max_dropped=R.MAX_DROPPED)
    keep_q, keep_t = q0.clone(), t0.clone()
    qv, tv, Sv, iv = vox.refine_posed_views(xyz, cen, q0, t0, None, R.REFINE_RADIUS, field, **kw)
    qb, tb, Sb, ib = vox.refine_posed_batch(xyz.repeat(P_, 1), np.arange(P_ + 1, dtype=np.int64) * n, cen, q0, t0, None, R.REFINE_RADIUS,
                                            field, **kw)
    assert torch.equal(q0, keep_q) and torch.equal(t0, keep_t)  # the input poses are not modified
    # every view keeps the whole cloud: the two forms give the same bits
    _, offsets = vox.select_posed_views(xyz, cen, q0, t0, None, R.REFINE_RADIUS)
    assert (np.diff(offsets) == n).all()
    assert torch.equal(iv["score_history"], ib["score_history"])
    assert torch.equal(qv, qb) and torch.equal(tv, tb) and torch.equal(Sv, Sb)
    for k in ("lam", "taken", "dropped"):
        assert torch.equal(iv[k], ib[k]), k
    q0h, t0h = R.refine_starts()
    for q, t, S, info in ((qv, tv, Sv, iv), (qb, tb, Sb, ib)):
        hist = info["score_history"].cpu().numpy()
        assert tuple(hist.shape) == (R.REFINE_ROUNDS + 1, P_) and info["evaluations"] == R.REFINE_ROUNDS + 1
        assert np.array_equal(hist[-1], S.cpu().numpy())
        assert info["taken"].dtype == torch.int32 and info["dropped"].dtype == torch.int32 and tuple(info["lam"].shape) == (P_,)
        a0, a1, s0, s1 = R.refine_conditions(hist, info["taken"].cpu().numpy(), q0h, t0h, q.cpu().numpy(), t.cpu().numpy())
    print(f"LM_GPU_REFINE taken {iv['taken'].tolist()} dropped {iv['dropped'].tolist()}; rotation {a0.max():.2f} -> {a1.max():.3f} deg at "
          f"most, shift {s0.max():.3f} -> {s1.max():.4f} A at most")


def test_the_first_trial_pose_is_the_cpu_loops():
    """One lm_step from the start evaluation, as the drivers take it, against the CPU loop's first trial. The bar follows the
    evaluation's own bars through the solve: with dG and dA the GRAD64 bars of G and of A = -H + lam I (lam = 1e-3 max|H|, so
    its bar is 1e-3 of H's largest), xi moves by at most 2 ||A^-1||_inf (||dG||_inf + ||dA||_inf ||xi||_inf) to first order with a
    factor 2 for the rest; t2 by that, q2 by half of it times |q|; each plus the 8 * 2^-52 of the step kernel's own arithmetic."""
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import LMState

    vox, xyz, cen, q0, t0, field = _refine_setup()
    q0h, t0h = R.refine_starts()
    S, G, H = vox.score_hessian_posed_views(xyz, cen, q0, t0, None, R.REFINE_RADIUS, field)
    lam = 1e-3 * H.abs().reshape(-1, 36).amax(dim=1)
    st = vox.lm_step(LMState(q0.clone(), t0.clone(), S.clone(), G.clone(), H.clone(), lam), lam_down=R.LAM_DOWN, lam_up=R.LAM_UP,
                     max_dropped=R.MAX_DROPPED)
    _, _, (q2, t2) = R.cpu_refinement()
    Sc, Gc, Hc, bG, bH = R.cpu_evaluate(q0h, t0h, bounds=True)
    got_q, got_t, xi = st.q2.cpu().numpy(), st.t2.cpu().numpy(), st.xi.cpu().numpy()
    worst = 0.0
    for b in range(R.REFINE_POSES):
        lam_b = 1e-3 * np.abs(Hc[b]).max()
        A = lam_b * np.eye(6) - Hc[b]
        dG = (GRAD64_REL * bG[b] + GRAD64_ABS).max()
        dH = GRAD64_REL * bH[b] + GRAD64_ABS
        dA = dH.sum(axis=1).max() + 1e-3 * dH.max()
        x = np.linalg.solve(A, Gc[b])
        dxi = 2.0 * np.abs(np.linalg.inv(A)).sum(axis=1).max() * (dG + dA * np.abs(x).max())
        bar_t = dxi + 8 * 2.0 ** -52 * (np.abs(t0h[b]).max() + np.abs(x).max())
        bar_q = (0.5 * np.sqrt(3.0) * dxi + 8 * 2.0 ** -52) * np.linalg.norm(q0h[b])
        eq, et = np.abs(got_q[b] - q2[b]).max(), np.abs(got_t[b] - t2[b]).max()
        worst = max(worst, eq / bar_q, et / bar_t)
        assert eq <= bar_q and et <= bar_t, (b, eq, bar_q, et, bar_t)
        assert np.abs(x).max() > 1e-3 and np.abs(xi[b] - x).max() <= dxi
    print(f"LM_FIRST_TRIAL worst error / bar {worst:.3g}")
    assert torch.isfinite(st.xi).all()
