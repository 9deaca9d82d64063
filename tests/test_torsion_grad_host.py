"""The adjoint of the conformer without a GPU: the numpy reference (tests/torsion_grad_reference.py) against central finite
differences of a smooth function of C(theta), its two forms against each other within the bar of the GPU test, the shortcut for
the angle gradients, inert torsions and an atom without a row, the C ABI entry mvx_apply_torsions_backward against the header and
the ctypes table, every rejection and its order, what the Python layer refuses before it needs the library, the kernel's
resources read from mvx_torsion_grad.o, and the conditions of the GPU refinement test on a numpy Adam loop.

Finite differences on the 12-atom tree (4 torsions, one branch, nesting depth 3), 4 angles and 36 coordinates: the worst error is
7.4e-5 / 7.4e-7 (angles) and 1.2e-5 / 1.2e-7 (coordinates) at h = 1e-3 / 1e-4 at random angles, 4.1e-4 / 4.1e-6 and 1.9e-6 /
1.9e-8 with every angle exactly 0 - the h^2 law, a factor of 100. Form (b), form (a) and form (a) on the pre-images of the
conformer against one another, worst difference over the bar (N_b + 128)(T_b + 1) 2^-53 bound: 0.0080 (base), 0.00065 (long),
0.00037 (deep); the shortcut 0.0010, 0.00019, 0.000095 of the same bar (deep: 8.7e-13 absolute at max |g| = 146). The numpy Adam
loop (learning rate 0.01, 20 steps): 8 starts, score 591.1 ... 616.5 -> 634.8 ... 641.3."""
import inspect
import os

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import flex_reference as fr
from tests import flex_rows as X
from tests import torsion_grad_reference as tg
from tests.abi import MVX_ERR_INVALID, P, call
from tests.fake_voxelizer import fake as _fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against finite differences -------------------------------------------------------------------------------
def _smooth(rng, N, J=3):
    """L(C) = sum_n sum_j a_nj sin(k_nj . C_n + phi_nj) and dL/dC."""
    al, kv, ph = rng.standard_normal((N, J)), 0.7 * rng.standard_normal((N, J, 3)), rng.uniform(0, 6, (N, J))

    def value(p):
        return float((al * np.sin(np.einsum("njk,nk->nj", kv, p) + ph)).sum())

    def grad(p):
        return np.einsum("nj,njk->nk", al * np.cos(np.einsum("njk,nk->nj", kv, p) + ph), kv)

    return value, grad


@pytest.mark.parametrize("zero", [False, True])
def test_the_reference_agrees_with_central_finite_differences_at_the_h2_rate(zero):
    rng = np.random.default_rng(3)
    p0, axes, moves = fr.tree_coords(rng), fr.TREE_AXES, fr.tree_moves()
    L, dL = _smooth(rng, 12)
    th0 = np.zeros(4) if zero else rng.uniform(-2, 2, 4)
    gc, ga, _, _ = tg.stored(p0, axes, moves, th0, dL(fr.apply_torsions(p0, axes, moves, th0)))
    assert ga.all() and gc.any(axis=1).all()  # (an angle of exactly 0 has its derivative all the same)
    err = {}
    for h in (1e-3, 1e-4):  # (truncation ~ h^2 |L'''| / 6 >= 1e-8 against rounding ~ 2^-53 |L| / h <= 1e-11)
        fa, fc = np.zeros(4), np.zeros((12, 3))
        for k in range(4):
            e = np.zeros(4)
            e[k] = h
            fa[k] = (L(fr.apply_torsions(p0, axes, moves, th0 + e)) - L(fr.apply_torsions(p0, axes, moves, th0 - e))) / (2 * h)
        for n in range(12):
            for i in range(3):
                e = np.zeros((12, 3))
                e[n, i] = h
                fc[n, i] = (L(fr.apply_torsions(p0 + e, axes, moves, th0)) - L(fr.apply_torsions(p0 - e, axes, moves, th0))) / (2 * h)
        err[h] = (np.abs(fa - ga).max(), np.abs(fc - gc).max())
        print(f"TORSION_GRAD_FD zero {int(zero)} h {h:g}: angle error {err[h][0]:.3g}, coordinate error {err[h][1]:.3g}, "
              f"max |grad| {np.abs(ga).max():.3g}, {np.abs(gc).max():.3g}")
    assert 50.0 <= err[1e-3][0] / err[1e-4][0] <= 200.0, err
    assert 50.0 <= err[1e-3][1] / err[1e-4][1] <= 200.0, err
    assert err[1e-4][0] <= 1e-6 * np.abs(ga).max() and err[1e-4][1] <= 1e-6 * np.abs(gc).max()


# ---- the two forms, the shortcut, inert torsions, an atom without a row ---------------------------------------------------------
def _molecules(name, seed=11):
    """Per molecule with atoms of a case of tests/flex_rows.py: (coords, axes, moves, angles, upstream rows)."""
    d = X.data(name)
    rng = np.random.default_rng(seed)
    ang, up = rng.uniform(-np.pi, np.pi, (d["B"], d["T"])), rng.standard_normal((d["N"], 3))
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi > lo:
            yield d["xyz"][lo:hi], d["axes"][b], d["moves"][lo:hi], ang[b], up[lo:hi]


@pytest.mark.parametrize("name", ("base", "long", "deep"))
def test_undoing_the_turns_agrees_with_the_stored_sweep_within_the_device_bar_and_the_shortcut_holds(name):
    worst = worst_s = 0.0
    for xyz, ax, mv, ang, up in _molecules(name):
        a = tg.stored(xyz, ax, mv, ang, up)
        conformer = fr.apply_torsions(xyz, ax, mv, ang)
        b = tg.undone(conformer, ax, mv, ang, up)
        bar = tg.bar_factor(xyz.shape[0], ax)
        c = tg.stored_from(conformer, ax, mv, ang, up)  # form (a) on the pre-images of a conformer that is given
        for got, ref, bound in ((b[0], a[0], a[2]), (b[1], a[1], a[3]), (c[0], a[0], a[2]), (c[1], a[1], a[3]), (b[0], c[0], c[2]), (b[1], c[1], c[3])):
            assert not got[bound == 0.0].any()
            err = np.abs(got - ref)
            assert (err <= bar * bound).all(), float((err / (bar * bound + 1e-300)).max())
            worst = max(worst, float((err / (bar * bound + 1e-300)).max()))
        err = np.abs(tg.shortcut_angles(conformer, ax, mv, up) - a[1])
        assert (err <= bar * a[3]).all(), float((err / (bar * a[3] + 1e-300)).max())
        worst_s = max(worst_s, float((err / (bar * a[3] + 1e-300)).max()))
    print(f"TORSION_GRAD_FORMS {name}: worst difference between the forms / bar {worst:.3g}, shortcut {worst_s:.3g}")
    assert worst > 0.0  # (the two forms round differently: the bar is measured, not met by identity)


def test_inert_torsions_in_the_reference_give_exact_zeros_and_leave_the_other_bits():
    rng = np.random.default_rng(5)
    p0, moves = fr.tree_coords(rng), fr.tree_moves().copy()
    moves[9:12] |= 1 << 4  # the fifth set is a live set: only its axis is not
    up, th = rng.standard_normal((12, 3)), np.array([0.3, -0.2, 0.5, 1.0, 0.7])
    want = tg.undone(fr.apply_torsions(p0, fr.TREE_AXES, moves, th[:4]), fr.TREE_AXES, moves, th[:4], up)
    for bad in ([-1, -1], [4, 12], [12, 4], [4, 4], [-3, 2]):
        axes = np.concatenate([fr.TREE_AXES, [bad]]).astype(np.int32)
        conformer = fr.apply_torsions(p0, axes, moves, th)
        for got in (tg.undone(conformer, axes, moves, th, up), tg.stored(p0, axes, moves, th, up)):
            assert got[1][4] == 0.0 and not np.signbit(got[1][4]) and got[3][4] == 0.0
        got = tg.undone(conformer, axes, moves, th, up)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1][:4], want[1])


def test_an_atom_without_a_row_may_have_nan_coordinates():
    rng = np.random.default_rng(6)
    p0, axes, moves = fr.tree_coords(rng), fr.TREE_AXES, fr.tree_moves()
    up, th = rng.standard_normal((12, 3)), rng.uniform(-2, 2, 4)
    up[11] = 0.0  # atom 11: a leaf of the branch, in the sets 0 and 3, on no axis
    conformer = fr.apply_torsions(p0, axes, moves, th)
    far, dead = conformer.copy(), conformer.copy()
    far[11] = [1e3, -2e3, 5e2]
    dead[11, 1] = np.nan
    want, got = tg.undone(far, axes, moves, th, up), tg.undone(dead, axes, moves, th, up)
    for a, b in zip(want, got):
        assert np.isfinite(b).all() and np.array_equal(a, b)
    assert not got[0][11].any() and got[1].all()
    p_dead = p0.copy()
    p_dead[11, 1] = np.nan
    stored = tg.stored(p_dead, axes, moves, th, up)
    assert all(np.isfinite(x).all() for x in stored) and not stored[0][11].any()


# ---- the entry against the header -----------------------------------------------------------------------------------------------
def test_the_entry_begins_like_apply_torsions():
    # the forward's arguments, with the conformer in place of coords, in front of the three gradients
    got, fwd = _lib.SIGNATURES["mvx_apply_torsions_backward"][1], _lib.SIGNATURES["mvx_apply_torsions"][1]
    assert got[:8] == fwd[:8] and got[-1] == fwd[-1]


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def _back(handle=None, conformer=P, offsets=(0, 3), B=1, T=2, axes=P, moves=P, angles=P, grad_out=P, grad_coords=P, grad_angles=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_apply_torsions_backward, handle, conformer, None if off is None else off.ctypes.data, B, T, axes, moves,
                angles, grad_out, grad_coords, grad_angles, None)


@pytest.mark.parametrize("kw, words", [
    (dict(B=-1), "B must be >= 0"), (dict(T=-1), "T must be 0 ... 32"), (dict(T=33), "T must be 0 ... 32"),
    (dict(offsets=None), "offsets must not be null"), (dict(offsets=(1, 3)), "offsets[0]"),
    (dict(B=2, offsets=(0, 3, 2)), "non-decreasing"), (dict(offsets=(0, 1 << 31)), "too many atoms"),
    (dict(conformer=None), "conformer / grad_out / grad_coords"), (dict(grad_out=None), "conformer / grad_out / grad_coords"),
    (dict(grad_coords=None), "conformer / grad_out / grad_coords"),
    (dict(axes=None), "with T > 0"), (dict(moves=None), "with T > 0"), (dict(angles=None), "with T > 0"),
    (dict(grad_angles=None), "with T > 0"),
    (dict(), "null handle"), (dict(T=0, axes=None, moves=None, angles=None, grad_angles=None), "null handle"),
    (dict(offsets=(0, 0), conformer=None, grad_out=None, grad_coords=None, axes=None), "null handle"),
])
def test_the_entry_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _back(**kw)
    assert rc == MVX_ERR_INVALID and words in msg, (rc, msg)


def test_the_rules_fire_in_the_order_of_apply_torsions_with_its_words():
    fwd = _lib.load().mvx_apply_torsions

    def forward(offsets=(0, 3), B=1, T=2, coords=P, axes=P):
        off = None if offsets is None else np.asarray(offsets, np.int64)
        return call(fwd, None, coords, None if off is None else off.ctypes.data, B, T, axes, P, P, P, None)

    # the rules the two entries share: the same words
    for kw in (dict(B=-1), dict(T=40), dict(offsets=None), dict(offsets=(1, 3)), dict(B=2, offsets=(0, 3, 2)), dict(offsets=(0, 1 << 31)),
               dict()):
        assert _back(**kw) == forward(**kw), kw
    assert "B must be" in _back(B=-1, T=40, offsets=None)[1]
    assert "T must be" in _back(T=40, offsets=None, conformer=None)[1]
    assert "offsets must not" in _back(offsets=None, conformer=None, axes=None)[1]
    assert "too many atoms" in _back(offsets=(0, 1 << 31), conformer=None, axes=None)[1]
    assert "conformer / grad_out / grad_coords" in _back(grad_out=None, grad_angles=None)[1]
    assert "with T > 0" in _back(grad_angles=None)[1]
    # a batch without atoms and no molecules: nothing to do
    assert _back(handle=P, offsets=(0, 0), conformer=None, grad_out=None, grad_coords=None)[0] == 0
    assert _back(handle=P, B=2, offsets=(0, 0, 0), conformer=None, grad_out=None, grad_coords=None, axes=None, grad_angles=None)[0] == 0
    assert _back(handle=P, B=0, offsets=None)[0] == 0


# ---- the Python layer ------------------------------------------------------------------------------------------------------------
def test_torsion_grad_is_a_constructor_option_that_needs_differentiable():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    init = inspect.signature(Voxelizer.__init__).parameters
    assert init["torsion_grad"].default is False
    with pytest.raises(ValueError, match="torsion_grad=True needs differentiable=True"):
        Voxelizer(0.5, 16, torsion_grad=True)  # (raised before anything touches a device)
    assert Voxelizer._tgrad is False
    par = lambda f: list(inspect.signature(f).parameters)  # noqa: E731
    assert par(Voxelizer.apply_torsions) == ["self", "coords", "offsets", "axes", "moves", "angles"]
    assert par(Voxelizer.apply_torsions_backward) == ["self", "conformer", "offsets", "axes", "moves", "angles", "grad"]
    assert "outside autograd;" not in Voxelizer.apply_torsions.__doc__ and "torsion_grad=True" in Voxelizer.apply_torsions.__doc__


def test_the_python_guards_fire_before_the_library_is_needed():
    import torch

    rng = np.random.default_rng(0)
    moves = np.zeros(6, np.int32)
    moves[2] = moves[5] = 1
    a = dict(coords=rng.uniform(-2, 2, (6, 3)), offsets=np.array([0, 3, 6]), axes=np.array([[[1, 2]], [[1, 2]]], np.int32), moves=moves)
    angles = np.zeros((2, 1))
    grad = np.ones((6, 3))
    a_back = {k: v for k, v in a.items() if k != "coords"}
    back = lambda v, **o: v.apply_torsions_backward(**{**dict(a_back, conformer=a["coords"], angles=angles, grad=grad), **o})  # noqa: E731
    with pytest.raises(ValueError, match="output='torch'"):
        back(_fake(output="numpy"))
    with pytest.raises(AssertionError, match="conformer should be"):
        back(_fake(), conformer=np.zeros((6, 2)))
    with pytest.raises(AssertionError, match="grad does not match dimension"):
        back(_fake(), grad=np.ones((5, 3)))
    with pytest.raises(AssertionError, match="offsets must span conformer"):
        back(_fake(), offsets=np.array([0, 3, 5]))
    with pytest.raises(AssertionError, match="angles does not match dimension"):
        back(_fake(), angles=np.zeros((2, 3)))
    with pytest.raises(AssertionError, match="axes does not match dimension"):
        back(_fake(), axes=np.zeros((3, 1, 2), np.int32))
    with pytest.raises(AssertionError, match="moves does not match dimension"):
        back(_fake(), moves=np.zeros(5, np.int32))
    # a tensor that requires grad and does not live on the voxelizer's device: the error of every differentiable call
    recording = dict(differentiable=True, _tgrad=True)
    for kw in (dict(coords=torch.tensor(a["coords"], requires_grad=True)), dict(angles=torch.zeros((2, 1), requires_grad=True))):
        call = {**a, "angles": angles, **kw}
        with pytest.raises(NotImplementedError, match="every tensor that requires grad on this voxelizer's device"):
            _fake(**recording).apply_torsions(**call)
    assert _fake(**recording)._torsion_grad_wanted(a["coords"], angles) is False  # (nothing requires grad: plain values)
    with torch.no_grad():
        assert _fake(**recording)._torsion_grad_wanted(torch.zeros((6, 3), requires_grad=True), angles) is False
    assert _fake(differentiable=True)._torsion_grad_wanted(torch.zeros((6, 3), requires_grad=True), angles) is False


# ---- kernel resources --------------------------------------------------------------------------------------------------------------
def test_the_kernel_uses_no_scratch_and_spills_nothing():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_torsion_grad.o")
    assert obj in regs.KERNEL_OBJECTS
    assert os.path.exists(obj), "mvx_torsion_grad.o not built (make -C molvoxel_amd/csrc)"
    res = regs.kernel_resources(obj)
    assert sorted(res) == ["torsion_backward_kernel"], sorted(res)
    r = res["torsion_backward_kernel"]
    print(f"torsion_backward_kernel: {r}")
    assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, r
    assert r["lds"] == 4 * 7 * 8, r  # the four waves' seven sums


# ---- what the GPU refinement test rests on ---------------------------------------------------------------------------------------
def _hamilton(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] - a[1] * b[3] + a[2] * b[0] + a[3] * b[1], a[0] * b[3] + a[1] * b[2] - a[2] * b[1] + a[3] * b[0]])


def cpu_score_and_gradients(q, t, theta):
    """(S, dS/dq, dS/dt, dS/dtheta) of flex_rows' refinement molecule at the poses (q / |q|, t) and angles theta, from
    flex_rows.cpu_evaluate's G = (F, N, theta_bar) about the pivot t: dS/dt = F, dS/dtheta = G[6:], and since the twist omega
    turns the pose as (1, omega / 2) (x) q, the tangent gradient at the unit quaternion is 2 sum_i N_i (e_i (x) q), divided by
    |q| behind the normalisation."""
    norm = np.linalg.norm(q, axis=1)[:, None]
    qn = q / norm
    S, G, _ = X.cpu_evaluate(qn, t, theta)
    gq = np.zeros_like(q)
    for b in range(len(q)):
        for i in range(3):
            gq[b] += 2.0 * G[b, 3 + i] * _hamilton(np.eye(4)[1 + i], qn[b])
    return S, gq / norm, G[:, :3], G[:, 6:]


def test_a_numpy_adam_loop_meets_the_condition_of_the_gpu_refinement_test():
    q0, t0, th0 = X.refine_starts()
    p = [np.array(q0), np.array(t0), np.array(th0)]
    m, v = [np.zeros_like(x) for x in p], [np.zeros_like(x) for x in p]
    start = None
    for it in range(1, tg.ADAM_STEPS + 1):  # torch.optim.Adam's defaults on -S
        S, *grads = cpu_score_and_gradients(*p)
        start = S if start is None else start
        for i in range(3):
            g = -grads[i]
            m[i] = 0.9 * m[i] + 0.1 * g
            v[i] = 0.999 * v[i] + 0.001 * g * g
            p[i] = p[i] - tg.ADAM_LR * (m[i] / (1.0 - 0.9 ** it)) / (np.sqrt(v[i] / (1.0 - 0.999 ** it)) + 1e-8)
    end = cpu_score_and_gradients(*p)[0]
    print(f"TORSION_GRAD_CPU_ADAM score {start.min():.1f} ... {start.max():.1f} -> {end.min():.1f} ... {end.max():.1f}")
    assert (end > start).all(), (start.tolist(), end.tolist())
