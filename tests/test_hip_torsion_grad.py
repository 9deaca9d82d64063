"""The adjoint of the conformer on the GPU (apply_torsions_backward, apply_torsions on a torsion_grad voxelizer) on the rows of
tests/flex_rows.py, every one with D = 16 at resolution 0.5: base (14 / 0 / 9 atoms with 4 / 0 / 2 torsions: an empty molecule,
padding, a branch, nesting depth 3), long (300 atoms, one torsion turning 150: past one round of the 256-lane loop, so lane
partials hold two terms) and deep (35 atoms, 32 torsions: mask bit 31 and the longest dependent chain).

To the bit: two runs; a molecule alone and in its batch; T = 0 returns the upstream; all angles 0 return the upstream rows with
non-zero angle gradients; inert torsions (padding, an index of N_b, coincident axis atoms) give +0.0 and otherwise the bits of the
call without them; an atom with a NaN coordinate and a zero upstream row against the same atom at a finite far position; the
in-place call grad_out == grad_coords against the out-of-place call; the caller's conformer is not modified. Autograd: x.grad and
theta.grad of a loss through score_posed_batch, moments_posed_batch and forward_posed_batch are apply_torsions_backward applied
to the conformer's gradient of the same loss, to the bit; without torsion_grad the output does not require grad, and the forward
bits are the same either way.
Within a bar: against form (a) of tests/torsion_grad_reference.py - the sweep over stored forward intermediates - fed the device's
own conformer (the stored positions are its pre-images, taken in extended precision) and the same upstream,
|got - ref| <= (N_b + 128)(T_b + 1) 2^-53 x bound (float64 sums of at most N_b terms with under 128 roundings per term,
compounded over at most T_b + 1 levels); theta.grad of the summed scores against score_hessian_flex_posed_batch's G[:, 6:] at
unit quaternions, 2 (GRAD_REL x bound + GRAD_ABS): each side is held to once that bar against the float64 reference by the
existing tests.
The refinement: the 8 starts of flex_rows.refine_starts() on the 14-atom molecule against its own grid, torch.optim.Adam on
-score over (q, t, theta) with the learning rate and step count chosen on the numpy loop of tests/test_torsion_grad_host.py; every
start ends above its start score.

Figures printed with -s (MI355X; DESIGN.md section 29, profiles/r23_torsion_grad.txt). Worst |got - ref| over the bar against
form (a): grad_coords 0.0050 (base), 0.0038 (long), 1.4e-8 (deep - the bound of the rows grows with every level of absolute
values); grad_angles 0.00014, 0.00056, 0.0010; with every angle 0: 0.0013, 0.00060, 0.00014. theta.grad against the flex Hessian
entry's G: 5.3e-13 (base), 6.9e-12 (deep) of its bar - two device paths that read the same rows of the one walk and differ in
float64 sums only. The refinement: scores 591.1 ... 616.5 -> 634.8 ... 641.3, the largest change of an angle 0.189 rad. 31 cases
in 5.1 s.
"""
import functools

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import flex_reference as fr
from tests import flex_rows as X
from tests import hessian_reference as hr
from tests import pose_reference as pr
from tests import torsion_grad_reference as tg
from tests import hip_support as hip
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

CASES = ("base", "long", "deep")


def _vox(d, **kw):
    import molvoxel_amd as mv

    return mv.create_voxelizer(0.5, X.D, d["radii_type"], d["density"], library="hip", precision=64 if d["kind"] == "f64" else 32, **kw)


@functools.lru_cache(maxsize=None)
def _rows(name, seed=23):
    """(angles (B, T), upstream rows (N, 3)) of a case, never modified."""
    d = X.data(name)
    rng = np.random.default_rng(seed)
    ang, up = rng.uniform(-np.pi, np.pi, (d["B"], d["T"])), rng.standard_normal((d["N"], 3))
    ang.setflags(write=False)
    up.setflags(write=False)
    return ang, up


def _back(vox, conformer, d, ang, up, axes=None, moves=None, off=None):
    gc, ga = vox.apply_torsions_backward(conformer, d["off"] if off is None else off, d["axes"] if axes is None else axes,
                                         d["moves"] if moves is None else moves, ang, hip.dev(up))
    return gc.cpu().numpy(), ga.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _got(name):
    """(conformer, grad_coords, grad_angles) of the case as host arrays, computed once and left unchanged."""
    d = X.data(name)
    vox = _vox(d)
    ang, up = _rows(name)
    conformer = vox.apply_torsions(hip.dev(d["xyz"]), d["off"], d["axes"], d["moves"], ang)
    kept = conformer.clone()
    gc, ga = _back(vox, conformer, d, ang, up)
    assert hip.same_bits(conformer.cpu().numpy(), kept.cpu().numpy())  # the caller's conformer is not modified
    return conformer.cpu().numpy(), gc, ga


# ---- bit identities -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_two_runs_agree_and_a_molecule_alone_is_the_molecule_in_its_batch(name):
    d = X.data(name)
    vox = _vox(d)
    ang, up = _rows(name)
    conformer, gc, ga = _got(name)
    assert gc.shape == (d["N"], 3) and ga.shape == (d["B"], d["T"]) and gc.dtype == np.float64 and ga.dtype == np.float64
    assert np.isfinite(gc).all() and np.isfinite(ga).all()
    again = _back(vox, hip.dev(conformer), d, ang, up)
    assert hip.same_bits(again[0], gc) and hip.same_bits(again[1], ga)
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        alone = _back(vox, hip.dev(conformer[lo:hi]), d, ang[b:b + 1], up[lo:hi], axes=d["axes"][b:b + 1], moves=d["moves"][lo:hi],
                      off=np.array([0, hi - lo], np.int64))
        assert hip.same_bits(alone[0], gc[lo:hi]) and hip.same_bits(alone[1][0], ga[b])
    live = (d["axes"][:, :, 0] >= 0) & (np.diff(d["off"]) > 0)[:, None]
    assert ga[live].all() and not ga[~live].any() and not np.signbit(ga[~live]).any()  # (padding and the empty molecule: +0.0)


@pytest.mark.parametrize("name", ("base", "long"))
def test_no_torsions_return_the_upstream(name):
    d = X.data(name)
    vox = _vox(d)
    _, up = _rows(name)
    gc, ga = _back(vox, hip.dev(d["xyz"]), d, np.zeros((d["B"], 0)), up, axes=np.zeros((d["B"], 0, 2), np.int32))
    assert hip.same_bits(gc, up) and ga.shape == (d["B"], 0)


@pytest.mark.parametrize("name", CASES)
def test_angles_of_exactly_zero_return_the_upstream_rows_and_their_true_derivatives(name):
    d = X.data(name)
    vox = _vox(d)
    _, up = _rows(name)
    zero = np.zeros((d["B"], d["T"]))
    gc, ga = _back(vox, hip.dev(d["xyz"]), d, zero, up)
    assert hip.same_bits(gc, up)
    live = (d["axes"][:, :, 0] >= 0) & (np.diff(d["off"]) > 0)[:, None]
    assert ga[live].all() and not ga[~live].any()
    worst = 0.0
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            continue
        _, ra, _, ba = tg.stored(d["xyz"][lo:hi], d["axes"][b], d["moves"][lo:hi], zero[b], up[lo:hi])
        bar = tg.bar_factor(hi - lo, d["axes"][b])
        assert (np.abs(ga[b] - ra) <= bar * ba).all()
        worst = max(worst, float((np.abs(ga[b] - ra) / (bar * ba + 1e-300)).max()))
    print(f"TORSION_GRAD_ZERO {name}: worst |got - ref| / bar {worst:.3g}")


@pytest.mark.parametrize("bad", [(-1, -1), (4, 14), (14, 4), (4, 4), (-3, 2)])
def test_an_inert_torsion_gives_plus_zero_and_leaves_the_other_bits(bad):
    d = X.data("base")
    vox = _vox(d)
    ang, up = _rows("base")
    conformer, gc4, ga4 = _got("base")
    axes = np.concatenate([d["axes"], np.full((3, 1, 2), -1, np.int32)], axis=1)
    axes[0, 4] = bad  # (molecule 0 has 14 atoms: 14 is the index N_b)
    moves = d["moves"].copy()
    moves[9:12] |= 1 << 4  # the fifth set is a live set: only its axis is not
    ang5 = np.concatenate([ang, np.full((3, 1), 0.7)], axis=1)
    gc, ga = _back(vox, hip.dev(conformer), d, ang5, up, axes=axes, moves=moves)
    assert hip.same_bits(gc, gc4) and hip.same_bits(ga[:, :4], ga4)
    assert not ga[:, 4].any() and not np.signbit(ga[:, 4]).any()


def test_an_atom_without_a_row_may_have_nan_coordinates():
    d = X.data("base")
    vox = _vox(d)
    ang, up = _rows("base")
    conformer = _got("base")[0]
    last = d["N"] - 1  # the last atom of the last molecule, in both of its sets and on no axis
    assert (int(d["moves"][last]) & 3) == 3 and last - int(d["off"][2]) not in d["axes"][2].ravel().tolist()
    up0 = up.copy()
    up0[last] = 0.0
    far, dead = conformer.copy(), conformer.copy()
    far[last] = [1e3, -2e3, 5e2]
    dead[last, 1] = np.nan
    want, got = _back(vox, hip.dev(far), d, ang, up0), _back(vox, hip.dev(dead), d, ang, up0)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert hip.same_bits(got[0], want[0]) and hip.same_bits(got[1], want[1])
    assert not got[0][last].any() and not np.signbit(got[0][last]).any() and got[1][2, :2].all()


@pytest.mark.parametrize("name", CASES)
def test_the_in_place_call_is_the_out_of_place_call(name):
    import torch

    d = X.data(name)
    vox = _vox(d)
    ang, up = _rows(name)
    conformer, gc, ga = _got(name)
    c, g = hip.dev(conformer), hip.dev(up)
    B, T, ax, mv, th = vox._torsion_arrays(d["off"], d["axes"], d["moves"], ang)
    ga2 = torch.empty((B, T), dtype=torch.float64, device="cuda")
    _lib.check(vox._lib.mvx_apply_torsions_backward(vox._handle, c.data_ptr(), d["off"].ctypes.data, B, T, ax.data_ptr(), mv.data_ptr(),
                                                    th.data_ptr(), g.data_ptr(), g.data_ptr(), ga2.data_ptr(), vox._stream()))
    assert hip.same_bits(g.cpu().numpy(), gc) and hip.same_bits(ga2.cpu().numpy(), ga) and hip.same_bits(c.cpu().numpy(), conformer)


# ---- against the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CASES)
def test_against_the_stored_sweep_fed_the_devices_own_conformer(name):
    """Measured worst error / bar (MI355X): see DESIGN.md section 29."""
    d = X.data(name)
    ang, up = _rows(name)
    conformer, gc, ga = _got(name)
    worst_c = worst_a = 0.0
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            assert not ga[b].any()
            continue
        rc, ra, bc, ba = tg.stored_from(conformer[lo:hi], d["axes"][b], d["moves"][lo:hi], ang[b], up[lo:hi])
        bar = tg.bar_factor(hi - lo, d["axes"][b])
        ec, ea = np.abs(gc[lo:hi] - rc) / (bar * bc + 1e-300), np.abs(ga[b] - ra) / (bar * ba + 1e-300)
        assert not gc[lo:hi][bc == 0.0].any() and not ga[b][ba == 0.0].any()
        worst_c, worst_a = max(worst_c, float(ec.max())), max(worst_a, float(ea.max()))
    print(f"TORSION_GRAD_REFERENCE {name}: worst |got - ref| / ((N_b + 128)(T_b + 1) 2^-53 bound): coordinates {worst_c:.3g}, "
          f"angles {worst_a:.3g}")
    assert worst_c <= 1.0 and worst_a <= 1.0, (worst_c, worst_a)


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def _field(d):
    import torch

    return torch.tensor(d["F"], device="cuda").to(torch.float64 if d["kind"] == "f64" else torch.float32)


def _losses(vox, d, entry):
    """conformer -> loss through one entry of the voxelizer, with fixed random weights."""
    import torch

    rng = np.random.default_rng(31)
    pose = (d["off"], hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), hip.dev(d["chan"]), hip.dev(d["radii"]))
    F = _field(d)
    if entry == "score":
        w = hip.dev(rng.standard_normal(d["B"]))
        return lambda c: (vox.score_posed_batch(c, *pose, F) * w).sum()
    if entry == "moments":
        w = hip.dev(rng.standard_normal((d["B"], d["C"], 3)))
        return lambda c: (vox.moments_posed_batch(c, *pose, target=F) * w).sum()
    w = hip.dev(rng.standard_normal((d["B"], d["C"]) + (X.D,) * 3)).to(F.dtype)
    return lambda c: (vox.forward_posed_batch(c, *pose) * w).sum()


@pytest.mark.parametrize("name, entry", [("base", "score"), ("long", "score"), ("deep", "score"), ("base", "moments"), ("deep", "moments"),
                                         ("base", "grids"), ("long", "grids")])
def test_autograd_through_apply_torsions_is_the_backward_entry_on_the_conformers_gradient(name, entry):
    d = X.data(name)
    vox = _vox(d, differentiable=True, torsion_grad=True, moments_grad=(entry == "moments"))
    ang, _ = _rows(name)
    loss = _losses(vox, d, entry)
    x, theta = hip.dev(d["xyz"]).requires_grad_(), hip.dev(ang).requires_grad_()
    conformer = vox.apply_torsions(x, d["off"], d["axes"], d["moves"], theta)
    assert conformer.requires_grad and conformer.dtype == x.dtype and hip.same_bits(conformer.detach().cpu().numpy(), _got(name)[0])
    loss(conformer).backward()
    leaf = conformer.detach().clone().requires_grad_()
    loss(leaf).backward()
    assert leaf.grad.abs().max() > 0
    gc, ga = vox.apply_torsions_backward(leaf.detach(), d["off"], d["axes"], d["moves"], ang, leaf.grad)
    assert x.grad.shape == x.shape and theta.grad.shape == theta.shape
    assert hip.same_bits(x.grad.cpu().numpy(), gc.cpu().numpy()) and hip.same_bits(theta.grad.cpu().numpy(), ga.cpu().numpy())
    assert not gc.requires_grad and not ga.requires_grad


def test_only_a_torsion_grad_voxelizer_records_and_the_forward_bits_are_the_same_either_way():
    import torch

    d = X.data("base")
    ang, _ = _rows("base")
    want = _got("base")[0]
    for kw in (dict(), dict(differentiable=True)):
        vox = _vox(d, **kw)
        out = vox.apply_torsions(hip.dev(d["xyz"]).requires_grad_(), d["off"], d["axes"], d["moves"], hip.dev(ang).requires_grad_())
        assert not out.requires_grad and hip.same_bits(out.cpu().numpy(), want)
    vox = _vox(d, differentiable=True, torsion_grad=True)
    x32 = hip.dev(d["xyz"].astype(np.float32)).requires_grad_()  # (gradients come back in the inputs' dtype)
    out = vox.apply_torsions(x32, d["off"], d["axes"], d["moves"], ang)
    assert out.requires_grad and out.dtype == torch.float64
    out.sum().backward()
    assert x32.grad.dtype == torch.float32 and x32.grad.shape == x32.shape
    only_theta = vox.apply_torsions(d["xyz"].copy(), d["off"], d["axes"], d["moves"], hip.dev(ang).requires_grad_())
    assert only_theta.requires_grad and hip.same_bits(only_theta.detach().cpu().numpy(), want)
    with torch.no_grad():
        assert not vox.apply_torsions(hip.dev(d["xyz"]).requires_grad_(), d["off"], d["axes"], d["moves"], ang).requires_grad
    assert not vox.apply_torsions(hip.dev(d["xyz"]), d["off"], d["axes"], d["moves"], ang).requires_grad


# ---- against the second-order path -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("base", "deep"))
def test_the_angle_gradients_of_the_scores_against_the_flex_hessian_entry(name):
    d = X.data(name)
    assert np.abs(np.linalg.norm(d["q"], axis=1) - 1.0).max() <= 1e-15  # unit quaternions
    vox = _vox(d, differentiable=True, torsion_grad=True)
    ang = np.random.default_rng(37).uniform(-1.0, 1.0, (d["B"], d["T"]))
    F = _field(d)
    pose = (d["off"], hip.dev(d["cen"]), hip.dev(d["q"]), hip.dev(d["t"]), hip.dev(d["chan"]), hip.dev(d["radii"]))
    theta = hip.dev(ang).requires_grad_()
    conformer = vox.apply_torsions(hip.dev(d["xyz"]), d["off"], d["axes"], d["moves"], theta)
    vox.score_posed_batch(conformer, *pose, F).sum().backward()
    got = theta.grad.cpu().numpy()
    _, G, _ = vox.score_hessian_flex_posed_batch(conformer.detach(), *pose, F, d["axes"], d["moves"])
    G = G.cpu().numpy()[:, 6:]
    # the bound: the sum of the absolute terms, from the float64 reference on the device's conformer
    conf = conformer.detach().cpu().numpy()
    p = pr.batch_positions(conf, d["off"], d["cen"], d["q"], d["t"])
    Fref = F.to(F.dtype).double().cpu().numpy()
    piv = d["t"].astype(np.float32).astype(np.float64)
    rel, ab = (GRAD64_REL, GRAD64_ABS) if d["kind"] == "f64" else (GRAD_REL, GRAD_ABS)
    worst = 0.0
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            assert not got[b].any() and not G[b].any()
            continue
        radii = d["radii"] if np.isscalar(d["radii"]) else d["radii"][lo:hi]
        ref = hr.reference(p[lo:hi], Fref, radii, d["radii_type"], w=None if d["chan"] is None else d["chan"][lo:hi], mode=d["mode"],
                           precision=64 if d["kind"] == "f64" else 32)
        _, bG, _, _ = fr.flex(p[lo:hi], ref["g"][0], ref["H"][0], piv[b], d["axes"][b], d["moves"][lo:hi], ref["g"][1], ref["H"][1])
        bar = 2.0 * (rel * bG[6:] + ab)
        err = np.abs(got[b] - G[b])
        assert (err <= bar).all(), (b, float((err / bar).max()))
        worst = max(worst, float((err / bar).max()))
    assert np.abs(G).max() > 0
    print(f"TORSION_GRAD_SECOND_ORDER {name}: worst |theta.grad - G[6:]| / (2 (REL bound + ABS)) {worst:.3g}")


# ---- a short refinement ------------------------------------------------------------------------------------------------------------
def test_adam_on_the_score_over_poses_and_torsions_improves_every_start():
    import torch

    import molvoxel_amd as mv

    xyz, cen, W, rad, axes, moves = X.refine_molecule()
    q0, t0, th0 = X.refine_starts()
    B = X.REFINE_POSES
    vox = mv.create_voxelizer(0.5, X.D, "atom-wise", "gaussian", library="hip", differentiable=True, torsion_grad=True)
    off1 = np.array([0, 14], np.int64)
    with torch.no_grad():
        field = vox.forward_posed_batch(hip.dev(xyz), off1, hip.dev(cen), hip.dev(np.array([[1.0, 0.0, 0.0, 0.0]])), hip.dev(np.zeros((1, 3))),
                                        hip.dev(W), hip.dev(rad))[0].clone()
    off = 14 * np.arange(B + 1, dtype=np.int64)
    rep = lambda x: hip.dev(np.concatenate([x] * B))  # noqa: E731  (B copies of the molecule, one per start)
    coords, chan, radii, cens = rep(xyz), rep(W), rep(rad), rep(cen)
    ax, mvs = np.concatenate([axes] * B), np.concatenate([moves] * B)
    q, t, theta = (hip.dev(x).requires_grad_() for x in (q0, t0, th0))

    def scores():
        conformer = vox.apply_torsions(coords, off, ax, mvs, theta)
        return vox.score_posed_batch(conformer, off, cens, q / q.norm(dim=1, keepdim=True), t, chan, radii, field)

    opt = torch.optim.Adam([q, t, theta], lr=tg.ADAM_LR)
    start = None
    for _ in range(tg.ADAM_STEPS):
        opt.zero_grad()
        S = scores()
        start = S.detach().clone() if start is None else start
        (-S.sum()).backward()
        opt.step()
    with torch.no_grad():
        end = scores()
    print(f"TORSION_GRAD_ADAM score {float(start.min()):.1f} ... {float(start.max()):.1f} -> {float(end.min()):.1f} ... {float(end.max()):.1f}; "
          f"largest |theta - theta0| {float((theta.detach() - hip.dev(th0)).abs().max()):.3f}")
    assert bool((end > start).all()), (start.tolist(), end.tolist())
    assert float((theta.detach() - hip.dev(th0)).abs().min()) > 0.0  # every torsion of every start moved
