"""Randomised sweep of the score, pose, sum and moments entries (mvx_score_batch, mvx_pose_grad_batch, mvx_forward_sum_batch,
mvx_moments_batch, mvx_moments_backward_batch) over the parameter space of the gradient fuzz, on the draws of
tests/entry_fuzz_rows.py (tests/test_entry_fuzz_host.py shows without a GPU what they reach, so nothing here is skipped).

Walk draws (96): per-atom and per-molecule scores against tests/score_reference.py, the gradient rows against
tests/grad_reference.py with G = F and against mvx_backward_batch bit for bit, dS/dfield against the float64 weighted sum of
forward_batch's grids, pose gradients against tests/pose_reference.py (the reference's dL/dp, and the chain rule on the call's own
dL/dcoords), posed grids against the oracles. Summed draws (48): forward_batch against the oracle molecule by molecule, forward_sum
against the oracle on the merged cloud, moments_batch against the exact moments of those grids, the moments gradient against the
float64 reference. Then the rows and draws of tests/sum_sweep_rows.py the moments entries never ran on.

No tolerance of its own: |got - ref| <= REL * bound + ABS with GRAD_REL / GRAD_ABS (GRAD64_REL / GRAD64_ABS for float64 grids and
for binary types / single, whose terms are exact), assert_gaussian / assert_exact for grids, moments_reference.bound for moments,
the 1e-12 summation-order rule of tests/test_hip_pose.py for the chain rule, tests/test_hip_sum.py's rule for dS/dfield.

Measured on an MI355X, worst error / bar over the sweep per output kind, for float32 / bfloat16 / float64 grids (the module prints
them at the end, and writes them to the path in MVX_ENTRY_FUZZ_REPORT when set): atom score 0.018 / 0.020 / 0.0046, molecule score
0.0047 / 0.0057 / 0.0027, dS/dcoords 0.039 / 0.023 / 0.023, dS/dfeatures 0.028 / 0.026 / 0.014, dS/dfield 0.0096 / 0.98 (the final
rounding of the bfloat16 gradient is the bar's own half ulp: the float32 part of that error is as small as in the first figure),
pose c 0.0036 / 0.0026 / 0.0028, pose q 0.0044 / 0.0021 / 0.0024, pose t 0.0055 / 0.0026 / 0.0030; float32 only: moments 0.0069 of
moments_reference.bound (binary types / single equal), moments gradient 0.038 on the summed draws and 0.0076 on tall, cut96, edge20d
and bd16. Every posed and summed grid met the oracle's membership, and no draw exceeded a bar. With the reference's sigma left at
0.5, 62 of the 144 score and moments cases fail; with every reference radius one unit in the last place smaller, so that the voxels
at dr == 1 leave its support, 50 fail, all 24 walk draws that claim a tie among them.
"""
import json
import os

import numpy as np
import pytest

from tests import entry_drivers as X
from tests import entry_fuzz_rows as E
from tests import grad_reference as gr
from tests import hip_support as hip
from tests import moments_grad_reference as MG
from tests import moments_reference as MR
from tests import pose_reference as pr
from tests import score_reference as sr
from tests import sum_sweep_rows as S
from tests.tolerance import GRAD_ABS, GRAD_REL, P64_TOL, assert_exact, assert_gaussian

pytestmark = pytest.mark.gpu

BF16_HALF_ULP = 2.0 ** -8  # (tests/test_hip_sum.py: the final rounding of a bfloat16 field gradient)
_W = X.Worst()  # (output kind, grid kind) -> worst error / bar over the sweep


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"{k[0]:>16s} {k[1]:>4s}: worst error / bar {v:.3g}" for k, v in sorted(_W.worst.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("MVX_ENTRY_FUZZ_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{k[0]} {k[1]}": v for k, v in sorted(_W.worst.items())}, fh, indent=1)


def _note(kind, grid, ratio):
    _W.note((kind, grid), ratio)


def _close(kind, d, got, ref, bound, what, exact_terms=False):
    """The gradient rule with the bars of the draw's precision; the worst error / bar goes into the report."""
    _W.close((kind, d["kind"]), d, got, ref, bound, f"{_tag(d)}: {what}", exact_terms)


def _tag(d):
    keys = ("seed", "D", "res", "sigma", "blockdim", "density", "mode", "radii_type", "C", "kind", "per_mol", "transform", "posed",
            "sizes", "tie_mols")
    return {k: d[k] for k in keys if k in d}


def _field(d):
    """(the field on the device in the grid's type, the float64 array the kernel reads): the same values."""
    import torch

    Fref = E.field_of(d)
    Fd = torch.tensor(Fref, device="cuda").to(hip.grid_dtype(d))
    assert torch.equal(Fd.to(torch.float64).cpu(), torch.tensor(Fref))  # (the host's rounding is the device type's)
    return Fd, Fref


def _reference_kw(d):
    return dict(res=d["res"], sigma=d["sigma"], blockdim=d["blockdim"], density=d["density"], precision=d["precision"])


def _sample(d):
    return np.array([a for s in d["sample"] for a in s], np.int64)


# ---- a - c. walk draws: scores, gradient rows, field and pose gradients -----------------------------------------------------------
def _check_scores(d, vox, Fd, Fref, p):
    import torch

    a = X.inputs(d)
    scores, atoms = X.score(vox, d, a, Fd, per_atom=True)
    assert scores.dtype == torch.float64 and atoms.dtype == torch.float64 and scores.is_cuda and atoms.is_cuda
    assert tuple(scores.shape) == (d["B"],) and tuple(atoms.shape) == (d["N"],)
    assert torch.equal(X.score(vox, d, a, Fd), scores)  # per_atom=False: the same bits
    S_, s = scores.cpu().numpy(), atoms.cpu().numpy()
    w, types = E.reference_channels(d)
    s_ref, b_ref, S_ref, Sb_ref = sr.batch_reference(p, d["off"], Fref, d["radii"], d["radii_type"], w=w, mode=d["mode"], types=types,
                                                     **_reference_kw(d))
    # binary types / single: the terms are field values times 1, summed in float64 in another order than the reference's
    exact_terms = d["density"] == "binary" and d["mode"] != "features"
    pick = _sample(d)
    _close("atom score", d, s[pick], s_ref[pick], b_ref[pick], "atom scores", exact_terms)
    _close("molecule score", d, S_, S_ref, Sb_ref, "molecule scores", exact_terms)
    # exact zeros: atoms the reference admits nowhere (the ones past a face that reach no voxel among them), types past the
    # channels, molecules without atoms
    assert np.all(s[b_ref == 0.0] == 0.0), _tag(d)
    if d["bad_types"]:
        assert np.all(s[list(d["bad_types"])] == 0.0) and np.all(b_ref[list(d["bad_types"])] == 0.0), _tag(d)
    for b, n in enumerate(d["sizes"]):
        if n == 0:
            assert S_[b] == 0.0 and not np.signbit(S_[b]), (_tag(d), b)
    return scores


def _abi_rows(vox, d, Fd):
    """mvx_score_batch and mvx_backward_batch (grad_out = the field laid out per molecule) through ctypes on one call record.
    Outputs start as NaN: whatever is not overwritten fails every comparison."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    call = X.spec(vox, d, X.inputs(d))
    B, N, C_ = call.B, call.N, call.C
    fdt = torch.float64 if d["kind"] == "f64" else torch.float32
    feat = d["mode"] == "features"
    out = dict(scores=hip.nan((B,)), atoms=hip.nan((N,)), gc=hip.nan((N, 3)), gf=hip.nan((N, C_), fdt) if feat else None)
    stride = 0 if Fd.dim() == 4 else C_ * d["D"] ** 3
    _lib.check(vox._lib.mvx_score_batch(*call.batch_args(vox), Fd.data_ptr(), stride, hip.ptr(out["scores"]), hip.ptr(out["atoms"]),
                                        hip.ptr(out["gc"]), hip.ptr(out["gf"]), vox._stream()))
    G = Fd.expand((B,) + tuple(Fd.shape)).contiguous() if Fd.dim() == 4 else Fd
    ref = dict(gc=hip.nan((N, 3)), gf=hip.nan((N, C_), fdt) if feat else None)
    _lib.check(vox._lib.mvx_backward_batch(*call.batch_args(vox), G.data_ptr(), hip.ptr(ref["gc"]), hip.ptr(ref["gf"]), vox._stream()))
    torch.cuda.synchronize()
    return out, ref


def _check_field_gradient(d, p):
    """field.grad under L = sum_b g_b S_b against sum_b g_b grid_b in float64, grid_b the float32 grids of forward_batch /
    forward_posed_batch; bound sum_b |g_b| |grid_b| (tests/test_hip_sum.py's rule, half a bfloat16 ulp of the bound added for a
    bfloat16 field)."""
    import torch

    vox = X.vox(d, differentiable=True, field_grad=True)
    Fd, _ = _field(d)
    field = Fd.clone().requires_grad_()
    g = np.random.default_rng(d["fseed"] + 1).standard_normal(d["B"])
    scores = X.score(vox, d, X.inputs(d), field)
    (scores * hip.dev(g)).sum().backward()
    assert field.grad is not None and field.grad.dtype == Fd.dtype and field.grad.shape == Fd.shape
    grids = X.forward(X.vox(d, "f32"), d, X.inputs(d)).to(torch.float64)
    gw = torch.tensor(g, device="cuda").reshape(-1, 1, 1, 1, 1)
    ref = (gw * grids).sum(0).cpu().numpy()
    bound = (gw.abs() * grids.abs()).sum(0).cpu().numpy()
    err = np.abs(field.grad.to(torch.float64).cpu().numpy() - ref)
    bar = GRAD_REL * bound + GRAD_ABS + (BF16_HALF_ULP * bound if d["kind"] == "bf16" else 0.0)
    worst = float((err / bar).max())
    _note("dS/dfield", d["kind"], worst)
    assert worst <= 1.0, (_tag(d), worst)
    assert float(bound.max()) > 0 or d["N"] == 0, _tag(d)


@pytest.mark.parametrize("seed", range(E.N_WALK))
def test_walk_draw_scores_and_gradients(seed):
    import torch

    d = E.walk_draw(seed)
    Fd, Fref = _field(d)
    p = E.positions_of(d)
    plain = X.vox(d)
    scores = _check_scores(d, plain, Fd, Fref, p)

    # b. gradient rows through autograd on a differentiable voxelizer: L = sum_b S_b, so dL/dgrid_b = F
    vox = X.vox(d, differentiable=True)
    a = X.inputs(d, grad=True)
    recorded = X.score(vox, d, a, Fd)
    assert torch.equal(recorded.detach(), scores)  # recording the graph does not change the scores
    gauss = d["density"] == "gaussian"
    feat = d["mode"] == "features"
    if d["N"] == 0:
        return
    assert recorded.requires_grad
    recorded.sum().backward()
    gc = a["xyz"].grad.cpu().numpy()
    gf = a["chan"].grad.double().cpu().numpy() if feat else None
    quats = E.quaternions_of(d)
    w, types = E.reference_channels(d)
    pose_ref = []
    for b in range(d["B"]):
        lo, hi, radii = E.molecule(d, b)
        if hi == lo:
            pose_ref.append(None)
            continue
        M = pr.rotation(quats[b])
        o = gr.reference(p[lo:hi], Fref if Fref.ndim == 4 else Fref[b], radii, d["radii_type"], w=None if w is None else w[lo:hi],
                         mode=d["mode"], types=None if types is None else types[lo:hi], **_reference_kw(d))
        gp, bp = o["coords"]  # dL/dp and its bound for every atom; dL/dcoords = M^T dL/dp (the reference's own `rot` rule)
        rows = np.array([n - lo for n in d["sample"][b]], np.int64)
        if gauss:
            _close("dS/dcoords", d, gc[lo:hi][rows], (gp @ M)[rows], (bp @ np.abs(M))[rows], f"dS/dcoords of molecule {b}")
        else:
            assert not gc[lo:hi].any(), (_tag(d), b)
        if feat:
            gfr, bfr = o["features"]
            _close("dS/dfeatures", d, gf[lo:hi][rows], gfr[rows], bfr[rows], f"dS/dfeatures of molecule {b}")
        pose_ref.append(pr.pose_grads(d["xyz"][lo:hi], d["cen"][b], quats[b], gp, bp) if gauss else None)
    for n in d["bad_types"]:
        assert not gc[n].any(), (_tag(d), n)

    # ... and through the C entries: the score entry's rows are mvx_backward_batch's with grad_out = F, bit for bit, and autograd's
    got, ref = _abi_rows(plain, d, Fd)
    assert not torch.isnan(got["gc"]).any() and not torch.isnan(got["atoms"]).any() and not torch.isnan(got["scores"]).any()
    assert torch.equal(got["gc"], ref["gc"]) and torch.equal(got["scores"], scores), _tag(d)
    assert torch.equal(got["gc"], a["xyz"].grad), _tag(d)
    if feat:
        assert not torch.isnan(got["gf"]).any() and torch.equal(got["gf"], ref["gf"]) and torch.equal(got["gf"], a["chan"].grad), _tag(d)

    # c. pose gradients; the centre is minus the sum of the molecule's rows under a random rotation too
    names = (("center", "cen"), ("quaternion", "q"), ("translation", "t")) if d["posed"] else (("center", "cen"),)
    for b in range(d["B"]):
        lo, hi, _ = E.molecule(d, b)
        if hi == lo or not gauss:
            for _, key in names:  # molecules without atoms, and a binary density: zero rows
                assert not bool(a[key].grad[b].any()), (_tag(d), b, key)
            continue
        chain = pr.from_coords_grad(d["xyz"][lo:hi], d["cen"][b], quats[b], gc[lo:hi])
        for name, key in names:
            got_row = a[key].grad[b].double().cpu().numpy()
            val, scale = chain[name]  # the float64 chain rule on the call's own dL/dcoords (tests/test_hip_pose.py's rule)
            assert np.all(np.abs(got_row - val) <= 1e-12 * np.abs(val) + 1e-12 * scale), (_tag(d), b, name, got_row, val)
            if d["posed"]:
                val, bound = pose_ref[b][name]
                _close({"cen": "pose c", "q": "pose q", "t": "pose t"}[key], d, got_row, val, bound, f"dL/d{name} of molecule {b}")

    if d["field_grad"]:
        _check_field_gradient(d, p)


# ---- d. posed grids against the oracles -------------------------------------------------------------------------------------------
POSED_WALK = [s for s in range(E.N_WALK) if E.walk_draw(s)["posed"]]


@pytest.mark.parametrize("seed", POSED_WALK)
def test_walk_draw_posed_grids_match_the_oracle_on_the_reference_positions(seed):
    import torch

    d = E.walk_draw(seed)
    p = E.positions_of(d)
    got = X.forward(X.vox(d), d, X.inputs(d))
    assert tuple(got.shape) == (d["B"], d["C"]) + (d["D"],) * 3 and got.dtype == hip.grid_dtype(d)
    if d["kind"] == "bf16":  # a bfloat16 grid is the float32 grid rounded once (tests/test_hip_bf16.py); that one meets the oracle
        base = X.forward(X.vox(d, "f32"), d, X.inputs(d))
        assert torch.equal(got, base.to(torch.bfloat16)), _tag(d)
        got = base
    got = got.cpu().numpy()
    for b in range(d["B"]):
        ref = E.oracle_grid(d, p, b)
        if d["density"] == "binary" and d["mode"] != "features":
            assert_exact(got[b], ref)
        else:
            assert_gaussian(got[b], ref, *(() if d["precision"] == 32 else (P64_TOL,)))


# ---- e. summed draws ------------------------------------------------------------------------------------------------------------------
def _summed(seed):
    d = E.summed_draw(seed)
    vox = X.vox(d)
    a = X.inputs(d)
    grids = X.forward(vox, d, a)
    assert tuple(grids.shape) == (d["B"], d["C"]) + (d["D"],) * 3
    return d, vox, a, grids, E.positions_of(d)


@pytest.mark.parametrize("seed", range(E.N_SUMMED))
def test_summed_draw_grids_and_their_sum_match_the_oracle(seed):
    from oracle import c_oracle

    from tests.test_hip_sum_sweep import _check_merged

    d, vox, a, grids, p = _summed(seed)
    got = grids.cpu().numpy()
    for b in range(d["B"]):  # the anchor: the grids the references below describe are the grids the library writes
        ref = E.oracle_grid(d, p, b)
        if d["density"] == "binary" and d["mode"] != "features":
            assert_exact(got[b], ref)
        else:
            assert_gaussian(got[b], ref)
    if d["posed"]:
        total = vox.forward_posed_sum(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], num_channels=hip.nc(d))
    else:
        total = vox.forward_sum(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], num_channels=hip.nc(d))
    merged = c_oracle.voxelize(p, E.features_of(d), d["r_atom"].astype(np.float32), resolution=d["res"], dimension=d["D"],
                               density=d["density"], blockdim=d["blockdim"], sigma=d["sigma"], radii_type="atom-wise")
    _check_merged(total.cpu().numpy(), merged, d["density"], str(_tag(d)))


def _check_moments(d, got, ref, bnd, what):
    import torch

    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == ref.shape, (what, got.dtype, tuple(got.shape))
    g = got.cpu().numpy()
    err = np.abs(g - ref)
    live = bnd > 0
    assert live.any(), what
    _note("moments", d["kind"], float((err[live] / bnd[live]).max()))
    assert (err <= bnd).all(), (what, float((err[live] / bnd[live]).max()))  # (a bound of 0 - no atom reaches the channel: equality with 0)
    if d["density"] == "binary" and d["mode"] in ("types", "single"):  # sums of small integers: voxel counts
        assert np.array_equal(g[..., :2], ref[..., :2]) and (g[..., :2] == np.round(g[..., :2])).all(), what


@pytest.mark.parametrize("seed", range(E.N_SUMMED))
def test_summed_draw_moments_and_their_gradient(seed):
    import torch

    from tests.test_hip_moments_grad import _entry

    d, vox, a, grids, p = _summed(seed)
    target = E.target_of(d)
    T = hip.dev(target)
    g32 = grids.cpu().numpy()
    ref, bnd = MR.moments_and_bound(g32, target)
    kw = dict(num_channels=hip.nc(d))
    if d["posed"]:
        call = lambda t: vox.moments_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], target=t, **kw)  # noqa: E731
    else:
        call = lambda t: vox.moments_batch(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], target=t, **kw)  # noqa: E731
    plain, with_t = call(None), call(T)
    _check_moments(d, plain, ref[..., :2], bnd[..., :2], f"{_tag(d)} without a target")
    _check_moments(d, with_t, ref, bnd, f"{_tag(d)} with a target")
    assert torch.equal(with_t[..., :2], plain), _tag(d)  # the first two moments do not depend on the target
    assert (ref[..., 1] > 0).any()
    empty = [b for b, n in enumerate(d["sizes"]) if n == 0]
    assert (with_t[empty] == 0).all() and (plain[empty] == 0).all()

    # the moments gradient with the drawn dL/dm against the float64 reference with G = a0 + a1 g + a2 t
    # (tests/test_hip_moments_grad.py: test_general_coefficients_match_the_float64_reference)
    spec = X.spec(vox, d, a)
    quats = E.quaternions_of(d)
    w, types = E.reference_channels(d)
    for K in (3, 2):
        gm = E.dm_of(d, K)
        gc, gf = _entry(vox, spec, gm, T if K == 3 else None)
        gc = gc.cpu().numpy()
        gf = None if gf is None else gf.cpu().numpy()
        assert not np.isnan(gc).any() and (gf is None or not np.isnan(gf).any()), _tag(d)  # fully overwritten
        if d["density"] == "binary":  # the a.e. derivative: no coordinate gradient
            assert (gc == 0).all(), _tag(d)
        live = 0
        for b in range(d["B"]):
            lo, hi, radii = E.molecule(d, b)
            mine = [n - lo for n in d["sample"] if lo <= n < hi]
            if not mine:
                continue
            G, Gabs = MG.upstream(g32[b], gm[b], target if K == 3 else None)
            rkw = dict(w=None if w is None else w[lo:hi], mode=d["mode"], types=None if types is None else types[lo:hi], atoms=mine,
                       rot=pr.rotation(quats[b]) if d["posed"] else None, **_reference_kw(d))
            val = gr.reference(p[lo:hi], G, radii, d["radii_type"], **rkw)
            bound = gr.reference(p[lo:hi], Gabs, radii, d["radii_type"], **rkw)
            rows = np.array(mine) + lo
            _close("moments_grad", d, gc[rows], val["coords"][0], bound["coords"][1], f"K = {K}: coordinate rows of molecule {b}")
            live += int((bound["coords"][1] > 0).any(axis=1).sum())
            if gf is not None:
                _close("moments_grad", d, gf[rows], val["features"][0], bound["features"][1], f"K = {K}: feature rows of molecule {b}")
                live += int((bound["features"][1] > 0).any(axis=1).sum())
        for n in d["bad_types"]:
            assert (gc[n] == 0).all(), (_tag(d), n)
        if d["density"] != "binary" or d["mode"] == "features":
            assert live > 0, _tag(d)


# ---- f. the rows and draws of the summed sweep the moments entries never ran on -------------------------------------------------------
MOMENT_ROWS = ["cut132", "cut144", "edge44", "bd16u", "bd24"]
MOMENT_DRAWS = [f"draw{s}" for s in S.SWEEP_SEEDS]
MOMENTS_GRAD_ROWS = ["tall", "cut96", "edge20d", "bd16"]


def test_the_rows_here_are_the_ones_the_moments_tests_leave_out():
    import tests.test_hip_moments as HM
    import tests.test_hip_moments_grad as HG

    assert not set(MOMENT_ROWS) & set(HM.ROW_IDS) and set(MOMENT_ROWS) | set(HM.SWEEP_IDS) == set(S.ROW_IDS)
    assert not set(MOMENTS_GRAD_ROWS) & set(HG.ROW_IDS) and set(MOMENTS_GRAD_ROWS) <= set(S.ROW_IDS) and len(MOMENT_DRAWS) == 48


@pytest.mark.parametrize("row_id", MOMENT_ROWS + MOMENT_DRAWS)
def test_moments_on_the_rows_and_draws_they_never_saw(row_id):
    """tests/test_hip_moments.py's own checks on these ids: the moments with and without the target against forward_batch's grids
    reduced exactly, and a molecule alone, two runs and the target leave the bits as they are."""
    import tests.test_hip_moments as HM

    HM.test_moments_are_those_of_forward_batchs_grids(row_id)
    HM.test_a_molecule_alone_two_runs_and_the_target_do_not_change_the_bits(row_id)


@pytest.mark.parametrize("row_id", MOMENTS_GRAD_ROWS)
def test_the_moments_gradient_on_rows_with_a_z_cut_nine_waves_and_a_blockdim_of_16(row_id):
    """tests/test_hip_moments_grad.py's float64 check (a sample of 96 atoms) on rows it never ran on."""
    import tests.test_hip_moments_grad as HG

    assert HG.SAMPLE == 96
    HG.test_general_coefficients_match_the_float64_reference(row_id, "centred")


@pytest.mark.parametrize("row_id", ["tall", "cut96"])
def test_the_moments_gradient_in_molecule_chunks_gives_the_uncut_bits(row_id):
    import tests.test_hip_moments_grad as HG

    HG.test_molecule_chunks_give_the_uncut_bits(row_id, "mall_budget_kb", 1, 3)
