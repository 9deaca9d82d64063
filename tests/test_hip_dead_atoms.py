"""Atoms that reach no voxel, in every entry (rows: tests/dead_atom_rows.py; tests/test_dead_atoms_host.py shows on the CPU that
the oracles give the clean batch's grid for the dirty batch and that the live atoms contribute). A dead atom has a NaN, infinite
or astronomically large coordinate, an atom-wise radius that is 0, negative, NaN or infinite, or a type outside [0, C).

Every entry runs on the dirty batch and on the clean one - the same batch with the dead atoms deleted and the offsets moved up - on
the same voxelizer. Per-voxel and per-atom outputs are compared bit for bit (the live rows) and with zero (the dead rows, in
buffers that start as NaN where the test owns them); the clean call is held to the entry's existing reference under the bars of
tests/tolerance.py. Reductions over atoms are held to the clean batch's float64 reference (a float64 reference of the dirty batch
turns 0 * NaN into NaN) and, where the placement keeps every live atom on its lane, to the clean call's bits:
  pose rows (dL/dc, dL/dq, dL/dt) and molecule scores: one workgroup per molecule - bit for bit under `tail` and `call_tail`;
  dL/dsigma, dL/d(scalar radius), dL/dradii by channel or type: one reduction per call - bit for bit under `call_tail`;
  grids, sums, moments, dL/dfield, per-atom rows: bit for bit under every placement.
Where "bit for bit" cannot hold, the reason:
  molecule scores under `scattered`: score_reduce_kernel adds a molecule's per-atom scores lane by lane; a dead atom in front of
    a live one moves it to another lane, so the same terms (and zeros) are added in another order. Held to the score's bar.
  view entries with atom-wise radii: the view selection is the box cull alone (mvx_box_cull.inc), which an atom inside the box with
    a radius of 0, -1 or inf passes; the radius test drops it afterwards. Such atoms are listed by select_views (the documented
    superset), have zero rows, and move the live atoms of their view to other lanes of the per-view reductions. Grids, sums,
    per-atom values and the rows reduced onto the shared cloud stay bit for bit; the view scores are held to the score's bar, and
    dS/dc, dS/dq, dS/dt of every view to tests/pose_reference.py on the clean cloud under the pose bar and to the clean call's rows
    under the summation-order rule of tests/test_hip_pose.py. Every other dead kind is never selected, and there everything is
    bit for bit.
score_posed_views and score_posed_batch on the repeated dirty cloud must agree: this is the test that needs
pose_grad_kernel to skip an atom whose gradient row is zero before it reads the atom's coordinates. A molecule whose own pose is not
finite has dead atoms only: zero grid, score, moments and rows (mvx_grad_body.inc writes zeros where M^T 0 is not a number), and
the other molecules keep their bits.

Measured on an MI355X, 148 cases in 7.8 s; worst error / bar per entry (cases): dL/dcoords 0.010 (48), dL/dfeatures 0.010 (24),
atom-wise dL/dradii 0.011 (21), dL/dradii by channel or type 2.7e-4 (4), dL/d(scalar radius) 1.1e-4 (5), dL/dsigma 2.9e-4 (16),
pose rows through the grids and through the scores c 5.5e-4 (48 each), q 7.2e-4 (27), t 6.7e-4 (27), through the moments c 1.1e-4,
q 3.7e-4, t 1.8e-4 (18 each), of the views c 4.4e-4, q 2.7e-4, t 7.7e-4 (12 each) and 1.4e-5 of the summation-order rule against
the clean call (36), atom scores 4.8e-3 (17), molecule scores 4.3e-4 (17), view scores 2.2e-4 (12), moments 9.4e-4 (22), dL/dsigma
and dL/d(scalar radius) beside a non-finite pose 7.3e-5 (4) and 7.1e-5 (2),
moments gradient rows 0.012 (96), dS/dfield 0.99 (8; the half ulp of the bfloat16 rounding, which is the bar's own term for such
a field). The bit identities have no figure. The module prints these under -s.
"""
import functools

import numpy as np
import pytest

from tests import dead_atom_rows as R
from tests import density_reference as dref
from tests import entry_drivers as X
from tests import entry_fuzz_rows as E
from tests import grad_reference as gr
from tests import hip_support as hip
from tests import moments_grad_reference as MG
from tests import moments_reference as MR
from tests import pose_reference as pr
from tests import score_reference as sr
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL, P64_TOL, assert_exact, assert_gaussian

pytestmark = pytest.mark.gpu

BF16_HALF_ULP = 2.0 ** -8  # (tests/test_hip_sum.py: the final rounding of a bfloat16 field gradient)
_W = X.Worst()  # entry -> worst error / bar, and the cases
POSE_KEYS = (("center", "cen"), ("quaternion", "q"), ("translation", "t"))

ALL = R.ROW_IDS
POSED = [i for i in ALL if R.ROWS[i][5] == "posed"]
# forward_sum / moments_batch: float32 sums, no channel-wise radii with features, no blockdim through the sub-tiles
SUMMED = [i for i in ALL if R.ROWS[i][3] != "f64" and R.ROWS[i][7] == "d16" and R.ROWS[i][:2] != ("features", "channel-wise")]


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\n" + "\n".join(f"{k:>28s}: worst error / bar {v:.3g} over {_W.cases[k]} cases" for k, v in sorted(_W.worst.items())))


_note = _W.note


def _close(entry, d, got, ref, bound, what, exact_terms=False):
    """The gradient rule with the bars of the row's precision; the worst error / bar goes into the report under `entry`."""
    _W.close(entry, d, got, ref, bound, f"{d['seed']}: {what}", exact_terms)


def _pair(row_id):
    import torch

    r = R.row(row_id)
    return r, R.dirty(r), R.clean(r), torch.tensor(R.live(r), device="cuda")


def _field(d):
    """(the row's field on the device in the grid's type, the float64 array the kernels read)."""
    import torch

    Fref = E.field_of(d)
    return torch.tensor(Fref, device="cuda").to(hip.grid_dtype(d)), Fref


def _upstream(d, F):
    """dL/dgrid = the field, laid out per molecule: the gradients of sum_b S_b."""
    return F.expand((d["B"],) + tuple(F.shape)).contiguous() if F.dim() == 4 else F


def _same_rows(got, want, live, what):
    """got[live] is want bit for bit, got[~live] is zero, nothing is NaN."""
    import torch

    assert not bool(torch.isnan(got).any()), f"{what}: NaN in the dirty call"
    assert torch.equal(got[live], want), f"{what}: the live rows differ from the clean call's"
    assert not bool(got[~live].any()), f"{what}: a dead atom has a non-zero row"


def _kw(d):
    return dict(res=d["res"], sigma=d["sigma"], blockdim=d["blockdim"], density=d["density"], precision=d["precision"])


@functools.lru_cache(maxsize=None)
def _reference(row_id):
    """The float64 references of the CLEAN batch with dL/dgrid_b = the row's field (computed once, never modified): positions,
    scores, per molecule the gradient rows and the pose gradients, and over the call dL/dsigma and the radius gradients."""
    r = R.row(row_id)
    c = R.clean(r)
    F = E.field_of(c)
    p = R.positions_of(c)
    w, types = E.reference_channels(c)
    quats = E.quaternions_of(c)
    s_ref, b_ref, S_ref, Sb_ref = sr.batch_reference(p, c["off"], F, c["radii"], c["radii_type"], w=w, mode=c["mode"], types=types, **_kw(c))
    by_type = c["mode"] == "types" and c["radii_type"] == "channel-wise"
    mols, tot = [], {}
    for b in range(c["B"]):
        lo, hi, radii = E.molecule(c, b)
        if hi == lo:
            mols.append(None)
            continue
        G = F if F.ndim == 4 else F[b]
        mk = dict(w=None if w is None else w[lo:hi], mode=c["mode"], types=None if types is None else types[lo:hi])
        o = gr.reference(p[lo:hi], G, radii, c["radii_type"], radii_by_type=by_type, **mk, **_kw(c))
        M = pr.rotation(quats[b])
        gp, bp = o["coords"]
        o["rows"] = (gp @ M, bp @ np.abs(M))  # dL/dcoords = M^T dL/dp
        o["pose"] = pr.pose_grads(c["xyz"][lo:hi], c["cen"][b], quats[b], gp, bp) if c["density"] == "gaussian" else None
        mols.append(o)
        if c["density"] == "gaussian":
            kw = {k: v for k, v in _kw(c).items() if k not in ("sigma", "precision")}
            dg = dref.density_grads(p[lo:hi], G, radii, c["radii_type"], sigma=c["sigma"], precision=c["precision"], **mk, **kw)
            if c["radii_type"] == "channel-wise":
                dg["radii"] = o["radii"]
            o["call"] = dg  # this molecule's share of the reductions over the call
            for k, (v, bnd) in dg.items():
                tv, tb = tot.get(k, (0.0, 0.0))
                tot[k] = (tv + v, tb + bnd)
    return dict(p=p, F=F, atoms=(s_ref, b_ref), scores=(S_ref, Sb_ref), mols=mols, call=tot, quats=quats)


# ---- 1. grids ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [0, 1], ids=["binned", "direct"])
@pytest.mark.parametrize("row_id", ALL)
def test_grids_of_the_dirty_batch_are_the_clean_batchs(row_id, direct):
    import torch

    r, d, c, live = _pair(row_id)
    vox = X.vox(d)
    vox.debug_option("direct", direct)
    got, want = X.forward(vox, d, X.inputs(d)), X.forward(vox, c, X.inputs(c))
    assert got.dtype == hip.grid_dtype(d) and tuple(got.shape) == (d["B"], d["C"]) + (d["D"],) * 3
    assert torch.equal(got, want), f"{int((got != want).sum())} voxels differ"
    for b, n in enumerate(R.LIVE):
        assert bool(got[b].any()) == (n > 0), b  # the all-dead molecule and the empty one: zeros
    if direct:
        return
    if d["kind"] == "bf16":  # a bfloat16 grid is the float32 grid rounded once (tests/test_hip_bf16.py); that one meets the oracle
        base = X.forward(X.vox(d, "f32"), c, X.inputs(c))
        assert torch.equal(want, base.to(torch.bfloat16))
        want = base
    want = want.cpu().numpy()
    p = _reference(row_id)["p"]
    for b in range(c["B"]):
        ref = R.oracle_grid(c, p, b)
        if c["density"] == "binary" and c["mode"] != "features":
            assert_exact(want[b], ref)
        else:
            assert_gaussian(want[b], ref, *(() if c["precision"] == 32 else (P64_TOL,)))
    _note("grids", 0.0)


@pytest.mark.parametrize("variant", ["channels_last", "numpy", "chunks"])
@pytest.mark.parametrize("row_id", ["feat-atom-bf16-tail-posed", "types-scalar-f32-scattered-rot", "feat-atom-f32-scattered-centred"])
def test_grids_in_other_layouts_from_host_arrays_and_in_molecule_chunks(row_id, variant):
    import torch

    r, d, c, live = _pair(row_id)
    base = X.forward(X.vox(d), c, X.inputs(c))
    if variant == "channels_last":
        vox = X.vox(d, grid_layout="channels_last")
        got, want = X.forward(vox, d, X.inputs(d)), X.forward(vox, c, X.inputs(c))
        assert got.is_contiguous(memory_format=torch.channels_last_3d)
    elif variant == "numpy":
        vox = X.vox(d, "f32", output="numpy")
        got, want = X.forward(vox, d, X.inputs(d, host=True)), X.forward(vox, c, X.inputs(c, host=True))
        assert isinstance(got, np.ndarray)
        got, want = torch.tensor(got, device="cuda"), torch.tensor(want, device="cuda")
        base = X.forward(X.vox(d, "f32"), c, X.inputs(c))
    else:
        vox = X.vox(d)
        vox.debug_option("direct", 0)
        # a cache budget of 16 KB cuts these five molecules into several launches (mvx_plan.hip: ceil(workspace / budget) chunks,
        # at most one per molecule). tests/test_hip_batch_cuts.py uses this option and "chunks", which cuts only batches of
        # 4 x chunks molecules or more - eight for two chunks, and the rows have five.
        vox.debug_option("mall_budget_kb", 16)
        got = X.forward(vox, d, X.inputs(d))
        assert 2 <= vox.last_plan()["nchunk"] <= d["B"]  # cut into several launches, the all-dead molecule in one of them
        want = X.forward(vox, c, X.inputs(c))
    assert torch.equal(got, want) and torch.equal(got, base)
    _note("grids", 0.0)


# ---- 2. summed grids and moments -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", SUMMED)
def test_summed_grids_of_the_dirty_batch_are_the_clean_batchs(row_id):
    import torch

    from oracle import c_oracle

    r, d, c, live = _pair(row_id)
    vox = X.vox(d)
    rng = np.random.default_rng(r["fseed"] + 5)
    wb = rng.uniform(0.5, 1.5, d["B"]).astype(np.float32)
    wa = rng.uniform(0.5, 1.5, d["N"]).astype(np.float32)
    wa[~R.live(r)] = np.nan  # the dead atoms' weights are NaN
    plain = None
    for name, wd, wc in (("none", None, None), ("molecule", wb, wb), ("atom", wa, wa[R.live(r)])):
        got, want = X.sum(vox, d, X.inputs(d), hip.dev(wd)), X.sum(vox, c, X.inputs(c), hip.dev(wc))
        assert got.dtype == torch.float32 and not bool(torch.isnan(got).any()), name
        assert torch.equal(got, want), (name, int((got != want).sum()))
        assert bool(got.any())
        plain = want if name == "none" else plain
    p = _reference(row_id)["p"]
    merged = c_oracle.voxelize(p, R.weights_of(c), c["r_atom"].astype(np.float32), resolution=c["res"], dimension=c["D"],
                               density=c["density"], blockdim=c["blockdim"], sigma=c["sigma"], radii_type="atom-wise")
    # tests/test_hip_sum_sweep.py's rule for the merged cloud: binary bit for bit, Gaussian by the project's one rule
    if c["density"] == "binary":
        assert_exact(plain.cpu().numpy(), merged)
    else:
        assert_gaussian(plain.cpu().numpy(), merged)
    assert float(np.abs(merged).max()) > 0
    _note("forward_sum", 0.0)


def _entry(vox, call, gm, target):
    """mvx_moments_backward_batch through ctypes: (grad_coords, grad_features or None) in buffers that start as NaN (the call of
    tests/test_hip_moments_grad.py's helper of the same name, restated here so that this file stands on its own)."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    g = torch.tensor(np.ascontiguousarray(gm, np.float64), device="cuda")
    assert tuple(g.shape) == (call.B, call.C, 2 if target is None else 3)
    gc, gf = hip.nan((call.N, 3)), (hip.nan((call.N, call.C), torch.float32) if call.mode == "features" else None)
    _lib.check(vox._lib.mvx_moments_backward_batch(*call.batch_args(vox), hip.ptr(target), g.data_ptr(), gc.data_ptr(), hip.ptr(gf),
                                                   vox._stream()))
    return gc, gf


def _target(d):
    return np.random.default_rng(d["fseed"] + 9).standard_normal((d["C"],) + (d["D"],) * 3).astype(np.float32)


@pytest.mark.parametrize("row_id", SUMMED)
def test_moments_and_their_gradient_rows(row_id):
    import torch

    r, d, c, live = _pair(row_id)
    vox = X.vox(d)
    T = hip.dev(_target(c))
    ad, ac = X.inputs(d), X.inputs(c)
    g32 = X.forward(X.vox(c, "f32"), c, ac).cpu().numpy()
    ref, bnd = MR.moments_and_bound(g32, _target(c))
    for t, K in ((None, 2), (T, 3)):
        got, want = X.moments(vox, d, ad, t), X.moments(vox, c, ac, t)
        assert got.dtype == torch.float64 and torch.equal(got, want), K
        g = got.cpu().numpy()
        err, b = np.abs(g - ref[..., :K]), bnd[..., :K]
        assert (err <= b).all(), K
        _note("moments", float((err[b > 0] / b[b > 0]).max()))
        assert not g[[R.EMPTY_MOL, R.ALL_DEAD_MOL]].any()
    # mvx_moments_backward_batch: per-atom rows in buffers that start as NaN
    p, quats = _reference(row_id)["p"], _reference(row_id)["quats"]
    w, types = E.reference_channels(c)
    sd, sc = X.spec(vox, d, ad), X.spec(vox, c, ac)
    for K in (3, 2):
        gm = np.random.default_rng(r["fseed"] + K).standard_normal((d["B"], d["C"], K))
        (gcd, gfd), (gcc, gfc) = _entry(vox, sd, gm, T if K == 3 else None), _entry(vox, sc, gm, T if K == 3 else None)
        _same_rows(gcd, gcc, live, f"moments gradient, K = {K}: coordinates")
        if gfd is not None:
            _same_rows(gfd, gfc, live, f"moments gradient, K = {K}: features")
        gc = gcc.cpu().numpy()
        for b in range(c["B"]):
            lo, hi, radii = E.molecule(c, b)
            if hi == lo:
                continue
            mine = list(range(0, hi - lo, max(1, (hi - lo) // 24)))  # a sample; the reference needs the whole molecule's grid only
            G, Gabs = MG.upstream(g32[b], gm[b], _target(c) if K == 3 else None)
            rkw = dict(w=None if w is None else w[lo:hi], mode=c["mode"], types=None if types is None else types[lo:hi], atoms=mine,
                       rot=pr.rotation(quats[b]), **_kw(c))
            val = gr.reference(p[lo:hi], G, radii, c["radii_type"], **rkw)
            bound = gr.reference(p[lo:hi], Gabs, radii, c["radii_type"], **rkw)
            _close("moments gradient rows", c, gc[np.array(mine) + lo], val["coords"][0], bound["coords"][1], f"K = {K}, molecule {b}")
            if gfc is not None:
                _close("moments gradient rows", c, gfc.cpu().numpy()[np.array(mine) + lo], val["features"][0], bound["features"][1],
                       f"K = {K}, molecule {b}: features")


# ---- 3. scores, their rows, the backward entry and dS/dfield -----------------------------------------------------------------------
def _abi_rows(vox, d, Fd, G=None):
    """mvx_score_batch and mvx_backward_batch (grad_out = the field laid out per molecule, or G) through ctypes on one call
    record. Outputs start as NaN: whatever is not overwritten fails every comparison."""
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
    G = _upstream(d, Fd) if G is None else G
    ref = dict(gc=hip.nan((N, 3)), gf=hip.nan((N, C_), fdt) if feat else None)
    _lib.check(vox._lib.mvx_backward_batch(*call.batch_args(vox), G.data_ptr(), hip.ptr(ref["gc"]), hip.ptr(ref["gf"]), vox._stream()))
    torch.cuda.synchronize()
    return out, ref


def _lanes_kept(r, scope):
    """Does the placement keep every live atom on its lane in a reduction per molecule / per call?"""
    return r["placement"] in (("tail", "call_tail") if scope == "molecule" else ("call_tail",))


@pytest.mark.parametrize("row_id", ALL)
def test_scores_their_rows_and_the_backward_entry(row_id):
    import torch

    r, d, c, live = _pair(row_id)
    vox = X.vox(d)
    Fd, _ = _field(c)
    ref = _reference(row_id)
    Sd, sd = X.score(vox, d, X.inputs(d), Fd, per_atom=True)
    Sc, sc = X.score(vox, c, X.inputs(c), Fd, per_atom=True)
    _same_rows(sd, sc, live, "atom scores")
    assert bool(torch.isfinite(Sd).all())
    exact = c["density"] == "binary" and c["mode"] != "features"
    _close("molecule scores", c, Sd.cpu().numpy(), *ref["scores"], "molecule scores of the dirty batch", exact)
    _close("atom scores", c, sc.cpu().numpy(), *ref["atoms"], "atom scores", exact)
    if _lanes_kept(r, "molecule"):
        assert torch.equal(Sd, Sc)
    assert not bool(Sd[[R.EMPTY_MOL, R.ALL_DEAD_MOL]].any())
    (gd, bd), (gc_, bc) = _abi_rows(vox, d, Fd), _abi_rows(vox, c, Fd)
    assert torch.equal(gd["scores"], Sd) and torch.equal(gd["atoms"], sd)
    for k in ("gc", "gf"):
        if gd[k] is not None:
            _same_rows(gd[k], gc_[k], live, f"mvx_score_batch {k}")
            _same_rows(bd[k], bc[k], live, f"mvx_backward_batch {k}")
            assert torch.equal(gd[k], bd[k])
    rows, feats = gc_["gc"].cpu().numpy(), None if gc_["gf"] is None else gc_["gf"].double().cpu().numpy()
    for b, o in enumerate(ref["mols"]):
        if o is None:
            continue
        lo, hi, _ = E.molecule(c, b)
        if c["density"] == "gaussian":
            _close("dL/dcoords", c, rows[lo:hi], *o["rows"], f"molecule {b}")
        else:
            assert not rows[lo:hi].any()
        if feats is not None:
            _close("dL/dfeatures", c, feats[lo:hi], *o["features"], f"molecule {b}")


@pytest.mark.parametrize("row_id", [i for i in SUMMED if not R.row(i)["per_mol"]])
def test_the_field_gradient_of_the_dirty_batch_is_the_clean_batchs(row_id):
    import torch

    r, d, c, live = _pair(row_id)
    vox = X.vox(d, differentiable=True, field_grad=True)
    Fd, _ = _field(c)
    g = np.random.default_rng(r["fseed"] + 1).standard_normal(d["B"])
    grads = []
    for x in (d, c):
        field = Fd.clone().requires_grad_()
        (X.score(vox, x, X.inputs(x), field) * hip.dev(g)).sum().backward()
        grads.append(field.grad)
    assert grads[0].dtype == Fd.dtype and not bool(torch.isnan(grads[0]).any())
    assert torch.equal(grads[0], grads[1]), int((grads[0] != grads[1]).sum())
    grids = X.forward(X.vox(c, "f32"), c, X.inputs(c)).to(torch.float64)
    gw = torch.tensor(g, device="cuda").reshape(-1, 1, 1, 1, 1)
    want, bound = (gw * grids).sum(0).cpu().numpy(), (gw.abs() * grids.abs()).sum(0).cpu().numpy()
    err = np.abs(grads[0].to(torch.float64).cpu().numpy() - want)
    bar = GRAD_REL * bound + GRAD_ABS + (BF16_HALF_ULP * bound if d["kind"] == "bf16" else 0.0)  # (tests/test_hip_sum.py's rule)
    _note("dS/dfield", float((err / bar).max()))
    assert float((err / bar).max()) <= 1.0 and float(bound.max()) > 0


# ---- 4. autograd: per-atom rows, pose rows and the reductions over the call ----------------------------------------------------------
def _backward(row_id, d, entry, upstream=None):
    """One differentiable call of `entry` ("grid" | "score") on a voxelizer with radii_grad and sigma_grad and everything that can
    require grad doing so; L = <field, grid> (sum of the scores). Returns the leaves and the sigma tensor."""
    import torch

    sigma = torch.tensor(d["sigma"], dtype=torch.float64, requires_grad=True)
    grid_entry = entry == "grid"
    kw = dict(radii_grad=True, sigma_grad=True, sigma=sigma) if grid_entry else {}
    vox = X.vox(d, differentiable=True, **kw)
    a = X.inputs(d, grad=True, radii_grad=grid_entry)
    Fd, _ = _field(d)
    if grid_entry:
        grid = X.forward(vox, d, a)
        grid.backward(gradient=_upstream(d, Fd) if upstream is None else upstream)
    else:
        X.score(vox, d, a, Fd).sum().backward()
    a["sigma"] = sigma
    return a


def _check_reductions(row_id, r, d, c, got, want, live, entry):
    import torch

    ref = _reference(row_id)
    gauss = c["density"] == "gaussian"
    _same_rows(got["xyz"].grad, want["xyz"].grad, live, f"{entry}: coords.grad")
    if c["mode"] == "features":
        _same_rows(got["chan"].grad, want["chan"].grad, live, f"{entry}: features.grad")
    names = POSE_KEYS if c["posed"] else POSE_KEYS[:1]
    for name, key in names:
        rows = got[key].grad
        assert rows is not None and bool(torch.isfinite(rows).all()), f"{entry}: {key}.grad is not finite: {rows}"
        if _lanes_kept(r, "molecule") and c["posed"]:  # (the centre of a batch that is only centred: a sum outside the library)
            assert torch.equal(rows, want[key].grad), f"{entry}: {key}.grad differs from the clean call's"
        for b, o in enumerate(ref["mols"]):
            row = rows[b].double().cpu().numpy()
            if o is None or not gauss:
                assert not row.any(), (entry, key, b)  # no live atom, or a binary density: zero rows
            elif c["posed"]:
                _close(f"{entry}: pose {key}", c, row, *o["pose"][name], f"dL/d{name} of molecule {b}")
            else:
                val, bound = o["rows"]
                _close(f"{entry}: pose {key}", c, row, -val.sum(0), bound.sum(0), f"dL/dcenter of molecule {b}")
    if entry != "grid":
        return
    # the radius and sigma gradients of the same backward
    rg, rw = got["radii"].grad, want["radii"].grad
    assert rg is not None and bool(torch.isfinite(rg).all()), f"radii.grad is not finite: {rg}"
    if c["radii_type"] == "atom-wise":
        _same_rows(rg, rw, live, "radii.grad")
        have = rw.double().cpu().numpy()
        for b, o in enumerate(ref["mols"]):
            if o is not None and gauss:
                lo, hi, _ = E.molecule(c, b)
                _close("dL/dradii (atom-wise)", c, have[lo:hi], *o["radii"], f"molecule {b}")
    elif gauss:
        key, what = ("radius", "dL/d(scalar radius)") if c["radii_type"] == "scalar" else ("radii", "dL/dradii (channel, type)")
        _close(what, c, rg.double().cpu().numpy().reshape(-1), *(np.atleast_1d(v) for v in ref["call"][key]), what)
        if _lanes_kept(r, "call"):
            assert torch.equal(rg, rw), what
    sg, sw = got["sigma"].grad, want["sigma"].grad
    assert sg is not None and bool(torch.isfinite(sg).all())
    if gauss:
        _close("dL/dsigma", c, sg.double().cpu().numpy().reshape(-1), *(np.atleast_1d(v) for v in ref["call"]["sigma"]), "dL/dsigma")
        assert float(sg) != 0.0
    else:
        assert float(sg) == 0.0 and not bool(rg.any())
    if _lanes_kept(r, "call"):
        assert torch.equal(sg, sw), "dL/dsigma differs from the clean call's"


@pytest.mark.parametrize("entry", ["grid", "score"])
@pytest.mark.parametrize("row_id", ALL)
def test_backward_through_the_grids_and_the_scores(row_id, entry):
    """forward_batch / forward_posed_batch(...).backward() with radii and sigma gradients, and score_batch /
    score_posed_batch(...).sum().backward(): the live rows bit for bit, zero rows for the dead atoms, finite pose rows, and the
    reductions against the clean batch's float64 reference."""
    r, d, c, live = _pair(row_id)
    got, want = _backward(row_id, d, entry), _backward(row_id, c, entry)
    _check_reductions(row_id, r, d, c, got, want, live, entry)


@pytest.mark.parametrize("row_id", [i for i in SUMMED if i in POSED])
def test_backward_through_the_posed_moments(row_id):
    import torch

    r, d, c, live = _pair(row_id)
    vox = X.vox(d, differentiable=True, moments_grad=True)
    T = hip.dev(_target(c))
    gm = torch.tensor(np.random.default_rng(r["fseed"] + 3).standard_normal((d["B"], d["C"], 3)), device="cuda")
    out = []
    for x in (d, c):
        a = X.inputs(x, grad=True)
        m = X.moments(vox, x, a, T)
        assert m.requires_grad
        (m * gm).sum().backward()
        out.append(a)
    got, want = out
    _same_rows(got["xyz"].grad, want["xyz"].grad, live, "moments: coords.grad")
    if c["mode"] == "features":
        _same_rows(got["chan"].grad, want["chan"].grad, live, "moments: features.grad")
    g32 = X.forward(X.vox(c, "f32"), c, X.inputs(c)).cpu().numpy()
    p, quats = _reference(row_id)["p"], _reference(row_id)["quats"]
    w, types = E.reference_channels(c)
    for b in range(c["B"]):
        lo, hi, radii = E.molecule(c, b)
        rows = {key: got[key].grad[b].cpu().numpy() for _, key in POSE_KEYS}
        assert all(np.isfinite(v).all() for v in rows.values()), (b, rows)
        if _lanes_kept(r, "molecule"):
            assert all(torch.equal(got[key].grad[b], want[key].grad[b]) for _, key in POSE_KEYS), b
        if hi == lo:
            assert not any(v.any() for v in rows.values()), b
            continue
        G, Gabs = MG.upstream(g32[b], gm[b].cpu().numpy(), _target(c))
        rkw = dict(w=None if w is None else w[lo:hi], mode=c["mode"], types=None if types is None else types[lo:hi], **_kw(c))
        val = gr.reference(p[lo:hi], G, radii, c["radii_type"], **rkw)["coords"][0]
        bound = gr.reference(p[lo:hi], Gabs, radii, c["radii_type"], **rkw)["coords"][1]
        o = pr.pose_grads(c["xyz"][lo:hi], c["cen"][b], quats[b], val, bound)
        for name, key in POSE_KEYS:
            _close(f"moments: pose {key}", c, rows[key], *o[name], f"dL/d{name} of molecule {b}")


# ---- 5. one shared cloud: views ------------------------------------------------------------------------------------------------------
def _cloud_pair(cloud_id):
    import torch

    c = R.cloud(cloud_id)
    return c, R.dirty_cloud(c), R.clean_cloud(c), torch.tensor(R.live(c), device="cuda")


def _view_args(x, grad=False):
    return (hip.dev(x["xyz"], grad), hip.dev(x["cen"], grad), hip.dev(x["q"], grad), hip.dev(x["t"], grad), hip.dev(x["chan"]), hip.dev(x["radii"]))


def _radius_dead(c):
    """The dead atoms the box cull lets through (module docstring): an atom-wise radius of 0, -1 or inf inside the box."""
    return np.isin(c["dead_kind"], ["r 0", "r -1", "r inf"])


@pytest.mark.parametrize("cloud_id", R.CLOUD_IDS)
def test_views_of_a_cloud_with_dead_atoms(cloud_id):
    import torch

    from tests import views_reference as vr

    c, d, k, live = _cloud_pair(cloud_id)
    vox = X.vox(d)
    nc = hip.nc(d)
    got, want = vox.forward_posed_views(*_view_args(d), num_channels=nc), vox.forward_posed_views(*_view_args(k), num_channels=nc)
    assert torch.equal(got, want) and all(bool(want[b].any()) for b in range(c["B"]))
    rep = R.repeated(d)
    assert torch.equal(got, X.forward(vox, rep, X.inputs(rep)))  # ... and forward_posed_batch on the repeated dirty cloud
    if d["precision"] == 32 and not (d["mode"] == "features" and d["radii_type"] == "channel-wise"):
        w = hip.dev(np.random.default_rng(c["fseed"]).uniform(0.5, 1.5, c["B"]).astype(np.float32))
        for weights in (None, w):
            sd = vox.forward_posed_views_sum(*_view_args(d), weights=weights, num_channels=nc)
            sk = vox.forward_posed_views_sum(*_view_args(k), weights=weights, num_channels=nc)
            assert torch.equal(sd, sk) and bool(sd.any()) and not bool(torch.isnan(sd).any())
    # the same under identity views (forward_views / forward_views_sum: the cloud seen from each centre)
    plain = lambda x: (hip.dev(x["xyz"]), hip.dev(x["cen"]), hip.dev(x["chan"]), hip.dev(x["radii"]))  # noqa: E731
    gv, wv = vox.forward_views(*plain(d), num_channels=nc), vox.forward_views(*plain(k), num_channels=nc)
    assert torch.equal(gv, wv) and bool(wv.any())
    if d["precision"] == 32 and not (d["mode"] == "features" and d["radii_type"] == "channel-wise"):
        assert torch.equal(vox.forward_views_sum(*plain(d), num_channels=nc), vox.forward_views_sum(*plain(k), num_channels=nc))
    # select_views / select_posed_views take no channel count and count the channels from the types they are given, so a type C
    # or C + 2 names a channel there: on the types cloud the selection is the one forward_views and score_views make, with the
    # call's channel count (_select_views); the other clouds go through the public entries
    def select(x, posed):
        xyz, cen, q, t, chan, radii = _view_args(x)
        if d["mode"] == "types":
            return vox._select_views(xyz, cen, chan, radii, num_channels=nc, posed=(q, t) if posed else None)
        return vox.select_posed_views(xyz, cen, q, t, chan, radii) if posed else vox.select_views(xyz, cen, chan, radii)

    i1, o1 = select(d, False)
    i2, o2 = select(k, False)
    i1 = i1.cpu().numpy()
    assert np.array_equal((np.cumsum(R.live(c)) - 1)[i1[R.live(c)[i1]]], i2.cpu().numpy())
    assert not (~R.live(c)[i1] & ~_radius_dead(c)[i1]).any() and (_radius_dead(c).any() or np.array_equal(o1, o2))
    # the selection: the clean selection after mapping to the dirty numbering, plus - atom-wise radii only - the dead atoms the box
    # cull lets through; it is the reference selection of the dirty cloud
    index, offsets = select(d, True)
    kindex, koffsets = select(k, True)
    idx = index.cpu().numpy()
    with np.errstate(all="ignore"):
        p = pr.view_positions(d["xyz"], d["cen"], d["q"], d["t"])
        ref_index, ref_offsets = vr.select_exact(p, d["res"], d["D"], R.view_source(d), d["radii"], d["precision"],
                                                 types=d["chan"] if d["mode"] == "types" else None, num_channels=nc)
    assert vr.selection_mismatch(idx, np.asarray(offsets), ref_index, ref_offsets) is None
    alive = R.live(c)[idx]
    assert not (~alive & ~_radius_dead(c)[idx]).any()  # no dead coordinate, NaN radius or type outside [0, C) is ever selected
    to_clean = np.cumsum(R.live(c)) - 1
    view = np.repeat(np.arange(c["B"]), np.diff(np.asarray(offsets)))
    assert np.array_equal(to_clean[idx[alive]], kindex.cpu().numpy())
    assert np.array_equal(np.bincount(view[alive], minlength=c["B"]).cumsum(), np.asarray(koffsets)[1:])
    if not _radius_dead(c).any():
        assert np.array_equal(np.asarray(offsets), np.asarray(koffsets))

    # score_posed_views: scores, atom scores in selection order, and - through autograd - the rows reduced onto the shared cloud
    Fd, Fref = _field(d)
    dvox = X.vox(d, differentiable=True)
    res = []
    for x in (d, k):
        a = _view_args(x, grad=True)
        S, s, ix, off = dvox.score_posed_views(*a[:4], a[4], a[5], Fd, num_channels=nc, per_atom=True)
        (S.sum() + 0.5 * s.sum()).backward()
        res.append((S, s, ix, a))
    (Sd, sd, ixd, ad), (Sk, sk, ixk, ak) = res
    assert torch.equal(ixd, index)
    keep = torch.tensor(alive, device="cuda")
    assert torch.equal(sd[keep], sk) and not bool(sd[~keep].any()) and not bool(torch.isnan(sd).any())
    _same_rows(ad[0].grad, ak[0].grad, live, "score_posed_views: coords.grad (views_reduce)")
    pk = pr.view_positions(k["xyz"], k["cen"], k["q"], k["t"])
    w, types = E.reference_channels(k)
    for b in range(c["B"]):
        s_ref, b_ref, S_ref, Sb_ref = sr.batch_reference(pk[b], np.array([0, k["N"]]), Fref, k["radii"], k["radii_type"], w=w, mode=k["mode"],
                                                         types=types, **_kw(k))
        _close("view scores", k, Sd[b:b + 1].detach().cpu().numpy(), S_ref, Sb_ref, f"view {b}")
    # dS/dc, dS/dq, dS/dt of every view, L = sum_b S_b + 0.5 sum_k s_k (dL/dgrid = 1.5 F): against tests/pose_reference.py on the
    # clean cloud under the pose bar, and against the clean call's rows under tests/test_hip_pose.py's summation-order rule, its
    # scale the reference's bound (the sum of the absolute values of the terms, voxel by voxel)
    for b in range(c["B"]):
        gp, bp = gr.reference(pk[b], 1.5 * Fref, k["radii"], k["radii_type"], w=w, mode=k["mode"], types=types, **_kw(k))["coords"]
        o = pr.pose_grads(k["xyz"], k["cen"][b], k["q"][b], gp, bp)
        for (name, _), key in zip(POSE_KEYS, (1, 2, 3)):
            x, y = ad[key].grad[b].cpu().numpy(), ak[key].grad[b].cpu().numpy()
            assert np.isfinite(x).all() and np.all(o[name][1] > 0), (b, name, x)
            _close(f"views: pose {'cqt'[key - 1]}", k, x, *o[name], f"dS/d{name} of view {b}")
            excess = np.abs(x - y) / (1e-12 * np.abs(y) + 1e-12 * o[name][1])
            _note("views: pose rows against the clean call", float(excess.max()))
            assert np.all(excess <= 1.0), (b, name, x, y)
    if not _radius_dead(c).any():  # nothing dead is selected: every view reduction sees the clean call's batch
        assert torch.equal(Sd, Sk) and all(torch.equal(ad[key].grad, ak[key].grad) for key in (1, 2, 3))
    else:
        assert _radius_dead(c)[idx].any()  # (the reason written in the module docstring does occur)


@pytest.mark.parametrize("cloud_id", R.CLOUD_IDS)
def test_posed_views_and_the_posed_batch_on_the_repeated_dirty_cloud_agree(cloud_id):
    """score_posed_views is score_posed_batch on the repeated cloud - the scores and dS/dc, dS/dq, dS/dt
    within the summation-order rules of tests/test_hip_pose.py, here on a cloud with dead atoms: the batch's pose_grad_kernel sees
    the dead atoms' coordinates, the views' does not."""
    import torch

    c, d, k, live = _cloud_pair(cloud_id)
    vox = X.vox(d, differentiable=True)
    Fd, _ = _field(d)
    nc = hip.nc(d)
    a = _view_args(d, grad=True)
    S = vox.score_posed_views(*a, Fd, num_channels=nc)
    S.sum().backward()
    rep = R.repeated(d)
    b_ = X.inputs(rep, grad=True)
    S2, s2 = X.score(vox, rep, b_, Fd, per_atom=True)
    S2.sum().backward()
    # (tests/test_hip_score_views.py's rule: dropping the zero rows of the atoms a view does not keep regroups a float64 sum)
    bound = s2.detach().abs().reshape(c["B"], d["N"]).sum(1)
    assert bool(((S - S2).abs() <= GRAD64_REL * bound + GRAD64_ABS).all()) and bool(torch.isfinite(S).all()) and bool(S.any())
    gc2 = b_["xyz"].grad.cpu().numpy().reshape(c["B"], d["N"], 3)
    assert not gc2[:, ~R.live(c)].any()
    fin = np.isfinite(d["xyz"]).all(axis=1)
    for v in range(c["B"]):
        o = pr.from_coords_grad(d["xyz"][fin], d["cen"][v], d["q"][v], gc2[v][fin])  # (the scale of the summation-order rule)
        for name, got, ref in (("center", a[1], b_["cen"]), ("quaternion", a[2], b_["q"]), ("translation", a[3], b_["t"])):
            x, y = got.grad[v].cpu().numpy(), ref.grad[v].cpu().numpy()
            assert np.isfinite(y).all(), (v, name, "score_posed_batch", y)
            assert np.isfinite(x).all() and np.any(y != 0), (v, name, x, y)
            assert np.all(np.abs(x - y) <= 1e-12 * np.abs(y) + 1e-12 * o[name][1]), (v, name, x, y)
    total, scale = gc2.sum(0), np.abs(gc2).sum(0)
    assert np.all(np.abs(a[0].grad.cpu().numpy() - total) <= 1e-12 * np.abs(total) + 1e-12 * scale)
    _note("views against the batch", 0.0)


# ---- 6. a non-finite pose ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["q", "t"])
@pytest.mark.parametrize("row_id", ["feat-scalar-f32-scattered-posed", "types-atom-f64-scattered-posed"])
def test_a_molecule_with_a_non_finite_pose_contributes_nothing(row_id, where):
    """Molecule 2 of the clean batch gets a NaN in q or t: its grid, score, moments and gradient rows (mvx_score_batch,
    mvx_backward_batch, mvx_moments_backward_batch, autograd, atom-wise dL/dradii) are zero, everything of the other molecules keeps
    its bits, and dL/dsigma and dL/d(scalar radius) are the other molecules' within their bars. Its own pose row is unspecified (like q = 0) and not looked at."""
    import torch

    r, _, c, _ = _pair(row_id)
    b = 2
    bad = dict(c)
    pose = np.array(c[where])
    pose[b, 1] = np.nan
    bad[where] = pose
    lo, hi, _ = E.molecule(c, b)
    others = [m for m in range(c["B"]) if m != b]
    mine = torch.zeros(c["N"], dtype=torch.bool, device="cuda")
    mine[lo:hi] = True
    vox = X.vox(c)
    Fd, _ = _field(c)
    got, want = X.forward(vox, bad, X.inputs(bad)), X.forward(vox, c, X.inputs(c))
    assert not bool(got[b].any()) and torch.equal(got[others], want[others]) and bool(want[b].any())
    (Sg, sg), (Sw, sw) = X.score(vox, bad, X.inputs(bad), Fd, per_atom=True), X.score(vox, c, X.inputs(c), Fd, per_atom=True)
    assert float(Sg[b]) == 0.0 and torch.equal(Sg[others], Sw[others]) and float(Sw[b]) != 0.0
    assert not bool(sg[mine].any()) and torch.equal(sg[~mine], sw[~mine])
    if c["precision"] == 32:
        mg, mw = X.moments(vox, bad, X.inputs(bad), hip.dev(_target(c))), X.moments(vox, c, X.inputs(c), hip.dev(_target(c)))
        assert not bool(mg[b].any()) and torch.equal(mg[others], mw[others]) and bool(mw[b].any())
    (gb, bb), (gw, bw) = _abi_rows(vox, bad, Fd), _abi_rows(vox, c, Fd)
    for k in ("gc", "gf"):
        for x, y in ((gb[k], gw[k]), (bb[k], bw[k])):
            if x is not None:
                assert not bool(x[mine].any()) and torch.equal(x[~mine], y[~mine]) and bool(y[mine].any()), k
    if c["precision"] == 32:  # mvx_moments_backward_batch: the same walk, the same guard
        gm = np.random.default_rng(r["fseed"] + 3).standard_normal((c["B"], c["C"], 3))
        T = hip.dev(_target(c))
        rows_bad = _entry(vox, X.spec(vox, bad, X.inputs(bad)), gm, T)
        rows_ok = _entry(vox, X.spec(vox, c, X.inputs(c)), gm, T)
        for x, y in zip(rows_bad, rows_ok):
            if x is not None:
                assert not bool(x[mine].any()) and torch.equal(x[~mine], y[~mine]) and bool(y[mine].any())
    a1, a2 = _backward(row_id, bad, "grid"), _backward(row_id, c, "grid")
    assert not bool(a1["xyz"].grad[mine].any()) and torch.equal(a1["xyz"].grad[~mine], a2["xyz"].grad[~mine])
    for _, key in POSE_KEYS:
        assert torch.equal(a1[key].grad[others], a2[key].grad[others]) and bool(torch.isfinite(a1[key].grad[others]).all()), key
    # the radius and sigma gradients of the same backward: atom-wise rows zero / unchanged; the reductions over the call finite and
    # within their bar of the float64 reference of the other molecules (the molecule's own share is gone, so not the clean call's bits)
    mols = _reference(row_id)["mols"]
    share = lambda key: tuple(np.atleast_1d(sum(mols[m]["call"][key][i] for m in others if mols[m] is not None)) for i in (0, 1))  # noqa: E731
    rg = a1["radii"].grad
    assert bool(torch.isfinite(rg).all()) and bool(torch.isfinite(a1["sigma"].grad).all())
    if c["radii_type"] == "atom-wise":
        assert not bool(rg[mine].any()) and torch.equal(rg[~mine], a2["radii"].grad[~mine]) and bool(a2["radii"].grad[mine].any())
    else:
        _close("a non-finite pose: dL/dr", c, rg.double().cpu().numpy().reshape(-1), *share("radius"), "dL/d(scalar radius)")
    _close("a non-finite pose: dL/dsigma", c, a1["sigma"].grad.double().cpu().numpy().reshape(-1), *share("sigma"), "dL/dsigma")
    assert float(a1["sigma"].grad) != float(a2["sigma"].grad)
    _note("a non-finite pose", 0.0)


# ---- 7. an upstream that is non-finite where no atom reaches --------------------------------------------------------------------------
def _unreached(c):
    """(B, 1, D, D, D) bool: the voxels of each molecule's grid that no atom reaches in any channel - where the oracle's grid of the
    clean batch with a weight of one in every channel is zero (a sum of cancelling or zero features is not such a voxel)."""
    p = R.positions_of(c)
    out = []
    for b in range(c["B"]):
        lo, hi = int(c["off"][b]), int(c["off"][b + 1])
        g = R.oracle_grid(c, p, b, w=np.ones((hi - lo, c["C"]), np.float64 if c["precision"] == 64 else np.float32))
        out.append(~(g != 0).any(axis=0, keepdims=True))
    return np.stack(out)


@pytest.mark.parametrize("row_id", ["feat-scalar-f32-scattered-posed", "feat-atom-bf16-tail-posed", "feat-chan-f64-call_tail-posed",
                                    "types-bytype-f32-call_tail-centred", "single-atom-f64-scattered-posed", "feat-atom-f32-scattered-d20"])
def test_a_non_finite_upstream_where_no_atom_reaches_changes_nothing(row_id):
    """What log, sqrt or a division in a loss produces: dL/dgrid is NaN or inf in voxels whose density is zero. The walks read the
    upstream only where rho != 0 (mvx_grad_body.inc), so every gradient keeps its bits. (Moments with a target are not part of this:
    sum g * t over those voxels is NaN by rights.)"""
    import torch

    r, _, c, _ = _pair(row_id)
    Fd, _ = _field(c)
    hole = torch.tensor(_unreached(c), device="cuda")
    assert bool(hole.any(dim=(1, 2, 3, 4)).all())
    G = _upstream(c, Fd)
    poison = torch.where(torch.arange(G[0].numel(), device="cuda").reshape(G[0].shape) % 2 == 0, float("nan"), float("inf")).to(G.dtype)
    Gp = torch.where(hole, poison, G)
    assert int(torch.isnan(Gp).sum()) > 1000 and int(torch.isinf(Gp).sum()) > 1000
    a1, a2 = _backward(row_id, c, "grid", upstream=Gp), _backward(row_id, c, "grid")
    for key in ("xyz", "chan", "radii", "sigma", "cen", "q", "t"):
        if a2[key] is not None and torch.is_tensor(a2[key]) and a2[key].grad is not None:
            assert torch.equal(a1[key].grad, a2[key].grad), key
    assert bool(a2["xyz"].grad.any()) and bool(torch.isfinite(a1["xyz"].grad).all())
    # the score entries with such a field: per molecule where the row's field is, else the voxels no molecule reaches
    Fp = torch.where(hole if Fd.dim() == 5 else hole.all(dim=0), poison, Fd)
    assert int(torch.isnan(Fp).sum()) > 100
    vox = X.vox(c)
    (S1, s1), (S2, s2) = X.score(vox, c, X.inputs(c), Fp, per_atom=True), X.score(vox, c, X.inputs(c), Fd, per_atom=True)
    assert torch.equal(S1, S2) and torch.equal(s1, s2)
    (g1, _), (g2, _) = _abi_rows(vox, c, Fp), _abi_rows(vox, c, Fd)
    for k in ("scores", "atoms", "gc", "gf"):
        assert g1[k] is None or torch.equal(g1[k], g2[k]), k
    _note("a non-finite upstream", 0.0)
