"""Hessians of views and the on-device Levenberg-Marquardt step without a GPU: the two C ABI entries (mvx_score_hessian_views,
mvx_lm_step; prototypes: tests/test_abi_header_host.py), what they reject before they touch a device - mvx_score_views' rules in its
order, then the two rules of mvx_score_hessian_batch -, what the Python layer refuses before it needs the library, lm_step_kernel's
resources read from mvx_lm.o, the numpy restatement of the step (tests/lm_reference.py) on a quadratic and on hand-made rows, the
residual np.linalg.solve itself attains on the systems of tests/test_hip_lm_step.py, and the conditions of the GPU refinement test
on the CPU loop. (A stride that is neither 0 nor C * D^3 is judged against the handle: tests/test_hip_score_hessian_views.py.)

np.linalg.solve's largest ||A xi - G||_inf / (2^-52 (||A||_inf ||xi||_inf + ||G||_inf)) on those systems: 0.570 (numpy 2.2.6;
the largest condition number 7.1e3). The GPU test takes four times the figure it measures the same way as its gamma."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import lm_reference as lm
from tests import lm_rows as R
from tests.abi import MVX_ERR_INVALID, P, call, records
from tests.fake_voxelizer import fake as _fake  # (a voxelizer without a handle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONE = records([0])


def test_the_views_entry_begins_like_score_views():
    assert _lib.SIGNATURES["mvx_score_hessian_views"][1][:15] == _lib.SIGNATURES["mvx_score_views"][1][:15]
    assert _lib.SIGNATURES["mvx_score_hessian_views"][1][15:] == _lib.SIGNATURES["mvx_score_hessian_batch"][1][13:]


# ---- mvx_lm_step's rejections -------------------------------------------------------------------------------------------------
STATE = ("q", "t", "S", "G", "H", "lam", "taken", "dropped", "q2", "t2")


def _lm(handle=None, B=2, have_trial=1, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3, xi=P, **ptrs):
    a = {k: P for k in STATE + ("S2", "G2", "H2")}
    a.update(ptrs)
    return call(_lib.load().mvx_lm_step, handle, B, have_trial, lam_down, lam_up, max_dropped, *(a[k] for k in STATE), a["S2"], a["G2"],
                a["H2"], xi, None)


@pytest.mark.parametrize("kw, words", [(dict(B=-1), "B must be >= 0")]
                         + [({k: None}, "must not be null") for k in STATE]
                         + [({k: None}, "with have_trial") for k in ("S2", "G2", "H2")]
                         + [(dict(max_dropped=0), "max_dropped"), (dict(max_dropped=-2), "max_dropped")]
                         + [({k: v}, "finite and > 0") for k in ("lam_down", "lam_up") for v in (0.0, -1.0, np.inf, np.nan)]
                         + [(dict(), "null handle"), (dict(B=0), "null handle")])
def test_lm_step_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _lm(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_lm_step_rules_fire_in_their_order_and_need_no_arrays_where_there_is_nothing_to_do():
    assert "B must be" in _lm(B=-1, q=None, max_dropped=0)[1]
    assert "must not be null" in _lm(q=None, S2=None, max_dropped=0)[1]
    assert "with have_trial" in _lm(S2=None, max_dropped=0, lam_up=0.0)[1]
    assert "max_dropped" in _lm(max_dropped=0, lam_up=0.0)[1]
    assert "finite and > 0" in _lm(lam_up=0.0)[1]
    # without a trial S2, G2 and H2 may be null, and xi always; the call gets as far as the handle
    for kw in (dict(have_trial=0, S2=None, G2=None, H2=None), dict(xi=None)):
        assert "null handle" in _lm(**kw)[1]
    # no poses: nothing is needed but a handle
    none = dict(B=0, **{k: None for k in STATE + ("S2", "G2", "H2")}, xi=None)
    assert "null handle" in _lm(**none)[1]
    assert _lm(handle=P, **none)[0] == 0
    assert "max_dropped" in _lm(handle=P, **dict(none, max_dropped=0))[1]


# ---- mvx_score_hessian_views' rejections --------------------------------------------------------------------------------------
def _hess(handle=None, mode=0, coords=P, channels=P, radii=None, radii_type=0, N=3, C_=4, xforms=ONE, B=1, index=None, offsets=None,
          field=P, stride=0, pivots=None, scores=P, atom_grad=None, atom_hess=None, twist_grad=P, twist_hess=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_score_hessian_views, handle, mode, coords, channels, radii, 1.0, radii_type, N, C_,
                None if xforms is None else C.addressof(xforms), B, index, None if off is None else off.ctypes.data,
                field, stride, pivots, scores, atom_grad, atom_hess, twist_grad, twist_hess, None)


SCORE_VIEWS_RULES = [
    # what validate_views rejects (tests/test_score_views_host.py, in mvx_score_views' order)
    (dict(mode=3), "bad mode"),
    (dict(mode=-1), "bad mode"),
    (dict(radii_type=7), "radii_type"),
    (dict(B=-1), "B and N must be"),
    (dict(N=-1), "B and N must be"),
    (dict(C_=0), "C > 0"),
    (dict(xforms=None), "xforms must not be null"),
    (dict(mode=2, C_=1, radii_type=2, radii=P), "Channel-Wise"),
    (dict(mode=2, C_=3), "single mode has one channel"),
    (dict(coords=None), "coords must not be null"),
    (dict(radii_type=1), "radii array required"),
    (dict(radii_type=2), "radii array required"),
    (dict(mode=1, channels=None), "types must not be null"),
    (dict(N=1 << 31), "too many atoms"),
    # what mvx_score_batch rejects for field, stride and scores
    (dict(stride=-1), "field_view_stride"),
    (dict(stride=-4 * 16 ** 3), "field_view_stride"),
    (dict(scores=None), "scores must not be null"),
    # per-row outputs without an index
    (dict(atom_grad=P), "need an index"),
    (dict(atom_hess=P), "need an index"),
    (dict(offsets=(0, 2), atom_grad=P, atom_hess=P), "need an index"),
    # an index without offsets, and bad offsets
    (dict(index=P), "offsets_host must not be null"),
    (dict(index=P, offsets=(1, 3)), "offsets[0]"),
    (dict(index=P, B=2, xforms=records([0, 0]), offsets=(0, 3, 2)), "non-decreasing"),
    (dict(index=P, offsets=(0, 1 << 31)), "2^31"),
    (dict(channels=None), "channels must not be null"),
    (dict(field=None), "field must not be null"),
    (dict(field=None, index=P, offsets=(0, 2)), "field must not be null"),
    (dict(), "null handle"),
    (dict(handle=P, xforms=records([_lib.MVX_XF_POSE_PTR | _lib.MVX_XF_ROTATE])), "other flag bit"),
    (dict(handle=P, xforms=records([_lib.MVX_XF_POSE_PTR], ptr=None)), "center_ptr"),
]
# a call that breaks both of the entry's own rules: every rule of mvx_score_views must still win
BOTH = dict(mode=0, radii_type=2, radii=P, twist_grad=None)


@pytest.mark.parametrize("kw, words", SCORE_VIEWS_RULES)
def test_hessian_views_rejects_what_score_views_rejects_before_touching_a_device(kw, words):
    rc, msg = _hess(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_score_views_rules_fire_in_its_order():
    """Each call breaks a rule and every rule after it in SCORE_VIEWS_RULES' groups: the earlier one is reported."""
    assert "field_view_stride" in _hess(stride=-1, scores=None, atom_grad=P, channels=None, field=None)[1]
    assert "scores must not be null" in _hess(scores=None, atom_grad=P, channels=None, field=None)[1]
    assert "need an index" in _hess(atom_grad=P, channels=None, field=None)[1]
    assert "offsets_host must not be null" in _hess(index=P, channels=None, field=None)[1]
    assert "channels must not be null" in _hess(channels=None, field=None)[1]
    assert "too many atoms" in _hess(N=1 << 31, stride=-1)[1]
    # mvx_score_views reports the same rule for the same call
    lib = _lib.load()
    for kw in (dict(stride=-1, scores=None), dict(scores=None, channels=None), dict(channels=None, field=None)):
        a = dict(stride=0, scores=P, channels=P, field=P)
        a.update(kw)
        rc, first = call(lib.mvx_score_views, None, 0, P, a["channels"], None, 1.0, 0, 3, 4, C.addressof(ONE), 1, None, None, a["field"],
                         a["stride"], a["scores"], None, None, None, None)
        assert rc == MVX_ERR_INVALID and _hess(**kw)[1] == first


@pytest.mark.parametrize("kw, words", [r for r in SCORE_VIEWS_RULES if not ({"mode", "radii_type"} & set(r[0]))])
def test_score_views_rules_come_before_the_entrys_own(kw, words):
    rc, msg = _hess(**dict(BOTH, **kw))
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_the_hessian_rules_fire_last_and_before_a_device_is_touched():
    # (P stands for a handle: with a stride of 0 no rule reads it, and the call would go on to the device behind these two)
    rc, msg = _hess(handle=P, mode=0, radii_type=2, radii=P)
    assert rc == MVX_ERR_INVALID and "channel-wise radii in features mode" in msg and "mvx_score_views" in msg, (rc, msg)
    rc, msg = _hess(handle=P, twist_grad=None)
    assert rc == MVX_ERR_INVALID and "twist_hess needs twist_grad" in msg, (rc, msg)
    rc, msg = _hess(handle=P, **BOTH)  # channel-wise radii first
    assert rc == MVX_ERR_INVALID and "channel-wise radii in features mode" in msg, (rc, msg)
    # with a selection and its rows, and with a cloud of no atoms
    sel = dict(handle=P, index=P, offsets=(0, 2), atom_grad=P, atom_hess=P)
    assert "twist_hess needs twist_grad" in _hess(**dict(sel, twist_grad=None))[1]
    assert "channel-wise radii in features mode" in _hess(**dict(sel, radii_type=2, radii=P))[1]
    assert "twist_hess needs twist_grad" in _hess(handle=P, N=0, coords=None, channels=None, field=None, twist_grad=None)[1]
    # no views at all: the same two rules, then nothing to do
    none = dict(handle=P, B=0, xforms=None, scores=None, field=None)
    assert "twist_hess needs twist_grad" in _hess(**dict(none, twist_grad=None))[1]
    assert _hess(**none)[0] == 0
    assert _hess(**dict(none, twist_grad=None, twist_hess=None))[0] == 0
    # channel-wise radii by type are served: the call gets as far as the handle
    rc, msg = _hess(mode=1, radii_type=2, radii=P)
    assert rc == MVX_ERR_INVALID and "null handle" in msg, (rc, msg)


def test_hessian_views_gets_as_far_as_the_handle_with_good_arguments():
    for kw in (dict(), dict(index=P, offsets=(0, 2)), dict(index=P, offsets=(0, 2), atom_grad=P, atom_hess=P),
               dict(index=P, offsets=(0, 0), field=None), dict(B=0, xforms=None, scores=None, field=None),
               dict(N=0, coords=None, channels=None, field=None), dict(stride=4 * 16 ** 3), dict(pivots=P),
               dict(twist_grad=None, twist_hess=None), dict(twist_hess=None)):
        rc, msg = _hess(**kw)
        assert rc == MVX_ERR_INVALID and "null handle" in msg, (kw, rc, msg)


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), centers=np.zeros((B, 3)), channels=rng.standard_normal((N, C_)).astype(np.float32),
                radii=1.0)


def _posed(a, B=2):
    return dict(a, quaternions=np.ones((B, 4)), translations=np.zeros((B, 3)))


def test_voxelizer_has_the_methods():
    from molvoxel_amd.voxelizer.hip import voxelizer
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    tail = ["channels", "radii", "field", "num_channels", "pivots", "per_atom"]
    assert list(inspect.signature(Voxelizer.score_hessian_views).parameters) == ["self", "coords", "centers"] + tail
    assert list(inspect.signature(Voxelizer.score_hessian_posed_views).parameters) == [
        "self", "coords", "centers", "quaternions", "translations"] + tail
    for f in (Voxelizer.score_hessian_views, Voxelizer.score_hessian_posed_views):
        p = inspect.signature(f).parameters
        assert p["num_channels"].default is None and p["pivots"].default is None and p["per_atom"].default is False
    knobs = ["steps", "lam0", "lam_down", "lam_up", "max_dropped", "stop_when_done"]
    assert list(inspect.signature(Voxelizer.refine_posed_batch).parameters) == [
        "self", "coords", "offsets", "centers", "quaternions", "translations", "channels", "radii", "field", "num_channels"] + knobs
    assert list(inspect.signature(Voxelizer.refine_posed_views).parameters) == [
        "self", "coords", "centers", "quaternions", "translations", "channels", "radii", "field", "num_channels"] + knobs
    for f in (Voxelizer.refine_posed_batch, Voxelizer.refine_posed_views, Voxelizer.lm_step):
        p = inspect.signature(f).parameters
        assert p["lam_down"].default == 1.0 / 3.0 and p["lam_up"].default == 10.0 and p["max_dropped"].default == 3
    p = inspect.signature(Voxelizer.refine_posed_views).parameters
    assert p["steps"].default == 40 and p["lam0"].default is None and p["stop_when_done"].default is False
    assert list(inspect.signature(Voxelizer.lm_step).parameters) == ["self", "state", "trial", "lam_down", "lam_up", "max_dropped"]
    assert inspect.signature(Voxelizer.lm_step).parameters["trial"].default is None
    assert inspect.isclass(voxelizer.LMState)


@pytest.mark.parametrize("shape", [(4, 16, 16), (3, 16, 16, 16), (4, 16, 16, 15), (3, 4, 16, 16, 16), (2, 5, 16, 16, 16), ()])
def test_a_field_of_the_wrong_shape_is_an_assertion_error(shape):
    import torch

    a = _args()
    with pytest.raises(AssertionError, match="field does not match dimension"):
        _fake().score_hessian_views(field=torch.zeros(shape), **a)
    with pytest.raises(AssertionError, match="field does not match dimension"):
        _fake().score_hessian_posed_views(field=torch.zeros(shape), **_posed(a))
    with pytest.raises(AssertionError, match="quaternions does not match dimension"):  # (the posed form checks its poses first)
        _fake().score_hessian_posed_views(field=torch.zeros(shape), **dict(_posed(a), quaternions=np.ones((2, 3))))
    with pytest.raises(AssertionError, match="field does not match dimension"):
        _fake().refine_posed_views(field=torch.zeros(shape), **_posed(a))
    with pytest.raises(AssertionError, match="translations does not match dimension"):
        _fake().refine_posed_views(field=torch.zeros(shape), **dict(_posed(a), translations=np.zeros((3, 3))))


def test_the_other_shape_checks_are_those_of_the_views_path():
    import torch

    a = _args()
    F = torch.zeros((4, 16, 16, 16))
    with pytest.raises(AssertionError, match="centers does not match dimension"):
        _fake().score_hessian_views(field=F, **dict(a, centers=None))
    with pytest.raises(AssertionError, match="centers does not match dimension"):
        _fake().score_hessian_views(field=F, **dict(a, centers=np.zeros((2, 2))))
    with pytest.raises(AssertionError, match="atom features does not match"):
        _fake().score_hessian_views(field=F, **dict(a, channels=a["channels"][:5]))
    with pytest.raises(AssertionError, match="radii should be scalar"):
        _fake().score_hessian_views(field=F, **dict(a, radii=np.ones(6, np.float32)))
    with pytest.raises(AssertionError, match="pivots does not match dimension"):
        _fake().score_hessian_views(field=F, pivots=np.zeros((3, 3)), **a)
    with pytest.raises(AssertionError, match="pivots does not match dimension"):
        _fake().score_hessian_posed_views(field=F, pivots=np.zeros((2, 4)), **_posed(a))
    # the batch driver applies the batch path's rules: the poses against the offsets' molecule count
    with pytest.raises(AssertionError, match="quaternions does not match dimension"):
        _fake().refine_posed_batch(field=F, offsets=np.array([0, 2, 4, 6]), **_posed(a))


def test_the_results_need_torch_output():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    a = _args()
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_hessian_views(field=F, **a)
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_hessian_posed_views(field=F, **_posed(a))
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").refine_posed_views(field=F, **_posed(a))
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").refine_posed_batch(field=F, offsets=np.array([0, 2, 6]), **_posed(a))


def test_channel_wise_radii_with_features_name_the_first_order_alternative():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    a = dict(_args(), radii=np.ones(4, np.float32))
    for call in (lambda v: v.score_hessian_views(field=F, **a), lambda v: v.score_hessian_posed_views(field=F, **_posed(a)),
                 lambda v: v.refine_posed_views(field=F, **_posed(a)),
                 lambda v: v.refine_posed_batch(field=F, offsets=np.array([0, 2, 6]), **_posed(a))):
        with pytest.raises(NotImplementedError, match="channel-wise radii with features.*score_posed_batch"):
            call(_fake("channel-wise"))


def test_lm_step_checks_its_state_before_it_needs_the_library():
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import LMState

    B = 3
    f64 = dict(dtype=torch.float64)
    st = LMState(torch.zeros((B, 4), **f64), torch.zeros((B, 3), **f64), torch.zeros(B, **f64), torch.zeros((B, 6), **f64),
                 torch.zeros((B, 6, 6), **f64), torch.ones(B, **f64))
    assert st.taken.dtype == torch.int32 and st.dropped.dtype == torch.int32 and tuple(st.taken.shape) == (B,)
    assert st.q2 is None and st.t2 is None and st.xi is None
    with pytest.raises(AssertionError, match="state.q should be"):  # (host tensors: not on the voxelizer's device)
        _fake().lm_step(st)


# ---- kernel resources -----------------------------------------------------------------------------------------------------------
def test_lm_step_kernel_uses_no_scratch_and_spills_nothing():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_lm.o")
    assert obj in regs.KERNEL_OBJECTS
    if not os.path.exists(obj):
        pytest.skip("mvx_lm.o not built")
    res = regs.kernel_resources(obj)
    assert list(res) == ["lm_step_kernel"], sorted(res)
    r = res["lm_step_kernel"]
    print(f"lm_step_kernel: {r}")
    assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0 and r["lds"] == 0, r
    assert r["vgpr"] <= 128, r  # (the 6x7 system is 84 registers)


# ---- the reference itself --------------------------------------------------------------------------------------------------------
def test_one_undamped_step_lands_on_the_maximum_of_a_quadratic():
    """S(xi) = -0.5 xi^T A xi + b^T xi with A positive definite: G = b and H = -A at xi = 0, and one step from lam = 0 is A^-1 b."""
    rng = np.random.default_rng(2)
    B = 5
    M = rng.standard_normal((B, 6, 6))
    A = M @ M.transpose(0, 2, 1) + 0.5 * np.eye(6)
    b = rng.standard_normal((B, 6))
    q = np.tile([1.0, 0.0, 0.0, 0.0], (B, 1))
    st = lm.State(q, np.zeros((B, 3)), np.zeros(B), b, -A, np.zeros(B))
    assert lm.step(st) == [None] * B
    for k in range(B):
        want = np.linalg.solve(A[k], b[k])
        assert np.abs(st.xi[k] - want).max() <= 1e-12 * np.abs(want).max()
        assert np.array_equal(st.t2[k], st.xi[k, :3])
        q2, _ = lm.apply_twist(q[k], np.zeros(3), want)
        assert np.abs(st.q2[k] - q2).max() <= 1e-12 and abs(np.linalg.norm(st.q2[k]) - 1.0) <= 1e-14
    assert not st.taken.any() and not st.dropped.any() and not st.lam.any()


def test_decisions_and_counters_on_hand_made_rows():
    #      accepted  tie (dropped)  worse  worse for the 3rd time  finished  NaN trial
    S = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    S2 = np.array([2.0, 1.0, 0.5, 0.5, 9.0, np.nan])
    dropped = np.array([2, 0, 1, 2, 3, 0], np.int32)
    taken = np.array([4, 0, 1, 2, 5, 0], np.int32)
    B = 6
    q = np.tile([1.0, 0.0, 0.0, 0.0], (B, 1))
    st = lm.State(q, np.zeros((B, 3)), S, np.ones((B, 6)), -np.tile(np.eye(6), (B, 1, 1)), np.full(B, 0.5), taken, dropped)
    st.q2, st.t2 = np.tile([0.0, 1.0, 0.0, 0.0], (B, 1)), np.full((B, 3), 7.0)
    G2, H2 = np.full((B, 6), 2.0), -3.0 * np.tile(np.eye(6), (B, 1, 1))
    got = lm.step(st, (S2, G2, H2), lam_down=0.25, lam_up=4.0, max_dropped=3)
    assert got == ["accept", "drop", "drop", "drop", None, "drop"]
    assert st.taken.tolist() == [5, 0, 1, 2, 5, 0] and st.dropped.tolist() == [0, 1, 2, 3, 3, 1]
    assert st.lam.tolist() == [0.125, 2.0, 2.0, 2.0, 0.5, 2.0]
    assert st.S.tolist() == [2.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    assert np.array_equal(st.q[0], [0.0, 1.0, 0.0, 0.0]) and np.array_equal(st.t[0], [7.0] * 3)
    assert np.array_equal(st.G[0], G2[0]) and np.array_equal(st.H[0], H2[0])
    assert np.array_equal(st.q[1:], q[1:]) and not st.t[1:].any()
    # finished rows: the pose itself and no twist; the others: xi = G / (diag + lam)
    for k in (3, 4):
        assert np.array_equal(st.q2[k], st.q[k]) and np.array_equal(st.t2[k], st.t[k]) and not st.xi[k].any()
    assert np.allclose(st.xi[0], 2.0 / 3.125) and np.allclose(st.xi[1], 1.0 / 3.0)
    # a finished row stays as it is on later calls, whatever the trial says
    before = st.copy()
    lm.step(st, (np.full(B, 99.0), G2, H2), max_dropped=3)
    for k in (3, 4):
        for name in ("q", "t", "S", "G", "H", "lam", "taken", "dropped", "q2", "t2", "xi"):
            assert np.array_equal(getattr(st, name)[k], getattr(before, name)[k]), (k, name)


def test_a_singular_or_non_finite_system_gives_no_step():
    B = 4
    q = np.tile([0.6, 0.0, 0.8, 0.0], (B, 1))
    H = np.zeros((B, 6, 6))
    H[1] = -np.eye(6)
    H[1, 2, 3] = np.nan
    H[2] = -np.eye(6)
    H[3] = -np.eye(6)
    lam = np.array([0.0, 1.0, np.inf, 1.0])
    t = np.ones((B, 3))
    t[3, 1] = np.nan
    st = lm.State(q, t, np.zeros(B), np.ones((B, 6)), H, lam)
    lm.step(st)
    assert not st.xi.any() and np.array_equal(st.q2, st.q) and np.array_equal(st.t2, st.t, equal_nan=True)
    assert lm.solve(np.zeros((6, 6)), np.ones(6), 2.0).tolist() == [0.5] * 6


def test_apply_twist_is_the_library_helper_and_exact_at_zero_rotation():
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import apply_twist

    rng = np.random.default_rng(9)
    q, t, xi = rng.standard_normal((5, 4)), rng.standard_normal((5, 3)), rng.standard_normal((5, 6))
    xi[1, 3:] = 0.0
    xi[2, 3:] *= np.pi / np.linalg.norm(xi[2, 3:])
    want_q, want_t = apply_twist(torch.tensor(q), torch.tensor(t), torch.tensor(xi))
    for b in range(5):
        q2, t2 = lm.apply_twist(q[b], t[b], xi[b])
        assert np.abs(q2 - want_q[b].numpy()).max() <= 8 * 2.0 ** -52 * np.linalg.norm(q[b])
        assert np.array_equal(t2, want_t[b].numpy())
    assert np.array_equal(lm.apply_twist(q[1], t[1], xi[1])[0], q[1])


# ---- what the GPU tests rest on ----------------------------------------------------------------------------------------------------
def test_every_batch_of_rows_mixes_every_kind_and_numpy_solves_them_to_rounding():
    for B in R.SIZES:
        kinds = {R.kind_of(B, b) for b in range(B)}
        assert kinds == set(R.KINDS) if B >= len(R.KINDS) else len(kinds) == B
        st, trial = R.reference_state(B)
        got = lm.step(st, trial, R.LAM_DOWN, R.LAM_UP, R.MAX_DROPPED)
        for b in range(B):
            k = R.kind_of(B, b)
            assert got[b] == {"accepted": "accept", "unnormalised": "accept", "finished": None}.get(k, "drop"), (B, b, k, got[b])
            stays = k in R.FAILS or k in ("finished", "dropped_last")
            assert stays == (not st.xi[b].any()), (B, b, k)
            if k == "omega_zero":
                assert not st.xi[b, 3:].any() and st.xi[b, :3].all() and np.array_equal(st.q2[b], st.q[b])
            if k == "omega_pi":
                assert abs(np.linalg.norm(st.xi[b, 3:]) - (np.pi - 1e-3)) < 1e-9
    worst, cond = R.numpy_residual()
    print(f"LM_NUMPY_RESIDUAL np.linalg.solve: worst residual ratio {worst:.3f}, largest condition number {cond:.3g}")
    assert cond < 1e8  # (the residual bar is the meaningful one: no forward-error claim is made)
    assert 0.0 < worst < 8.0  # backward stable: a small multiple of the unit roundoff, as LAPACK's own tests expect of dgesv


def test_the_cpu_refinement_meets_the_conditions_of_the_gpu_test():
    st, history, first = R.cpu_refinement()
    q0, t0 = R.refine_starts()
    assert tuple(history.shape) == (R.REFINE_ROUNDS + 1, R.REFINE_POSES)
    assert (R.angle_deg(q0) <= 5.0).all() and (np.linalg.norm(t0, axis=1) <= 0.3).all()
    a0, a1, s0, s1 = R.refine_conditions(history, st.taken, q0, t0, st.q, st.t)
    print(f"LM_CPU_REFINE taken {st.taken.tolist()} dropped {st.dropped.tolist()}; rotation {a0.max():.2f} -> {a1.max():.3f} deg at "
          f"most, shift {s0.max():.3f} -> {s1.max():.4f} A at most; score {history[0].min():.3f} -> {history[-1].min():.3f} at least")
