"""mvx_lm_step on the GPU (Voxelizer.lm_step) against its numpy restatement (tests/lm_reference.py), on the rows of
tests/lm_rows.py: batches of 1, 63, 64, 65 and 257 poses that cycle through every kind of row - accepted, dropped, dropped for the
max_dropped-th time, finished, a NaN trial score, a NaN inside H, H = 0 with lam = 0 (singular) and with lam > 0, omega = 0
exactly, |omega| near pi, an unnormalised q - with and without a trial.

To the bit: every decision, lam, taken, dropped, the copied q, t, S, G and H, finished rows across two more calls, xi = 0 and
(q2, t2) = (q, t) where the step fails, and two runs. Within a bar: the residual of xi, ||A xi - G||_inf <= gamma 2^-52
(||A||_inf ||xi||_inf + ||G||_inf) in np.longdouble, gamma four times the largest ratio np.linalg.solve itself attains on the
same systems (measured here as tests/test_lm_host.py measures it: 0.570, so gamma = 2.28; the systems' condition numbers stay
below 7.1e3); q2 and t2 against the reference's apply_twist of the kernel's own xi to 8 * 2^-52 |q| (t2: of |t| + |tau|).
"""
import numpy as np
import pytest

from tests import lm_reference as lm
from tests import lm_rows as R
from tests import hip_support as hip

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
KW = dict(lam_down=R.LAM_DOWN, lam_up=R.LAM_UP, max_dropped=R.MAX_DROPPED)
NAMES = ("q", "t", "S", "G", "H", "lam", "taken", "dropped")


@pytest.fixture(scope="module")
def vox():
    import molvoxel_amd as mv

    return mv.create_voxelizer(0.5, 16, "scalar", "gaussian", library="hip")


def _device_state(B):
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import LMState

    s, trial = R.rows(B)
    d = {k: torch.tensor(v, device="cuda") for k, v in s.items()}
    st = LMState(d["q"], d["t"], d["S"], d["G"], d["H"], d["lam"], d["taken"], d["dropped"])
    st.q2, st.t2, st.xi = d["q2"], d["t2"], torch.full((B, 6), np.nan, dtype=torch.float64, device="cuda")
    return st, tuple(torch.tensor(x, device="cuda") for x in trial)


def _host(st):
    return {k: getattr(st, k).cpu().numpy() for k in NAMES + ("q2", "t2", "xi")}


def _run(vox, B, have_trial):
    st, trial = _device_state(B)
    vox.lm_step(st, trial if have_trial else None, **KW)
    return st, trial


@pytest.mark.parametrize("have_trial", [True, False])
@pytest.mark.parametrize("B", R.SIZES)
def test_step_against_the_reference(vox, B, have_trial):
    st, trial = _run(vox, B, have_trial)
    got = _host(st)
    ref, rtrial = R.reference_state(B)
    s0, _ = R.rows(B)
    decisions = lm.step(ref, rtrial if have_trial else None, xi_from=got["xi"], **KW)
    # decisions, damping, counters and the copied state: to the bit
    for k in NAMES:
        assert hip.same_bits(got[k], getattr(ref, k)), (k, np.argwhere(got[k] != getattr(ref, k))[:3].tolist())
    for b in range(B):
        kind = R.kind_of(B, b)
        if decisions[b] == "accept":
            assert hip.same_bits(got["q"][b], s0["q2"][b]) and hip.same_bits(got["H"][b], rtrial[2][b]) and got["taken"][b] == s0["taken"][b] + 1
        else:
            assert hip.same_bits(got["q"][b], s0["q"][b]) and hip.same_bits(got["H"][b], s0["H"][b]) and got["taken"][b] == s0["taken"][b]
        stays = kind in R.FAILS or kind == "finished" or (have_trial and kind == "dropped_last")
        if stays:  # no step: xi = 0 and the pose itself, to the bit
            assert not got["xi"][b].any() and not np.signbit(got["xi"][b]).any(), (b, kind)
            assert hip.same_bits(got["q2"][b], got["q"][b]) and hip.same_bits(got["t2"][b], got["t"][b]), (b, kind)
        else:
            assert got["xi"][b].any() and np.isfinite(got["xi"][b]).all(), (b, kind)
        if kind == "omega_zero":
            assert not got["xi"][b, 3:].any() and hip.same_bits(got["q2"][b], got["q"][b])
    # the solve: the residual of the kernel's xi against four times np.linalg.solve's own
    numpy_worst, cond = R.numpy_residual()
    gamma = 4.0 * numpy_worst
    assert cond < 1e8
    worst = 0.0
    for b in range(B):
        if got["xi"][b].any():
            worst = max(worst, lm.residual_ratio(got["H"][b], got["G"][b], got["lam"][b], got["xi"][b]))
    # the twist: q2 and t2 against the reference's apply_twist of the kernel's own xi
    qerr = np.abs(got["q2"] - ref.q2).max(axis=1) / (8 * EPS * np.linalg.norm(got["q"], axis=1))
    terr = np.abs(got["t2"] - ref.t2).max(axis=1) / (8 * EPS * (np.abs(got["t"]).max(axis=1) + np.abs(got["xi"][:, :3]).max(axis=1) + 1e-300))
    print(f"LM_STEP B {B} trial {int(have_trial)}: residual ratio {worst:.3f} (numpy {numpy_worst:.3f}, gamma {gamma:.3f}); "
          f"q2 error / bar {qerr.max():.3g}, t2 error / bar {terr.max():.3g}")
    assert worst <= gamma, (worst, gamma)
    assert (qerr <= 1.0).all(), (int(qerr.argmax()), R.kind_of(B, int(qerr.argmax())), float(qerr.max()))
    assert (terr <= 1.0).all(), (int(terr.argmax()), float(terr.max()))


@pytest.mark.parametrize("B", [65, 257])
def test_finished_rows_stay_untouched_and_two_runs_agree(vox, B):
    import torch

    st, trial = _run(vox, B, True)
    again, _ = _run(vox, B, True)
    for k in NAMES + ("q2", "t2", "xi"):
        assert torch.equal(getattr(st, k), getattr(again, k)) or hip.same_bits(getattr(st, k).cpu().numpy(), getattr(again, k).cpu().numpy()), k
    first = _host(st)
    done = first["dropped"] >= R.MAX_DROPPED
    kinds = {R.kind_of(B, b) for b in np.flatnonzero(done)}
    assert kinds == {"finished", "dropped_last"}
    # two more calls with a trial that would be accepted everywhere: finished rows keep every bit
    S2 = st.S + 100.0
    for _ in range(2):
        vox.lm_step(st, (S2, trial[1], trial[2]), **KW)
        S2 = S2 + 100.0
    later = _host(st)
    for k in NAMES + ("q2", "t2", "xi"):
        assert hip.same_bits(later[k][done], first[k][done]), k
    assert not later["xi"][done].any() and hip.same_bits(later["q2"][done], later["q"][done]) and hip.same_bits(later["t2"][done], later["t"][done])
    live = ~done & np.isfinite(first["S"])
    assert (later["taken"][live] == first["taken"][live] + 2).all() and not later["dropped"][live].any()


def test_the_trial_pose_tensors_are_made_once_and_xi_may_be_left_out(vox):
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import LMState

    B = 65
    s, _ = R.rows(B)
    d = {k: torch.tensor(v, device="cuda") for k, v in s.items()}
    st = LMState(d["q"], d["t"], d["S"], d["G"], d["H"], d["lam"], d["taken"], d["dropped"])
    assert vox.lm_step(st, **KW) is st
    q2, t2, xi = st.q2, st.t2, st.xi
    assert tuple(q2.shape) == (B, 4) and tuple(t2.shape) == (B, 3) and tuple(xi.shape) == (B, 6)
    full, _ = _run(vox, B, False)
    assert torch.equal(q2, full.q2) or hip.same_bits(q2.cpu().numpy(), full.q2.cpu().numpy())
    vox.lm_step(st, **KW)
    assert st.q2 is q2 and st.t2 is t2 and st.xi is xi
    # the C entry without xi: the same trial poses
    out_q, out_t = torch.empty_like(q2), torch.empty_like(t2)
    rc = vox._lib.mvx_lm_step(vox._handle, B, 0, R.LAM_DOWN, R.LAM_UP, R.MAX_DROPPED, st.q.data_ptr(), st.t.data_ptr(), st.S.data_ptr(),
                              st.G.data_ptr(), st.H.data_ptr(), st.lam.data_ptr(), st.taken.data_ptr(), st.dropped.data_ptr(),
                              out_q.data_ptr(), out_t.data_ptr(), None, None, None, None, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, vox._lib.mvx_last_error()
    assert hip.same_bits(out_q.cpu().numpy(), q2.cpu().numpy()) and hip.same_bits(out_t.cpu().numpy(), t2.cpu().numpy())
