"""Second-order scores without a GPU: the C ABI entry (mvx_score_hessian_batch) and the checks it makes before it touches a
device, in mvx_score_batch's order; what the Python layer refuses before it needs the
library; the registers of both kernels read from mvx_hess.o; the float64 reference (tests/hessian_reference.py) against central
differences of tests/grad_reference.py's coordinate gradient; its twist helper against differences of a smooth function under
exp twists; and apply_twist on CPU tensors. (Rules judged against the handle's dimension - a stride that is neither 0 nor
C * D^3 - need a real handle: tests/test_hip_score_hessian.py.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import grad_reference as gr
from tests import hessian_reference as hr
from tests.abi import MVX_ERR_INVALID, P, call, records
from tests.fake_voxelizer import fake as _fake  # (a voxelizer without a handle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hess(handle=None, mode=0, coords=P, channels=P, radii=None, radii_type=0, offsets=(0, 3), xforms=None, B=1, C_=4, field=P,
          stride=0, pivots=None, scores=P, atom_grad=None, atom_hess=None, twist_grad=P, twist_hess=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_score_hessian_batch, handle, mode, coords, channels, radii, 1.0, radii_type,
                None if off is None else off.ctypes.data, None if xforms is None else C.addressof(xforms), B, C_, field, stride, pivots,
                scores, atom_grad, atom_hess, twist_grad, twist_hess, None)


# a call that breaks both of the entry's own rules: every rule of mvx_score_batch must still win
BOTH = dict(mode=0, radii_type=2, radii=P, twist_grad=None)

SCORE_RULES = [
    # what mvx_score_batch rejects, in its order (tests/test_score_host.py)
    (dict(mode=3), "mode"),
    (dict(mode=-1), "mode"),
    (dict(C_=0), "C must be > 0"),
    (dict(mode=2, C_=3), "C = 1"),
    (dict(stride=-1), "field_mol_stride"),
    (dict(scores=None), "scores"),
    (dict(B=-1), "B must be"),
    (dict(radii_type=7), "radii_type"),
    (dict(mode=2, C_=1, radii_type=2, radii=P), "Channel-Wise"),
    (dict(offsets=None), "offsets"),
    (dict(offsets=(1, 3)), "offsets[0]"),
    (dict(B=2, offsets=(0, 3, 2)), "non-decreasing"),
    (dict(), "null handle"),
    (dict(handle=P, xforms=records([_lib.MVX_XF_POSE_PTR | _lib.MVX_XF_ROTATE])), "other flag bit"),
    (dict(handle=P, xforms=records([_lib.MVX_XF_POSE_PTR], ptr=None)), "center_ptr"),
    (dict(handle=P, offsets=(0, 1 << 31)), "too many atoms"),
    (dict(handle=P, coords=None), "coords / field"),
    (dict(handle=P, field=None), "coords / field"),
    (dict(handle=P, channels=None), "channels"),
    (dict(handle=P, radii_type=1), "radii array"),
]


@pytest.mark.parametrize("kw, words", SCORE_RULES)
def test_rejects_what_score_batch_rejects_before_touching_a_device(kw, words):
    rc, msg = _hess(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


@pytest.mark.parametrize("kw, words", [r for r in SCORE_RULES if not ({"mode", "radii_type"} & set(r[0]))])
def test_score_batch_rules_come_before_the_entrys_own(kw, words):
    rc, msg = _hess(**dict(BOTH, **kw))
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_its_own_rules_fire_before_a_device_is_touched():
    # (a molecule without atoms: no rule reads the handle, and the call would go on to the device behind these two)
    empty = dict(handle=P, offsets=(0, 0))
    rc, msg = _hess(**dict(empty, mode=0, radii_type=2, radii=P))
    assert rc == MVX_ERR_INVALID and "channel-wise radii in features mode" in msg and "mvx_score_batch" in msg, (rc, msg)
    rc, msg = _hess(**dict(empty, twist_grad=None))
    assert rc == MVX_ERR_INVALID and "twist_hess needs twist_grad" in msg, (rc, msg)
    rc, msg = _hess(**dict(empty, **BOTH))  # channel-wise radii first
    assert rc == MVX_ERR_INVALID and "channel-wise radii in features mode" in msg, (rc, msg)
    # no molecules at all: the same two rules, then nothing to do
    none = dict(handle=P, B=0, offsets=(0,), scores=None, field=None, coords=None)
    rc, msg = _hess(**dict(none, twist_grad=None))
    assert rc == MVX_ERR_INVALID and "twist_hess needs twist_grad" in msg, (rc, msg)
    assert _hess(**none)[0] == 0
    assert _hess(**dict(none, twist_grad=None, twist_hess=None))[0] == 0
    # channel-wise radii by type are served: the call gets as far as the handle
    rc, msg = _hess(mode=1, radii_type=2, radii=P)
    assert rc == MVX_ERR_INVALID and "null handle" in msg, (rc, msg)


def test_the_entry_begins_like_score_batch():
    # the arguments up to the field's stride are mvx_score_batch's
    assert _lib.SIGNATURES["mvx_score_hessian_batch"][1][:13] == _lib.SIGNATURES["mvx_score_batch"][1][:13]


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), offsets=np.array([0, 2, N][:B + 1]), centers=None,
                channels=rng.standard_normal((N, C_)).astype(np.float32), radii=1.0)


def _posed(a):
    a = dict(a)
    a.pop("centers")
    return dict(a, centers=None, quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)))


def test_voxelizer_has_the_methods_and_apply_twist_is_exported():
    from molvoxel_amd.voxelizer.hip import _quaternion, voxelizer
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    bat = inspect.signature(Voxelizer.score_hessian_batch).parameters
    assert list(bat) == ["self", "coords", "offsets", "centers", "channels", "radii", "field", "num_channels", "pivots", "per_atom"]
    pos = inspect.signature(Voxelizer.score_hessian_posed_batch).parameters
    assert list(pos) == ["self", "coords", "offsets", "centers", "quaternions", "translations", "channels", "radii", "field",
                         "num_channels", "pivots", "per_atom"]
    for sig in (bat, pos):
        assert sig["num_channels"].default is None and sig["pivots"].default is None and sig["per_atom"].default is False
    assert voxelizer.apply_twist is _quaternion.apply_twist and callable(voxelizer.transform_on_device)
    assert list(inspect.signature(voxelizer.apply_twist).parameters) == ["quaternions", "translations", "twist"]


@pytest.mark.parametrize("shape", [(4, 16, 16), (3, 16, 16, 16), (4, 16, 16, 15), (3, 4, 16, 16, 16), (2, 5, 16, 16, 16), ()])
def test_a_field_of_the_wrong_shape_is_an_assertion_error(shape):
    import torch

    a = _args()
    with pytest.raises(AssertionError, match="field does not match dimension"):
        _fake().score_hessian_batch(field=torch.zeros(shape), **a)
    with pytest.raises(AssertionError, match="quaternions does not match dimension"):  # (the posed form checks its poses first)
        _fake().score_hessian_posed_batch(field=torch.zeros(shape), **dict(_posed(a), quaternions=np.ones((2, 3))))


def test_the_other_shape_checks_are_those_of_the_batch_path():
    import torch

    a = _args()
    F = torch.zeros((4, 16, 16, 16))
    with pytest.raises(AssertionError, match="offsets must span coords"):
        _fake().score_hessian_batch(field=F, **dict(a, offsets=np.array([0, 2, 5])))
    with pytest.raises(AssertionError, match="atom features does not match"):
        _fake().score_hessian_batch(field=F, **dict(a, channels=a["channels"][:5]))
    with pytest.raises(AssertionError, match="radii should be scalar"):
        _fake().score_hessian_batch(field=F, **dict(a, radii=np.ones(6, np.float32)))
    with pytest.raises(AssertionError, match="pivots does not match dimension"):
        _fake().score_hessian_batch(field=F, pivots=np.zeros((3, 3)), **a)


def test_the_results_need_torch_output():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_hessian_batch(field=F, **_args())
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_hessian_posed_batch(field=F, **_posed(_args()))


def test_channel_wise_radii_with_features_name_the_first_order_alternative():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    a = dict(_args(), radii=np.ones(4, np.float32))
    with pytest.raises(NotImplementedError, match="channel-wise radii with features.*score_posed_batch"):
        _fake("channel-wise").score_hessian_batch(field=F, **a)
    with pytest.raises(NotImplementedError, match="channel-wise radii with features.*score_posed_batch"):
        _fake("channel-wise").score_hessian_posed_batch(field=F, **_posed(a))


# ---- kernel resources --------------------------------------------------------------------------------------------------------
def test_hessian_kernels_use_no_scratch_and_keep_two_waves_per_simd():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_hess.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_hess.o not built")
    res = regs.kernel_resources(obj)
    walk = {k: v for k, v in res.items() if "score_hess_kernel" in k}
    assert len(walk) == 12, sorted(walk)  # 3 grid types x (features, types / single) x (Gaussian, binary)
    seen = set()
    for k, r in walk.items():
        m = re.search(r"score_hess_kernel<(float|double|__bf16), (\d), (true|false)>", k)
        assert m, k
        seen.add(m.groups())
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["lds"] == 0, (k, r)
        assert r["vgpr"] < 256, (k, r)  # grad_kernel's two waves per SIMD
    assert len(seen) == 12
    red = res["twist_reduce_kernel"]
    assert red["scratch"] == 0 and red["vspill"] == 0 and red["sspill"] == 0 and red["lds"] == 4 * 27 * 8, red


# ---- the reference against finite differences (precision 64: at precision 32 the reference rounds distances to float32) --------
FD_H = 2.0 ** -14
NEAR = 2.0 ** -12
D_, C_FD, N_FD = 16, 3, 24


def _draw(seed):
    rng = np.random.default_rng(seed)
    half = 0.5 * (D_ - 1) / 2.0
    xyz = rng.uniform(-half - 0.5, half + 0.5, (N_FD, 3))
    w = rng.standard_normal((N_FD, C_FD))
    F = rng.standard_normal((C_FD, D_, D_, D_))
    if seed % 2 == 0:
        return xyz, w, F, 1.5, "scalar"
    return xyz, w, F, rng.uniform(0.8, 2.0, N_FD), "atom-wise"


def _clear_of_the_radius(xyz, radii, radii_type):
    """(N,) bool: no voxel centre lies within NEAR of the atom's radius, so membership cannot change under the step."""
    ax = gr.axis(D_)
    out = np.zeros(xyz.shape[0], bool)
    for n, p in enumerate(xyz):
        r = float(radii) if radii_type == "scalar" else float(radii[n])
        d = np.sqrt(((p[0] - ax) ** 2)[:, None, None] + ((p[1] - ax) ** 2)[None, :, None] + ((p[2] - ax) ** 2)[None, None, :])
        out[n] = np.abs(d - r).min() > NEAR
    return out


def _fd(xyz, w, F, radii, radii_type, h):
    """(N, 3, 3): central differences of the yardstick's coordinate gradient, column a from steps along axis a."""
    out = np.zeros((xyz.shape[0], 3, 3))
    for a in range(3):
        step = np.zeros(3)
        step[a] = h
        kw = dict(w=w, mode="features", precision=64)
        gp = gr.reference(xyz + step, F, radii, radii_type, **kw)["coords"][0]
        gm = gr.reference(xyz - step, F, radii, radii_type, **kw)["coords"][0]
        out[:, :, a] = (gp - gm) / (2.0 * h)
    return out


@pytest.mark.parametrize("seed", range(6))
def test_reference_hessian_matches_differences_of_the_gradient_reference(seed):
    xyz, w, F, radii, radii_type = _draw(seed)
    ref = hr.reference(xyz, F, radii, radii_type, w=w, mode="features", precision=64)
    yard = gr.reference(xyz, F, radii, radii_type, w=w, mode="features", precision=64)["coords"]
    assert np.array_equal(ref["g"][0], yard[0]) or np.abs(ref["g"][0] - yard[0]).max() <= 1e-13 * yard[1].max()
    H, bH = hr.full(ref["H"][0]), hr.full(ref["H"][1])
    live = ref["s"][1] > 0
    keep = live & _clear_of_the_radius(xyz, radii, radii_type)
    assert keep.sum() >= 0.75 * live.sum(), (int(keep.sum()), int(live.sum()))
    fd1, fd2 = _fd(xyz, w, F, radii, radii_type, FD_H), _fd(xyz, w, F, radii, radii_type, FD_H / 2)
    err = np.abs(H - fd2)[keep]
    bar = (2.0 * np.abs(fd1 - fd2) + 1e-9 * bH)[keep]
    print(f"seed {seed}: {int(keep.sum())} of {int(live.sum())} live atoms compared, worst error / bar {float((err / bar).max()):.3g}")
    assert (err <= bar).all(), float((err / bar).max())


# ---- the twist helper against differences of a smooth analytic S(p) under exp twists ---------------------------------------------
def _smooth(seed=3, N=7):
    """S(p) = sum_n a_n . p_n + 0.5 p_n^T B_n p_n + sum_ijk T_n[ijk] p_i p_j p_k, with its gradient and Hessian per atom."""
    rng = np.random.default_rng(seed)
    a, Bm, T = rng.standard_normal((N, 3)), rng.standard_normal((N, 3, 3)), 0.3 * rng.standard_normal((N, 3, 3, 3))
    Bm = 0.5 * (Bm + Bm.transpose(0, 2, 1))
    T = sum(T.transpose((0,) + tuple(1 + np.array(pm))) for pm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))) / 6.0

    def S(p):
        return float(sum(a[n] @ p[n] + 0.5 * p[n] @ Bm[n] @ p[n] + np.einsum("ijk,i,j,k", T[n], p[n], p[n], p[n]) for n in range(N)))

    def g(p):
        return np.array([a[n] + Bm[n] @ p[n] + 3.0 * np.einsum("ijk,j,k", T[n], p[n], p[n]) for n in range(N)])

    def H(p):
        return np.array([Bm[n] + 6.0 * np.einsum("ijk,k", T[n], p[n]) for n in range(N)])

    return rng.uniform(-1, 1, (N, 3)), rng.uniform(-1, 1, 3), S, g, H


def test_twist_helper_matches_differences_under_exp_twists():
    p, pivot, S, g, H = _smooth()

    def moved(xi):
        return (p - pivot) @ hr.exp_so3(xi[3:]).T + pivot + xi[:3]

    G, _, X, _ = hr.twist(p, g(p), H(p), pivot)
    h = 1e-4
    E = np.eye(6)
    fdG = np.array([(S(moved(h * E[i])) - S(moved(-h * E[i]))) / (2 * h) for i in range(6)])
    fdX = np.zeros((6, 6))
    for i in range(6):
        for j in range(6):
            fdX[i, j] = (S(moved(h * (E[i] + E[j]))) - S(moved(h * (E[i] - E[j]))) - S(moved(h * (E[j] - E[i])))
                         + S(moved(-h * (E[i] + E[j])))) / (4 * h * h)
    eG, eX = np.abs(G - fdG).max(), np.abs(X - fdX).max()
    print(f"twist helper: |G - FD| {eG:.3g} of max |G| {np.abs(G).max():.3g}, |Hxi - FD| {eX:.3g} of max |Hxi| {np.abs(X).max():.3g}")
    assert np.abs(X - X.T).max() <= 1e-14 * np.abs(X).max()  # (numpy's products: symmetric to rounding)
    assert eG <= 1e-5 * np.abs(G).max()
    assert eX <= 1e-5 * np.abs(X).max()


def test_twist_helper_skips_dead_atoms_and_bounds_its_values():
    p, pivot, S, g, H = _smooth()
    gg, HH = g(p), H(p)
    G, bG, X, bX = hr.twist(p, gg, HH, pivot)
    assert (np.abs(G) <= bG * (1 + 1e-12)).all() and (np.abs(X) <= bX * (1 + 1e-12)).all()
    p2 = np.concatenate([p, [[np.nan, np.inf, 0.0]]])
    got = hr.twist(p2, np.concatenate([gg, np.zeros((1, 3))]), np.concatenate([HH, np.zeros((1, 3, 3))]), pivot)
    for x, y in zip(got, (G, bG, X, bX)):
        assert np.array_equal(x, y)


# ---- apply_twist on CPU tensors --------------------------------------------------------------------------------------------------
def test_apply_twist_realises_the_twist_about_the_image_of_the_centre():
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import apply_twist
    from tests.pose_reference import rotation as matrix

    rng = np.random.default_rng(5)
    B = 4
    q = rng.standard_normal((B, 4))
    q[1] /= np.linalg.norm(q[1])  # (one unit quaternion, the others unnormalised: M scales by |q|^2)
    t, c = rng.standard_normal((B, 3)), rng.standard_normal((B, 3))
    xi = 0.5 * rng.standard_normal((B, 6))
    xi[2, 3:] = 0.0  # omega = 0
    xi[3] = 0.0
    q2, t2 = apply_twist(torch.tensor(q), torch.tensor(t), torch.tensor(xi))
    assert q2.dtype == torch.float64 and t2.dtype == torch.float64 and tuple(q2.shape) == (B, 4) and tuple(t2.shape) == (B, 3)
    assert torch.isfinite(q2).all() and torch.isfinite(t2).all()
    x = rng.standard_normal((9, 3))
    for b in range(B):
        posed = (x - c[b]) @ matrix(q[b]).T + t[b]
        want = (posed - t[b]) @ hr.exp_so3(xi[b, 3:]).T + t[b] + xi[b, :3]
        got = (x - c[b]) @ matrix(q2[b].numpy()).T + t2[b].numpy()
        assert np.abs(got - want).max() <= 1e-12, (b, np.abs(got - want).max())
    assert np.array_equal(q2[3].numpy(), q[3]) and np.array_equal(t2[3].numpy(), t[3])  # xi = 0: the pose itself
    # numpy poses are taken too
    q3, t3 = apply_twist(q, t, xi)
    assert torch.equal(q3, q2) and torch.equal(t3, t2)
