"""Scores against a field grid without a GPU: the C ABI entry (mvx_score_batch) and the checks it makes before it touches a
device, the errors the Python layer raises before it needs the library, and the score
kernels' registers read from mvx_score.o. (A stride that is neither 0 nor C * D^3 and a channel of 4 GiB are judged against the
handle's dimension: tests/test_hip_score.py checks them with a real handle.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, P, call, records
from tests.fake_voxelizer import fake as _fake  # (a voxelizer without a handle)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _score(handle=None, mode=0, coords=P, channels=P, radii=None, radii_type=0, offsets=(0, 3), xforms=None, B=1, C_=4, field=P,
           stride=0, scores=P, atom_scores=None, grad_coords=None, grad_features=None):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_score_batch, handle, mode, coords, channels, radii, 1.0, radii_type,
                None if off is None else off.ctypes.data, None if xforms is None else C.addressof(xforms), B, C_, field, stride, scores,
                atom_scores, grad_coords, grad_features, None)


@pytest.mark.parametrize("kw, words", [
    # what mvx_backward_batch rejects
    (dict(mode=3), "mode"),
    (dict(mode=-1), "mode"),
    (dict(mode=1, grad_features=P), "grad_features"),
    (dict(mode=2, C_=1, grad_features=P), "grad_features"),
    (dict(C_=0), "C must be > 0"),
    (dict(mode=2, C_=3), "C = 1"),
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
    (dict(handle=P, channels=None), "channels"),
    (dict(handle=P, radii_type=1), "radii array"),
    # its own
    (dict(scores=None), "scores"),
    (dict(handle=P, field=None), "coords / field"),
    (dict(stride=-1), "field_mol_stride"),
    (dict(stride=-4 * 16 ** 3), "field_mol_stride"),
])
def test_score_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _score(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_all_optional_outputs_may_be_null():
    # (scores only: the both-outputs-NULL rule of mvx_backward_batch does not apply; the call gets as far as the handle)
    rc, msg = _score(atom_scores=None, grad_coords=None, grad_features=None)
    assert rc == MVX_ERR_INVALID and "null handle" in msg, (rc, msg)
    rc, msg = _score(atom_scores=P, grad_coords=P, grad_features=P)
    assert rc == MVX_ERR_INVALID and "null handle" in msg, (rc, msg)


def test_no_molecules_need_no_scores():
    rc, msg = _score(B=0, offsets=(0,), scores=None, field=None, coords=None)
    assert rc == MVX_ERR_INVALID and "null handle" in msg, (rc, msg)


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), offsets=np.array([0, 2, N][:B + 1]), centers=None,
                channels=rng.standard_normal((N, C_)).astype(np.float32), radii=1.0)


def test_voxelizer_has_the_score_methods():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    bat = inspect.signature(Voxelizer.score_batch).parameters
    assert list(bat) == ["self", "coords", "offsets", "centers", "channels", "radii", "field", "num_channels", "random_translation",
                         "random_rotation", "per_atom"]
    pos = inspect.signature(Voxelizer.score_posed_batch).parameters
    assert list(pos) == ["self", "coords", "offsets", "centers", "quaternions", "translations", "channels", "radii", "field",
                         "num_channels", "per_atom"]
    assert bat["num_channels"].default is None and bat["random_translation"].default == 0.0
    assert bat["random_rotation"].default is False and bat["per_atom"].default is False
    assert pos["num_channels"].default is None and pos["per_atom"].default is False


@pytest.mark.parametrize("shape", [(4, 16, 16), (3, 16, 16, 16), (4, 16, 16, 15), (3, 4, 16, 16, 16), (2, 5, 16, 16, 16), ()])
def test_a_field_of_the_wrong_shape_is_an_assertion_error(shape):
    import torch

    a = _args()
    with pytest.raises(AssertionError, match="field does not match dimension"):
        _fake().score_batch(field=torch.zeros(shape), **a)
    a.pop("centers")
    with pytest.raises(AssertionError, match="quaternions does not match dimension"):  # (the posed form checks its poses first)
        _fake().score_posed_batch(field=torch.zeros(shape), centers=None, quaternions=np.ones((2, 3)), translations=np.zeros((2, 3)), **a)


def test_the_other_shape_checks_are_those_of_the_batch_path():
    import torch

    a = _args()
    F = torch.zeros((4, 16, 16, 16))
    with pytest.raises(AssertionError, match="offsets must span coords"):
        _fake().score_batch(field=F, **dict(a, offsets=np.array([0, 2, 5])))
    with pytest.raises(AssertionError, match="atom features does not match"):
        _fake().score_batch(field=F, **dict(a, channels=a["channels"][:5]))
    with pytest.raises(AssertionError, match="radii should be scalar"):
        _fake().score_batch(field=F, **dict(a, radii=np.ones(6, np.float32)))


def test_a_field_that_requires_grad_is_not_supported():
    import torch

    F = torch.zeros((4, 16, 16, 16), requires_grad=True)
    for diff in (False, True):
        with pytest.raises(NotImplementedError, match="dS/dfield is the grid itself.*forward_batch"):
            _fake(differentiable=diff).score_batch(field=F, **_args())
    a = _args()
    a.pop("centers")
    with pytest.raises(NotImplementedError, match="forward_batch"):
        _fake().score_posed_batch(field=F, centers=None, quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)), **a)


def test_scores_need_torch_output():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_batch(field=F, **_args())
    a = _args()
    a.pop("centers")
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").score_posed_batch(field=F, centers=None, quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)), **a)


def test_radii_and_sigma_that_require_grad_are_not_supported():
    import torch

    F = torch.zeros((4, 16, 16, 16))
    a = _args()
    r = torch.ones(6, requires_grad=True)
    with pytest.raises(NotImplementedError, match="no gradient with respect to radii"):
        _fake("atom-wise", differentiable=True, radii_grad=True).score_batch(field=F, **dict(a, radii=r))
    sig = torch.tensor(0.5, requires_grad=True)
    with pytest.raises(NotImplementedError, match="no gradient with respect to sigma"):
        _fake(differentiable=True, sigma_grad=True, _sigma_src=(sig, sig._version, 0.5)).score_batch(field=F, **a)
    rs = torch.tensor([1.0], requires_grad=True)
    with pytest.raises(NotImplementedError, match="no gradient with respect to a scalar radius"):
        _fake(differentiable=True, radii_grad=True).score_batch(field=F, **dict(a, radii=rs))


# ---- kernel resources --------------------------------------------------------------------------------------------------------
# <grid type, mode (0 features, 1 types / single), gaussian, channel-wise radii>: VGPRs of the shipped build (tools/regs.py)
SHIPPED_VGPR = {
    ("float", 0, True, False): 178, ("float", 0, True, True): 184, ("float", 0, False, False): 166, ("float", 0, False, True): 178,
    ("float", 1, True, False): 34, ("float", 1, False, False): 18,
    ("double", 0, True, False): 193, ("double", 0, True, True): 140, ("double", 0, False, False): 157, ("double", 0, False, True): 112,
    ("double", 1, True, False): 54, ("double", 1, False, False): 18,
}
VGPR_SLACK = 6  # (every float kernel then still fits two waves per SIMD: 512 / 190)


def _variant(name):
    """('float' | 'bf16' | 'double', mode, gauss, chanwise) of a score_kernel name (tools/regs.py demangles __bf16 too)."""
    m = re.search(r"score_kernel<(float|double|__bf16), (\d), (true|false), (true|false)>", name)
    assert m, name
    return m.group(1).strip("_"), int(m.group(2)), m.group(3) == "true", m.group(4) == "true"


def test_score_kernels_keep_their_registers():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_score.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_score.o not built")
    assert obj in regs.KERNEL_OBJECTS
    res = regs.kernel_resources(obj)
    walk = {k: v for k, v in res.items() if "score_kernel" in k}
    assert len(walk) == 18, sorted(walk)  # 3 grid types x (features: 2 x 2, types / single: 2), as grad_kernel
    seen = set()
    for k, r in walk.items():
        gt, mode, gauss, chanwise = _variant(k)
        seen.add((gt, mode, gauss, chanwise))
        assert r["vspill"] == 0 and r["lds"] == 0, (k, r)
        assert r["vgpr"] <= SHIPPED_VGPR[("float" if gt == "bf16" else gt, mode, gauss, chanwise)] + VGPR_SLACK, (k, r)
        # float32 arithmetic: no scratch at all; float64 features: the 272 bytes of wave_sum32's address selects, as grad_kernel
        assert r["scratch"] == (272 if (gt == "double" and mode == 0) else 0), (k, r)
    assert len(seen) == 18
    red = res["score_reduce_kernel"]
    assert red["scratch"] == 0 and red["vspill"] == 0 and red["sspill"] == 0 and red["lds"] == 4 * 8 and red["vgpr"] <= 16, red
