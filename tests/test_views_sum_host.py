"""Host half of tests/test_hip_views_sum.py and tests/test_hip_sum_parts.py: no GPU, nothing is launched.

* the method surface of forward_views_sum / forward_posed_views_sum and of set_sum_parts / sum_parts;
* the ORDER of mvx_forward_views_sum's rejections, in the manner of tests/test_reject_order_host.py: every call breaks two rules
  that follow each other and must report the earlier one, texts compared in full (the rules that read the handle - the four
  unsupported configurations and the alignment of `out` - need a real handle: tests/test_hip_views_sum.py);
* the guards the Python layer raises, with forward_sum's messages, before it needs the library;
* the registers of voxelize_sum_parts_kernel read from mvx_sum.o.
"""
import inspect
import os
import re

import numpy as np
import pytest

import tests.test_reject_order_host as RO  # (the rules every views entry shares, and their texts)
import tests.test_sum_rows_host as SH  # (_fake: a voxelizer without a handle)
from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, P, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the method surface ------------------------------------------------------------------------------------------------------
def test_voxelizer_has_the_views_sum_methods():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    s = inspect.signature(Voxelizer.forward_views_sum).parameters
    assert list(s) == ["self", "coords", "centers", "channels", "radii", "weights", "num_channels", "out_grid", "accumulate",
                       "random_translation", "random_rotation"]
    assert s["weights"].default is None and s["num_channels"].default is None and s["out_grid"].default is None
    assert s["accumulate"].default is False and s["random_translation"].default == 0.0 and s["random_rotation"].default is False
    p = inspect.signature(Voxelizer.forward_posed_views_sum).parameters
    assert list(p) == ["self", "coords", "centers", "quaternions", "translations", "channels", "radii", "weights", "num_channels",
                       "out_grid", "accumulate"]
    assert p["weights"].default is None and p["out_grid"].default is None and p["accumulate"].default is False
    for m in (Voxelizer.forward_views_sum, Voxelizer.forward_posed_views_sum):
        assert "autograd" in m.__doc__


def test_voxelizer_has_the_sum_parts_setting():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    assert list(inspect.signature(Voxelizer.set_sum_parts).parameters) == ["self", "parts"]
    assert isinstance(Voxelizer.sum_parts, property) and Voxelizer.sum_parts.fset is None  # read-only
    assert SH._fake().sum_parts == 1
    assert "DIFFER" in Voxelizer.set_sum_parts.__doc__  # the bits of K > 1 are not those of K = 1, and the docstring says so


# ---- the C ABI entries -------------------------------------------------------------------------------------------------------
def _vsum(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, N=3, C_=4, xforms=RO.ONE, B=1, weights=None, out=P, accumulate=0):
    return call(_lib.load().mvx_forward_views_sum, h, mode, coords, channels, radii, 1.0, rt, N, C_, RO._addr(xforms), B, weights,
                out, accumulate, None)


M_ACC = "accumulate must be 0 or 1"
M_OUT = "out must not be null"


def test_forward_views_sum_reports_the_earlier_of_two_mistakes():
    """The rules every views entry shares (device arrays only: no memory kind to get wrong), then the entry's own - accumulate,
    out, channels - then the handle, then the records. The last row breaks the last rule that is reached without a real handle."""
    RO._check(_vsum, RO._views_chain(dict(accumulate=2), with_in_kind=False) + [
        (dict(accumulate=2, out=None), M_ACC),
        (dict(accumulate=-1, out=None), M_ACC),
        (dict(out=None, channels=None), M_OUT),
        (dict(channels=None), RO.M_CHANNELS),  # (and a null handle)
        (dict(xforms=RO.BAD_POSE), RO.M_HANDLE),
        (dict(weights=P), RO.M_HANDLE),  # (weights are not looked at before the handle)
        (dict(h=P, xforms=RO.BAD_POSE), RO.M_POSE),
    ])


def test_no_views_are_answered_before_anything_is_read():
    """B == 0: MVX_OK, nothing written - but only behind the rules that do not depend on B, the handle among them."""
    rc, msg = _vsum(h=P, B=0, xforms=None, channels=None, out=None)  # (P is never read: the handle's configuration matters to B > 0 only)
    assert rc == 0, msg
    rc, msg = _vsum(B=0, xforms=None, out=None)
    assert rc == MVX_ERR_INVALID and msg == RO.M_HANDLE
    rc, msg = _vsum(h=P, B=0, xforms=None, accumulate=2)
    assert rc == MVX_ERR_INVALID and msg == M_ACC


def test_set_sum_parts_refuses_what_is_out_of_range_and_a_null_handle():
    lib = _lib.load()
    for h, parts, want in ((P, 0, "sum parts must be 1 ... 64"), (P, 65, "sum parts must be 1 ... 64"), (P, -3, "sum parts must be 1 ... 64"),
                           (None, 4, "null handle"), (None, 0, "null handle")):
        assert call(lib.mvx_set_sum_parts, h, parts) == (MVX_ERR_INVALID, want), (h, parts)


# ---- the Python guards -------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), centers=np.zeros((B, 3)), channels=rng.standard_normal((N, C_)).astype(np.float32),
                radii=1.0)


def _posed(a):
    B = a["centers"].shape[0]
    return dict(a, quaternions=np.ones((B, 4)), translations=np.zeros((B, 3)))


@pytest.mark.parametrize("attrs, kw, words", [
    (dict(precision=64), {}, "precision 64"),
    (dict(radii_type="channel-wise"), dict(radii=np.ones(4, np.float32)), "channel-wise radii with features"),
    (dict(dimension=18), {}, "no multiple of 4"),
    (dict(dimension=24, blockdim=5), {}, "blockdim=5"),
    (dict(dimension=24, blockdim=12), {}, "blockdim=12"),
])
def test_the_unsupported_configurations_raise_forward_sums_messages(attrs, kw, words):
    a = dict(_args(), **kw)
    match = "forward_sum does not support.*" + re.escape(words) + r".*forward_batch\(\.\.\.\)\.sum\(0\)"
    with pytest.raises(NotImplementedError, match=match):
        SH._fake(**attrs).forward_views_sum(**a)
    with pytest.raises(NotImplementedError, match=match):
        SH._fake(**attrs).forward_posed_views_sum(**_posed(a))


def test_views_sums_need_torch_output_and_accumulate_needs_a_grid():
    for call in (lambda v, **kw: v.forward_views_sum(**kw), lambda v, **kw: v.forward_posed_views_sum(**_posed(kw))):
        with pytest.raises(ValueError, match="forward_sum / forward_posed_sum need output='torch'"):
            call(SH._fake(output="numpy"), **_args())
    with pytest.raises(ValueError, match="accumulate=True needs out_grid: there is nothing to add to"):
        SH._fake().forward_views_sum(accumulate=True, **_args())
    with pytest.raises(AssertionError, match="radii should be scalar"):
        SH._fake().forward_views_sum(**dict(_args(), radii=np.ones(6, np.float32)))
    with pytest.raises(AssertionError, match="centers does not match dimension"):
        SH._fake().forward_views_sum(**dict(_args(), centers=np.zeros(3)))
    import torch

    with pytest.raises(ValueError, match="contiguous float32 tensor on this voxelizer's device"):
        SH._fake(_device_index=0).forward_views_sum(out_grid=torch.empty((4, 16, 16, 16)), **_args())
    with pytest.raises(AssertionError, match="Output grid dimension incorrect"):
        SH._fake(_device_index=0).forward_views_sum(out_grid=torch.empty((4, 16, 16, 8)), **_args())


# ---- kernel resources --------------------------------------------------------------------------------------------------------
def test_sum_parts_kernels_keep_the_budget_of_the_sum_kernel():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_sum.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_sum.o not built")
    res = regs.kernel_resources(obj)
    ks = {k: v for k, v in res.items() if k.startswith("voxelize_sum_parts_kernel<")}
    assert sorted(ks) == sorted(f"voxelize_sum_parts_kernel<{g}, {t}>" for g in ("true", "false") for t in (512, 1024)), sorted(ks)
    for name, r in ks.items():
        assert r["vgpr"] <= 128 and r["vspill"] == 0 and r["scratch"] == 0, (name, r)  # two 8-wave workgroups per compute unit
    for name in ("sum_parts_reduce_kernel", "view_weights_kernel"):
        assert res[name]["vspill"] == 0 and res[name]["scratch"] == 0 and res[name]["lds"] == 0, (name, res[name])
