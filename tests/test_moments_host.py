"""Host half of tests/test_hip_moments.py: no GPU, nothing is launched.

* the method surface of moments_batch / moments_posed_batch and the guards they raise before the library is needed;
* the C ABI entry mvx_moments_batch: its rejections and their order (the four
  unsupported configurations read the handle and need a real one: tests/test_hip_moments.py);
* the registers of moments_kernel and moments_finish_kernel read from mvx_moments.o;
* tests/moments_reference.py itself: exact sums against math.fsum, and a float64 numpy sum inside bound().
"""
import ctypes as C
import inspect
from fractions import Fraction
import math
import os
import re

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import moments_reference as MR
from tests.abi import MVX_ERR_INVALID, P, call, declarations, records
from tests.fake_voxelizer import fake as _fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 31
POSE = _lib.MVX_XF_POSE_PTR


# ---- the method surface ------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), offsets=np.array([0, 2, N][:B + 1]), centers=None,
                channels=rng.standard_normal((N, C_)).astype(np.float32), radii=1.0)


def _posed(a):
    a = dict(a)
    a.pop("centers")
    return dict(centers=None, quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)), **a)


def test_voxelizer_has_the_moments_methods():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    s = inspect.signature(Voxelizer.moments_batch).parameters
    assert list(s) == ["self", "coords", "offsets", "centers", "channels", "radii", "target", "num_channels", "random_translation",
                       "random_rotation"]
    assert s["target"].default is None and s["num_channels"].default is None
    assert s["random_translation"].default == 0.0 and s["random_rotation"].default is False
    p = inspect.signature(Voxelizer.moments_posed_batch).parameters
    assert list(p) == ["self", "coords", "offsets", "centers", "quaternions", "translations", "channels", "radii", "target",
                       "num_channels"]
    assert p["target"].default is None and p["num_channels"].default is None
    assert "autograd" in Voxelizer.moments_batch.__doc__ and "autograd" in Voxelizer.moments_posed_batch.__doc__


@pytest.mark.parametrize("attrs, kw, words", [
    (dict(precision=64), {}, "precision 64"),
    (dict(radii_type="channel-wise"), dict(radii=np.ones(4, np.float32)), "channel-wise radii with features"),
    (dict(dimension=18), {}, "no multiple of 4"),
    (dict(dimension=24, blockdim=12), {}, "blockdim=12"),
])
def test_the_unsupported_configurations_name_moments_batch_and_the_way_out(attrs, kw, words):
    a = dict(_args(), **kw)
    want = r"moments_batch does not support .*" + re.escape(words) + r".*forward_batch\(\.\.\.\)"
    with pytest.raises(NotImplementedError, match=want):
        _fake(**attrs).moments_batch(**a)
    with pytest.raises(NotImplementedError, match=want):
        _fake(**attrs).moments_posed_batch(**_posed(a))


def test_moments_need_torch_output_and_a_target_of_the_grids_shape():
    with pytest.raises(ValueError, match="moments_batch / moments_posed_batch need output='torch'"):
        _fake(output="numpy").moments_batch(**_args())
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").moments_posed_batch(**_posed(_args()))
    for bad in (np.zeros((4, 16, 16, 8), np.float32), np.zeros((3, 16, 16, 16), np.float32), np.zeros((2, 4, 16, 16, 16), np.float32)):
        with pytest.raises(AssertionError, match="target does not match dimension"):
            _fake().moments_batch(target=bad, **_args())  # (the posed form packs its poses on the device first: tests/test_hip_moments.py)
    # forward_batch's argument rules come first
    with pytest.raises(AssertionError, match="offsets must span coords"):
        _fake().moments_batch(target=np.zeros((3, 16, 16, 16), np.float32), **dict(_args(), offsets=np.array([0, 2, 5])))


def test_a_voxelizer_made_with_new_still_has_every_default():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    v = Voxelizer.__new__(Voxelizer)
    assert v.precision == 32 and v.blockdim == 8 and v._sum_parts == 1  # (the class-level defaults; moments_batch adds no attribute)
    assert not [k for k in vars(Voxelizer) if "moment" in k and not callable(getattr(Voxelizer, k))]


# ---- the C ABI entry ---------------------------------------------------------------------------------------------------------
def test_the_header_has_a_float_target_and_double_moments():
    # the types, not only pointer or not
    types = {name: text for text, name in declarations()["mvx_moments_batch"][1]}
    assert types["target"] == "const float *" and types["moments"] == "double *"


BAD_POSE = records([POSE | _lib.MVX_XF_ROTATE])


def _moments(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, offsets=(0, 3), xforms=None, B=1, C_=4, target=None, moments=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_moments_batch, h, mode, coords, channels, radii, 1.0, rt, None if off is None else off.ctypes.data,
                None if xforms is None else C.addressof(xforms), B, C_, target, moments, None)


M_MODE = "bad mode (0 features, 1 types, 2 single)"
M_C = "C must be > 0"
M_SINGLE = "single mode has one channel (C = 1)"
M_B = "B must be >= 0"
M_OUT = "moments must not be null"
M_RTYPE = "bad radii_type"
M_CHANWISE = "Channel-Wise Radii Type is not supported"
M_OFFNULL = "offsets must not be null"
M_OFF0 = "offsets[0] must be 0"
M_OFFDEC = "offsets must be non-decreasing"
M_HANDLE = "null handle"
M_POSE = "a MVX_XF_POSE_PTR record must have every other flag bit clear and a non-null center_ptr"
M_MANY = "too many atoms"
M_COORDS = "coords must not be null"
M_CHANNELS = "channels must not be null"
M_RADII = "radii array required"


def test_moments_batch_reports_the_earlier_of_two_mistakes():
    """Every call breaks two rules that follow each other in the entry's chain and must report the earlier one; the last call
    breaks the last rule that can be reached without a real handle alone. Texts are compared in full. Nothing here touches a
    device: this machine has none."""
    rows = [
        (dict(mode=3, C_=0), M_MODE),
        (dict(mode=-1, C_=0), M_MODE),
        (dict(C_=0, B=-1), M_C),
        (dict(mode=2, C_=3, B=-1), M_SINGLE),
        (dict(B=-1, moments=None), M_B),
        (dict(moments=None, rt=7), M_OUT),
        (dict(rt=7, offsets=None), M_RTYPE),
        (dict(mode=2, C_=1, rt=2, radii=P, offsets=None), M_CHANWISE),
        (dict(offsets=None), M_OFFNULL),  # (no offsets: the offset rules cannot be broken as well; the handle is null too)
        (dict(offsets=(1, 3)), M_OFF0),
        (dict(B=2, offsets=(0, 3, 2)), M_OFFDEC),
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE, offsets=(0, BIG)), M_POSE),
        (dict(h=P, offsets=(0, BIG), coords=None), M_MANY),
        (dict(h=P, coords=None, channels=None), M_COORDS),
        (dict(h=P, channels=None, rt=1), M_CHANNELS),
        (dict(h=P, rt=1), M_RADII),
        # across the seams between the entry's own rule (moments, behind B) and the chains it shares with the other entries
        (dict(C_=0, moments=None), M_C),
        (dict(mode=2, C_=3, moments=None), M_SINGLE),
        (dict(B=-1, moments=None, rt=7), M_B),
        (dict(moments=None, mode=2, C_=1, rt=2, radii=P), M_OUT),
        (dict(moments=None, offsets=None), M_OUT),
        (dict(moments=None, offsets=(1, 3)), M_OUT),
    ]
    for kw, want in rows:
        rc, msg = _moments(**kw)
        assert rc == MVX_ERR_INVALID and msg == want, (kw, rc, msg, want)


def test_no_molecules_and_a_target_get_as_far_as_the_handle():
    for kw in (dict(B=0, offsets=(0,), coords=None, channels=None, moments=None), dict(target=P), dict(B=0, offsets=(0,), moments=P)):
        rc, msg = _moments(**kw)
        assert rc == MVX_ERR_INVALID and msg == M_HANDLE, (kw, rc, msg)


# ---- kernel resources --------------------------------------------------------------------------------------------------------
# <gaussian, threads, target>: VGPRs of the shipped build (tools/regs.py); no instantiation spills or uses scratch
SHIPPED_VGPR = {(g, t, tg): (94 if tg else 88) for g in (True, False) for t in (512, 1024) for tg in (True, False)}
VGPR_SLACK = 6


def test_moments_kernels_keep_their_accumulators_in_registers():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_moments.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_moments.o not built")
    assert obj in regs.KERNEL_OBJECTS
    res = regs.kernel_resources(obj)
    ks = {k: v for k, v in res.items() if k.startswith("moments_kernel<")}
    tf = ("true", "false")
    assert sorted(ks) == sorted(f"moments_kernel<{g}, {t}, {tg}>" for g in tf for t in (512, 1024) for tg in tf), sorted(ks)
    for name, r in ks.items():
        m = re.match(r"moments_kernel<(true|false), (\d+), (true|false)>", name)
        key = (m.group(1) == "true", int(m.group(2)), m.group(3) == "true")
        assert r["vgpr"] <= 128, (name, r)  # two 8-wave workgroups per compute unit, as the summed kernel
        assert r["vspill"] == 0 and r["sspill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= SHIPPED_VGPR[key] + VGPR_SLACK, (name, r)
    fin = res["moments_finish_kernel"]
    assert fin["vspill"] == 0 and fin["sspill"] == 0 and fin["scratch"] == 0 and fin["lds"] == 0, fin
    # the names stay clear of the patterns other host tests count kernels by
    for name in res:
        assert not name.startswith(("voxelize_kernel<", "voxelize_sum_kernel<", "voxelize_sum_parts_kernel<", "voxelize_pair_kernel<",
                                    "voxelize_narrow_kernel<", "voxelize64_kernel<", "xbin_kernel<")), name
        assert not any(w in name for w in ("grad_kernel", "score_kernel", "_bf16_kernel", "_ndhwc_kernel")), name


# ---- the reference itself ----------------------------------------------------------------------------------------------------
def _grids(seed, B=3, C_=2, D=6):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal((B, C_, D, D, D)) * np.exp2(rng.integers(-30, 12, (B, C_, D, D, D)))).astype(np.float32)
    g[rng.random(g.shape) < 0.4] = 0.0  # most voxels of a grid are empty
    g[0, 0] = 0.0  # an empty channel
    t = rng.standard_normal((C_, D, D, D)).astype(np.float32)
    return g, t


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_exact_sums_are_math_fsum_of_the_exact_terms(seed):
    g, t = _grids(seed)
    terms = MR.terms_of(g, t)
    assert terms.shape == (3, 2, 3, 216) and terms.dtype == np.float64
    g64, t64 = g.reshape(3, 2, -1).astype(np.float64), t.reshape(2, -1).astype(np.float64)
    assert np.array_equal(terms[:, :, 0], g64) and np.array_equal(terms[:, :, 1], g64 * g64) and np.array_equal(terms[:, :, 2], g64 * t64)
    for a, b, p in zip(g64[1, 1, :40], t64[1, :40], terms[1, 1, 2, :40]):  # the products are exact
        assert Fraction(float(a)) * Fraction(float(b)) == Fraction(float(p))
    got = MR.moments_of(g, t)
    assert got.shape == (3, 2, 3) and got.dtype == np.float64
    want = np.array([[[math.fsum(terms[b, c, k].tolist()) for k in range(3)] for c in range(2)] for b in range(3)])
    assert np.array_equal(got, want)
    assert (got[0, 0] == 0).all()
    assert np.array_equal(MR.moments_of(g), want[:, :, :2]) and np.array_equal(MR.moments_of(g[1], t), want[1])
    m, b = MR.moments_and_bound(g, t)
    assert np.array_equal(m, want) and np.array_equal(b, MR.bound(terms))


def test_exact_sums_survive_cancellation_and_small_blocks(monkeypatch):
    x = np.array([[1e100, 1.0, -1e100, 2.0 ** -300], [3.0, 2.0 ** -60, -3.0, 2.0 ** -61], [0.0, 0.0, 0.0, 0.0]])
    assert np.array_equal(MR.exact_sums(x), [math.fsum(r) for r in x.tolist()])
    assert MR.exact_sums(x)[0] == 1.0 and MR.exact_sums(x)[2] == 0.0
    monkeypatch.setattr(MR, "ROWS_AT_ONCE", 8)  # one or two rows per block
    assert np.array_equal(MR.exact_sums(x), [math.fsum(r) for r in x.tolist()])
    g, t = _grids(5, B=5, C_=3, D=4)
    monkeypatch.setattr(MR, "ROWS_AT_ONCE", 4 ** 3 * 3 * 2)  # two molecules at once
    m, _ = MR.moments_and_bound(g, t)
    monkeypatch.setattr(MR, "ROWS_AT_ONCE", 1 << 22)
    assert np.array_equal(m, MR.moments_of(g, t))


@pytest.mark.parametrize("seed", [3, 4])
def test_a_float64_numpy_sum_lies_within_the_bound(seed):
    g, t = _grids(seed, D=8)
    terms = MR.terms_of(g, t)
    exact, bnd = MR.moments_of(g, t), MR.bound(terms)
    assert bnd.shape == exact.shape and (bnd >= 0).all() and (bnd[0, 0] == 0).all()
    n = 8 ** 3
    assert np.allclose(bnd, (n - 1) * 2.0 ** -53 * np.abs(terms).sum(-1), rtol=1e-12, atol=0)
    for s in (terms.sum(-1), np.cumsum(terms, axis=-1)[..., -1], terms[..., ::-1].cumsum(-1)[..., -1]):  # pairwise, forward, backward
        assert (np.abs(s - exact) <= bnd).all()
    assert (np.abs(np.cumsum(terms, axis=-1)[..., -1] - exact) > 0).any()  # (the check is not vacuous: plain sums do round)
