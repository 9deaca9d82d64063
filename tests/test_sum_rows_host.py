"""Host half of tests/test_hip_sum.py: no GPU, nothing is launched.

* every row of tests/sum_rows.py reaches what its `reaches` column says, by numpy and the pre-pass's own culls alone;
* the method surface of forward_sum / forward_posed_sum and the field_grad constructor option;
* the C ABI entry mvx_forward_sum_batch: its rejections and their order (the rules that read the handle -
  the four unsupported configurations and the alignment of `out` - need a real handle: tests/test_hip_sum.py);
* the NotImplementedErrors the Python layer raises before it needs the library;
* the registers of voxelize_sum_kernel read from mvx_sum.o.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, P, call, records
from tests.fake_voxelizer import fake as _fake  # (a voxelizer without a handle)
from tests import sum_rows as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 31
POSE = _lib.MVX_XF_POSE_PTR


# ---- the rows ----------------------------------------------------------------------------------------------------------------
def test_the_table_is_the_one_the_issue_sets():
    got = [(r.id, r.D, r.C, r.mode, r.radii_type, r.density, len(r.sizes), sum(r.sizes)) for r in R.ROWS]
    assert got == [
        ("light", 16, 5, "features", "scalar", "gaussian", 7, 81),
        ("carry", 16, 32, "features", "atom-wise", "gaussian", 12, 480),
        ("rounds", 16, 32, "features", "scalar", "gaussian", 3, 410),
        ("chunks", 24, 33, "features", "scalar", "gaussian", 9, 270),
        ("wide", 24, 65, "features", "atom-wise", "gaussian", 4, 200),
        ("types", 24, 8, "types", "channel-wise", "gaussian", 5, 300),
        ("single", 40, 1, "single", "scalar", "binary", 6, 480),
        ("long", 72, 4, "features", "scalar", "gaussian", 3, 600),
    ]
    assert R.BY_ID["light"].sizes == (0, 1, 3, 40, 0, 12, 25) and R.BY_ID["rounds"].sizes == (20, 300, 90)
    for r in R.ROWS:
        assert r.D % 4 == 0
        d = R.make(r.id)
        assert d["xyz"].shape == (d["N"], 3) and d["off"][-1] == d["N"] and d["cen"].shape == (d["B"], 3)
        assert np.abs(d["cen"]).max() > 5.0  # (the centres matter: the merged molecule is not the coordinates themselves)


def test_light_has_empty_molecules_and_one_outside_the_box():
    d = R.make("light")
    sizes = np.diff(d["off"])
    assert sizes[0] == 0 and sizes[4] == 0 and 0 < sizes[3] and 0 < sizes[5]  # empty first and in the middle
    o = R.OUTSIDE_MOLECULE
    lo, hi = int(d["off"][o]), int(d["off"][o + 1])
    assert hi - lo == 3
    _, upper = R.counts(d, lo, hi)
    assert upper.sum() == 0  # no slab has a candidate from it: every atom fails the box cull
    half = R.RES * 15 / 2
    assert (np.abs(R.merged(d)[lo:hi]) > half + 1.0 + 1.0).all()
    for b in (1, 3, 5, 6):  # the others are inside
        assert R.counts(d, int(d["off"][b]), int(d["off"][b + 1]))[0].max() > 0
    # split at 5 (tests/test_hip_sum.py), the first call also ENDS with an empty molecule
    assert sizes[:5][-1] == 0


def test_carry_overflows_a_line_only_as_a_batch():
    d = R.make("carry")
    for b in range(d["B"]):
        _, upper = R.counts(d, int(d["off"][b]), int(d["off"][b + 1]))
        assert upper.max() <= R.ONE_ROUND
    lower, _ = R.counts(d, 0, d["N"])
    assert lower.max() > R.LINE_CAP, int(lower.max())
    assert 0.8 <= d["r_atom"].min() and d["r_atom"].max() <= 1.6 and d["r_atom"].std() > 0.1


def test_rounds_has_the_extension_and_the_x_list_inside_one_molecule():
    d = R.make("rounds")
    lo90, up90 = R.counts(d, int(d["off"][2]), int(d["off"][3]))
    assert lo90.max() > R.ONE_ROUND and up90.max() <= R.LINE_CAP  # rounds over line + extension
    lo300, _ = R.counts(d, int(d["off"][1]), int(d["off"][2]))
    assert lo300.max() > R.LINE_CAP  # the (molecule, x-slab) list
    _, up20 = R.counts(d, 0, int(d["off"][1]))
    assert up20.max() <= R.ONE_ROUND
    assert np.linalg.norm(R.merged(d), axis=1).max() <= 1.0  # clustered within 1 A


def test_types_has_one_type_outside_the_channels():
    d = R.make("types")
    t = d["chan"]
    bad = (t < 0) | (t >= 8)
    assert bad.sum() == 1 and bad[R.BAD_TYPE_ATOM]
    assert set(t[~bad]) == set(range(8)) and d["radii"].shape == (8,)
    w = R.features_of(d)
    assert w[R.BAD_TYPE_ATOM].sum() == 0 and (w.sum(axis=1)[~bad] == 1).all()


def test_channel_chunks_and_waves_per_slab():
    ncc = {r.id: -(-r.C // 32) for r in R.ROWS}
    assert ncc["chunks"] == 2 and R.BY_ID["chunks"].C == 33 and ncc["wide"] == 3 and ncc["light"] == 1
    assert R.nw_of(R.BY_ID["single"]) == 5 and R.BY_ID["single"].density == "binary"
    assert R.nw_of(R.BY_ID["long"]) == 9
    for r in R.ROWS:  # the library's own plan of a 32-channel binned call gives these waves per slab
        p = _lib.plan_call(r.D, 32 * ncc[r.id], len(r.sizes), total_atoms=10 ** 8, mode="features")  # (atoms enough for the binned route)
        assert p["route"] == _lib.MVX_ROUTE_BINNED and p["ct"] == 32 and p["ct_rem"] == 0 and p["ncc"] == ncc[r.id], (r.id, p)
        assert p["nw"] == R.nw_of(r) and p["vec_store"] == 1 and p["lane_range"] == 0, (r.id, p)


# ---- the method surface ------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), offsets=np.array([0, 2, N][:B + 1]), centers=None,
                channels=rng.standard_normal((N, C_)).astype(np.float32), radii=1.0)


def test_voxelizer_has_the_sum_methods():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    s = inspect.signature(Voxelizer.forward_sum).parameters
    assert list(s) == ["self", "coords", "offsets", "centers", "channels", "radii", "weights", "num_channels", "out_grid",
                       "accumulate", "random_translation", "random_rotation"]
    assert s["weights"].default is None and s["num_channels"].default is None and s["out_grid"].default is None
    assert s["accumulate"].default is False and s["random_translation"].default == 0.0 and s["random_rotation"].default is False
    p = inspect.signature(Voxelizer.forward_posed_sum).parameters
    assert list(p) == ["self", "coords", "offsets", "centers", "quaternions", "translations", "channels", "radii", "weights",
                       "num_channels", "out_grid", "accumulate"]
    assert p["weights"].default is None and p["out_grid"].default is None and p["accumulate"].default is False
    assert "autograd" in Voxelizer.forward_sum.__doc__ and "autograd" in Voxelizer.forward_posed_sum.__doc__


def test_field_grad_is_a_constructor_option_that_needs_differentiable():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    init = inspect.signature(Voxelizer.__init__).parameters
    assert init["field_grad"].default is False
    with pytest.raises(ValueError, match="field_grad=True needs differentiable=True"):
        Voxelizer(0.5, 16, field_grad=True)  # (raised before anything touches a device)


@pytest.mark.parametrize("attrs, kw, words", [
    (dict(precision=64), {}, "precision 64"),
    (dict(radii_type="channel-wise"), dict(radii=np.ones(4, np.float32)), "channel-wise radii with features"),
    (dict(dimension=18), {}, "no multiple of 4"),
    (dict(dimension=24, blockdim=5), {}, "blockdim=5"),
    (dict(dimension=24, blockdim=12), {}, "blockdim=12"),
])
def test_the_unsupported_configurations_name_the_way_out(attrs, kw, words):
    a = dict(_args(), **kw)
    with pytest.raises(NotImplementedError, match=re.escape(words) + r".*forward_batch\(\.\.\.\)\.sum\(0\)"):
        _fake(**attrs).forward_sum(**a)
    a.pop("centers")
    with pytest.raises(NotImplementedError, match=re.escape(words) + r".*forward_batch\(\.\.\.\)\.sum\(0\)"):
        _fake(**attrs).forward_posed_sum(centers=None, quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)), **a)


def test_supported_blockdims_get_past_the_guard():
    for D, bd in ((16, 8), (24, 16), (16, 16), (12, 12), (24, 24), (16, 5000)):  # whole sub-tiles per block, or one block
        _fake(dimension=D, blockdim=bd)._sum_guard(None)
    for D, bd, lr in ((24, 12, 1), (24, 8, 0), (16, 4, 1), (12, 12, 0), (24, 16, 0)):  # ... exactly mvx_plan.lane_range
        assert _lib.plan_call(D, 32, 2, total_atoms=10, blockdim=bd)["lane_range"] == lr
        if lr:
            with pytest.raises(NotImplementedError):
                _fake(dimension=D, blockdim=bd)._sum_guard(None)


def test_sums_need_torch_output_and_accumulate_needs_a_grid():
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").forward_sum(**_args())
    with pytest.raises(ValueError, match="accumulate=True needs out_grid"):
        _fake().forward_sum(accumulate=True, **_args())
    with pytest.raises(AssertionError, match="offsets must span coords"):
        _fake().forward_sum(**dict(_args(), offsets=np.array([0, 2, 5])))
    with pytest.raises(AssertionError, match="radii should be scalar"):
        _fake().forward_sum(**dict(_args(), radii=np.ones(6, np.float32)))


def test_a_field_that_requires_grad_needs_the_option_and_a_shared_field():
    import torch

    F4 = torch.zeros((4, 16, 16, 16), requires_grad=True)
    F5 = torch.zeros((2, 4, 16, 16, 16), requires_grad=True)
    old = "dS/dfield is the grid itself.*forward_batch"
    with pytest.raises(NotImplementedError, match=old):  # without the option: today's text
        _fake(differentiable=True).score_batch(field=F4, **_args())
    with pytest.raises(NotImplementedError, match=old):  # a field per molecule: its gradient is the B grids
        _fake(differentiable=True, field_grad=True).score_batch(field=F5, **_args())
    a = _args()
    a.pop("centers")
    posed = dict(centers=None, quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)))
    with pytest.raises(NotImplementedError, match=old):
        _fake(differentiable=True, field_grad=True).score_posed_batch(field=F5, **posed, **a)
    # the views forms keep today's message with the option on
    v = dict(coords=a["coords"], centers=np.zeros((2, 3)), channels=a["channels"], radii=1.0)
    with pytest.raises(NotImplementedError, match=old):
        _fake(differentiable=True, field_grad=True).score_views(field=F4, **v)
    # what forward_sum cannot serve is refused when the score is taken, not in backward()
    with pytest.raises(NotImplementedError, match=r"no multiple of 4.*forward_batch\(\.\.\.\)\.sum\(0\)"):
        _fake(dimension=18, differentiable=True, field_grad=True).score_batch(
            field=torch.zeros((4, 18, 18, 18), requires_grad=True), **_args())


# ---- the C ABI entry ---------------------------------------------------------------------------------------------------------
BAD_POSE = records([POSE | _lib.MVX_XF_ROTATE])


def _sum(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, offsets=(0, 3), xforms=None, B=1, C_=4, weights=None, out=P,
         accumulate=0):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_forward_sum_batch, h, mode, coords, channels, radii, 1.0, rt, None if off is None else off.ctypes.data,
                None if xforms is None else C.addressof(xforms), B, C_, weights, out, accumulate, None)


M_MODE = "bad mode (0 features, 1 types, 2 single)"
M_C = "C must be > 0"
M_SINGLE = "single mode has one channel (C = 1)"
M_OUT = "out must not be null"
M_ACC = "accumulate must be 0 or 1"
M_B = "B must be >= 0"
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


def test_forward_sum_batch_reports_the_earlier_of_two_mistakes():
    """Every call breaks two rules that follow each other in the entry's chain and must report the earlier one; the last call
    breaks the last rule that can be reached without a real handle alone. Texts are compared in full."""
    rows = [
        (dict(mode=3, C_=0), M_MODE),
        (dict(mode=-1, C_=0), M_MODE),
        (dict(C_=0, out=None), M_C),
        (dict(mode=2, C_=3, out=None), M_SINGLE),
        (dict(out=None, accumulate=2), M_OUT),
        (dict(accumulate=2, B=-1), M_ACC),
        (dict(accumulate=-1, B=-1), M_ACC),
        (dict(B=-1, rt=7), M_B),
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
        # across the seams between the entry's own rules (out, accumulate) and the chains it shares with the other entries
        (dict(mode=2, C_=3, accumulate=2), M_SINGLE),
        (dict(out=None, B=-1), M_OUT),
        (dict(out=None, rt=7), M_OUT),
        (dict(accumulate=2, rt=7), M_ACC),
        (dict(accumulate=2, offsets=None), M_ACC),
        (dict(B=-1, offsets=None), M_B),
    ]
    for kw, want in rows:
        rc, msg = _sum(**kw)
        assert rc == MVX_ERR_INVALID and msg == want, (kw, rc, msg, want)


def test_no_molecules_and_no_weights_get_as_far_as_the_handle():
    for kw in (dict(B=0, offsets=(0,), coords=None, channels=None), dict(weights=P), dict(accumulate=1)):
        rc, msg = _sum(**kw)
        assert rc == MVX_ERR_INVALID and msg == M_HANDLE, (kw, rc, msg)


# ---- kernel resources --------------------------------------------------------------------------------------------------------
# <gaussian, threads>: VGPRs of the shipped build (tools/regs.py); no instantiation spills or uses scratch
SHIPPED_VGPR = {(True, 512): 76, (False, 512): 76, (True, 1024): 76, (False, 1024): 76}
VGPR_SLACK = 6


def test_sum_kernels_keep_their_accumulators_in_registers():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_sum.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_sum.o not built")
    assert obj in regs.KERNEL_OBJECTS
    res = regs.kernel_resources(obj)
    ks = {k: v for k, v in res.items() if k.startswith("voxelize_sum_kernel<")}
    assert sorted(ks) == sorted(f"voxelize_sum_kernel<{g}, {t}>" for g in ("true", "false") for t in (512, 1024)), sorted(ks)
    for name, r in ks.items():
        m = re.match(r"voxelize_sum_kernel<(true|false), (\d+)>", name)
        key = (m.group(1) == "true", int(m.group(2)))
        assert r["vgpr"] <= 128, (name, r)  # two 8-wave workgroups per compute unit
        assert r["vspill"] <= 20 and r["scratch"] <= 80, (name, r)  # (the bound of the rarest 32-channel slab variants)
        assert r["vgpr"] <= SHIPPED_VGPR[key] + VGPR_SLACK and r["vspill"] == 0 and r["scratch"] == 0, (name, r)
    sc = res["scale_rows_kernel"]
    assert sc["vspill"] == 0 and sc["scratch"] == 0 and sc["lds"] == 0, sc
