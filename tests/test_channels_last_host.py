"""Channels-last (NDHWC) grids without a GPU: the Python option's checks (raised before the library is loaded), the C ABI
additions (mvx_set_grid_layout, mvx_plan_call_layout) and the plan of the layout as a pure function."""
import ctypes as C
import os
import re

import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, call
from tests.test_hip_fuzz import DIMS as FUZZ_DIMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NDHWC, NCDHW = 1, 0


# ---- Python option --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [dict(grid_layout="channels_last", precision=64), dict(grid_layout="channels_last", output="numpy"),
                                dict(grid_layout="nhwc"), dict(grid_layout=3)])
def test_factory_rejects_impossible_layouts_without_a_device(kw, monkeypatch):
    import molvoxel_amd

    def no_load():
        raise AssertionError("the library was loaded before the option was checked")

    monkeypatch.setattr(_lib, "load", no_load)
    with pytest.raises(ValueError, match="grid_layout"):
        molvoxel_amd.create_voxelizer(0.5, 32, "scalar", "gaussian", "hip", **kw)


def test_layout_values_are_parsed_without_a_device():
    import torch

    from molvoxel_amd.voxelizer.hip import Voxelizer

    for v in ("channels_last", torch.channels_last_3d):
        assert Voxelizer._is_channels_last(v, 32, "torch") is True
    for v in (None, "contiguous", torch.contiguous_format):
        assert Voxelizer._is_channels_last(v, 32, "torch") is False
        assert Voxelizer._is_channels_last(v, 64, "numpy") is False
    with pytest.raises(ValueError, match="precision"):
        Voxelizer._is_channels_last(torch.channels_last_3d, 64, "torch")
    assert isinstance(Voxelizer.grid_layout, property)


# ---- C ABI --------------------------------------------------------------------------------------------------------------------
def test_setter_is_declared_in_the_header_and_bound_by_ctypes():
    header = open(os.path.join(ROOT, "include", "mvx.h")).read()
    assert re.search(r"int\s+mvx_set_grid_layout\(mvx_handle \*h, int32_t layout\);", header)
    assert re.search(r"enum mvx_grid_layout \{ MVX_LAYOUT_NCDHW = 0, MVX_LAYOUT_NDHWC = 1 \};", header)
    assert "mvx_plan_call_layout" in header
    assert _lib.SIGNATURES["mvx_set_grid_layout"] == (C.c_int, [_lib.Handle, C.c_int32])
    assert (_lib.MVX_LAYOUT_NCDHW, _lib.MVX_LAYOUT_NDHWC) == (0, 1)
    lib = _lib.load()  # (raises if the library does not export a declared symbol)
    assert lib.mvx_set_grid_layout and lib.mvx_plan_call_layout


@pytest.mark.parametrize("layout, word", [(2, "layout"), (-1, "layout"), (100, "layout"), (NDHWC, "handle"), (NCDHW, "handle")])
def test_setter_rejects_before_a_device_is_looked_for(layout, word):
    """No handle can exist on a machine without a GPU: the setter's checks that need none - the layout value first, then the
    handle - answer MVX_ERR_INVALID, never MVX_ERR_NO_DEVICE."""
    rc, msg = call(_lib.load().mvx_set_grid_layout, None, layout)
    assert rc == MVX_ERR_INVALID
    assert word in msg


# ---- plan ----------------------------------------------------------------------------------------------------------------------
def _raw(query_args, grid_type=None, layout=None):
    q = _lib.MvxPlanQuery(*query_args)
    p = _lib.MvxPlan()
    lib = _lib.load()
    if layout is not None:
        rc = lib.mvx_plan_call_layout(C.byref(q), grid_type or 0, layout, C.byref(p))
    elif grid_type is not None:
        rc = lib.mvx_plan_call_grid(C.byref(q), grid_type, C.byref(p))
    else:
        rc = lib.mvx_plan_call(C.byref(q), C.byref(p))
    return rc, bytes(p)


def _cl(D, Ch, B=1, atoms=None, grid_type=0, **kw):
    if atoms is None:
        atoms = max(1, int(round(4000 * ((D - 1) / 63.0) ** 3)))
    return _lib.plan_call(D, Ch, B, total_atoms=B * atoms, max_atoms=atoms, grid_type=grid_type, layout=NDHWC, **kw)


CHANNELS = (1, 2, 4, 5, 8, 12, 16, 24, 32, 33, 36, 40, 64, 65, 72)


def test_vector_form_exactly_when_channel_runs_are_16_byte_aligned():
    for D in (16, 48, 49, 63, 64, 72, 96):
        for Ch in CHANNELS:
            if Ch == 1:
                continue
            for grid_type, esz in ((_lib.MVX_GRID_REAL, 4), (_lib.MVX_GRID_BF16, 2)):
                for B in (1, 3, 64):
                    want = 1 if (Ch * esz) % 16 == 0 else 0
                    p = _cl(D, Ch, B, grid_type=grid_type)
                    assert p["vec_store"] == want, (D, Ch, grid_type, B)
                    assert _cl(D, Ch, B, grid_type=grid_type, out_aligned16=False)["vec_store"] == 0
                    assert p["xcd_ranges"] == 0 and p["pace"] == 0


def test_every_fuzz_dimension_is_planned_with_slabs_of_at_most_eight_waves():
    for D in sorted(set(FUZZ_DIMS) | {16, 48, 49, 63, 64, 72, 96, 101, 120, 128, 200}):
        for Ch in CHANNELS:
            for B in (1, 4, 256):
                for bd in (8, 5, 12):
                    p = _cl(D, Ch, B, blockdim=bd)
                    if Ch == 1:
                        continue
                    nsz = -(-D // 8)
                    assert 1 <= p["nw"] <= 8 and p["nzc"] * p["nw"] >= nsz > (p["nzc"] - 1) * p["nw"], (D, Ch, B, p)
                    assert p["nsx"] == -(-D // 2) and p["nsy"] == -(-D // 4)
                    assert p["route"] in (0, 1) and p["ct"] in (4, 8, 16, 32)
                    assert p["nfull"] * p["ct"] + p["ct_rem"] >= Ch if p["ct_rem"] else p["ncc"] * p["ct"] >= Ch
                    if p["route"] == 1:
                        assert p["nzc"] == 1
    # rows longer than 8 sub-tiles: as few, equally long chunks as 8 waves allow
    assert (_cl(72, 32, 16)["nw"], _cl(72, 32, 16)["nzc"]) == (5, 2)
    assert (_cl(96, 32, 16)["nw"], _cl(96, 32, 16)["nzc"]) == (6, 2)
    assert (_cl(128, 32, 4)["nw"], _cl(128, 32, 4)["nzc"]) == (8, 2)
    assert (_cl(64, 32, 256)["nw"], _cl(64, 32, 256)["nzc"]) == (8, 1)


def test_one_channel_is_the_contiguous_plan():
    for D in (16, 48, 49, 63, 64, 72, 96, 128):
        for B in (1, 4, 256):
            for al in (1, 0):
                for mode in (0, 1, 2):
                    q = (D, 8, 32, mode, 0, B, 1, al, B * 500, 500)
                    assert _raw(q, 0, NDHWC) == _raw(q), q
                    assert _raw(q, _lib.MVX_GRID_BF16, NDHWC) == _raw(q, _lib.MVX_GRID_BF16), q


def test_layout_zero_is_exactly_mvx_plan_call_grid():
    for D in (16, 49, 64, 72, 128):
        for Ch in CHANNELS:
            for B in (1, 4, 256):
                for prec in (32, 64):
                    q = (D, 8, prec, 0, 0, B, Ch, 1, B * 500, 500)
                    assert _raw(q, 0, NCDHW) == _raw(q), q


def test_layout_query_validation():
    q32 = (64, 8, 32, 0, 0, 256, 32, 1, 256 * 4000, 4000)
    q64 = (64, 8, 64, 0, 0, 256, 32, 1, 256 * 4000, 4000)
    assert _raw(q64, 0, NDHWC)[0] == MVX_ERR_INVALID
    assert _raw(q64, 0, NCDHW)[0] == 0
    for layout in (2, -1, 7):
        assert _raw(q32, 0, layout)[0] == MVX_ERR_INVALID
    assert _raw(q32, 5, NDHWC)[0] == MVX_ERR_INVALID  # unknown grid_type


def test_mvx_plan_call_rows_are_unchanged():
    """A sample of the rows tests/test_plan.py pins, asked through the unchanged entry point."""
    def plan(D, Ch, B=1, atoms=None, **kw):
        if atoms is None:
            atoms = int(round(4000 * ((D - 1) / 63.0) ** 3))
        return _lib.plan_call(D, Ch, B, total_atoms=B * atoms, max_atoms=atoms, **kw)

    p = plan(64, 32, 256, 4000)
    assert (p["route"], p["nsx"], p["nsy"], p["nzc"], p["nw"], p["ct"], p["ncc"], p["nchunk"], p["pace"]) == (0, 32, 16, 1, 8, 32, 1, 1, 2)
    assert p["weights_in_place"] == 1 and p["vec_store"] == 1 and p["lane_range"] == 0 and p["ct_rem"] == 0
    assert plan(64, 32, 1, 4000)["route"] == 1
    p = plan(128, 32, 1, 10000, radii_type="atom-wise")
    assert (p["route"], p["nw"], p["nzc"], p["nsx"], p["nsy"], p["pace"]) == (0, 8, 2, 64, 32, 0)
    p = plan(64, 16, 128, 50)
    assert (p["route"], p["ct"], p["pace"]) == (0, 16, 2)
    p = plan(64, 40, 1, 4000, radii_type="channel-wise")
    assert (p["route"], p["grouped"], p["ct"], p["ncc"], p["weights_in_place"], p["ct_rem"]) == (0, 1, 32, 2, 1, 0)
    assert plan(72, 32, 16)["nw"] == 9 and plan(49, 32, 64)["vec_store"] == 0 and plan(49, 32, 64)["xcd_ranges"] == 1
