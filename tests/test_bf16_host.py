"""bfloat16 grids without a GPU: the C ABI addition (mvx_config.grid_type, mvx_plan_call_grid), the checks mvx_create makes
before it looks for a device, and the Python option (grid_dtype) that rides on them."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, VERSION, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_as_c99_with_grid_type_in_the_old_reserved_slot(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "abi.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "mvx.h"\n'
        "int main(void) {\n"
        "  mvx_config c = {0};\n"
        "  c.grid_type = MVX_GRID_BF16;\n"
        '  printf("%zu %zu %zu %d %d %d\\n", sizeof(mvx_config), offsetof(mvx_config, grid_type), sizeof(c.grid_type),\n'
        "         (int)MVX_GRID_REAL, (int)c.grid_type, MVX_VERSION);\n"
        "  int (*f)(const mvx_plan_query *, int32_t, mvx_plan *) = mvx_plan_call_grid;\n"
        "  return f ? 0 : 1;\n}\n")
    obj = tmp_path / "abi.o"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    exe = tmp_path / "abi"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, str(obj), "-L", libdir, "-lmvx_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.check_output([str(exe)]).decode().split()
    assert [int(v) for v in out] == [40, 36, 4, 0, 1, VERSION]
    assert _lib.MvxConfig.grid_type.offset == 36 and C.sizeof(_lib.MvxConfig) == 40


def _create(precision, grid_type, dimension=32):
    cfg = _lib.MvxConfig(0.5, 0.5, dimension, 8, _lib.MVX_GAUSSIAN, 0, precision, grid_type)
    h = _lib.Handle()
    lib = _lib.load()
    rc, msg = call(lib.mvx_create, C.byref(cfg), C.byref(h))
    if rc == 0:
        lib.mvx_destroy(h)
    return rc, msg


@pytest.mark.parametrize("precision, grid_type", [(64, 1), (32, 2), (32, -1), (0, 7)])
def test_create_rejects_bad_grid_types_before_looking_for_a_device(precision, grid_type):
    rc, msg = _create(precision, grid_type)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert "grid" in msg


def test_create_rejects_bf16_with_precision_64_even_with_valid_geometry():
    rc, msg = _create(64, _lib.MVX_GRID_BF16, dimension=64)
    assert rc == MVX_ERR_INVALID and "precision" in msg


@pytest.mark.parametrize("kw", [dict(grid_dtype="bfloat16", precision=64), dict(grid_dtype="bfloat16", output="numpy"),
                                dict(grid_dtype="float16"), dict(grid_dtype="float32", precision=64)])
def test_factory_rejects_impossible_grid_dtypes_without_a_device(kw):
    import molvoxel_amd

    with pytest.raises(ValueError, match="grid_dtype"):
        molvoxel_amd.create_voxelizer(0.5, 32, "scalar", "gaussian", "hip", **kw)


def test_factory_rejects_torch_bfloat16_with_precision_64():
    import torch

    import molvoxel_amd

    with pytest.raises(ValueError, match="precision"):
        molvoxel_amd.create_voxelizer(0.5, 32, grid_dtype=torch.bfloat16, precision=64)


def test_grid_dtype_values_are_parsed_without_a_device():
    import torch

    from molvoxel_amd.voxelizer.hip import Voxelizer

    for v in ("bfloat16", torch.bfloat16):
        assert Voxelizer._is_bf16_grid(v, 32, "torch") is True
    for v in (None, "float32", torch.float32):
        assert Voxelizer._is_bf16_grid(v, 32, "torch") is False
    assert Voxelizer._is_bf16_grid(None, 64, "numpy") is False


# ---- mvx_plan_call_grid ------------------------------------------------------------------------------------------------------
def _raw(query_args, grid_type=None):
    q = _lib.MvxPlanQuery(*query_args)
    p = _lib.MvxPlan()
    lib = _lib.load()
    rc = lib.mvx_plan_call(C.byref(q), C.byref(p)) if grid_type is None else lib.mvx_plan_call_grid(C.byref(q), grid_type, C.byref(p))
    return rc, bytes(p)


def _queries():
    """The shapes tests/test_plan.py pins, and their neighbours: dimensions of every write-out path, channel counts of every
    chunking, batch sizes of every route / pacing / chunking regime."""
    for D, Ch, B, mode, radii, prec, bd, al in itertools.product(
            (8, 24, 32, 40, 48, 49, 50, 56, 60, 63, 64, 65, 68, 72, 96, 101, 120, 128), (1, 4, 5, 16, 32, 33, 40, 64, 65),
            (1, 2, 4, 64, 128, 256, 1024), (0, 1, 2), (0, 1, 2), (32, 64), (8, 5), (1, 0)):
        if (D + Ch + B) % 3:  # (a third of the product: every value of every axis still occurs)
            continue
        atoms = max(1, int(round(4000 * ((D - 1) / 63.0) ** 3)))
        yield (D, bd, prec, mode, radii, B, Ch, al, B * atoms, atoms)
    for atoms in (8, 4000, 8000, 24000, 48000):  # route rows
        yield (64, 8, 32, 0, 0, 1, 32, 1, atoms, atoms)


def test_grid_type_zero_is_exactly_mvx_plan_call():
    n = 0
    for q in _queries():
        a, b = _raw(q), _raw(q, 0)
        assert a == b, q
        n += 1
    assert n > 5000


def test_bf16_plans_keep_the_float32_decisions():
    for q in _queries():
        if q[2] == 64:
            continue
        assert _raw(q, _lib.MVX_GRID_BF16) == _raw(q), q


def test_bf16_query_validation():
    q = (64, 8, 64, 0, 0, 256, 32, 1, 256 * 4000, 4000)
    assert _raw(q, _lib.MVX_GRID_BF16)[0] == MVX_ERR_INVALID  # precision 64
    for gt in (2, -1, 100):
        assert _raw((64, 8, 32, 0, 0, 256, 32, 1, 256 * 4000, 4000), gt)[0] == MVX_ERR_INVALID
    with pytest.raises(RuntimeError):
        _lib.plan_call(64, 32, 256, 256 * 4000, precision=64, grid_type=_lib.MVX_GRID_BF16)


def _bf16(D, Ch, B=1, atoms=None, **kw):
    if atoms is None:
        atoms = int(round(4000 * ((D - 1) / 63.0) ** 3))
    return _lib.plan_call(D, Ch, B, total_atoms=B * atoms, max_atoms=atoms, grid_type=_lib.MVX_GRID_BF16, **kw)


def test_headline_bf16_keeps_route_slab_plan_and_chunking():
    p = _bf16(64, 32, 256, 4000)
    assert (p["route"], p["nsx"], p["nsy"], p["nzc"], p["nw"], p["ct"], p["ncc"], p["nchunk"], p["pace"]) == (0, 32, 16, 1, 8, 32, 1, 1, 2)
    assert p["vec_store"] == 1 and p["weights_in_place"] == 1 and p["lane_range"] == 0
    assert _bf16(64, 32, 1, 4000)["route"] == 1  # one pocket per call: one launch


def test_bf16_store_form_rows():
    """Form (a): the float32 slot map, four voxels (8 bytes) per store - rows of whole groups of four take vector stores,
    D % 8 == 4 included; other rows, and grids that are not 8-byte aligned (out_aligned16 = 0), go run by run."""
    for D in (48, 60, 64, 68, 76, 96, 100, 120, 128):
        assert _bf16(D, 8)["vec_store"] == 1, D
        assert _bf16(D, 8, out_aligned16=False)["vec_store"] == 0, D
    for D in (49, 50, 63, 65, 101):
        p = _bf16(D, 8)
        assert p["vec_store"] == 0, D
    assert _bf16(49, 32)["xcd_ranges"] == 1
