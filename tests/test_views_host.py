"""Views of a shared cloud without a GPU: the C ABI entries (mvx_select_views, mvx_forward_views), the checks they make before
they touch a device, the ctypes prototypes against the header, the numpy restatement of the selection on the cull face, the
public signatures, and the new kernels' register use read from mvx_views.o."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import views_reference as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MVX_ERR_INVALID = -1
P = 16  # any non-null pointer: nothing is dereferenced before the checks are through


def _select(handle=None, coords=P, types=None, radii=None, rs=1.0, radii_type=0, mode=0, N=3, C_=4, xforms=P, B=1, index=None,
            cap=0, offsets=P, in_kind=1):
    lib = _lib.load()
    rc = lib.mvx_select_views(handle, coords, types, radii, rs, radii_type, mode, N, C_, xforms, B, index, cap, offsets, in_kind, None)
    return rc, (lib.mvx_last_error() or b"").decode()


def _forward(handle=None, mode=0, coords=P, channels=P, radii=None, rs=1.0, radii_type=0, N=3, C_=4, xforms=P, B=1, out=P,
             in_kind=1, out_kind=1):
    lib = _lib.load()
    rc = lib.mvx_forward_views(handle, mode, coords, channels, radii, rs, radii_type, N, C_, xforms, B, out, in_kind, out_kind, None)
    return rc, (lib.mvx_last_error() or b"").decode()


SHARED = [
    (dict(mode=3), "bad mode"),
    (dict(mode=-1), "bad mode"),
    (dict(radii_type=3), "radii_type"),
    (dict(radii_type=-1), "radii_type"),
    (dict(in_kind=2), "memory kind"),
    (dict(B=-1), "B and N"),
    (dict(N=-1), "B and N"),
    (dict(C_=0), "C > 0"),
    (dict(C_=-3), "C > 0"),
    (dict(xforms=None), "xforms"),
    (dict(mode=2, C_=1, radii_type=2, radii=P), "Channel-Wise"),
    (dict(mode=2, C_=3), "one channel"),
    (dict(coords=None), "coords"),
    (dict(radii_type=1, radii=None), "radii array"),
    (dict(radii_type=2, radii=None), "radii array"),
    (dict(), "null handle"),
]


@pytest.mark.parametrize("kw, words", SHARED + [
    (dict(mode=1, types=None), "types"),
    (dict(offsets=None), "offsets_out_host"),
    (dict(index=None, cap=5), "index_out"),
    (dict(cap=-1), "index_out"),
])
def test_select_views_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _select(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


@pytest.mark.parametrize("kw, words", SHARED + [
    (dict(mode=1, channels=None), "types"),
    (dict(mode=0, channels=None), "channels"),
    (dict(out=None), "out must not be null"),
    (dict(out_kind=5), "memory kind"),
])
def test_forward_views_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _forward(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_library_exports_the_views_entries():
    lib = _lib.load()
    for name in ("mvx_select_views", "mvx_forward_views"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert lib.mvx_version() == 140  # (additive entries)


_CTYPE = {"mvx_handle *": C.c_void_p, "int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "mvx.h")).read()
    m = re.search(r"\bint " + name + r"\(([^;]*?)\);", text, re.S)
    assert m, name
    out = []
    for arg in m.group(1).replace("\n", " ").split(","):
        arg = arg.strip()
        if "*" in arg:
            out.append(C.c_void_p)
        else:
            out.append(_CTYPE[arg.rsplit(" ", 1)[0].strip()])
    return out


@pytest.mark.parametrize("name", ["mvx_select_views", "mvx_forward_views"])
def test_ctypes_prototypes_match_the_header(name):
    res, args = _lib.SIGNATURES[name]
    assert res is C.c_int
    assert args == _header_args(name)


def test_header_compiles_as_c99_with_the_views_prototypes(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "views.c"
    src.write_text(
        '#include <stdio.h>\n#include "mvx.h"\n'
        "int main(void) {\n"
        "  int64_t off[2];\n"
        "  mvx_xform xf = {{0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0}, 0, NULL};\n"
        "  double xyz[3] = {0, 0, 0};\n"
        "  float grid[8];\n"
        "  int a = mvx_select_views(NULL, xyz, NULL, NULL, 1.0, 0, 2, 1, 1, &xf, 1, NULL, 0, off, MVX_HOST, NULL);\n"
        "  int b = mvx_forward_views(NULL, 2, xyz, NULL, NULL, 1.0, 0, 1, 1, &xf, 1, grid, MVX_HOST, MVX_HOST, NULL);\n"
        '  printf("%d %d\\n", a, b);\n'
        "  return 0;\n}\n")
    exe = tmp_path / "views"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lmvx_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == [str(MVX_ERR_INVALID)] * 2


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_reference_selection_on_the_cull_face(axis):
    # res 0.5, D 16: half = 3.75; r = 1.5: the face lies at 5.25, all exactly representable
    xyz, expect = vr.face_cloud(0.5, 16, 1.5, axis)
    (kept,) = vr.select(xyz, np.zeros((1, 3)), 1.5, 0.5, 16)
    assert np.array_equal(kept, np.flatnonzero(expect))
    # atom-wise radii take the other form of the test (p + r > lb, p - r < ub): the same decisions at representable values
    (kept,) = vr.select(xyz, np.zeros((1, 3)), np.full(6, 1.5), 0.5, 16)
    assert np.array_equal(kept, np.flatnonzero(expect))
    # the loose bound counts every atom of the face cloud
    assert vr.count_within(xyz, np.zeros((1, 3)), 1.5, 0.5, 16, 0.5) == [6]


def test_reference_cull_radius():
    r = np.array([1.0, 2.5, 1.5], np.float32)
    assert vr.cull_radius(1.25, "scalar") == 1.25
    assert np.array_equal(vr.cull_radius(r, "atom-wise"), r.astype(np.float64))
    assert vr.cull_radius(r, "channel-wise", features_mode=True) == 2.5
    assert np.array_equal(vr.cull_radius(r, "channel-wise", types=np.array([2, 0, 1, 1])), [1.5, 1.0, 2.5, 2.5])


def test_voxelizer_has_the_views_methods():
    import inspect

    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    sel = inspect.signature(Voxelizer.select_views).parameters
    fwd = inspect.signature(Voxelizer.forward_views).parameters
    assert list(sel) == ["self", "coords", "centers", "channels", "radii", "random_translation", "random_rotation"]
    assert sel["random_rotation"].default is False
    bat = inspect.signature(Voxelizer.forward_batch).parameters  # (unchanged by the shared helper)
    assert list(bat) == ["self", "coords", "offsets", "centers", "channels", "radii", "num_channels", "out_grid",
                         "random_translation", "random_rotation"]
    assert list(fwd) == ["self", "coords", "centers", "channels", "radii", "num_channels", "out_grid", "random_translation",
                         "random_rotation"]
    assert list(fwd)[:7] == ["self", "coords", "centers", "channels", "radii", "num_channels", "out_grid"]
    assert "overlap_prepass" in Voxelizer.forward_views.__doc__


def test_view_kernels_use_no_scratch():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_views.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_views.o not built")
    res = regs.kernel_resources(obj)
    names = {k.split("<")[0] for k in res}
    assert {"view_count_kernel", "view_scan_kernel", "view_fill_kernel", "view_gather_kernel", "view_rmax_kernel"} <= names, sorted(res)
    for k, r in res.items():
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (k, r)
        if "count" in k or "fill" in k:  # the B x N kernels: at least three waves per SIMD (512 VGPRs / 3 = 170, granule 8)
            assert r["vgpr"] <= 168, (k, r)
