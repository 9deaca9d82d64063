"""Radius gradients without a GPU: the C ABI entry (mvx_backward_radii_batch), the checks it makes before it touches a device,
the `radii_grad` option's validation and the radius kernels' register use read from mvx_grad_radii.o."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "molvoxel_amd", "csrc")


def test_header_compiles_as_c99_with_the_radii_prototype(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "bwdr.c"
    src.write_text(
        '#include <stdio.h>\n#include "mvx.h"\n'
        "int main(void) {\n"
        "  int (*f)(mvx_handle *, int32_t, const double *, const void *, const mvx_real *, double, int32_t, const int64_t *,\n"
        "           const mvx_xform *, int32_t, int32_t, const void *, double *, mvx_real *, double *, void *) =\n"
        "      mvx_backward_radii_batch;\n"
        "  int64_t off[2] = {0, 1};\n"
        "  double g[3], gr[1];\n"
        "  int rc = mvx_backward_radii_batch(NULL, 0, NULL, NULL, NULL, 1.0, 1, off, NULL, 1, 4, NULL, g, NULL, gr, NULL);\n"
        '  printf("%d\\n", rc);\n'
        "  return f ? 0 : 1;\n}\n")
    obj = tmp_path / "bwdr.o"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    exe = tmp_path / "bwdr"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, str(obj), "-L", libdir, "-lmvx_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == [str(MVX_ERR_INVALID)]


def _call(mode=0, B=1, C_=4, offsets=(0, 3), grad_coords=None, grad_features=None, grad_radii=16, radii_type=1, handle=None):
    off = np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_backward_radii_batch, handle, mode, 16, 16, 16, 1.0, radii_type, off.ctypes.data, None, B, C_, 16,
                grad_coords, grad_features, grad_radii, None)


@pytest.mark.parametrize("kw, words", [
    (dict(grad_radii=None), "grad_radii"),
    (dict(grad_radii=None, grad_coords=16), "grad_radii"),
    (dict(radii_type=0), "radii_type"),
    (dict(radii_type=0, mode=1), "radii_type"),
    (dict(radii_type=2, mode=2, C_=1), "radii_type"),
    (dict(radii_type=7), "radii_type"),
    (dict(mode=3), "mode"),
    (dict(mode=1, grad_features=16), "grad_features"),
    (dict(C_=0), "C must be > 0"),
    (dict(B=2, offsets=(0, 3, 2)), "non-decreasing"),
    (dict(), "null handle"),
])
def test_radii_entry_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _call(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_radii_grad_needs_differentiable():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    with pytest.raises(ValueError, match="differentiable"):
        Voxelizer(0.5, 16, "atom-wise", radii_grad=True)
    with pytest.raises(ValueError, match="differentiable"):
        Voxelizer(0.5, 16, "atom-wise", output="numpy", radii_grad=True)


def test_radii_grad_is_an_option_that_defaults_off():
    import inspect

    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    assert inspect.signature(Voxelizer.__init__).parameters["radii_grad"].default is False


@pytest.fixture(scope="module")
def radii_res():
    from tools import regs

    obj = os.path.join(CSRC, "mvx_grad_radii.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_grad_radii.o not built")
    return {k: v for k, v in regs.kernel_resources(obj).items() if "grad_radii_kernel" in k}


def test_radius_kernels_cover_every_backward_instantiation(radii_res):
    # 3 grid types x (features: one radius per atom, channel-wise; types / single), Gaussian only (binary radii: zeros)
    assert len(radii_res) == 9, sorted(radii_res)
    assert not any("grad_kernel" in k for k in radii_res)


def test_float_and_bfloat16_radius_kernels_do_not_spill(radii_res):
    hot = [k for k in radii_res if "double" not in k]
    assert len(hot) == 6, sorted(radii_res)
    for k in hot:
        assert radii_res[k]["scratch"] == 0 and radii_res[k]["vspill"] == 0, (k, radii_res[k])


def test_grad_object_keeps_its_eighteen_gradient_kernels():
    from tools import regs

    obj = os.path.join(CSRC, "mvx_grad.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_grad.o not built")
    res = regs.kernel_resources(obj)
    assert len([k for k in res if "grad_kernel" in k]) == 18, sorted(res)
    assert not any("grad_radii" in k for k in res)
