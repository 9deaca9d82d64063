"""The backward pass without a GPU: the C ABI entry (mvx_backward_batch), the checks it makes before it touches a device, the
`differentiable` option's validation and the gradient kernels' register use read from mvx_grad.o."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, VERSION, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_compiles_as_c99_with_the_backward_prototype(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "bwd.c"
    src.write_text(
        '#include <stdio.h>\n#include "mvx.h"\n'
        "int main(void) {\n"
        "  int (*f)(mvx_handle *, int32_t, const double *, const void *, const mvx_real *, double, int32_t, const int64_t *,\n"
        "           const mvx_xform *, int32_t, int32_t, const void *, double *, mvx_real *, void *) = mvx_backward_batch;\n"
        "  int64_t off[2] = {0, 1};\n"
        "  double g[3];\n"
        "  int rc = mvx_backward_batch(NULL, 0, NULL, NULL, NULL, 1.0, 0, off, NULL, 1, 4, NULL, g, NULL, NULL);\n"
        '  printf("%d %d\\n", rc, MVX_VERSION);\n'
        "  return f ? 0 : 1;\n}\n")
    obj = tmp_path / "bwd.o"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    exe = tmp_path / "bwd"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, str(obj), "-L", libdir, "-lmvx_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == [str(MVX_ERR_INVALID), str(VERSION)]


def _call(mode=0, B=1, C_=4, offsets=(0, 3), grad_coords=1, grad_features=None, radii_type=0, handle=None):
    off = np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_backward_batch, handle, mode, 16, 16, None, 1.0, radii_type, off.ctypes.data, None, B, C_, 16,
                grad_coords, grad_features, None)


@pytest.mark.parametrize("kw, words", [
    (dict(mode=3), "mode"),
    (dict(mode=-1), "mode"),
    (dict(mode=1, grad_features=16), "grad_features"),
    (dict(mode=2, C_=1, grad_features=16), "grad_features"),
    (dict(C_=0), "C must be > 0"),
    (dict(C_=-5), "C must be > 0"),
    (dict(grad_coords=None, grad_features=None), "both null"),
    (dict(B=2, offsets=(0, 3, 2)), "non-decreasing"),
    (dict(B=3, offsets=(0, 1, 0, 4)), "non-decreasing"),
    (dict(offsets=(1, 3)), "offsets[0]"),
    (dict(mode=2, C_=3), "C = 1"),
    (dict(radii_type=7), "radii_type"),
    (dict(), "null handle"),
])
def test_backward_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _call(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_differentiable_needs_torch_output():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    with pytest.raises(ValueError, match="differentiable"):
        Voxelizer(0.5, 16, output="numpy", differentiable=True)


def test_differentiable_is_a_create_voxelizer_option():
    import inspect

    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    p = inspect.signature(Voxelizer.__init__).parameters["differentiable"]
    assert p.default is False


@pytest.fixture(scope="module")
def grad_res():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_grad.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_grad.o not built")
    return {k: v for k, v in regs.kernel_resources(obj).items() if "grad_kernel" in k}


def test_float32_gaussian_feature_gradient_kernel_has_no_scratch(grad_res):
    # the headline shape (C = 32, features, Gaussian, one radius per atom): float32 and bfloat16 grids
    hot = [k for k in grad_res if ("<float, 0, true, false>" in k or "<__bf16, 0, true, false>" in k)]
    assert len(hot) == 2, sorted(grad_res)
    for k in hot:
        assert grad_res[k]["scratch"] == 0 and grad_res[k]["vspill"] == 0, (k, grad_res[k])


def test_gradient_kernels_of_float_grids_do_not_spill(grad_res):
    assert len(grad_res) == 18, sorted(grad_res)  # 3 grid types x (features: 2 x 2, types / single: 2)
    for k, r in grad_res.items():
        if "double" not in k:
            assert r["scratch"] == 0 and r["vspill"] == 0, (k, r)
