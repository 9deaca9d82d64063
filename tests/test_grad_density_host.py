"""Sigma and scalar-radius gradients without a GPU: the C ABI entry (mvx_backward_density_batch), the checks it makes before it
touches a device, the `sigma_grad` option's validation and the reduction kernels' register use read from mvx_grad_density.o."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, call

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "molvoxel_amd", "csrc")


def test_the_density_entry_has_eighteen_arguments():
    assert len(_lib.SIGNATURES["mvx_backward_density_batch"][1]) == 18


def test_header_compiles_as_c99_with_the_density_prototype(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "bwdd.c"
    src.write_text(
        '#include <stdio.h>\n#include "mvx.h"\n'
        "int main(void) {\n"
        "  int (*f)(mvx_handle *, int32_t, const double *, const void *, const mvx_real *, double, int32_t, const int64_t *,\n"
        "           const mvx_xform *, int32_t, int32_t, const void *, double *, mvx_real *, double *, double *, double *, void *) =\n"
        "      mvx_backward_density_batch;\n"
        "  int64_t off[2] = {0, 1};\n"
        "  double g[3], gs[1];\n"
        "  int rc = mvx_backward_density_batch(NULL, 0, NULL, NULL, NULL, 1.0, 0, off, NULL, 1, 4, NULL, g, NULL, NULL, gs, gs, NULL);\n"
        '  printf("%d\\n", rc);\n'
        "  return f ? 0 : 1;\n}\n")
    obj = tmp_path / "bwdd.o"
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), "-c", str(src),
                           "-o", str(obj)])
    exe = tmp_path / "bwdd"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, str(obj), "-L", libdir, "-lmvx_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == [str(MVX_ERR_INVALID)]


def _call(mode=0, B=1, C_=4, offsets=(0, 3), grad_coords=None, grad_features=None, grad_radii=None, grad_sigma=16,
          grad_rscalar=None, radii_type=0, handle=None):
    off = np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_backward_density_batch, handle, mode, 16, 16, 16, 1.0, radii_type, off.ctypes.data, None, B, C_, 16,
                grad_coords, grad_features, grad_radii, grad_sigma, grad_rscalar, None)


@pytest.mark.parametrize("kw, words", [
    (dict(grad_sigma=None), "all null"),
    (dict(grad_sigma=None, grad_coords=16, grad_features=16), "all null"),
    (dict(grad_rscalar=16, radii_type=1), "grad_radius_scalar"),
    (dict(grad_rscalar=16, radii_type=2, grad_sigma=None), "grad_radius_scalar"),
    (dict(grad_radii=16, radii_type=0), "grad_radii"),
    (dict(grad_radii=16, radii_type=0, grad_sigma=None, mode=1), "grad_radii"),
    (dict(radii_type=2, mode=2, C_=1), "single mode"),
    (dict(radii_type=2, mode=2, C_=1, grad_radii=16, grad_sigma=None), "single mode"),
    (dict(radii_type=7), "radii_type"),
    (dict(mode=3), "mode"),
    (dict(mode=-1), "mode"),
    (dict(mode=1, grad_features=16), "grad_features"),
    (dict(C_=0), "C must be > 0"),
    (dict(mode=2, C_=3), "single mode"),
    (dict(B=-1), "B must be"),
    (dict(B=2, offsets=(0, 3, 2)), "non-decreasing"),
    (dict(B=1, offsets=(1, 3)), "offsets[0]"),
    (dict(), "null handle"),
    (dict(grad_rscalar=16, grad_sigma=None), "null handle"),
    (dict(radii_type=1, grad_radii=16), "null handle"),
])
def test_density_entry_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _call(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_sigma_grad_needs_differentiable():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    with pytest.raises(ValueError, match="sigma_grad=True needs differentiable=True"):
        Voxelizer(0.5, 16, sigma_grad=True)
    with pytest.raises(ValueError, match="differentiable"):
        Voxelizer(0.5, 16, "atom-wise", output="numpy", sigma_grad=True)


def test_sigma_grad_is_an_option_that_defaults_off():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    assert inspect.signature(Voxelizer.__init__).parameters["sigma_grad"].default is False
    assert callable(getattr(Voxelizer, "set_sigma")) and isinstance(Voxelizer.sigma_tensor, property)


def test_a_sigma_tensor_without_sigma_grad_is_rejected_by_name():
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    with pytest.raises(ValueError, match="sigma_grad=True"):
        Voxelizer(0.5, 16, sigma=torch.tensor(0.7))


@pytest.fixture(scope="module")
def density_res():
    from tools import regs

    obj = os.path.join(CSRC, "mvx_grad_density.o")
    assert os.path.exists(obj), "mvx_grad_density.o not built"
    return regs.kernel_resources(obj)


def test_density_object_holds_its_reduction_kernels(density_res):
    # the sum over the atoms (float and double radii), the finish of one sum, the channel-wise finish (float and double kc);
    # no walk of its own: the walk is grad_radii_kernel's, whose names and count tests/test_grad_radii_host.py pins
    assert sorted(density_res) == ["density_chan_finish_kernel<double>", "density_chan_finish_kernel<float>",
                                   "density_finish_kernel", "density_sum_kernel<double>", "density_sum_kernel<float>"]
    assert not any("grad_kernel" in k or "grad_radii_kernel" in k for k in density_res)


def test_density_kernels_use_no_scratch_and_do_not_spill(density_res):
    # float32 and bfloat16 grids run the <float> kernels (bfloat16 grids keep float radii and coefficients); the double ones too
    for k, r in density_res.items():
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (k, r)


def test_radius_and_gradient_objects_keep_their_kernels():
    """The walk is shared, not copied: mvx_grad.o and mvx_grad_radii.o hold what they held."""
    from tools import regs

    for name, sub, count in (("mvx_grad.o", "grad_kernel", 18), ("mvx_grad_radii.o", "grad_radii_kernel", 9)):
        res = regs.kernel_resources(os.path.join(CSRC, name))
        assert len([k for k in res if sub in k]) == count, sorted(res)
        assert not any("density" in k for k in res)
