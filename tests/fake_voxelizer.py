"""A hip Voxelizer without a handle, for the host tests: every attribute `Voxelizer.__init__` sets except the handle, so the
checks that fire before the library is needed (and, with a stub in place of `_lib`, the host-array entries) run without a
device. `_lib` is None: a call that does reach the library fails in Python instead of handing a null handle to C."""
import ctypes as C

import numpy as np


def fake(radii_type="scalar", dimension=16, **attrs):
    """`attrs` override what the constructor would have set (`precision=64`, `output="numpy"`, `differentiable=True`, ...)."""
    import torch

    from molvoxel_amd.voxelizer.contract import BaseVoxelizer
    from molvoxel_amd.voxelizer.hip import _lib
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    v = Voxelizer.__new__(Voxelizer)
    v._handle = None
    v._sigma_src = v._rscalar_src = None
    BaseVoxelizer.__init__(v, 0.5, dimension, radii_type, "gaussian")
    precision = attrs.get("precision", 32)
    blockdim = attrs.get("blockdim", 8)
    tfp = torch.float32 if precision == 32 else torch.float64
    xf = _lib.MvxXform()
    init = dict(differentiable=False, field_grad=False, radii_grad=False, sigma_grad=False, _bf16=False, _cl=False,
                precision=precision, fp=np.float32 if precision == 32 else np.float64, _tfp=tfp, _gdt=tfp, blockdim=blockdim,
                num_blocks=-(-dimension // blockdim), output="torch", _lib=None, _device_index=0, _types_cache=None,
                _types_i32=None, _types_fresh=False, _xf=xf, _xf_addr=C.addressof(xf), _has_torch_cuda=False,
                overlap_prepass=False, _sum_parts=1, _views_total=0)
    for k, val in dict(init, **attrs).items():
        setattr(v, k, val)
    return v
