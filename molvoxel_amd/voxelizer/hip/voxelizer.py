"""`library='hip'` backend: the reference's Voxelizer interface on hand-written MI355X kernels.

Host layer only: argument checks (same AssertionError messages as the reference numpy backend,
molvoxel/voxelizer/numpy/voxelizer.py:171-192, 317-342, 438-455), dtype fixes (:125-130, :268-271),
channel-count inference (:275-278), RNG draws for the random transform in the reference's order
(numpy/transform.py:63-80) and the call through the C ABI (include/mvx.h). All arithmetic of the
hot path — centring, rigid transform, culls, distances, densities, accumulation — runs on the GPU.
There is no CPU fallback: construction fails without the shared library or without a HIP device.

Array arguments may be numpy arrays (host: staged through pinned memory by the library) or torch
CUDA tensors on this voxelizer's device (zero-copy via data_ptr on the current torch stream).
Grids this backend allocates are torch CUDA tensors by default (`output="torch"`), so results stay
in HBM; pass `output="numpy"` (or a numpy `out_grid`) for host arrays. `grid_dtype="bfloat16"` makes the
kernels write bfloat16 grids directly: the float32 grid rounded to nearest even as it is stored, bit for bit
what `.to(torch.bfloat16)` of the float32 grid gives, at half the bytes. `differentiable=True` makes grids computed from device
tensors that require grad (`coords`, `features`, `center`) part of the autograd graph: the backward pass runs on the GPU
(mvx_backward_batch) and returns gradients with respect to those tensors. `radii_grad=True` (with `differentiable=True`)
adds a radii tensor that requires grad to them (mvx_backward_radii_batch, atom-wise or channel-wise radii; on a scalar-radii
voxelizer a one-element radii tensor, mvx_backward_density_batch). `grid_layout="channels_last"` makes the kernels write
channels-last (NDHWC, `torch.channels_last_3d`) grids directly: same logical shape, same bits, the strides 3D convolutions want
(faster than converting afterwards with bfloat16 grids; experimental with float32 grids: DESIGN.md section 14).
`sigma_grad=True` (with `differentiable=True`) lets `sigma=`
/ `set_sigma()` take a one-element tensor that gets dL/dsigma (mvx_backward_density_batch).
`forward_posed_batch` / `forward_posed_views` / `select_posed_views` take explicit rigid poses p = q (x - c) conj(q) + t instead of
drawing random transforms; on a differentiable voxelizer the poses get their gradients (mvx_pose_grad_batch).
`forward_sum` / `forward_posed_sum` write ONE float32 grid, the (weighted) sum of a batch's grids, without the B grids
(mvx_forward_sum_batch); `field_grad=True` (with `differentiable=True`) lets `score_batch` / `score_posed_batch` take a shared
field that requires grad: dL/dfield is such a weighted sum.
`forward_views_sum` / `forward_posed_views_sum` are that one grid for B views of ONE shared cloud (mvx_forward_views_sum);
`set_sum_parts(K)` cuts every summed call into K parts with a partial grid each (mvx_set_sum_parts; other bits than K = 1).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ..contract import BaseVoxelizer
from . import _lib
from .transform import RandomTransform, draw_forward_transform

try:  # torch is plumbing (device memory + streams); the library also works without it
    import torch
except Exception:  # pragma: no cover
    torch = None


def _is_torch(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor)


try:  # the raw stream handle without building a torch.cuda.Stream object per call (~1.5 us -> ~0.2 us)
    _raw_stream = torch._C._cuda_getCurrentRawStream
except Exception:  # pragma: no cover
    _raw_stream = None


def _np_isscalar(x) -> bool:
    return np.isscalar(x)


class Voxelizer(BaseVoxelizer):
    LIB = "HIP"
    transform_class = RandomTransform

    def __init__(
        self,
        resolution: float = 0.5,
        dimension: int = 64,
        radii_type: str = "scalar",
        density_type: str = "gaussian",
        precision: int = 32,
        blockdim: int | None = None,
        device=None,
        output: str = "torch",
        overlap_prepass: bool = False,
        grid_dtype=None,
        differentiable: bool = False,
        radii_grad: bool = False,
        sigma_grad: bool = False,
        grid_layout=None,
        field_grad: bool = False,
        **kwargs,
    ):
        # sigma as a tensor (sigma_grad): kept as `sigma_tensor`; `_sigma` stays the python float the base class stores
        self._sigma_src = None  # (tensor, its _version when read, the value read)
        self._rscalar_src = None  # the same for a scalar-radius tensor (radii_grad on a scalar-radii voxelizer)
        sigma_src = None
        if _is_torch(kwargs.get("sigma")):
            if not sigma_grad:
                raise ValueError("sigma is a tensor: create the voxelizer with sigma_grad=True (and differentiable=True) to learn "
                                 "sigma, or pass a python float")
            sigma_src = self._read_scalar_tensor(kwargs["sigma"], "sigma")
            kwargs = dict(kwargs, sigma=sigma_src[2])
        super().__init__(resolution, dimension, radii_type, density_type, **kwargs)
        assert precision in [32, 64]
        assert output in ("torch", "numpy")
        if differentiable and output != "torch":
            raise ValueError("differentiable=True needs output='torch': gradients flow through torch tensors")
        if radii_grad and not differentiable:
            raise ValueError("radii_grad=True needs differentiable=True: radius gradients are part of the autograd graph")
        if sigma_grad and not differentiable:
            raise ValueError("sigma_grad=True needs differentiable=True: the sigma gradient is part of the autograd graph")
        if field_grad and not differentiable:
            raise ValueError("field_grad=True needs differentiable=True: the field gradient is part of the autograd graph")
        self.differentiable = bool(differentiable)
        self.field_grad = bool(field_grad)
        self.radii_grad = bool(radii_grad)
        self.sigma_grad = bool(sigma_grad)
        self._sigma_src = sigma_src
        self._bf16 = self._is_bf16_grid(grid_dtype, precision, output)  # (checked before anything touches a device)
        self._cl = self._is_channels_last(grid_layout, precision, output)  # (the same)
        if output == "torch" and torch is None:
            raise ImportError("output='torch' needs PyTorch; use output='numpy'")
        self.precision = precision
        self.fp = np.float32 if precision == 32 else np.float64  # numpy/voxelizer.py:34
        self._tfp = None if torch is None else (torch.float32 if precision == 32 else torch.float64)
        self._gdt = torch.bfloat16 if self._bf16 else self._tfp  # element type of the grids (torch)
        self.blockdim = blockdim if blockdim is not None else 8  # numpy/voxelizer.py:38
        self.num_blocks = -(-dimension // self.blockdim)
        self.output = output
        self._lib = _lib.load()
        self._device_index = self._resolve_device(device)
        self._handle = _lib.Handle()
        self._types_cache = None
        self._types_i32 = None
        self._types_fresh = False
        self._xf = _lib.MvxXform()  # reused per call: the library copies it before the call returns
        self._xf_addr = C.addressof(self._xf)
        self._has_torch_cuda = torch is not None and torch.cuda.is_available()  # asked on every call otherwise
        cfg = _lib.MvxConfig(
            float(resolution),
            float(getattr(self, "_sigma", 0.5)),
            int(dimension),
            int(self.blockdim),
            _lib.MVX_GAUSSIAN if density_type == "gaussian" else _lib.MVX_BINARY,
            self._device_index,
            int(precision),
            _lib.MVX_GRID_BF16 if self._bf16 else _lib.MVX_GRID_REAL,
        )
        _lib.check(self._lib.mvx_create(C.byref(cfg), C.byref(self._handle)))
        if self._cl:
            _lib.check(self._lib.mvx_set_grid_layout(self._handle, _lib.MVX_LAYOUT_NDHWC))
        self.overlap_prepass = bool(overlap_prepass)
        if self.overlap_prepass:
            self.set_overlap_prepass(True)

    @staticmethod
    def _is_bf16_grid(grid_dtype, precision, output) -> bool:
        """grid_dtype: None (the precision's type), "float32" / torch.float32 (precision 32), "bfloat16" / torch.bfloat16
        (precision 32, torch output: numpy has no bfloat16)."""
        if grid_dtype is None:
            return False
        name = str(grid_dtype).replace("torch.", "") if (torch is not None and isinstance(grid_dtype, torch.dtype)) else grid_dtype
        if name not in ("float32", "bfloat16"):
            raise ValueError(f"grid_dtype must be None, 'float32' or 'bfloat16' (or the torch dtypes), not {grid_dtype!r}")
        if precision != 32:
            raise ValueError(f"grid_dtype={name!r} needs precision=32 (a precision-64 voxelizer writes float64 grids)")
        if name == "bfloat16" and output != "torch":
            raise ValueError("grid_dtype='bfloat16' needs output='torch': numpy has no bfloat16")
        return name == "bfloat16"

    @staticmethod
    def _is_channels_last(grid_layout, precision, output) -> bool:
        """grid_layout: None / "contiguous" / torch.contiguous_format (NCDHW), or "channels_last" / torch.channels_last_3d
        (NDHWC strides on the same logical shape; precision 32, torch output)."""
        names = {None: False, "contiguous": False, "channels_last": True}
        if torch is not None:
            names.update({torch.contiguous_format: False, torch.channels_last_3d: True})
        try:
            cl = names[grid_layout]
        except (KeyError, TypeError):
            raise ValueError(f"grid_layout must be None, 'contiguous' or 'channels_last' (or torch.contiguous_format / "
                             f"torch.channels_last_3d), not {grid_layout!r}") from None
        if cl and precision != 32:
            raise ValueError("grid_layout='channels_last' needs precision=32 (float32 or bfloat16 grids)")
        if cl and output != "torch":
            raise ValueError("grid_layout='channels_last' needs output='torch': the layout is a torch memory format")
        return cl

    @property
    def grid_layout(self) -> str:
        """"contiguous" (C, D, H, W with W fastest) or "channels_last" (the same logical shape with the channel fastest)."""
        return "channels_last" if self._cl else "contiguous"

    def _dense_in_layout(self, t) -> bool:
        """Is the torch grid `t` dense in this voxelizer's layout (what the kernels write without a temporary)?"""
        if not self._cl:
            return t.is_contiguous()
        return (t if t.dim() == 5 else t.unsqueeze(0)).is_contiguous(memory_format=torch.channels_last_3d)

    def _empty_torch(self, shape, init_zero=False):
        fn = torch.zeros if init_zero else torch.empty
        if not self._cl:
            return fn(tuple(shape), dtype=self._gdt, device=self.device)
        if len(shape) == 5:  # exactly torch.empty(shape, memory_format=torch.channels_last_3d)
            t = torch.empty(tuple(shape), dtype=self._gdt, device=self.device, memory_format=torch.channels_last_3d)
            return t.zero_() if init_zero else t
        # a single grid: the permute(3, 0, 1, 2) view of a (D, H, W, C) buffer - unsqueeze(0) is channels-last-3d contiguous
        return fn(tuple(shape[1:]) + (shape[0],), dtype=self._gdt, device=self.device).permute(3, 0, 1, 2)

    @property
    def grid_dtype(self):
        """Element type of the grids this voxelizer writes: torch.float32 / torch.float64 (the precision's), or
        torch.bfloat16. (numpy dtype without torch.)"""
        return self._gdt if self._gdt is not None else self.fp

    def set_overlap_prepass(self, enable: bool):
        """Loops of large `forward_batch` calls: run the pre-pass of call k+1 under the voxelize launches of call k
        (mvx_set_overlap). The caller then promises that the input tensors of a call are complete when the call is made
        (not merely ordered on the stream) and stay unchanged until its launches have run; outputs keep stream order."""
        _lib.check(self._lib.mvx_set_overlap(self._handle, 1 if enable else 0))
        self.overlap_prepass = bool(enable)

    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _resolve_device(device) -> int:
        if device is None or device == "cuda":
            if torch is not None and torch.cuda.is_available():
                return torch.cuda.current_device()
            return 0
        if isinstance(device, int):
            return device
        if torch is not None:
            d = torch.device(device)
            assert d.type == "cuda", "the HIP backend runs on a GPU device only"
            return d.index if d.index is not None else torch.cuda.current_device()
        raise ValueError(f"cannot interpret device={device!r}")

    @property
    def device(self):
        return torch.device("cuda", self._device_index) if torch is not None else self._device_index

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h is not None and h.value:
            try:
                self._lib.mvx_destroy(h)
            except Exception:
                pass
            self._handle = None

    @property
    def sigma_tensor(self):
        """The tensor `sigma=` / `set_sigma()` gave (sigma_grad=True), or None: sigma is a python float."""
        return None if self._sigma_src is None else self._sigma_src[0]

    @staticmethod
    def _read_scalar_tensor(t, what):
        """(tensor, its _version, its value as a python float): one read to the host (a synchronisation for a device tensor)."""
        if t.numel() != 1:
            raise ValueError(f"{what} should be a python float or a one-element tensor, not a tensor of shape {tuple(t.shape)}")
        value = float(t.detach().reshape(()).item())
        if not value > 0.0:
            raise ValueError(f"{what} must be positive, got {value}")
        return t, t._version, value

    def set_sigma(self, value):
        """Replace sigma: a python float, or with sigma_grad=True a one-element tensor (kept as `sigma_tensor`; it gets
        dL/dsigma when it requires grad). A tensor is read to the host here and again before a call only after it was written
        in place (its `_version` moved, as `optimizer.step()` does): one synchronisation per step, none per call."""
        if _is_torch(value):
            if not self.sigma_grad:
                raise ValueError("sigma is a tensor: create the voxelizer with sigma_grad=True (and differentiable=True) to learn "
                                 "sigma, or pass a python float")
            src = self._read_scalar_tensor(value, "sigma")
        else:
            if not float(value) > 0.0:
                raise ValueError(f"sigma must be positive, got {float(value)}")
            src = None
        self._sigma_src = src
        if self.is_density_type_gaussian:  # (binary density stores no sigma: base class)
            self._sigma = src[2] if src is not None else float(value)
            self._density_changed()

    def _sync_sigma(self):
        """Before a call: re-read a sigma tensor that was written since its last read and hand the value to the library."""
        t, version, _ = self._sigma_src
        if t._version != version:
            self._sigma_src = self._read_scalar_tensor(t, "sigma")
            if self.is_density_type_gaussian:
                self._sigma = self._sigma_src[2]
                self._density_changed()

    def _on_density_type(self, value):
        if value == "gaussian":  # the default sigma comes back (base class): a sigma tensor no longer describes the density
            self._sigma_src = None
        super()._on_density_type(value)

    def _scalar_radius(self, radii):
        """radii_grad on a scalar-radii voxelizer: a one-element radii tensor -> (python float, the tensor). Read to the host when
        the tensor is new or was written in place since its last read (`_types_extent`'s rule). Anything else: (radii, None)."""
        if not (self.radii_grad and self.is_radii_type_scalar and _is_torch(radii) and radii.numel() == 1):
            return radii, None
        hit = self._rscalar_src
        if hit is None or hit[0] is not radii or hit[1] != radii._version:
            hit = self._rscalar_src = self._read_scalar_tensor(radii, "radii")
        return hit[2], radii

    def _density_changed(self):
        if getattr(self, "_handle", None) is not None:
            dens = _lib.MVX_GAUSSIAN if self.is_density_type_gaussian else _lib.MVX_BINARY
            _lib.check(self._lib.mvx_set_density(self._handle, dens, float(getattr(self, "_sigma", 0.5))))

    # ------------------------------------------------------------------------------------------
    # allocation / conversion (numpy/voxelizer.py:60-70, 562-583)
    def get_empty_grid(self, num_channels: int, batch_size: int | None = None, init_zero: bool = False):
        shape = self.grid_dimension(num_channels)
        if batch_size is not None:
            shape = (batch_size,) + shape
        if self.output == "torch":
            return self._empty_torch(shape, init_zero)
        if torch is not None and torch.cuda.is_available():
            # numpy grids live in pinned host memory (torch's caching host allocator): the copy back is a direct DMA
            # at PCIe speed instead of a staged pageable copy (3.4 -> ~0.7 ms per cfg-2 grid)
            fn = torch.zeros if init_zero else torch.empty
            return fn(shape, dtype=self._tfp, pin_memory=True).numpy()
        return (np.zeros if init_zero else np.empty)(shape, dtype=self.fp)

    def asarray(self, array, obj: str):
        if obj in ("coords", "center"):
            np_dt, t_dt = np.float64, "float64"
        elif obj in ("features", "radii"):
            np_dt, t_dt = (np.float32, "float32") if self.precision == 32 else (np.float64, "float64")
        elif obj == "types":
            np_dt, t_dt = np.int16, "int16"
        else:
            raise ValueError("obj should be ['coords', 'center', 'radii', types', 'features']")
        if self.output == "torch":
            if _is_torch(array):
                return array.to(device=self.device, dtype=getattr(torch, t_dt))
            return torch.as_tensor(np.asarray(array, dtype=np_dt), device=self.device)
        if _is_torch(array):
            array = array.detach().cpu().numpy()
        return np.asarray(array, dtype=np_dt)

    def to(self, device):
        """torch-backend compatibility: a handle is bound to one GPU; moving re-creates it."""
        idx = self._resolve_device(device)
        if idx != self._device_index:
            kw = {"sigma": self._sigma if self._sigma_src is None else self._sigma_src[0]} if self.is_density_type_gaussian else {}
            moved = type(self)(self._resolution, self._dimension, self._radii_type, self._density_type, self.precision,
                               self.blockdim, idx, self.output, self.overlap_prepass,
                               grid_dtype="bfloat16" if self._bf16 else None, differentiable=self.differentiable,
                               radii_grad=self.radii_grad, sigma_grad=self.sigma_grad, grid_layout=self.grid_layout,
                               field_grad=getattr(self, "field_grad", False), **kw)
            if self.sum_parts != 1:
                moved.set_sum_parts(self.sum_parts)
            return moved
        return self

    def cuda(self):
        return self

    def cpu(self):
        raise NotImplementedError("the HIP backend has no CPU path; use the upstream numpy backend on the host")

    # ------------------------------------------------------------------------------------------
    # argument plumbing
    def _stream(self):
        """The caller's current torch stream as a hipStream_t value (0 = the null stream)."""
        if self._has_torch_cuda:
            if _raw_stream is not None:
                return _raw_stream(self._device_index)
            return torch.cuda.current_stream(self._device_index).cuda_stream
        return 0

    def _on_device(self, x) -> bool:
        return _is_torch(x) and x.is_cuda and x.device.index == self._device_index

    def _prepare_inputs(self, coords, chan, chan_kind, radii):
        """Returns (coords, chan, radii_array_or_None, in_kind, keepalive). chan_kind in {features, types, None}."""
        dev = self._on_device(coords)
        keep = []
        if dev:
            c = coords if (coords.dtype == torch.float64 and coords.is_contiguous()) else coords.to(torch.float64).contiguous()
            ch = None
            if chan_kind == "features":
                ch = (chan if _is_torch(chan) else torch.as_tensor(np.asarray(chan), device=self.device)).to(
                    device=self.device, dtype=self._tfp).contiguous()
            elif chan_kind == "types":
                t = chan if _is_torch(chan) else torch.as_tensor(np.asarray(chan), device=self.device)
                ch = self._types_as_int32(t)
            r = None
            if not _np_isscalar(radii):
                r = (radii if _is_torch(radii) else torch.as_tensor(np.asarray(radii), device=self.device)).to(
                    device=self.device, dtype=self._tfp).contiguous()
            keep += [c, ch, r]
            return c, ch, r, _lib.MVX_DEVICE, keep
        if _is_torch(coords):
            coords = coords.detach().cpu().numpy()
        c = np.ascontiguousarray(coords, dtype=np.float64)
        ch = None
        if chan_kind == "features":
            ch = chan.detach().cpu().numpy() if _is_torch(chan) else np.asarray(chan)
            ch = np.ascontiguousarray(ch, dtype=self.fp)
        elif chan_kind == "types":
            t = chan.detach().cpu().numpy() if _is_torch(chan) else np.asarray(chan)
            ch = np.ascontiguousarray(t.astype(np.int16), dtype=np.int32)
        r = None
        if not _np_isscalar(radii):
            r = radii.detach().cpu().numpy() if _is_torch(radii) else np.asarray(radii)
            r = np.ascontiguousarray(r, dtype=self.fp)
        keep += [c, ch, r]
        return c, ch, r, _lib.MVX_HOST, keep

    @staticmethod
    def _ptr(x):
        """Address for a `void *` argument (ctypes takes None / int)."""
        if x is None:
            return None
        if _is_torch(x):
            return x.data_ptr()
        return x.ctypes.data

    def _make_xform(self, center, random_translation, random_rotation, on_device=False, keep=None):
        """Address of one mvx_xform (the library copies it during the call): centring + the random transform drawn in
        the reference's RNG order. A `center` tensor on this device is handed over by pointer (MVX_XF_CENTER_PTR) when
        the coordinates live there too: its value never visits the host, so the call does not synchronise."""
        xf = self._xf
        flags = 0
        if center is not None:
            if on_device and self._on_device(center):
                cen = center if (center.dtype == torch.float64 and center.is_contiguous()) else center.to(torch.float64).contiguous()
                assert cen.numel() == 3, "center should be Array[3,]"
                if keep is not None:
                    keep.append(cen)
                xf.center_ptr = cen.data_ptr()
                flags |= _lib.MVX_XF_CENTER | _lib.MVX_XF_CENTER_PTR
            else:
                cen = center.detach().cpu().numpy() if _is_torch(center) else np.asarray(center)
                cen = cen.reshape(3).astype(np.float64)
                xf.center[0], xf.center[1], xf.center[2] = float(cen[0]), float(cen[1]), float(cen[2])
                flags |= _lib.MVX_XF_CENTER
        if random_rotation or (random_translation is not None and random_translation > 0.0):
            translation, quaternion = draw_forward_transform(random_translation, random_rotation)
            if quaternion is not None:
                xf.quat[0], xf.quat[1], xf.quat[2], xf.quat[3] = (float(q) for q in quaternion)
                flags |= _lib.MVX_XF_ROTATE
            if translation is not None:
                t = translation.reshape(3)
                xf.trans[0], xf.trans[1], xf.trans[2] = float(t[0]), float(t[1]), float(t[2])
                flags |= _lib.MVX_XF_TRANSLATE
        xf.flags = flags
        return self._xf_addr if flags else None

    def _resolve_out(self, out_grid, shape):
        """Returns (buffer passed to the library, out_kind, object to return)."""
        if out_grid is None:
            out_grid = self.get_empty_grid(shape[0])
        if _is_torch(out_grid):
            if self._on_device(out_grid) and self._dense_in_layout(out_grid) and out_grid.dtype == self._gdt:
                return out_grid, _lib.MVX_DEVICE, out_grid, None
            tmp = self._empty_torch(tuple(out_grid.shape))
            return tmp, _lib.MVX_DEVICE, out_grid, "copy_torch"
        if self._bf16 or self._cl:  # a numpy grid (no bfloat16, no channels-last there): made on the device, copied as float32
            tmp = self._empty_torch(tuple(out_grid.shape))
            return tmp, _lib.MVX_DEVICE, out_grid, "copy_numpy_bf16"
        if out_grid.flags.c_contiguous and out_grid.dtype == self.fp:
            return out_grid, _lib.MVX_HOST, out_grid, None
        tmp = np.empty(out_grid.shape, dtype=self.fp)
        return tmp, _lib.MVX_HOST, out_grid, "copy_numpy"

    @staticmethod
    def _finish_out(buf, ret, how):
        if how == "copy_torch":
            ret.copy_(buf)
        elif how == "copy_numpy":
            ret[...] = buf
        elif how == "copy_numpy_bf16":
            ret[...] = buf.float().cpu().numpy()
        return ret

    def _radii_type_code(self):
        if self.is_radii_type_scalar:
            return _lib.MVX_RADII_SCALAR
        if self.is_radii_type_atom_wise:
            return _lib.MVX_RADII_ATOM
        return _lib.MVX_RADII_CHANNEL

    # ------------------------------------------------------------------------------------------
    # VECTOR  (replaces numpy/voxelizer.py:97-236)
    def forward_features(self, coords, center, features, radii, random_translation=0.0, random_rotation=False,
                         out_grid=None):
        """coords (V,3), center (3,) | None, features (V,C), radii scalar | (V,) | (C,); out (C,D,H,W)."""
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        self._check_args_features(coords, features, radii, out_grid)
        C_ = features.shape[1]
        grad = self._grad_wanted(coords, features, center, radii, out_grid, rten)
        c, f, r, in_kind, keep = self._prepare_inputs(coords, features, "features", radii)
        center = self._grad_center(center) if grad else center
        xf = self._make_xform(center, random_translation, random_rotation, in_kind == _lib.MVX_DEVICE, keep)
        buf, out_kind, ret, how = self._resolve_out(out_grid, (C_,))
        rs = float(radii) if r is None else 0.0
        launch = lambda: self._lib.mvx_forward_features(  # noqa: E731
            self._handle, self._ptr(c), self._ptr(f), self._ptr(r), rs, self._radii_type_code(), c.shape[0], C_,
            xf, self._ptr(buf), in_kind, out_kind, self._stream())
        if grad:
            return self._autograd(launch, ret, "features", c, f, center, None, r, rs, np.array([0, c.shape[0]], np.int64),
                                  self._xform_copy(xf), 1, C_, rten)
        rc = launch()
        if rc:
            _lib.check(rc)
        return self._finish_out(buf, ret, how) if how else ret

    def _check_args_features(self, coords, features, radii, out_grid=None):
        V = coords.shape[0]
        C_ = features.shape[1]
        D = H = W = self.dimension
        assert features.shape[0] == V, f"atom features does not match number of atoms: {features.shape[0]} vs {V}"
        assert features.ndim == 2, f"atom features does not match dimension: {features.shape} vs {(V,'*')}"
        if self.is_radii_type_scalar:
            assert _np_isscalar(radii), "the radii type of voxelizer is `scalar`, radii should be scalar"
        elif self.is_radii_type_channel_wise:
            assert not _np_isscalar(radii), f"the radii type of voxelizer is `channel-wise`, radii should be Array[{C_},]"
            assert tuple(radii.shape) == (C_,), f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(C_,)}"
        else:
            assert not _np_isscalar(radii), f"the radii type of voxelizer is `atom-wise`, radii should be Array[{V},]"
            assert tuple(radii.shape) == (V,), f"radii does not match dimension (number of atoms,): {tuple(radii.shape)} vs {(V,)}"
        if out_grid is not None:
            assert tuple(out_grid.shape) == (C_, D, H, W), f"Output grid dimension incorrect: {tuple(out_grid.shape)} vs {(C_,D,H,W)}"

    # ------------------------------------------------------------------------------------------
    # INDEX  (replaces numpy/voxelizer.py:240-366)
    def forward_types(self, coords, center, types, radii, random_translation=0.0, random_rotation=False,
                      out_grid=None):
        """coords (V,3), center (3,) | None, types (V,), radii scalar | (V,) | (C,); out (C,D,H,W)."""
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        n_types = self._check_args_types(coords, types, radii, out_grid)
        if out_grid is not None:
            C_ = out_grid.shape[0]  # extra channels stay zero (numpy/voxelizer.py:337)
        elif self.is_radii_type_channel_wise:
            C_ = radii.shape[0]  # numpy/voxelizer.py:275-276
        else:
            C_ = n_types  # max(types) + 1 over ALL atoms, numpy/voxelizer.py:278
        grad = self._grad_wanted(coords, None, center, radii, out_grid, rten)
        c, t, r, in_kind, keep = self._prepare_inputs(coords, types, "types", radii)
        if self.is_radii_type_channel_wise and r is not None and r.shape[0] < C_:
            # channel-wise radii are indexed by type only; pad so the (C,) contract of the ABI holds
            pad = C_ - r.shape[0]
            r = torch.cat([r, r.new_ones(pad)]) if _is_torch(r) else np.concatenate([r, np.ones(pad, self.fp)])
        center = self._grad_center(center) if grad else center
        xf = self._make_xform(center, random_translation, random_rotation, in_kind == _lib.MVX_DEVICE, keep)
        buf, out_kind, ret, how = self._resolve_out(out_grid, (C_,))
        rs = float(radii) if r is None else 0.0
        launch = lambda: self._lib.mvx_forward_types(  # noqa: E731
            self._handle, self._ptr(c), self._ptr(t), self._ptr(r), rs, self._radii_type_code(), c.shape[0], int(C_),
            xf, self._ptr(buf), in_kind, out_kind, self._stream())
        if grad:
            return self._autograd(launch, ret, "types", c, None, center, t, r, rs, np.array([0, c.shape[0]], np.int64),
                                  self._xform_copy(xf), 1, int(C_), rten)
        rc = launch()
        if rc:
            _lib.check(rc)
        return self._finish_out(buf, ret, how) if how else ret

    def _types_as_int32(self, t):
        """Device types in the ABI's int32, through int16 like the reference's cast (numpy/voxelizer.py:269).
        The converted tensor is remembered while the same unmodified tensor keeps coming (two cast kernels per call
        otherwise)."""
        hit = self._types_i32
        self._types_fresh = False
        if hit is None or hit[0] is not t or hit[1] != t._version:
            # (the source tensor is held, not its address: a freed tensor's memory can come back with other content)
            hit = self._types_i32 = (t, t._version, t.to(device=self.device).to(torch.int16).to(torch.int32).contiguous())
            self._types_fresh = True  # converted on the current stream a moment ago
        return hit[2]

    def _types_extent(self, types):
        """(min, max) of the type indices. For a device tensor this costs a kernel and a synchronisation, so the
        answer is remembered for as long as the same tensor is passed unmodified (torch bumps `_version` on every
        in-place write) - the per-molecule loop of test/test_time_numpy.py:11-15 asks thousands of times.
        Limitation: a write that bypasses torch's version counter (`.data`, raw pointers, DLPack consumers, this
        library's own mvx_memcpy) is not seen; such callers should pass a fresh tensor (or clone) after writing."""
        if not _is_torch(types):
            return int(types.min()), int(types.max())
        hit = self._types_cache
        if hit is None or hit[0] is not types or hit[1] != types._version:
            lo, hi = torch.aminmax(types)
            hit = self._types_cache = (types, types._version, int(lo), int(hi))
        return hit[2], hit[3]

    def _check_args_types(self, coords, types, radii, out_grid=None):
        V = coords.shape[0]
        tmin, tmax = self._types_extent(types)
        C_ = tmax + 1
        D = H = W = self.dimension
        assert tuple(types.shape) == (V,), f"types does not match dimension: {tuple(types.shape)} vs {(V,)}"
        assert tmin >= 0, "types must be non-negative channel indices"
        if self.is_radii_type_scalar:
            assert _np_isscalar(radii), "the radii type of voxelizer is `scalar`, radii should be scalar"
        elif self.is_radii_type_channel_wise:
            assert not _np_isscalar(radii), f"the radii type of voxelizer is `channel-wise`, radii should be Array[{C_},]"
            assert tuple(radii.shape) == (C_,), f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(C_,)}"
        else:
            assert not _np_isscalar(radii), f"the radii type of voxelizer is `atom-wise`, radii should be Array[{V},]"
            assert tuple(radii.shape) == (V,), f"radii does not match dimension (number of atoms,): {tuple(radii.shape)} vs {(V,)}"
        if out_grid is not None:
            assert out_grid.shape[0] >= C_, f"Output channel is less than number of types: {out_grid.shape[0]} < {C_}"
            assert tuple(out_grid.shape[1:]) == (D, H, W), f'Output grid dimension incorrect: {tuple(out_grid.shape)} vs {("*",D,H,W)}'
        return C_

    # ------------------------------------------------------------------------------------------
    # SINGLE  (replaces numpy/voxelizer.py:370-477)
    def forward_single(self, coords, center, radii, random_translation=0.0, random_rotation=False, out_grid=None):
        """coords (V,3), center (3,) | None, radii scalar | (V,); out (1,D,H,W)."""
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        self._check_args_single(coords, radii, out_grid)
        grad = self._grad_wanted(coords, None, center, radii, out_grid, rten)
        c, _, r, in_kind, keep = self._prepare_inputs(coords, None, None, radii)
        center = self._grad_center(center) if grad else center
        xf = self._make_xform(center, random_translation, random_rotation, in_kind == _lib.MVX_DEVICE, keep)
        buf, out_kind, ret, how = self._resolve_out(out_grid, (1,))
        rs = float(radii) if r is None else 0.0
        launch = lambda: self._lib.mvx_forward_single(  # noqa: E731
            self._handle, self._ptr(c), self._ptr(r), rs, self._radii_type_code(), c.shape[0],
            xf, self._ptr(buf), in_kind, out_kind, self._stream())
        if grad:
            return self._autograd(launch, ret, "single", c, None, center, None, r, rs, np.array([0, c.shape[0]], np.int64),
                                  self._xform_copy(xf), 1, 1, rten)
        rc = launch()
        if rc:
            _lib.check(rc)
        return self._finish_out(buf, ret, how) if how else ret

    def _check_args_single(self, coords, radii, out_grid=None):
        V = coords.shape[0]
        D = H = W = self.dimension
        assert not self.is_radii_type_channel_wise, "Channel-Wise Radii Type is not supported"
        if self.is_radii_type_scalar:
            assert _np_isscalar(radii), "the radii type of voxelizer is `scalar`, radii should be scalar"
        else:
            assert not _np_isscalar(radii), f"the radii type of voxelizer is `atom-wise`, radii should be Array[{V},]"
            assert tuple(radii.shape) == (V,), f"radii does not match dimension (number of atoms,): {tuple(radii.shape)} vs {(V,)}"
        if out_grid is not None:
            assert out_grid.shape[0] == 1, "Output channel should be 1"
            assert tuple(out_grid.shape[1:]) == (D, H, W), f'Output grid dimension incorrect: {tuple(out_grid.shape)} vs {("*",D,H,W)}'

    # ------------------------------------------------------------------------------------------
    # BATCH (the loop of test/test_time_numpy.py:11-15 as one launch; molecules are independent)
    def forward_batch(self, coords, offsets, centers, channels, radii, num_channels=None, out_grid=None,
                      random_translation=0.0, random_rotation=False):
        """Voxelize B molecules stored back to back.

        coords (sumN,3) float64; offsets (B+1,) int64 (host); centers (B,3) | None;
        channels: (sumN,C) float -> features, (sumN,) int -> types, None -> single;
        radii: python float | (sumN,) | (C,) per this voxelizer's radii_type.
        out_grid: (B,C,D,H,W) of this voxelizer's grid_dtype (torch CUDA tensor on this device or numpy), fully overwritten.
        A random transform, if requested, is drawn per molecule in molecule order.
        """
        return self._forward_batch(coords, offsets, centers, channels, radii, num_channels, out_grid, random_translation,
                                   random_rotation)

    def _forward_batch(self, coords, offsets, centers, channels, radii, num_channels=None, out_grid=None,
                       random_translation=0.0, random_rotation=False, xforms=None, fresh_inputs=False, pose=None):
        """forward_batch's body. xforms: (records, device centres) already drawn by the caller (forward_views on a
        differentiable voxelizer, the posed forms) instead of new ones; fresh_inputs: the caller made the inputs on the current
        stream a moment ago, so with overlap_prepass the stream is synchronised before the side stream may read them; pose: the
        packed (B, 10) poses the records point at (the posed forms; `centers` is None then)."""
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.shape[0] - 1
        assert offsets[0] == 0 and offsets[-1] == coords.shape[0], "offsets must span coords"
        kind, C_ = self._batch_kind(channels, radii, num_channels)
        self._check_args_batch(coords, channels, kind, radii, C_)
        grad = self._grad_wanted(coords, channels if kind == "features" else None, centers if pose is None else pose, radii,
                                 out_grid, rten)
        user_centers = centers  # (a conversion made below, for autograd or for the ABI, is "fresh")
        if grad and centers is not None:
            centers = self._grad_center(centers)
        c, ch, r, in_kind, keep = self._prepare_inputs(coords, channels, kind, radii)
        # With overlap_prepass the library's side stream reads the inputs without waiting for the caller's stream.
        # Arrays this layer had to convert just now (dtype / layout fixes, the int32 copy of `types`) were produced
        # ON that stream a moment ago: make them complete first (first call with a given tensor only: the copies are
        # cached or the caller passes the right dtype)
        fresh = self.overlap_prepass and in_kind == _lib.MVX_DEVICE and (
            c is not coords or (kind == "features" and ch is not channels) or (r is not None and r is not radii)
            or (kind == "types" and self._types_fresh))
        r, padded = self._pad_type_radii(r, kind, C_)
        fresh = fresh or (self.overlap_prepass and (padded or (fresh_inputs and in_kind == _lib.MVX_DEVICE)))
        xfs, dev_cen = self._call_xforms(B, centers, in_kind, random_translation, random_rotation, keep, xforms)
        if xforms is None and dev_cen is not None:
            fresh = fresh or (self.overlap_prepass and dev_cen.data_ptr() != user_centers.data_ptr())
        xf_ptr = None if xfs is None else C.addressof(xfs)
        if out_grid is None:
            out_grid = self.get_empty_grid(C_, batch_size=B)
        assert tuple(out_grid.shape) == (B,) + self.grid_dimension(C_), (
            f"Output grid dimension incorrect: {tuple(out_grid.shape)} vs {(B,) + self.grid_dimension(C_)}")
        buf, out_kind, ret, how = self._resolve_out(out_grid, None)
        if fresh:
            torch.cuda.current_stream(self._device_index).synchronize()
        rs = float(radii) if _np_isscalar(radii) else 0.0
        off_ptr = offsets.ctypes.data
        rt = self._radii_type_code()
        if kind == "features":
            launch = lambda: self._lib.mvx_forward_features_batch(  # noqa: E731
                self._handle, self._ptr(c), self._ptr(ch), self._ptr(r), rs, rt, off_ptr, xf_ptr, B, C_,
                self._ptr(buf), in_kind, out_kind, self._stream())
        elif kind == "types":
            launch = lambda: self._lib.mvx_forward_types_batch(  # noqa: E731
                self._handle, self._ptr(c), self._ptr(ch), self._ptr(r), rs, rt, off_ptr, xf_ptr, B, C_,
                self._ptr(buf), in_kind, out_kind, self._stream())
        else:
            assert not self.is_radii_type_channel_wise, "Channel-Wise Radii Type is not supported"
            launch = lambda: self._lib.mvx_forward_single_batch(  # noqa: E731
                self._handle, self._ptr(c), self._ptr(r), rs, rt, off_ptr, xf_ptr, B, self._ptr(buf), in_kind, out_kind,
                self._stream())
        if grad:
            return self._autograd(launch, ret, kind or "single", c, ch if kind == "features" else None,
                                  dev_cen, ch if kind == "types" else None, r, rs, offsets, xfs, B, C_, rten, pose)
        _lib.check(launch())
        return self._finish_out(buf, ret, how)

    def _batch_kind(self, channels, radii, num_channels):
        """(kind, C) of a batch or views call from its channels: None -> single, (sumN,) int -> types, (sumN, C) -> features."""
        if channels is None:
            return None, 1
        if channels.ndim != 1:
            return "features", int(channels.shape[1])
        if num_channels is not None:
            return "types", int(num_channels)
        return "types", int(radii.shape[0] if self.is_radii_type_channel_wise else int(channels.max()) + 1)

    def _pad_type_radii(self, r, kind, C_):
        """Channel-wise radii are indexed by type only: padded with ones so that the (C,) contract of the ABI holds (as
        forward_types). Returns (radii, whether a new array was made)."""
        if not (kind == "types" and self.is_radii_type_channel_wise and r.shape[0] < C_):
            return r, False
        pad = C_ - r.shape[0]
        return (torch.cat([r, r.new_ones(pad)]) if _is_torch(r) else np.concatenate([r, np.ones(pad, self.fp)])), True

    def _call_xforms(self, B, centers, in_kind, random_translation, random_rotation, keep, xforms):
        """The records of a batch call as (records or None, device centres or None). xforms: the pair the caller drew already
        (forward_views on a differentiable voxelizer, the posed forms) instead of new ones."""
        if xforms is not None:
            return xforms
        if centers is not None or random_rotation or (random_translation and random_translation > 0.0):
            return self._make_xforms(B, centers, in_kind, random_translation, random_rotation, keep)
        return None, None

    def _device_coords(self, coords):
        """coords on this voxelizer's device (the score entries take device arrays only): host arrays are moved there."""
        if self._on_device(coords):
            return coords
        return (coords.detach() if _is_torch(coords) else torch.as_tensor(np.asarray(coords, dtype=np.float64))).to(self.device)

    def _field_tensor(self, field):
        """The field of a score call as the library reads it: on this device, of the grid's dtype, contiguous."""
        return (field if _is_torch(field) else torch.as_tensor(np.asarray(field))).to(device=self.device, dtype=self._gdt).contiguous()

    def _make_xforms(self, B, centers, in_kind, random_translation, random_rotation, keep):
        """B mvx_xform records, one per molecule (forward_batch) or view (forward_views): centring + the random transform,
        drawn record by record in order. Returns (records, the device centres handed over by pointer or None)."""
        xfs = (_lib.MvxXform * B)()
        cen = dev_cen = None
        if centers is not None:
            if in_kind == _lib.MVX_DEVICE and self._on_device(centers):  # by pointer: no copy to the host
                dev_cen = centers.to(torch.float64).contiguous().reshape(B, 3)
                keep.append(dev_cen)
            else:
                cen = centers.detach().cpu().numpy() if _is_torch(centers) else np.asarray(centers)
                cen = cen.reshape(B, 3)
        for b in range(B):
            self._make_xform(None if cen is None else cen[b], random_translation, random_rotation)
            if dev_cen is not None:
                self._xf.center_ptr = dev_cen.data_ptr() + 24 * b
                self._xf.flags |= _lib.MVX_XF_CENTER | _lib.MVX_XF_CENTER_PTR
            C.memmove(C.addressof(xfs) + b * C.sizeof(_lib.MvxXform), self._xf_addr, C.sizeof(_lib.MvxXform))
        return xfs, dev_cen

    def _check_args_batch(self, coords, channels, kind, radii, C_):
        """The per-molecule checks (_check_args_features / _types / _single) for atoms stored back to back: the
        library reads sumN rows of channels and sumN | C radii, so every array must really have them."""
        V = coords.shape[0]
        assert coords.ndim == 2 and coords.shape[1] == 3, f"coords does not match dimension: {tuple(coords.shape)} vs {(V, 3)}"
        if kind == "features":
            assert channels.shape[0] == V, f"atom features does not match number of atoms: {channels.shape[0]} vs {V}"
        elif kind == "types":
            assert tuple(channels.shape) == (V,), f"types does not match dimension: {tuple(channels.shape)} vs {(V,)}"
        else:
            assert not self.is_radii_type_channel_wise, "Channel-Wise Radii Type is not supported"
        if self.is_radii_type_scalar:
            assert _np_isscalar(radii), "the radii type of voxelizer is `scalar`, radii should be scalar"
        elif self.is_radii_type_channel_wise:
            assert not _np_isscalar(radii), f"the radii type of voxelizer is `channel-wise`, radii should be Array[{C_},]"
            if kind == "features":
                assert tuple(radii.shape) == (C_,), f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(C_,)}"
            else:  # types: radii are gathered by type; every type below num_channels needs one
                assert radii.ndim == 1 and 0 < radii.shape[0] <= C_, f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(C_,)}"
                if V > 0:
                    tmax = int(channels.max())
                    assert tmax < radii.shape[0], f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(tmax + 1,)}"
        else:
            assert not _np_isscalar(radii), f"the radii type of voxelizer is `atom-wise`, radii should be Array[{V},]"
            assert tuple(radii.shape) == (V,), f"radii does not match dimension (number of atoms,): {tuple(radii.shape)} vs {(V,)}"

    # ------------------------------------------------------------------------------------------
    # VIEWS (many boxes of one shared point cloud: mvx_select_views / mvx_forward_views)
    def _views_args(self, coords, centers, channels, radii, num_channels):
        """(kind, C, radii, scalar-radius tensor) of a views call: forward_batch's rules for one molecule of N atoms."""
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        kind, C_ = self._batch_kind(channels, radii, num_channels)
        self._check_args_batch(coords, channels, kind, radii, C_)
        assert centers is not None and centers.ndim == 2 and centers.shape[1] == 3, (
            f"centers does not match dimension: {tuple(getattr(centers, 'shape', ()))} vs ('B', 3)")
        return kind, C_, radii, rten

    def _views_inputs(self, coords, channels, kind, radii, C_):
        c, ch, r, in_kind, keep = self._prepare_inputs(coords, channels, kind, radii)
        r, padded = self._pad_type_radii(r, kind, C_)
        if padded:
            keep.append(r)
        return c, ch, r, in_kind, keep

    def _select(self, c, types, r, rs, kind, C_, xfs, B, in_kind):
        """mvx_select_views into an index buffer sized from the call's shape: B * N entries when that is small, else the
        last call's total with some room. One call (one synchronisation) unless the buffer turns out too small: the library
        then reports MVX_ERR_INVALID with the offsets filled in, and the call is repeated with the exact size."""
        N = int(c.shape[0])
        offsets = np.full(B + 1, -1, dtype=np.int64)
        args = (self._handle, self._ptr(c), self._ptr(types), self._ptr(r), rs, self._radii_type_code(),
                _lib.MODES[kind or "single"], N, C_, C.addressof(xfs), B)
        cap = B * N if B * N <= (1 << 20) else min(B * N, max(1 << 20, 2 * getattr(self, "_views_total", 0)))
        index = torch.empty(cap, dtype=torch.int64, device=self.device)
        rc = self._lib.mvx_select_views(*args, index.data_ptr() if cap else None, cap, offsets.ctypes.data, in_kind, self._stream())
        if rc != 0 and offsets[-1] > cap:  # too small: size it from the offsets and call again
            index = torch.empty(int(offsets[-1]), dtype=torch.int64, device=self.device)
            rc = self._lib.mvx_select_views(*args, index.data_ptr(), index.numel(), offsets.ctypes.data, in_kind, self._stream())
        _lib.check(rc)
        self._views_total = int(offsets[-1])
        return index[:int(offsets[-1])], offsets

    def select_views(self, coords, centers, channels=None, radii=None, random_translation=0.0, random_rotation=False):
        """The atoms each view of a shared cloud can see: (index, offsets), index an int64 tensor on this voxelizer's
        device, offsets a numpy int64 array of B + 1 entries; index[offsets[b]:offsets[b + 1]] are, in ascending order, the
        atoms that pass the forward's box cull for view b (every atom that reaches a voxel of that view's grid is among
        them). Arguments as forward_views; feature values are not read. Synchronises the stream (the offsets come to the host)."""
        return self._select_views(coords, centers, channels, radii, random_translation, random_rotation)

    def _select_views(self, coords, centers, channels, radii, random_translation=0.0, random_rotation=False, num_channels=None,
                      xforms=None):
        """select_views' body. num_channels: the channel count of a types call; xforms: records already drawn."""
        kind, C_, radii, _ = self._views_args(coords, centers, channels, radii, num_channels)
        B = int(centers.shape[0])
        c, ch, r, in_kind, keep = self._views_inputs(coords, channels if kind == "types" else None, kind if kind == "types" else None,
                                                     radii, C_)
        xfs, _ = xforms if xforms is not None else self._make_xforms(B, centers, in_kind, random_translation, random_rotation, keep)
        rs = float(radii) if _np_isscalar(radii) else 0.0
        return self._select(c, ch, r, rs, kind, C_, xfs, B, in_kind)

    def forward_views(self, coords, centers, channels, radii, num_channels=None, out_grid=None, random_translation=0.0,
                      random_rotation=False):
        """Voxelize B boxes of ONE shared point cloud: grid b is the cloud seen from centers[b] (and through view b's random
        transform). The (B, C, D, H, W) result is, bit for bit, forward_batch on the cloud repeated B times - without the B
        copies: each view's atoms are selected on the device (those that pass the forward's box cull), gathered into a
        compact batch and voxelized by the batched pipeline.

        coords (N,3) float64; centers (B,3); channels: (N,C) float -> features, (N,) int -> types, None -> single;
        radii: python float | (N,) | (C,) per this voxelizer's radii_type - forward_batch's rules for one molecule of N
        atoms, and in types mode the channel count is inferred as forward_batch infers it for the whole cloud.
        A random transform, if requested, is drawn per view in view order, exactly as forward_batch draws one per molecule:
        with the same seed both calls use the same transforms.
        The call synchronises the stream once (the per-view atom counts come to the host). `overlap_prepass` does not
        apply to this entry. On a differentiable voxelizer with inputs that require grad the call is select_views, a torch
        gather of the selected rows and forward_batch on them: autograd sums every view's gradient into the shared tensors.
        """
        return self._forward_views(coords, centers, channels, radii, num_channels, out_grid, random_translation, random_rotation)

    def _forward_views(self, coords, centers, channels, radii, num_channels=None, out_grid=None, random_translation=0.0,
                       random_rotation=False, posed=None):
        """forward_views' body. posed: (quaternions, translations) of forward_posed_views: the views' records are explicit
        poses instead of centres with random transforms."""
        kind, C_, cradii, rten = self._views_args(coords, centers, channels, radii, num_channels)
        B = int(centers.shape[0])
        pose = None
        if posed is not None:
            pose = self._pack_pose(B, centers, posed[0], posed[1], self._on_device(coords))
        if self._grad_wanted(coords, channels if kind == "features" else None, centers if pose is None else pose, cradii, out_grid,
                             rten):
            keep = []
            in_kind = _lib.MVX_DEVICE  # (_grad_wanted: coords live on this device)
            if pose is None:
                cen = self._grad_center(centers)
                xforms = self._make_xforms(B, cen, in_kind, random_translation, random_rotation, keep)
            else:
                cen, xforms = None, (self._pose_xforms(pose, B), None)
            with torch.no_grad():
                index, offsets = self._select_views(coords, centers, channels, cradii,
                                                    num_channels=C_ if kind == "types" else None, xforms=xforms)

            def take(x):
                if _is_torch(x):
                    return x[index.to(x.device)]
                return np.asarray(x)[index.cpu().numpy()]

            r_sel = take(cradii) if self.is_radii_type_atom_wise else radii
            # (the gathered rows are made on this stream just now: with overlap_prepass the side stream must not read them
            # early - fresh_inputs makes _forward_batch synchronise first)
            return self._forward_batch(coords[index], offsets, cen, None if channels is None else take(channels), r_sel,
                                       num_channels=C_ if kind == "types" else None, xforms=xforms, fresh_inputs=True, pose=pose)
        c, ch, r, in_kind, keep = self._views_inputs(coords, channels, kind, cradii, C_)
        if pose is None:
            xfs, _ = self._make_xforms(B, centers, in_kind, random_translation, random_rotation, keep)
        else:
            xfs = self._pose_xforms(pose, B)
        if out_grid is None:
            out_grid = self.get_empty_grid(C_, batch_size=B)
        assert tuple(out_grid.shape) == (B,) + self.grid_dimension(C_), (
            f"Output grid dimension incorrect: {tuple(out_grid.shape)} vs {(B,) + self.grid_dimension(C_)}")
        buf, out_kind, ret, how = self._resolve_out(out_grid, None)
        rs = float(cradii) if _np_isscalar(cradii) else 0.0
        _lib.check(self._lib.mvx_forward_views(
            self._handle, _lib.MODES[kind or "single"], self._ptr(c), self._ptr(ch), self._ptr(r), rs, self._radii_type_code(),
            int(c.shape[0]), C_, C.addressof(xfs), B, self._ptr(buf), in_kind, out_kind, self._stream()))
        return self._finish_out(buf, ret, how)

    # ------------------------------------------------------------------------------------------
    # POSES (explicit rigid transforms: MVX_XF_POSE_PTR records, mvx_pose_grad_batch)
    def _pack_pose(self, B, centers, quaternions, translations, on_device):
        """The (B, 10) float64 block [c | q | t] the records of a posed call point at. With coordinates on this device the block
        is a tensor there: torch tensors are packed with torch ops (recorded by autograd; their values never visit the host and
        nothing synchronises), numpy poses are packed on the host and uploaded. With host coordinates: a numpy array."""
        def shape(x):
            return tuple(getattr(x, "shape", ()))

        assert shape(quaternions) == (B, 4), f"quaternions does not match dimension: {shape(quaternions)} vs {(B, 4)}"
        assert shape(translations) == (B, 3), f"translations does not match dimension: {shape(translations)} vs {(B, 3)}"
        assert centers is None or shape(centers) == (B, 3), f"centers does not match dimension: {shape(centers)} vs {(B, 3)}"
        parts = [centers, quaternions, translations]
        if on_device and any(self._on_device(x) for x in parts):
            dev = [torch.zeros((B, 3), dtype=torch.float64, device=self.device) if x is None else
                   (x if _is_torch(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))).to(device=self.device, dtype=torch.float64)
                   for x in parts]
            return torch.cat(dev, dim=1).contiguous()
        host = [np.zeros((B, 3)) if x is None else
                np.asarray(x.detach().cpu().numpy() if _is_torch(x) else x, dtype=np.float64) for x in parts]
        block = np.ascontiguousarray(np.concatenate(host, axis=1), dtype=np.float64)
        return torch.as_tensor(block, device=self.device) if on_device else block

    def _pose_xforms(self, pose, B):
        """B MVX_XF_POSE_PTR records, record b pointing at row b of the packed poses."""
        xfs = (_lib.MvxXform * B)()
        base = self._ptr(pose)
        for b in range(B):
            xfs[b].flags = _lib.MVX_XF_POSE_PTR
            xfs[b].center_ptr = base + 80 * b
        return xfs

    def forward_posed_batch(self, coords, offsets, centers, quaternions, translations, channels, radii, num_channels=None,
                            out_grid=None):
        """forward_batch with one explicit rigid pose per molecule instead of random transforms: atom x of molecule b lands at
        p = q_b (x - c_b) conj(q_b) + t_b - the centre subtracted, the sandwich product in the random rotation's operation order
        with q as given (the linear part scales by |q|^2: normalise q in torch beforehand for a pure rotation, autograd carries
        the normalisation), then t, rounded to float32, added once.

        quaternions (B,4) as (q0, q1, q2, q3); translations (B,3); centers (B,3) | None (c = 0); any float dtype, torch tensors
        or numpy arrays. Tensors on this voxelizer's device are handed over by pointer: no host round trip, no synchronisation.
        The other arguments are forward_batch's. On a differentiable voxelizer, `centers`, `quaternions` and `translations`
        that require grad get dL/dc, dL/dq and dL/dt (mvx_pose_grad_batch; deterministic), next to the gradients of coords,
        features, radii and sigma. q = 0 gives non-finite pose gradients."""
        B = np.asarray(offsets).shape[0] - 1
        pose = self._pack_pose(B, centers, quaternions, translations, self._on_device(coords))
        return self._forward_batch(coords, offsets, None, channels, radii, num_channels, out_grid,
                                   xforms=(self._pose_xforms(pose, B), None), fresh_inputs=_is_torch(pose), pose=pose)

    def forward_posed_views(self, coords, centers, quaternions, translations, channels, radii, num_channels=None, out_grid=None):
        """forward_views with one explicit rigid pose per view instead of a centre and a random transform: B poses of ONE
        shared cloud (docking poses of a ligand, the 24 cube rotations, poses under refinement) without B copies of it - bit for
        bit forward_posed_batch on the cloud repeated B times. centers (B,3), quaternions (B,4), translations (B,3) as there.
        On a differentiable voxelizer every view's pose gets its own gradient and the per-atom gradients of all views sum into
        the shared tensors. Synchronises the stream once, as forward_views does."""
        return self._forward_views(coords, centers, channels, radii, num_channels, out_grid, posed=(quaternions, translations))

    def select_posed_views(self, coords, centers, quaternions, translations, channels=None, radii=None):
        """select_views for explicit poses: the atoms each pose of forward_posed_views keeps, as (index, offsets)."""
        B = int(centers.shape[0])
        pose = self._pack_pose(B, centers, quaternions, translations, self._on_device(coords))
        return self._select_views(coords, centers, channels, radii, xforms=(self._pose_xforms(pose, B), None))

    # ------------------------------------------------------------------------------------------
    # SUMS (one grid for a whole batch: mvx_forward_sum_batch)
    def forward_sum(self, coords, offsets, centers, channels, radii, weights=None, num_channels=None, out_grid=None,
                    accumulate=False, random_translation=0.0, random_rotation=False):
        """ONE (C,D,H,W) float32 grid: the sum over the B molecules, weighted or not, of the grids forward_batch would write
        with the same arguments - without writing them (an occupancy map of a trajectory, of conformers, of docking poses).
        The sum runs over the atoms in the caller's order, molecule after molecule, in the float32 fma chain the kernels run
        inside one molecule: deterministic, independent of how the batch is cut, and for molecules that are only centred bit
        for bit the per-molecule forward on the one merged molecule.

        Arguments, checks, RNG order and records are forward_batch's; host arrays are moved to the device. Needs
        output="torch". weights: None, (B,) one per molecule (expanded per atom on the device; this reading wins where B equals
        the atom count) or (sumN,) one per atom, converted to float32: atom n contributes float32(weights[n] * w[n, c]) * rho.
        out_grid: a contiguous float32 (C,D,H,W) tensor on this device, whatever the voxelizer's grid_dtype / grid_layout;
        fully overwritten, or - accumulate=True, which needs out_grid - read and updated (a batch of no atoms leaves it
        untouched). Returns the grid. The result is NOT part of the autograd graph: inputs that require grad are read as values.
        Not supported (NotImplementedError; use forward_batch(...).sum(0)): precision 64, channel-wise radii with features,
        dimensions that are no multiple of 4, and blockdims that cut through the kernels' 2 x 4 x 8 sub-tiles."""
        return self._forward_sum(coords, offsets, centers, channels, radii, weights, num_channels, out_grid, accumulate,
                                 random_translation, random_rotation)

    def forward_posed_sum(self, coords, offsets, centers, quaternions, translations, channels, radii, weights=None,
                          num_channels=None, out_grid=None, accumulate=False):
        """forward_sum with one explicit rigid pose per molecule (forward_posed_batch's arguments and records): the (weighted)
        sum of the grids of B poses in one float32 (C,D,H,W) grid. Not part of the autograd graph."""
        self._sum_guard(channels)
        B = np.asarray(offsets).shape[0] - 1
        pose = self._pack_pose(B, centers, quaternions, translations, True)
        return self._forward_sum(coords, offsets, None, channels, radii, weights, num_channels, out_grid, accumulate,
                                 xforms=(self._pose_xforms(pose, B), None), pose=pose)

    def _sum_guard(self, channels):
        """What a summed call refuses before it looks at anything else: the configurations voxelize_sum_kernel does not serve."""
        if self.output != "torch":
            raise ValueError("forward_sum / forward_posed_sum need output='torch': the grid is a tensor on the voxelizer's device")
        alt = "use forward_batch(...).sum(0) (forward_posed_batch(...).sum(0)) instead"
        if getattr(self, "precision", 32) == 64:
            raise NotImplementedError(f"forward_sum does not support precision 64 (float32 sums only): {alt}")
        if self.is_radii_type_channel_wise and channels is not None and getattr(channels, "ndim", 1) == 2:
            raise NotImplementedError(f"forward_sum does not support channel-wise radii with features: {alt}")
        D, bd = int(self.dimension), int(getattr(self, "blockdim", None) or 8)
        if D % 4 != 0:
            raise NotImplementedError(f"forward_sum does not support a dimension that is no multiple of 4 (got {D}): {alt}")
        if -(-D // bd) > 1 and bd % 8 != 0:  # (mvx_plan.lane_range: reference blocks that cut through 2 x 4 x 8 sub-tiles)
            raise NotImplementedError(f"forward_sum does not support blockdim={bd} at dimension {D} (per-lane ranges): {alt}")

    def _sum_weights(self, weights, offsets, N):
        """The weights of a summed call as the library reads them: None, or (sumN,) float32 on this device."""
        if weights is None:
            return None
        B = offsets.shape[0] - 1
        w = (weights.detach() if _is_torch(weights) else torch.as_tensor(np.asarray(weights))).to(device=self.device, dtype=torch.float32)
        shape = tuple(w.shape)
        assert shape in ((B,), (N,)), f"weights does not match dimension: {shape} vs {(B,)} or {(N,)}"
        if shape == (B,):
            lengths = torch.as_tensor(np.diff(offsets), device=self.device)
            w = torch.repeat_interleave(w, lengths, output_size=N)
        return w.contiguous()

    def _forward_sum(self, coords, offsets, centers, channels, radii, weights=None, num_channels=None, out_grid=None,
                     accumulate=False, random_translation=0.0, random_rotation=False, xforms=None, pose=None):
        """forward_sum's body, in the order of _forward_batch. xforms / pose: the posed form's records and packed poses."""
        self._sum_guard(channels)
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, _ = self._scalar_radius(radii)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.shape[0] - 1
        assert offsets[0] == 0 and offsets[-1] == coords.shape[0], "offsets must span coords"
        kind, C_ = self._batch_kind(channels, radii, num_channels)
        self._check_args_batch(coords, channels, kind, radii, C_)
        if accumulate and out_grid is None:
            raise ValueError("accumulate=True needs out_grid: there is nothing to add to")
        if out_grid is not None:
            assert tuple(getattr(out_grid, "shape", ())) == self.grid_dimension(C_), (
                f"Output grid dimension incorrect: {tuple(getattr(out_grid, 'shape', ()))} vs {self.grid_dimension(C_)}")
            if not (self._on_device(out_grid) and out_grid.dtype == torch.float32 and out_grid.is_contiguous()):
                raise ValueError("out_grid of forward_sum must be a contiguous float32 tensor on this voxelizer's device")
        with torch.no_grad():
            w = self._sum_weights(weights, offsets, int(coords.shape[0]))
            c, ch, r, in_kind, keep = self._prepare_inputs(self._device_coords(coords), channels, kind, radii)
            r, _ = self._pad_type_radii(r, kind, C_)
            xfs, _ = self._call_xforms(B, centers, in_kind, random_translation, random_rotation, keep, xforms)
            rs = float(radii) if _np_isscalar(radii) else 0.0
            return self._sum_call(kind or "single", c, ch, r, rs, offsets, xfs, B, C_, w, out_grid, accumulate)

    def _sum_call(self, mode, c, ch, r, rs, offsets, xfs, B, C_, w, out, accumulate):
        """One mvx_forward_sum_batch call on device arrays, on the current stream; out None: a new grid."""
        if out is None:
            out = torch.empty(self.grid_dimension(C_), dtype=torch.float32, device=self.device)
        _lib.check(self._lib.mvx_forward_sum_batch(
            self._handle, _lib.MODES[mode], self._ptr(c), self._ptr(ch), self._ptr(r), rs, self._radii_type_code(),
            offsets.ctypes.data, None if xfs is None else C.addressof(xfs), B, C_, self._ptr(w), self._ptr(out),
            1 if accumulate else 0, self._stream()))
        return out

    def forward_views_sum(self, coords, centers, channels, radii, weights=None, num_channels=None, out_grid=None, accumulate=False,
                          random_translation=0.0, random_rotation=False):
        """ONE (C,D,H,W) float32 grid: the sum over B boxes of ONE shared point cloud, weighted or not, of the grids forward_views
        would write with the same arguments - without the B copies of the cloud and without the B grids (the occupancy map of
        256 boxes of a pocket). Bit for bit forward_sum on the cloud repeated B times with the same centres and transforms:
        each view's atoms are selected on the device (forward_views' selection: culled atoms add nothing), gathered into a
        compact batch and summed by forward_sum's kernel in view and atom order.

        Arguments, checks, RNG order and records are forward_views': coords (N,3), centers (B,3), channels (N,C) float | (N,) int
        | None, radii per this voxelizer's radii_type; a random transform is drawn per view in view order, exactly as
        forward_views draws it. Host arrays are moved to the device. Needs output="torch". weights: None or (B,) one per view,
        converted to float32 and expanded per selected atom on the device, as (B,) molecule weights are in forward_sum.
        out_grid / accumulate and the configurations that are not supported (NotImplementedError) are forward_sum's: a
        contiguous float32 (C,D,H,W) tensor on this device, fully overwritten, or - accumulate=True, which needs out_grid - read
        and updated; a cloud of no atoms, or views that select none, write zeros or leave an accumulated grid untouched.
        Synchronises the stream once, as forward_views does. With set_sum_parts(K > 1) the views are cut into parts (see there).
        Returns the grid. The result is NOT part of the autograd graph: inputs that require grad are read as values."""
        return self._forward_views_sum(coords, centers, channels, radii, weights, num_channels, out_grid, accumulate,
                                       random_translation, random_rotation)

    def forward_posed_views_sum(self, coords, centers, quaternions, translations, channels, radii, weights=None, num_channels=None,
                                out_grid=None, accumulate=False):
        """forward_views_sum with one explicit rigid pose per view (forward_posed_views' arguments and records): the (weighted)
        sum of the grids of B poses of ONE shared cloud - 1 024 docking poses of a ligand - in one float32 (C,D,H,W) grid, bit
        for bit forward_posed_sum on the cloud repeated B times. Not part of the autograd graph."""
        self._sum_guard(channels)
        return self._forward_views_sum(coords, centers, channels, radii, weights, num_channels, out_grid, accumulate,
                                       posed=(quaternions, translations))

    def _forward_views_sum(self, coords, centers, channels, radii, weights=None, num_channels=None, out_grid=None, accumulate=False,
                           random_translation=0.0, random_rotation=False, posed=None):
        """forward_views_sum's body, in the order of _forward_sum and _forward_views. posed: (quaternions, translations)."""
        self._sum_guard(channels)
        kind, C_, cradii, _ = self._views_args(coords, centers, channels, radii, num_channels)
        B = int(centers.shape[0])
        if accumulate and out_grid is None:
            raise ValueError("accumulate=True needs out_grid: there is nothing to add to")
        if out_grid is not None:
            assert tuple(getattr(out_grid, "shape", ())) == self.grid_dimension(C_), (
                f"Output grid dimension incorrect: {tuple(getattr(out_grid, 'shape', ()))} vs {self.grid_dimension(C_)}")
            if not (self._on_device(out_grid) and out_grid.dtype == torch.float32 and out_grid.is_contiguous()):
                raise ValueError("out_grid of forward_sum must be a contiguous float32 tensor on this voxelizer's device")
        with torch.no_grad():
            w = None
            if weights is not None:
                w = (weights.detach() if _is_torch(weights) else torch.as_tensor(np.asarray(weights))).to(
                    device=self.device, dtype=torch.float32).contiguous()
                assert tuple(w.shape) == (B,), f"weights does not match dimension: {tuple(w.shape)} vs {(B,)}"
            c, ch, r, in_kind, keep = self._views_inputs(self._device_coords(coords), channels, kind, cradii, C_)
            if posed is None:
                xfs, _ = self._make_xforms(B, centers, in_kind, random_translation, random_rotation, keep)
            else:
                pose = self._pack_pose(B, centers, posed[0], posed[1], True)
                keep.append(pose)
                xfs = self._pose_xforms(pose, B)
            out = out_grid
            if out is None:
                out = torch.empty(self.grid_dimension(C_), dtype=torch.float32, device=self.device)
            rs = float(cradii) if _np_isscalar(cradii) else 0.0
            _lib.check(self._lib.mvx_forward_views_sum(
                self._handle, _lib.MODES[kind or "single"], self._ptr(c), self._ptr(ch), self._ptr(r), rs, self._radii_type_code(),
                int(c.shape[0]), C_, C.addressof(xfs), B, self._ptr(w), self._ptr(out), 1 if accumulate else 0, self._stream()))
            return out

    def set_sum_parts(self, parts: int):
        """Opt-in split of every summed call of this voxelizer (forward_sum, forward_posed_sum, forward_views_sum,
        forward_posed_views_sum and the field gradient of the score calls) into K = `parts` parts, 1 ... 64; 1, the default, is
        the one-pass sum. A summed call runs one workgroup per (slab, 32 channels) that walks all B molecules: many small
        molecules leave most of the card idle. With K > 1 the call's B molecules (views) are cut into parts of q = ceil(B / K)
        molecules, part g = [g q, min(B, (g + 1) q)), each summed into a partial grid S_g of its own (G = ceil(B / q) extra
        (C,D,H,W) float32 grids of workspace), and the result is the float32 chain (out_grid with accumulate=True, else 0)
        + S_0 + S_1 + ... + S_{G-1}, one rounding per add in that order. Deterministic, no atomics, independent of how the call
        is cut into molecule chunks - but the bits DIFFER from those of parts = 1, and therefore from the merged-molecule and
        split-call identities forward_sum documents."""
        _lib.check(self._lib.mvx_set_sum_parts(self._handle, int(parts)))
        self._sum_parts = int(parts)

    @property
    def sum_parts(self) -> int:
        """The number of parts summed calls are cut into (set_sum_parts); 1: the one-pass sum."""
        return getattr(self, "_sum_parts", 1)

    # ------------------------------------------------------------------------------------------
    # SCORES (poses against a constant field grid without the grids: mvx_score_batch)
    def score_batch(self, coords, offsets, centers, channels, radii, field, num_channels=None, random_translation=0.0,
                    random_rotation=False, per_atom=False):
        """S_b = sum(field * grid_b) for the B grids forward_batch would write with the same arguments - without writing them.
        The score is linear in the grid, so one walk of the atoms' boxes over the one field gives every molecule's score, the
        per-atom contributions and, on a differentiable voxelizer, dS/dcoords and dS/dfeatures (mvx_score_batch).

        field: (C,D,H,W), shared by all molecules, or (B,C,D,H,W), one per molecule; converted with
        `.to(device, grid_dtype).contiguous()` and read as NCDHW on a channels-last voxelizer too. A constant: a field that
        requires grad raises NotImplementedError - unless the voxelizer was made with field_grad=True and the field is the
        shared (C,D,H,W) one: backward() then returns dL/dfield, the grids summed with one weight per atom (forward_sum).
        The other arguments are forward_batch's (transforms drawn per molecule in the same RNG order); host arrays are moved to
        the device. Needs output="torch".
        Returns scores (B,) float64 on this device; with per_atom=True (scores, atom_scores (sumN,) float64) where
        scores[b] = sum of molecule b's atom_scores. Deterministic: no atomics, a molecule's values do not depend on its batch.
        On a differentiable voxelizer coords, features and centers that require grad get their gradients from the same walk;
        backward() only scales the saved rows. Gradients with respect to radii and sigma are not supported here."""
        return self._score_batch(coords, offsets, centers, channels, radii, field, num_channels, random_translation,
                                 random_rotation, per_atom)

    def score_posed_batch(self, coords, offsets, centers, quaternions, translations, channels, radii, field, num_channels=None,
                          per_atom=False):
        """score_batch with one explicit rigid pose per molecule (forward_posed_batch's arguments and records): the scores of
        B poses against `field`. On a differentiable voxelizer `centers`, `quaternions` and `translations` that require grad get
        dS/dc, dS/dq and dS/dt (mvx_pose_grad_batch on the scaled per-atom gradients)."""
        self._score_guard(field, True)
        B = np.asarray(offsets).shape[0] - 1
        pose = self._pack_pose(B, centers, quaternions, translations, True)
        return self._score_batch(coords, offsets, None, channels, radii, field, num_channels, per_atom=per_atom,
                                 xforms=(self._pose_xforms(pose, B), None), pose=pose)

    def _score_guard(self, field, shared_field_grad=False):
        """What a score call refuses before it looks at anything else. shared_field_grad: the call is one of those that, on a
        field_grad voxelizer, give a shared (C, D, H, W) field its gradient (score_batch / score_posed_batch)."""
        if self.output != "torch":
            raise ValueError("score_batch / score_posed_batch need output='torch': the scores are tensors on the voxelizer's device")
        if _is_torch(field) and field.requires_grad:
            if shared_field_grad and getattr(self, "field_grad", False) and field.dim() == 4:
                return  # dL/dfield = the weighted summed grid (forward_sum): _ScoreFunction.backward
            raise NotImplementedError("gradients with respect to the field are not supported: dS/dfield is the grid itself - "
                                      "use forward_batch (forward_posed_batch) and (grid * field).sum() for them")

    def _score_no_density_grads(self, radii, rten):
        """Radius and sigma gradients of the score are out of scope: a radii, sigma or scalar-radius tensor that requires grad."""
        if not self.differentiable or not torch.is_grad_enabled():
            return
        for what, x in (("radii", radii), ("sigma", self.sigma_tensor), ("a scalar radius", rten)):
            if _is_torch(x) and x.requires_grad:
                raise NotImplementedError(f"score calls give no gradient with respect to {what}: detach it, or use forward_batch "
                                          "and (grid * field).sum() for that gradient")

    def _check_args_score(self, field, B, C_):
        shape = tuple(getattr(field, "shape", ()))
        one = self.grid_dimension(C_)
        assert shape in (one, (B,) + one), f"field does not match dimension: {shape} vs {one} or {(B,) + one}"
        return len(shape) == 5

    def _score_batch(self, coords, offsets, centers, channels, radii, field, num_channels=None, random_translation=0.0,
                     random_rotation=False, per_atom=False, xforms=None, pose=None):
        """score_batch's body, in the order of _forward_batch. xforms / pose: the posed form's records and packed poses."""
        self._score_guard(field, True)
        fgrad = (_is_torch(field) and field.requires_grad and getattr(self, "field_grad", False) and self.differentiable
                 and torch.is_grad_enabled())
        if fgrad:  # (what forward_sum cannot serve is refused now, not in backward())
            self._sum_guard(channels)
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        self._score_no_density_grads(radii, rten)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.shape[0] - 1
        assert offsets[0] == 0 and offsets[-1] == coords.shape[0], "offsets must span coords"
        kind, C_ = self._batch_kind(channels, radii, num_channels)
        self._check_args_batch(coords, channels, kind, radii, C_)
        per_mol = self._check_args_score(field, B, C_)
        grad = self._grad_wanted(coords, channels if kind == "features" else None, centers if pose is None else pose, None, None)
        if grad and centers is not None:
            centers = self._grad_center(centers)
        c, ch, r, in_kind, keep = self._prepare_inputs(self._device_coords(coords), channels, kind, radii)
        r, _ = self._pad_type_radii(r, kind, C_)
        xfs, dev_cen = self._call_xforms(B, centers, in_kind, random_translation, random_rotation, keep, xforms)
        F = self._field_tensor(field)
        rs = float(radii) if _np_isscalar(radii) else 0.0
        N = c.shape[0]
        mode = kind or "single"
        feat = ch if kind == "features" else None
        need_gf = grad and feat is not None and feat.requires_grad

        def call():
            scores = torch.empty(B, dtype=torch.float64, device=self.device)
            atoms = torch.empty(N, dtype=torch.float64, device=self.device) if per_atom else None
            gc = torch.empty((N, 3), dtype=torch.float64, device=self.device) if grad else None
            gf = torch.empty((N, C_), dtype=self._tfp, device=self.device) if need_gf else None
            _lib.check(self._lib.mvx_score_batch(
                self._handle, _lib.MODES[mode], self._ptr(c), self._ptr(ch), self._ptr(r), rs, self._radii_type_code(),
                offsets.ctypes.data, None if xfs is None else C.addressof(xfs), B, C_, self._ptr(F),
                C_ * self.dimension ** 3 if per_mol else 0, self._ptr(scores), self._ptr(atoms), self._ptr(gc), self._ptr(gf),
                self._stream()))
            return scores, atoms, gc, gf

        if not grad and not fgrad:
            scores, atoms, _, _ = call()
            return (scores, atoms) if per_atom else scores
        spec = dict(offsets=offsets, xforms=xfs, B=B)
        if fgrad:  # the call as forward_sum repeats it in backward(): same offsets and records, the random draws included
            spec.update(mode=mode, channels=ch, radii=r, rs=rs, C=C_, keep=keep)
        cen = dev_cen if (_is_torch(dev_cen) and self._on_device(dev_cen)) else None
        out = _ScoreFunction.apply(self, call, spec, per_atom, c, feat, cen, pose, field if fgrad else None)
        return out if per_atom else out[0]

    # ------------------------------------------------------------------------------------------
    # SCORES OF VIEWS (many poses or boxes of one shared cloud against a field: mvx_score_views / mvx_views_reduce)
    def score_views(self, coords, centers, channels, radii, field, num_channels=None, random_translation=0.0,
                    random_rotation=False, per_atom=False):
        """S_b = sum(field * grid_b) for the B grids forward_views would write with the same arguments - without the grids and
        without B copies of the cloud: each view's atoms are selected on the device, gathered into a compact batch and walked
        once over the field (mvx_score_views). The values are score_batch's, bit for bit, on coords[index], the gathered
        channels and offsets of select_views.

        coords (N,3), centers (B,3), channels and radii as forward_views (transforms drawn per view in its RNG order); field
        (C,D,H,W), shared by all views, or (B,C,D,H,W), one per view, converted as score_batch converts it; host arrays are
        moved to the device. Needs output="torch". Returns scores (B,) float64; with per_atom=True (scores, atom_scores, index,
        offsets): atom_scores (total,) float64 in selection order - atom_scores[k] belongs to atom index[k] of its view - and
        (index, offsets) as select_views returns them. Without gradients and without per_atom the call is one library call
        (one stream synchronisation, for the selection). On a differentiable voxelizer coords, features and centers that
        require grad get their gradients: the per-(view, atom) rows of the one walk are saved, backward() scales them and sums
        them onto the shared atoms with mvx_views_reduce - deterministic (no atomics, a fixed order of additions), so two runs
        give the same bits. Gradients with respect to radii, sigma and the field are not supported here."""
        return self._score_views(coords, centers, channels, radii, field, num_channels, random_translation, random_rotation,
                                 per_atom)

    def score_posed_views(self, coords, centers, quaternions, translations, channels, radii, field, num_channels=None,
                          per_atom=False):
        """score_views with one explicit rigid pose per view (forward_posed_views' arguments and records): the scores of B
        poses of ONE shared cloud against `field`. On a differentiable voxelizer `centers`, `quaternions` and `translations`
        that require grad get dS/dc, dS/dq and dS/dt per view (mvx_pose_grad_batch on the scaled rows)."""
        self._score_guard(field)
        return self._score_views(coords, centers, channels, radii, field, num_channels, per_atom=per_atom,
                                 posed=(quaternions, translations))

    def views_reduce(self, rows, index, offsets, num_atoms):
        """Rows of a selection summed back onto the shared atoms: out[n] = the sum of rows[k] over the slots k with
        index[k] == n, one slot per view that holds atom n. rows (total,) or (total, W) float32 | float64 on this device,
        (index, offsets) as select_views returns them; returns (num_atoms,) or (num_atoms, W) of the rows' dtype. Accumulated in
        float64, rounded once; no atomics and a fixed order of additions (mvx_views_reduce): two runs give the same bits."""
        assert _is_torch(rows) and self._on_device(rows) and rows.dtype in (torch.float32, torch.float64), (
            "rows should be a float32 or float64 tensor on this voxelizer's device")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        total = int(offsets[-1]) if offsets.shape[0] else 0
        assert rows.ndim in (1, 2) and rows.shape[0] == total, f"rows does not match the selection: {tuple(rows.shape)} vs {(total, 'W')}"
        assert int(index.shape[0]) == total and index.dtype == torch.int64, "index does not match offsets"
        flat = rows.ndim == 1
        W = 1 if flat else int(rows.shape[1])
        r = rows.reshape(total, W).contiguous()
        out = torch.empty((int(num_atoms), W), dtype=r.dtype, device=self.device)
        if W > 0:
            idx = index if index.is_contiguous() else index.contiguous()
            _lib.check(self._lib.mvx_views_reduce(
                self._handle, self._ptr(idx) if total else None, offsets.ctypes.data, offsets.shape[0] - 1, int(num_atoms),
                self._ptr(r) if total else None, W, _lib.MVX_ROW_DOUBLE if r.dtype == torch.float64 else _lib.MVX_ROW_FLOAT,
                self._ptr(out) if num_atoms else None, self._stream()))
        return out.reshape(int(num_atoms)) if flat else out

    def _score_views(self, coords, centers, channels, radii, field, num_channels=None, random_translation=0.0,
                     random_rotation=False, per_atom=False, posed=None):
        """score_views' body, in the order of _score_batch. posed: (quaternions, translations) of score_posed_views."""
        self._score_guard(field)
        kind, C_, cradii, rten = self._views_args(coords, centers, channels, radii, num_channels)
        self._score_no_density_grads(cradii, rten)
        B = int(centers.shape[0])
        per_view = self._check_args_score(field, B, C_)
        pose = self._pack_pose(B, centers, posed[0], posed[1], True) if posed is not None else None
        grad = self._grad_wanted(coords, channels if kind == "features" else None, centers if pose is None else pose, None, None)
        c, ch, r, in_kind, keep = self._views_inputs(self._device_coords(coords), channels, kind, cradii, C_)
        if pose is None:
            xfs, dev_cen = self._make_xforms(B, self._grad_center(centers) if grad else centers, in_kind, random_translation,
                                             random_rotation, keep)
        else:
            xfs, dev_cen = self._pose_xforms(pose, B), None
        F = self._field_tensor(field)
        rs = float(cradii) if _np_isscalar(cradii) else 0.0
        N = int(c.shape[0])
        mode = kind or "single"
        feat = ch if kind == "features" else None
        need_gf = grad and feat is not None and feat.requires_grad
        stride = C_ * self.dimension ** 3 if per_view else 0

        def call(index, offsets):
            """One mvx_score_views call: with a selection, the per-row outputs this call needs; without, scores alone."""
            total = 0 if index is None else int(offsets[-1])
            scores = torch.empty(B, dtype=torch.float64, device=self.device)
            atoms = torch.empty(total, dtype=torch.float64, device=self.device) if (per_atom and index is not None) else None
            gc = torch.empty((total, 3), dtype=torch.float64, device=self.device) if (grad and index is not None) else None
            gf = torch.empty((total, C_), dtype=self._tfp, device=self.device) if (need_gf and index is not None) else None
            # (an empty selection: an empty tensor has no address, but a non-null index is what says "selected" to the library)
            some = index is not None and total > 0
            pad = torch.empty(1, dtype=torch.int64, device=self.device) if (index is not None and not some) else None
            _lib.check(self._lib.mvx_score_views(
                self._handle, _lib.MODES[mode], self._ptr(c), self._ptr(ch), self._ptr(r), rs, self._radii_type_code(), N, C_,
                C.addressof(xfs), B, None if index is None else (index if some else pad).data_ptr(),
                offsets.ctypes.data if index is not None else None, self._ptr(F), stride, self._ptr(scores),
                self._ptr(atoms) if some else None, self._ptr(gc) if some else None, self._ptr(gf) if some else None,
                self._stream()))
            return scores, atoms, gc, gf

        if not grad and not per_atom:
            return call(None, None)[0]
        with torch.no_grad():
            index, offsets = self._select(c, ch if kind == "types" else None, r, rs, kind, C_, xfs, B, in_kind)
        if not grad:
            scores, atoms, _, _ = call(index, offsets)
            return scores, atoms, index, offsets
        spec = dict(offsets=offsets, xforms=xfs, B=B, N=N, index=index)
        cen = dev_cen if (_is_torch(dev_cen) and self._on_device(dev_cen)) else None
        out = _ScoreViewsFunction.apply(self, lambda: call(index, offsets), spec, per_atom, c, feat, cen, pose)
        return (out[0], out[1], index, offsets) if per_atom else out[0]

    # ------------------------------------------------------------------------------------------
    # autograd (differentiable=True): the forward call runs inside _VoxelizeFunction, the backward is mvx_backward_batch
    def _grad_wanted(self, coords, features, center, radii, out_grid, rten=None) -> bool:
        """True when this call must record an autograd graph: differentiable voxelizer, grad mode on, and coords / features /
        center (or, with radii_grad, radii; with sigma_grad, the sigma tensor) a tensor that requires grad. `rten`: the
        scalar-radius tensor of the call (_scalar_radius). Raises for what the backward pass does not cover."""
        if not self.differentiable or torch is None or not torch.is_grad_enabled():
            return False
        if _is_torch(radii) and radii.requires_grad and not self.radii_grad:
            raise NotImplementedError("gradients with respect to radii are not supported unless the voxelizer is created with "
                                      "radii_grad=True")
        tracked = [x for x in (coords, features, center, radii) if _is_torch(x) and x.requires_grad]
        # sigma and a scalar radius travel as host values: their tensors may live anywhere
        scalars = [x for x in (self.sigma_tensor, rten) if x is not None and x.requires_grad]
        if not tracked and not scalars:
            return False
        for x in tracked + [coords]:
            if not self._on_device(x):
                raise NotImplementedError(
                    f"differentiable calls need coords and every tensor that requires grad on this voxelizer's device "
                    f"({self.device}); move them there first (got {getattr(x, 'device', 'a host array')})")
        if out_grid is not None:
            raise ValueError("out_grid cannot be combined with a recorded autograd graph: let the call allocate the grid")
        return True

    def _grad_center(self, center):
        """A device centre as the call hands it to the library (float64, contiguous); the conversion is recorded by autograd."""
        if self._on_device(center) and not (center.dtype == torch.float64 and center.is_contiguous()):
            return center.to(torch.float64).contiguous()
        return center

    @staticmethod
    def _xform_copy(xf):
        """The mvx_xform record of a single-molecule call (the voxelizer reuses its own), or None."""
        return None if xf is None else _lib.MvxXform.from_buffer_copy(_lib.MvxXform.from_address(xf))

    def _autograd(self, launch, ret, mode, c, f, center, types, r, rs, offsets, xforms, B, C_, rten=None, pose=None):
        cen = center if (_is_torch(center) and self._on_device(center)) else None
        # radii_grad: the radii as the call hands them to the library (dtype conversion / type padding recorded by autograd)
        rin = r if (self.radii_grad and _is_torch(r) and r.requires_grad) else None
        spec = dict(mode=mode, types=types, radii=r, rs=rs, offsets=np.ascontiguousarray(offsets, np.int64), xforms=xforms,
                    B=B, C=C_, settings=self._grad_settings())
        sig = self.sigma_tensor
        sig = sig if (sig is not None and sig.requires_grad) else None
        rsc = rten if (rten is not None and rten.requires_grad) else None
        return _VoxelizeFunction.apply(self, launch, ret, spec, c, f, cen, rin, sig, rsc, pose)

    def _grad_settings(self):
        """What the backward reads from the voxelizer rather than from the call: density, sigma and radii type."""
        return (self.density_type, float(getattr(self, "_sigma", 0.5)) if self.is_density_type_gaussian else None,
                self.radii_type)

    def _backward(self, spec, c, f, grad, need_features, need_radii=False, need_sigma=False, need_rscalar=False):
        """(dL/dcoords (N,3) float64, dL/dfeatures (N,C) or None, dL/dradii shaped and typed like the call's radii or None,
        dL/dsigma and dL/d(scalar radius) as 0-dim float64 device tensors or None) for dL/dgrid = grad, on the current stream."""
        now = self._grad_settings()
        if now != spec["settings"]:
            raise RuntimeError(
                "the voxelizer's density / sigma / radii type changed between the forward call and backward() "
                f"(forward: {spec['settings']}, now: {now}); the gradients would be those of another grid. Restore the "
                "settings before backward(), or use one voxelizer per setting")
        g = grad.to(device=self.device, dtype=self._gdt).contiguous()
        gc = torch.empty((c.shape[0], 3), dtype=torch.float64, device=self.device)
        gf = torch.empty((c.shape[0], spec["C"]), dtype=self._tfp, device=self.device) if need_features else None
        r = spec["radii"]
        gr = torch.zeros(r.shape[0], dtype=torch.float64, device=self.device) if need_radii else None
        gs = torch.zeros(2, dtype=torch.float64, device=self.device) if (need_sigma or need_rscalar) else None  # [sigma, radius]
        gsig = gs[0] if need_sigma else None
        grs = gs[1] if need_rscalar else None
        if c.shape[0] == 0:  # no atoms: no gradient rows (the library would see null outputs); channel-wise radii get zeros
            return gc, gf, None if gr is None else gr.to(r.dtype), gsig, grs
        mode = spec["mode"]
        ch = f if mode == "features" else spec["types"]
        xf = spec["xforms"]
        args = (self._handle, _lib.MODES[mode], self._ptr(c), self._ptr(ch), self._ptr(r), spec["rs"],
                self._radii_type_code(), spec["offsets"].ctypes.data, None if xf is None else C.addressof(xf), spec["B"],
                spec["C"], self._ptr(g), self._ptr(gc), self._ptr(gf))
        if gs is not None:  # the radius walk with its partials reduced over the call: dL/dsigma, dL/d(scalar radius)
            rc = self._lib.mvx_backward_density_batch(*args, self._ptr(gr), gs.data_ptr() if need_sigma else None,
                                                      gs.data_ptr() + 8 if need_rscalar else None, self._stream())
        elif gr is None:
            rc = self._lib.mvx_backward_batch(*args, self._stream())
        else:  # one walk: the same coordinate / feature bits as mvx_backward_batch, and dL/dradii
            rc = self._lib.mvx_backward_radii_batch(*args, self._ptr(gr), self._stream())
        _lib.check(rc)
        return gc, gf, None if gr is None else gr.to(r.dtype), gsig, grs

    def _pose_backward(self, spec, c, gc):
        """dL/dpose (B, 10) float64 = [dL/dc | dL/dq | dL/dt] per molecule from the call's dL/dcoords, on the current stream."""
        gp = torch.zeros((spec["B"], 10), dtype=torch.float64, device=self.device)
        if c.shape[0] == 0 or spec["B"] == 0:
            return gp
        _lib.check(self._lib.mvx_pose_grad_batch(self._handle, self._ptr(c), self._ptr(gc), spec["offsets"].ctypes.data,
                                                 C.addressof(spec["xforms"]), spec["B"], gp.data_ptr(), self._stream()))
        return gp

    # ------------------------------------------------------------------------------------------
    # measurement hooks used by bench.py (HIP events around the voxelize kernel on the launch stream)
    def debug_option(self, name: str, value: int):
        """Testing aid (mvx_debug_set_option): force code paths production sizes rarely reach."""
        _lib.check(self._lib.mvx_debug_set_option(self._handle, name.encode(), int(value)))

    def last_plan(self) -> dict:
        """Testing aid (mvx_debug_last_plan): the plan of the last forward call on this handle, debug options applied."""
        p = _lib.MvxPlan()
        _lib.check(self._lib.mvx_debug_last_plan(self._handle, C.byref(p)))
        return {name: getattr(p, name) for name, _ in _lib.MvxPlan._fields_ if name != "reserved"}

    def set_profiling(self, enable: bool):
        _lib.check(self._lib.mvx_set_profiling(self._handle, 1 if enable else 0))

    def read_kernel_times_ms(self):
        """Durations (ms) of the voxelize kernel for every launch since profiling was enabled / last read."""
        buf = (C.c_float * 1024)()
        n = C.c_int32(0)
        _lib.check(self._lib.mvx_profile_read(self._handle, buf, 1024, C.byref(n)))
        return [buf[i] for i in range(n.value)]

    def last_kernel_ms(self) -> float:
        ms = C.c_float(0.0)
        _lib.check(self._lib.mvx_last_kernel_ms(self._handle, C.byref(ms)))
        return ms.value

    @staticmethod
    def do_random_transform(coords, center, random_translation, random_rotation):
        from .transform import do_random_transform

        return do_random_transform(coords, center, random_translation, random_rotation)


def _row_upstream(gs, ga, lengths, total):
    """dL/ds of every saved row of a score call: dL/dS of the row's molecule (view) plus, with per_atom, dL/ds_n."""
    up = torch.zeros(total, dtype=torch.float64, device=lengths.device)
    if gs is not None:
        up = torch.repeat_interleave(gs.to(torch.float64), lengths, output_size=total)
    if ga is not None:
        up = up + ga.to(torch.float64)
    return up


def _center_grad(g, cen, lengths):
    """p = M (coords - center) + t: dL/dcenter = -sum of dL/dcoords over the molecule. lengths: the molecules' atom counts on
    g's device, or None: all rows belong to the one centre."""
    if lengths is None:
        return -g.sum(0).reshape(cen.shape)
    return -torch.segment_reduce(g, "sum", lengths=lengths, axis=0).reshape(cen.shape)


if torch is not None:

    class _VoxelizeFunction(torch.autograd.Function):
        """grid = voxelize(coords, features, center, radii, sigma, scalar radius, packed poses): the forward call as it runs without autograd
        (same kernels, same bits); backward = mvx_backward_batch (mvx_backward_radii_batch with radii, mvx_backward_density_batch
        with sigma or a scalar radius) from the saved inputs and the call's mvx_xform records."""

        @staticmethod
        def forward(ctx, vox, launch, ret, spec, c, f, cen, r, sig, rsc, pose):
            _lib.check(launch())
            ctx.vox, ctx.spec = vox, spec
            ctx.save_for_backward(c, f, cen, pose)  # (pose: the packed (B, 10) block the call's records point at; kept alive)
            ctx.scalars = (sig, rsc)  # (read for their shape, dtype and device only: the values travelled as host floats)
            return ret

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad):
            c, f, cen, pose = ctx.saved_tensors
            need_c, need_f, need_cen, need_r, need_sig, need_rsc, need_pose = ctx.needs_input_grad[4:11]
            gc, gf, gr, gsig, grs = ctx.vox._backward(ctx.spec, c, f, grad, need_f, need_r, need_sig, need_rsc)
            like = lambda g, t: None if g is None else g.to(dtype=t.dtype).reshape(t.shape).to(t.device)  # noqa: E731
            gsig, grs = like(gsig, ctx.scalars[0]), like(grs, ctx.scalars[1])
            gcen = None
            if need_cen:
                gcen = _center_grad(gc, cen, None if cen.numel() == 3 else
                                    torch.as_tensor(np.diff(ctx.spec["offsets"]), device=gc.device))
            # explicit poses: the per-atom gradients reduced to dL/dc, dL/dq, dL/dt per molecule (autograd splits the block)
            gpose = ctx.vox._pose_backward(ctx.spec, c, gc) if need_pose else None
            return None, None, None, None, gc if need_c else None, gf, gcen, gr, gsig, grs, gpose


    class _ScoreFunction(torch.autograd.Function):
        """scores (and atom_scores) = score(coords, features, center, packed poses): the one walk of mvx_score_batch also writes
        dS/dcoords and dS/dfeatures, which are saved; backward scales each atom's rows by its upstream (dL/dS of its molecule plus,
        with per_atom, dL/ds_n) and reduces centres and poses as _VoxelizeFunction does. No second walk."""

        @staticmethod
        def forward(ctx, vox, call, spec, per_atom, c, f, cen, pose, field=None):
            scores, atoms, gc, gf = call()
            ctx.vox, ctx.spec = vox, spec
            ctx.save_for_backward(c, cen, pose, gc, gf)
            ctx.field_like = None if field is None else (field.dtype, field.device)
            if per_atom:
                return scores, atoms
            return (scores,)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, gs, ga=None):
            c, cen, pose, gc, gf = ctx.saved_tensors
            need_c, need_f, need_cen, need_pose, need_field = ctx.needs_input_grad[4:9]
            lengths = torch.as_tensor(np.diff(ctx.spec["offsets"]), device=c.device)
            up = _row_upstream(gs, ga, lengths, c.shape[0])
            gcs = gc * up[:, None] if gc is not None else None
            gfs = (gf * up[:, None].to(gf.dtype)) if (need_f and gf is not None) else None
            gcen = _center_grad(gcs, cen, None if cen.numel() == 3 else lengths) if need_cen else None
            gpose = ctx.vox._pose_backward(ctx.spec, c, gcs) if need_pose else None
            gfield = None
            if need_field and ctx.field_like is not None:
                # dL/dfield[c, v] = sum_n up_n w[n,c] rho_{n,c}(v): the saved call's grids summed with one float32 weight per atom
                sp = ctx.spec
                gfield = ctx.vox._sum_call(sp["mode"], c, sp["channels"], sp["radii"], sp["rs"], sp["offsets"], sp["xforms"], sp["B"],
                                           sp["C"], up.to(torch.float32), None, False)
                gfield = gfield.to(dtype=ctx.field_like[0]).to(ctx.field_like[1])
            return None, None, None, None, gcs if need_c else None, gfs, gcen, gpose, gfield


    class _ScoreViewsFunction(torch.autograd.Function):
        """scores (and atom_scores) of B views of one shared cloud = score(coords, features, centres, packed poses): the one walk of
        mvx_score_views also writes dS/dcoords and dS/dfeatures per (view, atom) row, which are saved. backward scales each row by
        its upstream, as _ScoreFunction does, sums the rows onto the shared atoms with mvx_views_reduce (no autograd index
        backward, no atomics), and reduces centres and poses per view. No second walk."""

        @staticmethod
        def forward(ctx, vox, call, spec, per_atom, c, f, cen, pose):
            scores, atoms, gc, gf = call()
            ctx.vox, ctx.spec = vox, spec
            ctx.save_for_backward(c, cen, pose, gc, gf, spec["index"])
            if per_atom:
                return scores, atoms
            return (scores,)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, gs, ga=None):
            c, cen, pose, gc, gf, index = ctx.saved_tensors
            need_c, need_f, need_cen, need_pose = ctx.needs_input_grad[4:8]
            vox, spec = ctx.vox, ctx.spec
            # (through pinned memory: a pageable copy would synchronise the stream)
            lengths = torch.from_numpy(np.diff(spec["offsets"])).pin_memory().to(gc.device, non_blocking=True)
            up = _row_upstream(gs, ga, lengths, gc.shape[0])  # dL/ds of every (view, atom) row
            gcs = gc * up[:, None]
            gcoords = vox.views_reduce(gcs, index, spec["offsets"], spec["N"]) if need_c else None
            gfeat = None
            if need_f and gf is not None:
                gfeat = vox.views_reduce(gf * up[:, None].to(gf.dtype), index, spec["offsets"], spec["N"])
            gcen = _center_grad(gcs, cen, lengths) if need_cen else None
            gpose = vox._pose_backward(spec, c[index], gcs) if need_pose else None
            return None, None, None, None, gcoords, gfeat, gcen, gpose


def transform_on_device(coords, center, translation, quaternion):
    """do_transform for a torch CUDA tensor (N,3): runs mvx_transform_coords on the tensor's device."""
    lib = _lib.load()
    dev = coords.device.index if coords.device.index is not None else torch.cuda.current_device()
    vox = _transform_handles.get(dev)
    if vox is None:
        vox = _transform_handles[dev] = Voxelizer(0.5, 8, device=dev)
    xf = _lib.MvxXform()
    flags = 0
    if quaternion is not None:
        xf.quat[:] = [float(q) for q in quaternion]
        flags |= _lib.MVX_XF_ROTATE
        if center is not None:
            cen = center.detach().cpu().numpy() if _is_torch(center) else np.asarray(center)
            xf.center[:] = cen.reshape(3).astype(np.float64).tolist()
            flags |= _lib.MVX_XF_CENTER | _lib.MVX_XF_RECENTER
    if translation is not None:
        tr = translation.detach().cpu().numpy() if _is_torch(translation) else np.asarray(translation)
        xf.trans[:] = tr.reshape(3).astype(np.float32).tolist()
        flags |= _lib.MVX_XF_TRANSLATE
    xf.flags = flags
    src = coords.to(torch.float64).contiguous()
    out = torch.empty_like(src)
    stream = torch.cuda.current_stream(dev).cuda_stream
    _lib.check(lib.mvx_transform_coords(vox._handle, src.data_ptr(), src.shape[0], C.addressof(xf), out.data_ptr(),
                                        _lib.MVX_DEVICE, _lib.MVX_DEVICE, stream))
    return out


_transform_handles: dict = {}
