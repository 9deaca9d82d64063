"""`library='hip'` backend: the reference's Voxelizer interface on hand-written MI355X kernels.

Host layer only: argument checks (same AssertionError messages as the reference numpy backend,
molvoxel/voxelizer/numpy/voxelizer.py:171-192, 317-342, 438-455), dtype fixes (:125-130, :268-271),
channel-count inference (:275-278), RNG draws for the random transform in the reference's order
(numpy/transform.py:63-80) and the call through the C ABI (include/mvx.h). All arithmetic of the
hot path — centring, rigid transform, culls, distances, densities, accumulation — runs on the GPU.
There is no CPU fallback: construction fails without the shared library or without a HIP device.

Array arguments may be numpy arrays (host: staged through pinned memory by the library) or torch CUDA tensors on this
voxelizer's device (zero-copy via data_ptr on the current torch stream). Grids are torch CUDA tensors by default
(`output="torch"`); `output="numpy"` (or a numpy `out_grid`) gives host arrays.

Constructor options:
  grid_dtype="bfloat16"        the kernels write bfloat16 grids: the float32 grid rounded to nearest even as it is stored
  grid_layout="channels_last"  the kernels write NDHWC (`torch.channels_last_3d`) grids: same logical shape, same bits
  differentiable=True          grids computed from device tensors that require grad (coords, features, centres) are part of
                               the autograd graph; the backward pass runs on the GPU (mvx_backward_batch)
  radii_grad / sigma_grad / field_grad (with differentiable)  gradients for a radii tensor (mvx_backward_radii_batch; a
                               one-element tensor on a scalar-radii voxelizer), for a one-element `sigma=` / `set_sigma()`
                               tensor (mvx_backward_density_batch), and for the shared field of `score_batch`
  moments_grad=True (with differentiable)  `moments_batch` / `moments_posed_batch` record an autograd graph: coords, features,
                               centres and poses that require grad get their gradients through the moments
                               (mvx_moments_backward_batch), without B grids and without any grid of dL/dgrid
  torsion_grad=True (with differentiable)  `apply_torsions` records an autograd graph: coords and angles that require grad get
                               their gradients through the conformer (mvx_apply_torsions_backward), so that rotatable bonds
                               can be refined with a torch optimiser through any entry that takes device coords
  overlap_prepass=True         see `set_overlap_prepass`

Entries, next to the reference's `forward_features / forward_types / forward_single`:
  forward_batch                B molecules stored back to back, one launch
  forward_views, select_views  B boxes of ONE shared point cloud, without B copies of it
  forward_sum, forward_views_sum  one float32 grid, the (weighted) sum of a batch's or the views' grids; `set_sum_parts`
  score_batch, score_views     sum(field * grid) per molecule or view without the grids, with gradients
  score_hessian_batch          the scores with their gradient and Hessian under a rigid twist, per-atom Hessians (apply_twist moves poses)
  score_hessian_views          the same for B views of ONE shared cloud
  lm_step, refine_posed_batch, refine_posed_views  damped Newton refinement of B poses together, each step decided on the device
  forward_posed_* / select_posed_views / score_posed_*  the same with explicit rigid poses p = q (x - c) conj(q) + t
                               instead of random transforms; on a differentiable voxelizer the poses get gradients

Every batch and views entry builds one `_Call` - the call as the library reads it - and hands it to one C entry.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from ..contract import BaseVoxelizer
from . import _lib
from ._quaternion import apply_twist  # noqa: F401  (exported here, beside transform_on_device)
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


class _Call:
    """One batch or views call as the library reads it: what the builders (`Voxelizer._batch_call` / `_views_call`) make of
    the caller's arguments, and the `spec` the autograd Functions keep for backward().

    mode "features" | "types" | "single"; C, B, N (all atoms of the call); coords, channels, radii: the converted arrays
    (radii None with scalar radii, which travel as `rs`); views: a views call (N atoms of one shared cloud, B views of it);
    offsets: host int64 (B + 1,) - a batch's, or those of a views call's selection; index: the selection a views call
    attached (`Voxelizer._select_rows`: its per-row outputs are laid out in selection order), or None; xforms: the
    B mvx_xform records or None; centers: the device centres the records point at, or None; pose: the packed (B, 10) poses
    the records point at, or None; in_kind: MVX_HOST | MVX_DEVICE; keep: what must outlive the call; rten: the scalar-radius
    tensor of a radii_grad call; fresh: with overlap_prepass, an input was made on the stream a moment ago; grad: the call
    records an autograd graph. For backward(): settings (`Voxelizer._grad_settings` at the forward)."""

    __slots__ = ("mode", "C", "B", "N", "coords", "channels", "radii", "rs", "offsets", "xforms", "centers", "pose", "in_kind",
                 "keep", "rten", "fresh", "grad", "settings", "views", "index")

    def __init__(self, **fields):
        for name in self.__slots__:
            setattr(self, name, fields.pop(name, None))
        assert not fields, sorted(fields)

    def pick(self, batch, views):
        """Of a family's two forms - entries, argument builders - the one of this call's kind."""
        return views if self.views else batch

    @property
    def rows(self):
        """The number of per-row outputs of the call: N for a batch, the selection's total for views with a selection, None
        for views without one (no per-row outputs)."""
        if not self.views:
            return self.N
        return None if self.index is None else int(self.offsets[-1])

    def entry_args(self, vox, coords=None, channels=None):
        """The arguments the call's entry begins with: batch_args, or views_args and the selection (index, host offsets; two
        nulls without one: the library selects itself). coords / channels: as batch_args takes them."""
        if not self.views:
            return self.batch_args(vox, coords, channels)
        if self.index is None:
            return self.views_args(vox, coords, channels) + (None, None)
        index = self.index
        if not self.rows:  # an empty tensor has no address, but a non-null index is what says "selected" to the library
            index = torch.empty(1, dtype=torch.int64, device=vox.device)
            self.keep.append(index)
        return self.views_args(vox, coords, channels) + (index.data_ptr(), self.offsets.ctypes.data)

    def target_args(self, vox, T, stride):
        """The target of a moments entry: the views entries take a stride with it (one target per view), the batch entries
        take one shared target."""
        return (vox._ptr(T), stride) if self.views else (vox._ptr(T),)

    def row_lengths(self, device):
        """The rows of every molecule (view) as an int64 tensor on `device`, for backward()."""
        lengths = np.diff(self.offsets)
        if self.views:  # (through pinned memory: a pageable copy would synchronise the stream)
            return torch.from_numpy(lengths).pin_memory().to(device, non_blocking=True)
        return torch.as_tensor(lengths, device=device)

    def batch_args(self, vox, coords=None, channels=None):
        """The arguments mvx_backward_batch, mvx_backward_radii_batch, mvx_backward_density_batch, mvx_score_batch,
        mvx_forward_sum_batch and mvx_moments_batch begin with. coords / channels: the tensors autograd saved, in backward()."""
        return (vox._handle, _lib.MODES[self.mode], vox._ptr(self.coords if coords is None else coords),
                vox._ptr(self.channels if channels is None else channels), vox._ptr(self.radii), self.rs, vox._radii_type_code(),
                self.offsets.ctypes.data, None if self.xforms is None else C.addressof(self.xforms), self.B, self.C)

    def views_args(self, vox, coords=None, channels=None):
        """The arguments mvx_forward_views, mvx_forward_views_sum, mvx_score_views, mvx_moments_views and
        mvx_moments_backward_views begin with (mvx_select_views takes the same values with the mode behind radii_type:
        `Voxelizer._select`). coords / channels: the tensors autograd saved, in backward()."""
        return (vox._handle, _lib.MODES[self.mode], vox._ptr(self.coords if coords is None else coords),
                vox._ptr(self.channels if channels is None else channels), vox._ptr(self.radii), self.rs,
                vox._radii_type_code(), self.N, self.C, C.addressof(self.xforms), self.B)


class _StepState:
    """What LMState and FlexLMState share: the tensors of both, one constructor body, and what the step body
    (Voxelizer._lm_step) and the refinement loop read off a state class - POINT: the coordinates in the library's order,
    TRIAL: the trial point they lead to, STEP: the step's name, ENTRY, METHOD: the library entry and the method that serve it."""

    __slots__ = ("q", "t", "S", "G", "H", "lam", "taken", "dropped", "q2", "t2")

    def _fill(self, point, S, G, H, lam, taken, dropped):
        q, B = point[0], int(point[0].shape[0])
        for name, x in zip(self.POINT, point):
            setattr(self, name, x)
        self.S, self.G, self.H, self.lam = S, G, H, lam
        self.taken = torch.zeros(B, dtype=torch.int32, device=q.device) if taken is None else taken
        self.dropped = torch.zeros(B, dtype=torch.int32, device=q.device) if dropped is None else dropped
        for name in self.TRIAL + (self.STEP,):
            setattr(self, name, None)

    def point(self):  # the accepted coordinates: what a refinement returns in front of the scores
        return tuple(getattr(self, name) for name in self.POINT)

    def trial(self):  # the trial point: where the next evaluation is made
        return tuple(getattr(self, name) for name in self.TRIAL)


class LMState(_StepState):
    """The state lm_step works on, B poses as tensors on the voxelizer's device: q (B, 4), t (B, 3): the poses; S (B,), G (B, 6),
    H (B, 6, 6): their scores, twist gradients and twist Hessians (float64, contiguous); lam (B,): the damping; taken, dropped
    (B,) int32: accepted steps, and steps dropped in a row (zeros when not given). q2, t2, xi: the trial poses and their twists,
    made by the first lm_step and reused."""

    __slots__ = ("xi",)
    POINT, TRIAL, STEP, ENTRY, METHOD = ("q", "t"), ("q2", "t2"), "xi", "mvx_lm_step", "lm_step"

    def __init__(self, q, t, S, G, H, lam, taken=None, dropped=None):
        self._fill((q, t), S, G, H, lam, taken, dropped)


class FlexLMState(_StepState):
    """The state flex_lm_step works on: LMState's tensors for n = 6 + T coordinates - G (B, n), H (B, n, n) - with the torsion
    angles theta (B, T) next to the pose. q2, t2, theta2, x (B, n): the trial and its step, made by the first flex_lm_step and
    reused."""

    __slots__ = ("theta", "theta2", "x")
    POINT, TRIAL, STEP, ENTRY, METHOD = ("q", "t", "theta"), ("q2", "t2", "theta2"), "x", "mvx_flex_lm_step", "flex_lm_step"

    def __init__(self, q, t, theta, S, G, H, lam, taken=None, dropped=None):
        self._fill((q, t, theta), S, G, H, lam, taken, dropped)


def _host_array(x, dtype):
    return np.ascontiguousarray(x.detach().cpu().numpy() if _is_torch(x) else np.asarray(x), dtype=dtype)


def check_torsions(offsets, axes, moves):
    """The tree rules of the torsion entries, asserted on host copies (device tensors are copied: one synchronisation).
    offsets (B + 1,); axes (B, T, 2): the axis atoms (a_k, b_k) of every torsion, local to the molecule, T <= 32; moves (N,)
    int32: bit k set = the atom turns with torsion k. A torsion with an axis atom outside [0, N_b) - padding - or with the same atom
    at both ends is inert and is skipped.
    For the others: b_k turns and a_k does not; two sets are nested - the inner one behind the outer one, with both its axis
    atoms inside it - or disjoint; no two sets are the same. The message names the first offending (molecule, torsion)."""
    offsets = np.asarray(offsets, dtype=np.int64)
    axes, moves = _host_array(axes, np.int32), _host_array(moves, np.int32).view(np.uint32)
    B = offsets.shape[0] - 1
    assert axes.ndim == 3 and axes.shape[0] == B and axes.shape[2] == 2, (
        f"axes does not match dimension: {tuple(axes.shape)} vs {(B, 'T', 2)}")
    T = axes.shape[1]
    assert T <= 32, f"at most 32 torsions per molecule: {T}"
    assert moves.ndim == 1 and moves.shape[0] == offsets[-1], f"moves does not match dimension: {tuple(moves.shape)} vs {(int(offsets[-1]),)}"
    seen = set()  # (many poses of one molecule: a tree is checked once)
    for b in range(B):
        a0, N = int(offsets[b]), int(offsets[b + 1] - offsets[b])
        key = (N, axes[b].tobytes(), moves[a0:a0 + N].tobytes())
        if key in seen:
            continue
        seen.add(key)
        ax = axes[b].astype(np.int64)
        live = np.flatnonzero(((ax >= 0) & (ax < N)).all(axis=1) & (ax[:, 0] != ax[:, 1]))
        if live.size == 0:
            continue
        sets = ((moves[a0:a0 + N, None] >> live[None, :].astype(np.uint32)) & 1).astype(np.int64)  # (N, live)
        for j, k in enumerate(live):
            assert sets[ax[k, 1], j], f"molecule {b}, torsion {k}: the axis atom b = {ax[k, 1]} must turn with it"
            assert not sets[ax[k, 0], j], f"molecule {b}, torsion {k}: the axis atom a = {ax[k, 0]} must not turn with it"
        common, size = sets.T @ sets, sets.sum(axis=0)
        for j in range(1, live.size):  # torsion live[j] against every one before it
            for i in range(j):
                k, l, c = live[i], live[j], common[i, j]
                if c == 0:
                    continue
                assert not (c == size[i] == size[j]), f"molecule {b}, torsion {l}: the same set as torsion {k}"
                assert not (c == size[i] and size[i] < size[j]), f"molecule {b}, torsion {l}: contains the set of torsion {k}, which comes before it (parents come before children)"
                assert c == size[j], f"molecule {b}, torsion {l}: its set overlaps the set of torsion {k} without lying inside it"
                assert sets[ax[l, 0], i] and sets[ax[l, 1], i], (
                    f"molecule {b}, torsion {l}: both axis atoms must lie in the set of torsion {k} around it")


class Voxelizer(BaseVoxelizer):
    LIB = "HIP"
    transform_class = RandomTransform
    # the constructor's defaults of what used to be read through getattr(self, ..., default): a Voxelizer made with __new__
    # that sets only some attributes (host-test fakes written against earlier versions of this class) reads these
    precision = 32
    blockdim = 8
    field_grad = False
    _mgrad = False  # (the constructor's moments_grad)
    _tgrad = False  # (the constructor's torsion_grad)
    _sum_parts = 1
    _views_total = 0

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
        moments_grad: bool = False,
        torsion_grad: bool = False,
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
        if moments_grad and not differentiable:
            raise ValueError("moments_grad=True needs differentiable=True: the gradients of the moments are part of the autograd graph")
        if torsion_grad and not differentiable:
            raise ValueError("torsion_grad=True needs differentiable=True: the gradients of the conformer are part of the autograd graph")
        self.differentiable = bool(differentiable)
        self.field_grad = bool(field_grad)
        self._mgrad = bool(moments_grad)
        self._tgrad = bool(torsion_grad)
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
        self._sum_parts = 1  # (set_sum_parts)
        self._views_total = 0  # the last selection's size: sizes the next index buffer (_select)
        self._xf = _lib.MvxXform()  # reused per call: the library copies it before the call returns
        self._xf_addr = C.addressof(self._xf)
        self._has_torch_cuda = torch is not None and torch.cuda.is_available()  # asked on every call otherwise
        cfg = _lib.MvxConfig(
            float(resolution),
            float(self._sigma) if density_type == "gaussian" else 0.5,  # (binary density stores no sigma: base class)
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
                               field_grad=self.field_grad, moments_grad=self._mgrad, torsion_grad=self._tgrad, **kw)
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
            if not np.isscalar(radii):
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
        if not np.isscalar(radii):
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

    def _resolve_out_batch(self, out_grid, B, C_):
        """_resolve_out for the B grids of a batch or views call: the caller's out_grid, checked, or a new one."""
        if out_grid is None:
            out_grid = self.get_empty_grid(C_, batch_size=B)
        assert tuple(out_grid.shape) == (B,) + self.grid_dimension(C_), (
            f"Output grid dimension incorrect: {tuple(out_grid.shape)} vs {(B,) + self.grid_dimension(C_)}")
        return self._resolve_out(out_grid, None)

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
    # SINGLE MOLECULES  (replace numpy/voxelizer.py:97-236 VECTOR, :240-366 INDEX, :370-477 SINGLE)
    def forward_features(self, coords, center, features, radii, random_translation=0.0, random_rotation=False,
                         out_grid=None):
        """coords (V,3), center (3,) | None, features (V,C), radii scalar | (V,) | (C,); out (C,D,H,W)."""
        return self._forward_one("features", coords, center, features, radii, random_translation, random_rotation, out_grid)

    def forward_types(self, coords, center, types, radii, random_translation=0.0, random_rotation=False,
                      out_grid=None):
        """coords (V,3), center (3,) | None, types (V,), radii scalar | (V,) | (C,); out (C,D,H,W)."""
        return self._forward_one("types", coords, center, types, radii, random_translation, random_rotation, out_grid)

    def forward_single(self, coords, center, radii, random_translation=0.0, random_rotation=False, out_grid=None):
        """coords (V,3), center (3,) | None, radii scalar | (V,); out (1,D,H,W)."""
        return self._forward_one("single", coords, center, None, radii, random_translation, random_rotation, out_grid)

    def _forward_one(self, kind, coords, center, chan, radii, random_translation, random_rotation, out_grid):
        """The body of the three single-molecule entries. They are host-bound: no _Call is built
        unless the call records a graph."""
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        C_ = self._check_args_one(kind, coords, chan, radii, out_grid)
        grad = self._grad_wanted(coords, chan if kind == "features" else None, center, radii, out_grid, rten)
        c, ch, r, in_kind, keep = self._prepare_inputs(coords, chan, None if kind == "single" else kind, radii)
        if r is not None and kind == "types":  # (out_grid may have more channels than there are types: numpy/voxelizer.py:337)
            r, _ = self._pad_type_radii(r, kind, C_)
        center = self._grad_center(center) if grad else center
        xf = self._make_xform(center, random_translation, random_rotation, in_kind == _lib.MVX_DEVICE, keep)
        buf, out_kind, ret, how = self._resolve_out(out_grid, (C_,))
        rs = float(radii) if r is None else 0.0
        n = c.shape[0]
        if kind == "single":
            launch = lambda: self._lib.mvx_forward_single(  # noqa: E731
                self._handle, self._ptr(c), self._ptr(r), rs, self._radii_type_code(), n,
                xf, self._ptr(buf), in_kind, out_kind, self._stream())
        else:
            entry = self._lib.mvx_forward_features if kind == "features" else self._lib.mvx_forward_types
            launch = lambda: entry(  # noqa: E731
                self._handle, self._ptr(c), self._ptr(ch), self._ptr(r), rs, self._radii_type_code(), n, C_,
                xf, self._ptr(buf), in_kind, out_kind, self._stream())
        if grad:
            return self._autograd(launch, ret, _Call(
                mode=kind, C=C_, B=1, N=n, coords=c, channels=ch, radii=r, rs=rs, offsets=np.array([0, n], np.int64),
                xforms=self._xform_copy(xf), centers=center if self._on_device(center) else None, in_kind=in_kind, keep=keep,
                rten=rten, grad=True))
        rc = launch()
        if rc:
            _lib.check(rc)
        return self._finish_out(buf, ret, how) if how else ret

    def _check_args_one(self, kind, coords, chan, radii, out_grid):
        """The rules of the single-molecule entries, with the reference's texts; returns the channel count of the call."""
        V = coords.shape[0]
        D = H = W = self.dimension
        if kind == "features":
            C_ = chan.shape[1]
            assert chan.shape[0] == V, f"atom features does not match number of atoms: {chan.shape[0]} vs {V}"
            assert chan.ndim == 2, f"atom features does not match dimension: {chan.shape} vs {(V,'*')}"
        elif kind == "types":
            tmin, tmax = self._types_extent(chan)
            C_ = tmax + 1  # max(types) + 1 over ALL atoms, numpy/voxelizer.py:278 (= the channel-wise radii's count, :275-276)
            assert tuple(chan.shape) == (V,), f"types does not match dimension: {tuple(chan.shape)} vs {(V,)}"
            assert tmin >= 0, "types must be non-negative channel indices"
        else:
            C_ = 1
            assert not self.is_radii_type_channel_wise, "Channel-Wise Radii Type is not supported"
        self._check_radii(radii, V, C_)
        if out_grid is None:
            return C_
        if kind == "features":
            assert tuple(out_grid.shape) == (C_, D, H, W), f"Output grid dimension incorrect: {tuple(out_grid.shape)} vs {(C_,D,H,W)}"
            return C_
        if kind == "types":  # extra channels stay zero (numpy/voxelizer.py:337)
            assert out_grid.shape[0] >= C_, f"Output channel is less than number of types: {out_grid.shape[0]} < {C_}"
        else:
            assert out_grid.shape[0] == 1, "Output channel should be 1"
        assert tuple(out_grid.shape[1:]) == (D, H, W), f'Output grid dimension incorrect: {tuple(out_grid.shape)} vs {("*",D,H,W)}'
        return int(out_grid.shape[0])

    def _check_radii(self, radii, V, C_, batch_types=None):
        """The scalar / channel-wise / atom-wise radii rules of every entry. batch_types: the types of a batch or views call,
        whose channel-wise radii are gathered by type: every type below num_channels needs one, the rest are padded."""
        if self.is_radii_type_scalar:
            assert np.isscalar(radii), "the radii type of voxelizer is `scalar`, radii should be scalar"
        elif self.is_radii_type_channel_wise:
            assert not np.isscalar(radii), f"the radii type of voxelizer is `channel-wise`, radii should be Array[{C_},]"
            if batch_types is None:
                assert tuple(radii.shape) == (C_,), f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(C_,)}"
            else:
                assert radii.ndim == 1 and 0 < radii.shape[0] <= C_, f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(C_,)}"
                if V > 0:
                    tmax = int(batch_types.max())
                    assert tmax < radii.shape[0], f"radii does not match dimension (number of channels,): {tuple(radii.shape)} vs {(tmax + 1,)}"
        else:
            assert not np.isscalar(radii), f"the radii type of voxelizer is `atom-wise`, radii should be Array[{V},]"
            assert tuple(radii.shape) == (V,), f"radii does not match dimension (number of atoms,): {tuple(radii.shape)} vs {(V,)}"

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

    # ------------------------------------------------------------------------------------------
    # THE CALL RECORD (every batch and views entry: guard, build, family-specific checks, outputs, one library call)
    def _batch_call(self, coords, offsets, centers, channels, radii, num_channels=None, random_translation=0.0,
                    random_rotation=False, posed=None, *, device=False, score=False, check=None, out_grid=None, drawn=None):
        """The _Call of B molecules stored back to back, from forward_batch's arguments. posed: (quaternions, translations):
        explicit poses instead of centres with random transforms; their rules fire before every other rule of the call.
        device: host arrays are moved to the device (the sum and score entries). score: a score call, which gives no radius
        or sigma gradient and tracks coords, features and centres (poses) only. check(B, C, offsets): the rules of the
        entry's family that need the call's shape; they fire after the argument rules, before anything is converted or drawn.
        out_grid: the caller's grid, which a recorded graph refuses. drawn: (records, device centres, packed poses) drawn
        already for these molecules instead of new ones - the rows forward_views gathered on a differentiable voxelizer."""
        pose = None
        if posed is not None:
            pose = self._pack_pose(self._pose_count(offsets), centers, posed[0], posed[1], device or self._on_device(coords))
            centers = None
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        if score:
            self._score_no_density_grads(radii, rten)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        B = offsets.shape[0] - 1
        assert offsets[0] == 0 and offsets[-1] == coords.shape[0], "offsets must span coords"
        kind, C_ = self._batch_kind(channels, radii, num_channels)
        self._check_args_batch(coords, channels, kind, radii, C_)
        if check is not None:
            check(B, C_, offsets)
        call = _Call(mode=kind or "single", C=C_, B=B, offsets=offsets, rten=rten, pose=pose)
        return self._convert(call, coords, centers, channels, radii, random_translation, random_rotation,
                             device=device, score=score, out_grid=out_grid, drawn=drawn)

    def _views_call(self, coords, centers, channels, radii, num_channels=None, random_translation=0.0, random_rotation=False,
                    posed=None, *, device=False, score=False, check=None, out_grid=None, features=True):
        """The _Call of B views of ONE shared cloud (`views` set), from forward_views' arguments: forward_batch's rules for one
        molecule of N atoms. Keywords as _batch_call (check gets offsets = None); the poses are packed after the rules. features: are
        the feature values read, and therefore converted - False: no (select_views); "without_graph": only by a call that
        records no graph (forward_views, which otherwise selects, gathers and hands the rows to _batch_call)."""
        if self._sigma_src is not None:
            self._sync_sigma()
        radii, rten = self._scalar_radius(radii)
        kind, C_ = self._batch_kind(channels, radii, num_channels)
        self._check_args_batch(coords, channels, kind, radii, C_)
        assert centers is not None and centers.ndim == 2 and centers.shape[1] == 3, (
            f"centers does not match dimension: {tuple(getattr(centers, 'shape', ()))} vs ('B', 3)")
        if score:
            self._score_no_density_grads(radii, rten)
        B = int(centers.shape[0])
        if check is not None:
            check(B, C_, None)
        call = _Call(mode=kind or "single", C=C_, B=B, rten=rten, views=True)
        if posed is not None:
            call.pose = self._pack_pose(B, centers, posed[0], posed[1], device or self._on_device(coords))
        return self._convert(call, coords, centers, channels, radii, random_translation, random_rotation,
                             device=device, score=score, out_grid=out_grid, features=features)

    def _convert(self, call, coords, centers, channels, radii, random_translation, random_rotation, *, device, score, out_grid,
                 drawn=None, features=True):
        """The second half of both builders, behind the rules; fills in the _Call they began (mode, C, B, offsets, rten,
        pose): does the call record a graph, the arrays as the library reads them, the records (drawn here, record by
        record), and overlap_prepass's `fresh`. radii: behind _scalar_radius."""
        kind = None if call.mode == "single" else call.mode
        if drawn is not None:
            call.xforms, centers, call.pose = drawn
        pose = call.pose
        tracked = (coords, channels if kind == "features" else None, centers if pose is None else pose)
        if score:
            call.grad = self._grad_wanted(*tracked, None, None)
        else:
            call.grad = self._grad_wanted(*tracked, radii, out_grid, call.rten)
        user_centers = centers  # (a conversion made below, for autograd or for the ABI, is "fresh")
        if call.grad and centers is not None:
            centers = self._grad_center(centers)
        if kind == "features" and (features is False or (features == "without_graph" and call.grad)):
            channels = kind = None  # (feature values are not read: not converted either)
        c, ch, r, in_kind, keep = self._prepare_inputs(self._device_coords(coords) if device else coords, channels, kind, radii)
        # With overlap_prepass the library's side stream reads the inputs without waiting for the caller's stream.
        # Arrays this layer had to convert just now (dtype / layout fixes, the int32 copy of `types`) were produced
        # ON that stream a moment ago: make them complete first (first call with a given tensor only: the copies are
        # cached or the caller passes the right dtype). The same holds for padded radii, for rows gathered and poses
        # packed a moment ago (drawn, a pose tensor) and for a converted centres tensor.
        on_stream = self.overlap_prepass and in_kind == _lib.MVX_DEVICE
        fresh = on_stream and (c is not coords or (kind == "features" and ch is not channels) or (r is not None and r is not radii)
                               or (kind == "types" and self._types_fresh) or drawn is not None or _is_torch(pose))
        r, padded = self._pad_type_radii(r, kind, call.C)
        if padded:
            keep.append(r)
            fresh = fresh or self.overlap_prepass
        if drawn is None:
            call.xforms, centers = self._records(call.B, centers, pose, in_kind, random_translation, random_rotation, keep)
            if on_stream and centers is not None:
                fresh = fresh or centers.data_ptr() != user_centers.data_ptr()
        call.N, call.coords, call.channels, call.radii = int(c.shape[0]), c, ch, r
        call.rs = float(radii) if np.isscalar(radii) else 0.0
        call.centers, call.in_kind, call.keep, call.fresh = centers, in_kind, keep, fresh
        return call

    def _records(self, B, centers, pose, in_kind, random_translation, random_rotation, keep):
        """The B records of a call as (records or None, device centres or None): from the packed poses, or from the centres
        and the random transform, drawn now."""
        if pose is not None:
            keep.append(pose)
            return self._pose_xforms(pose, B), None
        if centers is not None or random_rotation or (random_translation and random_translation > 0.0):
            return self._make_xforms(B, centers, in_kind, random_translation, random_rotation, keep)
        return None, None

    def _batch_kind(self, channels, radii, num_channels):
        """(kind, C) of a batch or views call from its channels: None -> single, (sumN,) int -> types, (sumN, C) -> features."""
        if channels is None:
            return None, 1
        if channels.ndim != 1:
            return "features", int(channels.shape[1])
        if num_channels is not None:
            return "types", int(num_channels)
        return "types", int(radii.shape[0] if self.is_radii_type_channel_wise else int(channels.max()) + 1)

    def _check_args_batch(self, coords, channels, kind, radii, C_):
        """The per-molecule rules (_check_args_one) for atoms stored back to back: the library reads sumN rows of channels
        and sumN | C radii, so every array must really have them."""
        V = coords.shape[0]
        assert coords.ndim == 2 and coords.shape[1] == 3, f"coords does not match dimension: {tuple(coords.shape)} vs {(V, 3)}"
        if kind == "features":
            assert channels.shape[0] == V, f"atom features does not match number of atoms: {channels.shape[0]} vs {V}"
        elif kind == "types":
            assert tuple(channels.shape) == (V,), f"types does not match dimension: {tuple(channels.shape)} vs {(V,)}"
        else:
            assert not self.is_radii_type_channel_wise, "Channel-Wise Radii Type is not supported"
        self._check_radii(radii, V, C_, channels if kind == "types" else None)

    def _views_inputs(self, coords, channels, kind, radii, C_):
        """(coords, channels, radii, in_kind, keepalive) of a views call as the library reads them, channel-wise radii of a
        types call padded: _convert's conversions, for a caller that brings its own records."""
        c, ch, r, in_kind, keep = self._prepare_inputs(coords, channels, kind, radii)
        r, padded = self._pad_type_radii(r, kind, C_)
        if padded:
            keep.append(r)
        return c, ch, r, in_kind, keep

    def _pad_type_radii(self, r, kind, C_):
        """Channel-wise radii are indexed by type only: padded with ones so that the (C,) contract of the ABI holds.
        Returns (radii, whether a new array was made)."""
        if not (kind == "types" and self.is_radii_type_channel_wise and r.shape[0] < C_):
            return r, False
        pad = C_ - r.shape[0]
        return (torch.cat([r, r.new_ones(pad)]) if _is_torch(r) else np.concatenate([r, np.ones(pad, self.fp)])), True

    def _device_coords(self, coords):
        """coords on this voxelizer's device (the sum and score entries take device arrays only): host arrays are moved there."""
        if self._on_device(coords):
            return coords
        return (coords.detach() if _is_torch(coords) else torch.as_tensor(np.asarray(coords, dtype=np.float64))).to(self.device)

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

    def _pack_pose(self, B, centers, quaternions, translations, on_device):
        """The (B, 10) float64 block [c | q | t] the records of a posed call point at. With coordinates on this device the block
        is a tensor there: torch tensors are packed with torch ops (recorded by autograd; their values never visit the host and
        nothing synchronises), numpy poses are packed on the host and uploaded. With host coordinates: a numpy array."""
        Voxelizer._check_pose(B, centers, quaternions, translations)
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

    @staticmethod
    def _check_pose(B, centers, quaternions, translations):
        """The shape rules of explicit poses (_pack_pose; the posed entries that refuse something else first apply them early)."""
        def shape(x):
            return tuple(getattr(x, "shape", ()))

        assert shape(quaternions) == (B, 4), f"quaternions does not match dimension: {shape(quaternions)} vs {(B, 4)}"
        assert shape(translations) == (B, 3), f"translations does not match dimension: {shape(translations)} vs {(B, 3)}"
        assert centers is None or shape(centers) == (B, 3), f"centers does not match dimension: {shape(centers)} vs {(B, 3)}"

    @staticmethod
    def _pose_count(offsets, centers=None):
        """B as the pose rules need it before the call is built: from a batch's offsets, or - offsets None - from the centres
        of a views call."""
        if offsets is None:
            return int(getattr(centers, "shape", (0,))[0])
        return np.asarray(offsets).shape[0] - 1

    def _pose_xforms(self, pose, B):
        """B MVX_XF_POSE_PTR records, record b pointing at row b of the packed poses."""
        xfs = (_lib.MvxXform * B)()
        base = self._ptr(pose)
        for b in range(B):
            xfs[b].flags = _lib.MVX_XF_POSE_PTR
            xfs[b].center_ptr = base + 80 * b
        return xfs

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
        return self._forward_batch(coords, offsets, centers, channels, radii, num_channels, out_grid,
                                   posed=(quaternions, translations))

    def _forward_batch(self, coords, offsets, centers, channels, radii, num_channels=None, out_grid=None,
                       random_translation=0.0, random_rotation=False, posed=None, drawn=None):
        """forward_batch's body. posed, drawn: see _batch_call."""
        call = self._batch_call(coords, offsets, centers, channels, radii, num_channels, random_translation, random_rotation,
                                posed, out_grid=out_grid, drawn=drawn)
        B, C_ = call.B, call.C
        buf, out_kind, ret, how = self._resolve_out_batch(out_grid, B, C_)
        if call.fresh:
            torch.cuda.current_stream(self._device_index).synchronize()
        # (the three mvx_forward_*_batch entries have an argument order of their own)
        c, ch, r, rs, in_kind = call.coords, call.channels, call.radii, call.rs, call.in_kind
        off_ptr = call.offsets.ctypes.data
        xf_ptr = None if call.xforms is None else C.addressof(call.xforms)
        rt = self._radii_type_code()
        if call.mode == "single":
            launch = lambda: self._lib.mvx_forward_single_batch(  # noqa: E731
                self._handle, self._ptr(c), self._ptr(r), rs, rt, off_ptr, xf_ptr, B, self._ptr(buf), in_kind, out_kind,
                self._stream())
        else:
            entry = self._lib.mvx_forward_features_batch if call.mode == "features" else self._lib.mvx_forward_types_batch
            launch = lambda: entry(  # noqa: E731
                self._handle, self._ptr(c), self._ptr(ch), self._ptr(r), rs, rt, off_ptr, xf_ptr, B, C_,
                self._ptr(buf), in_kind, out_kind, self._stream())
        if call.grad:
            return self._autograd(launch, ret, call)
        _lib.check(launch())
        return self._finish_out(buf, ret, how)

    # ------------------------------------------------------------------------------------------
    # VIEWS (many boxes of one shared point cloud: mvx_select_views / mvx_forward_views)
    def _select(self, call):
        """mvx_select_views into an index buffer sized from the call's shape: B * N entries when that is small, else the
        last call's total with some room. One call (one synchronisation) unless the buffer turns out too small: the library
        then reports MVX_ERR_INVALID with the offsets filled in, and the call is repeated with the exact size."""
        handle, mode, c, ch, r, rs, rt, N, C_, xfs, B = call.views_args(self)
        args = (handle, c, ch if call.mode == "types" else None, r, rs, rt, mode, N, C_, xfs, B)  # (feature values are not read)
        offsets = np.full(B + 1, -1, dtype=np.int64)
        cap = B * N if B * N <= (1 << 20) else min(B * N, max(1 << 20, 2 * self._views_total))
        index = torch.empty(cap, dtype=torch.int64, device=self.device)
        rc = self._lib.mvx_select_views(*args, index.data_ptr() if cap else None, cap, offsets.ctypes.data, call.in_kind,
                                        self._stream())
        if rc != 0 and offsets[-1] > cap:  # too small: size it from the offsets and call again
            index = torch.empty(int(offsets[-1]), dtype=torch.int64, device=self.device)
            rc = self._lib.mvx_select_views(*args, index.data_ptr(), index.numel(), offsets.ctypes.data, call.in_kind,
                                            self._stream())
        _lib.check(rc)
        self._views_total = int(offsets[-1])
        return index[:int(offsets[-1])], offsets

    def select_views(self, coords, centers, channels=None, radii=None, random_translation=0.0, random_rotation=False):
        """The atoms each view of a shared cloud can see: (index, offsets), index an int64 tensor on this voxelizer's
        device, offsets a numpy int64 array of B + 1 entries; index[offsets[b]:offsets[b + 1]] are, in ascending order, the
        atoms that pass the forward's box cull for view b (every atom that reaches a voxel of that view's grid is among
        them). Arguments as forward_views; feature values are not read. Synchronises the stream (the offsets come to the host)."""
        return self._select_views(coords, centers, channels, radii, random_translation, random_rotation)

    def select_posed_views(self, coords, centers, quaternions, translations, channels=None, radii=None):
        """select_views for explicit poses: the atoms each pose of forward_posed_views keeps, as (index, offsets)."""
        self._check_pose(self._pose_count(None, centers), centers, quaternions, translations)  # (before the rules of the other arguments)
        return self._select_views(coords, centers, channels, radii, posed=(quaternions, translations))

    def _select_views(self, coords, centers, channels, radii, random_translation=0.0, random_rotation=False, num_channels=None,
                      posed=None):
        """select_views' body. num_channels: the channel count of a types call. (An index has no gradient: no graph.)"""
        with torch.no_grad():
            return self._select(self._views_call(coords, centers, channels, radii, num_channels, random_translation,
                                                 random_rotation, posed, features=False))

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

    def forward_posed_views(self, coords, centers, quaternions, translations, channels, radii, num_channels=None, out_grid=None):
        """forward_views with one explicit rigid pose per view instead of a centre and a random transform: B poses of ONE
        shared cloud (docking poses of a ligand, the 24 cube rotations, poses under refinement) without B copies of it - bit for
        bit forward_posed_batch on the cloud repeated B times. centers (B,3), quaternions (B,4), translations (B,3) as there.
        On a differentiable voxelizer every view's pose gets its own gradient and the per-atom gradients of all views sum into
        the shared tensors. Synchronises the stream once, as forward_views does."""
        return self._forward_views(coords, centers, channels, radii, num_channels, out_grid, posed=(quaternions, translations))

    def _forward_views(self, coords, centers, channels, radii, num_channels=None, out_grid=None, random_translation=0.0,
                       random_rotation=False, posed=None):
        """forward_views' body. posed: (quaternions, translations) of forward_posed_views."""
        call = self._views_call(coords, centers, channels, radii, num_channels, random_translation, random_rotation, posed,
                                out_grid=out_grid, features="without_graph")
        B, C_ = call.B, call.C
        if call.grad:  # select, gather, forward_batch on the gathered rows with the records drawn above
            with torch.no_grad():
                index, offsets = self._select(call)

            def take(x):
                if _is_torch(x):
                    return x[index.to(x.device)]
                return np.asarray(x)[index.cpu().numpy()]

            return self._forward_batch(coords[index], offsets, None, None if channels is None else take(channels),
                                       take(radii) if self.is_radii_type_atom_wise else radii,
                                       num_channels=C_ if call.mode == "types" else None,
                                       drawn=(call.xforms, call.centers, call.pose))
        buf, out_kind, ret, how = self._resolve_out_batch(out_grid, B, C_)
        _lib.check(self._lib.mvx_forward_views(*call.views_args(self), self._ptr(buf), call.in_kind, out_kind, self._stream()))
        return self._finish_out(buf, ret, how)

    # ------------------------------------------------------------------------------------------
    # SUMS (one grid for a whole batch or for the views of a cloud: mvx_forward_sum_batch / mvx_forward_views_sum)
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
        return self._forward_sum(coords, offsets, centers, channels, radii, weights, num_channels, out_grid, accumulate,
                                 posed=(quaternions, translations))

    def _sum_guard(self, channels, what="forward_sum", entries="forward_sum / forward_posed_sum", result="the grid is a tensor",
                   alt="use forward_batch(...).sum(0) (forward_posed_batch(...).sum(0)) instead"):
        """What a summed call refuses before it looks at anything else: the configurations voxelize_sum_kernel does not serve.
        what, entries, result, alt: the texts of another family on the same walk (moments_batch)."""
        if self.output != "torch":
            raise ValueError(f"{entries} need output='torch': {result} on the voxelizer's device")
        if self.precision == 64:
            raise NotImplementedError(f"{what} does not support precision 64 (float32 sums only): {alt}")
        if self.is_radii_type_channel_wise and channels is not None and getattr(channels, "ndim", 1) == 2:
            raise NotImplementedError(f"{what} does not support channel-wise radii with features: {alt}")
        D, bd = int(self.dimension), int(self.blockdim)
        if D % 4 != 0:
            raise NotImplementedError(f"{what} does not support a dimension that is no multiple of 4 (got {D}): {alt}")
        if -(-D // bd) > 1 and bd % 8 != 0:  # (mvx_plan.lane_range: reference blocks that cut through 2 x 4 x 8 sub-tiles)
            raise NotImplementedError(f"{what} does not support blockdim={bd} at dimension {D} (per-lane ranges): {alt}")

    def _sum_rules(self, out_grid, accumulate, weights):
        """The family rules of a summed call, for the builders' `check`: out_grid / accumulate, then the weights - before
        anything is converted or drawn. Returns (check, box); the weights as the library reads them land in box[0]."""
        box = []

        def check(B, C_, offsets):
            self._sum_out_rules(out_grid, accumulate, C_)
            box.append(self._sum_weights(weights, B, offsets))

        return check, box

    def _sum_out_rules(self, out_grid, accumulate, C_):
        if accumulate and out_grid is None:
            raise ValueError("accumulate=True needs out_grid: there is nothing to add to")
        if out_grid is not None:
            assert tuple(getattr(out_grid, "shape", ())) == self.grid_dimension(C_), (
                f"Output grid dimension incorrect: {tuple(getattr(out_grid, 'shape', ()))} vs {self.grid_dimension(C_)}")
            if not (self._on_device(out_grid) and out_grid.dtype == torch.float32 and out_grid.is_contiguous()):
                raise ValueError("out_grid of forward_sum must be a contiguous float32 tensor on this voxelizer's device")

    def _sum_weights(self, weights, B, offsets=None):
        """The weights of a summed call as the library reads them: None, or float32 on this device - for a batch (offsets
        given) (sumN,), (B,) weights expanded per atom here; for views (B,) only, expanded on the device in the library."""
        if weights is None:
            return None
        w = (weights.detach() if _is_torch(weights) else torch.as_tensor(np.asarray(weights))).to(device=self.device, dtype=torch.float32)
        shape = tuple(w.shape)
        if offsets is None:
            assert shape == (B,), f"weights does not match dimension: {shape} vs {(B,)}"
        else:
            N = int(offsets[-1])
            assert shape in ((B,), (N,)), f"weights does not match dimension: {shape} vs {(B,)} or {(N,)}"
            if shape == (B,):
                lengths = torch.as_tensor(np.diff(offsets), device=self.device)
                w = torch.repeat_interleave(w, lengths, output_size=N)
        return w.contiguous()

    def _forward_sum(self, coords, offsets, centers, channels, radii, weights=None, num_channels=None, out_grid=None,
                     accumulate=False, random_translation=0.0, random_rotation=False, posed=None):
        """forward_sum's body. posed: (quaternions, translations) of forward_posed_sum."""
        self._sum_guard(channels)
        with torch.no_grad():
            check, w = self._sum_rules(out_grid, accumulate, weights)
            call = self._batch_call(coords, offsets, centers, channels, radii, num_channels, random_translation, random_rotation,
                                    posed, device=True, check=check)
            return self._sum_call(call, w[0], out_grid, accumulate)

    def _sum_call(self, call, w, out, accumulate, coords=None):
        """One mvx_forward_sum_batch or mvx_forward_views_sum call on device arrays, on the current stream; out None: a new
        grid. coords: the tensor autograd saved (the field gradient of a score call)."""
        if out is None:
            out = torch.empty(self.grid_dimension(call.C), dtype=torch.float32, device=self.device)
        entry = call.pick(self._lib.mvx_forward_sum_batch, self._lib.mvx_forward_views_sum)
        args = call.pick(call.batch_args, call.views_args)(self, coords)  # (a summed call takes no selection)
        _lib.check(entry(*args, self._ptr(w), self._ptr(out), 1 if accumulate else 0, self._stream()))
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
        return self._forward_views_sum(coords, centers, channels, radii, weights, num_channels, out_grid, accumulate,
                                       posed=(quaternions, translations))

    def _forward_views_sum(self, coords, centers, channels, radii, weights=None, num_channels=None, out_grid=None, accumulate=False,
                           random_translation=0.0, random_rotation=False, posed=None):
        """forward_views_sum's body. posed: (quaternions, translations) of forward_posed_views_sum."""
        self._sum_guard(channels)
        with torch.no_grad():
            check, w = self._sum_rules(out_grid, accumulate, weights)
            call = self._views_call(coords, centers, channels, radii, num_channels, random_translation, random_rotation, posed,
                                    device=True, check=check)
            return self._sum_call(call, w[0], out_grid, accumulate)

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
        return self._sum_parts

    # ------------------------------------------------------------------------------------------
    # MOMENTS (per-channel sums and norms of every molecule's grid without the grids: mvx_moments_batch)
    def moments_batch(self, coords, offsets, centers, channels, radii, target=None, num_channels=None,
                      random_translation=0.0, random_rotation=False):
        """Per-channel sums and norms of the B grids forward_batch would write with the same arguments - without writing them.
        With g = grid[b, c] as float32 values (whatever this voxelizer's grid_dtype / grid_layout) and float64 sums over the voxels:

            m[b, c, 0] = sum g        m[b, c, 1] = sum g * g        m[b, c, 2] = sum g * target[c]    (only with a target)

        What sits on top of them: normalised cross-correlation m2 / sqrt(m1 * sum(target ** 2)), shape Tanimoto
        O_ab / (O_aa + O_bb - O_ab) with the self-overlaps m1, MSE against the target (m1 - 2 m2 + sum(target ** 2)) / D^3, and
        occupied volume or total mass m0 (binary density: the voxel count).

        Arguments, checks, RNG order and records are forward_batch's; host arrays are moved to the device. Needs
        output="torch". target: None or one (C,D,H,W) array shared by all molecules, converted with
        `.to(device, torch.float32).contiguous()`. Returns a (B, C, 2) - with a target (B, C, 3) - float64 tensor on this device.
        The products are exact in float64, so each moment lies within (D^3 - 1) * 2^-53 * sum|term| of the exact sum; sums of
        small integers (binary density with types or one channel) are exact. Deterministic, no atomics: a molecule's values do
        not depend on its batch, and the first two do not depend on the target. Molecules without atoms inside the box give
        exact zeros. The result is NOT part of the autograd graph: inputs that require grad are read as values - unless the
        voxelizer was made with moments_grad=True (and differentiable=True). Then, with grad mode on and coords, features or
        centers that require grad, the same call - the same bits - records a graph, and backward() gives their gradients through
        the moments (mvx_moments_backward_batch: dL/dgrid = dL/dm0 + 2 dL/dm1 g + dL/dm2 target is formed inside the backward
        walk, molecule chunk by molecule chunk, without B grids and without any grid of dL/dgrid). A target, radii or a sigma
        tensor that requires grad raises ValueError there: no gradients with respect to them.
        Not supported (NotImplementedError; use forward_batch(...) and reduce the grids): precision 64, channel-wise radii with
        features, dimensions that are no multiple of 4, and blockdims that cut through the kernels' 2 x 4 x 8 sub-tiles."""
        return self._moments_batch(coords, offsets, centers, channels, radii, target, num_channels, random_translation,
                                   random_rotation)

    def moments_posed_batch(self, coords, offsets, centers, quaternions, translations, channels, radii, target=None,
                            num_channels=None):
        """moments_batch with one explicit rigid pose per molecule (forward_posed_batch's arguments and records): the moments
        of the grids of B poses - every pose's cross-correlation with a map in one call. Not part of the autograd graph, unless
        the voxelizer was made with moments_grad=True: then `centers`, `quaternions` and `translations` that require grad get
        their gradients too (mvx_pose_grad_batch on the per-atom gradients), next to coords and features."""
        return self._moments_batch(coords, offsets, centers, channels, radii, target, num_channels,
                                   posed=(quaternions, translations))

    def _moments_record(self, radii, target):
        """Does a moments call build its _Call with grad mode as it is (moments_grad, grad mode on: the conversions and the
        packed poses are recorded, tracking what a score call tracks: coords, features and centres (poses))? Refuses the
        gradients such a call does not provide."""
        if not (self._mgrad and torch.is_grad_enabled()):
            return False
        if _is_torch(target) and target.requires_grad:
            raise ValueError("moments_grad gives no gradient with respect to the target: detach it (dL/dtarget[c] is "
                             "sum_b dL/dm[b, c, 2] * grid[b, c]: use forward_batch (forward_posed_batch) for it)")
        for what, x in (("radii", radii), ("sigma", self.sigma_tensor)):
            if _is_torch(x) and x.requires_grad:
                raise ValueError(f"moments_grad gives no gradient with respect to {what}: detach it, or use forward_batch "
                                 "(forward_posed_batch) and reduce the grids for that gradient")
        return True

    def _moments_batch(self, coords, offsets, centers, channels, radii, target=None, num_channels=None, random_translation=0.0,
                       random_rotation=False, posed=None):
        """moments_batch's call. posed: (quaternions, translations) of moments_posed_batch."""
        self._sum_guard(channels, "moments_batch", "moments_batch / moments_posed_batch", "the moments are a tensor",
                        "use forward_batch(...) (forward_posed_batch(...)) and reduce the grids instead")
        record = self._moments_record(radii, target)
        with torch.enable_grad() if record else torch.no_grad():
            call = self._batch_call(coords, offsets, centers, channels, radii, num_channels, random_translation, random_rotation,
                                    posed, device=True, score=record, check=self._target_rule(target, per_row=False))
        return self._moments(call, target)

    def _target_rule(self, target, per_row):
        """For the builders' `check`: the shape rule of a moments call's target, where there is one."""
        if target is None:
            return None
        return lambda B, C_, offsets: self._check_grid_operand(target, "target", B, C_, per_row)

    def _moments(self, call, target):
        """The body of the moments entries: one mvx_moments_batch or mvx_moments_views call, inside _MomentsFunction where the
        call records a graph (it then was built with grad mode on: _moments_record)."""
        self._select_rows(call, call.grad)
        entry = call.pick(self._lib.mvx_moments_batch, self._lib.mvx_moments_views)

        def run():
            with torch.no_grad():
                T, stride = self._grid_operand(target, call.C, torch.float32)
                out = torch.empty((call.B, call.C, 2 if T is None else 3), dtype=torch.float64, device=self.device)
                _lib.check(entry(*call.entry_args(self), *call.target_args(self, T, stride), self._ptr(out), self._stream()))
                return out, T

        if not call.grad:
            return run()[0]
        call.settings = self._grad_settings()
        return _MomentsFunction.apply(self, run, call, call.coords, call.channels if call.mode == "features" else None,
                                      call.centers, call.pose)

    def _moments_backward(self, spec, c, f, T, gm, need_features):
        """(dL/dcoords (rows, 3) float64, dL/dfeatures (rows, C) or None) for dL/dm = gm (B, C, K), on the current stream: one
        row per atom of a batch, per (view, atom) of the selection of a views call. spec: the forward call's _Call; c, f: its
        coords and features as autograd saved them; T: the target as the forward read it."""
        self._same_settings(spec)
        rows = spec.rows
        g = gm.to(device=self.device, dtype=torch.float64).contiguous()
        gc = torch.empty((rows, 3), dtype=torch.float64, device=self.device)
        gf = torch.empty((rows, spec.C), dtype=self._tfp, device=self.device) if need_features else None
        if rows == 0 or spec.B == 0:  # no atoms: no gradient rows
            return gc, gf
        entry = spec.pick(self._lib.mvx_moments_backward_batch, self._lib.mvx_moments_backward_views)
        _lib.check(entry(*spec.entry_args(self, c, f if spec.mode == "features" else None),
                         *spec.target_args(self, *self._grid_operand(T, spec.C, torch.float32)), self._ptr(g), self._ptr(gc),
                         self._ptr(gf), self._stream()))
        return gc, gf

    _moments_backward_views = _moments_backward  # (the name the rows of views went by)

    # ------------------------------------------------------------------------------------------
    # MOMENTS OF VIEWS (many poses or boxes of one shared cloud, each against its own target: mvx_moments_views)
    def moments_views(self, coords, centers, channels, radii, target=None, num_channels=None, random_translation=0.0,
                      random_rotation=False):
        """The moments of the B grids forward_views would write with the same arguments - without the grids and without B copies
        of the cloud: each view's atoms are selected on the device, gathered into a compact batch and walked once
        (mvx_moments_views). The values are moments_batch's, bit for bit, on coords[index], the gathered channels and radii and
        the offsets of select_views.

        coords (N,3), centers (B,3), channels and radii as forward_views (transforms drawn per view in its RNG order); host
        arrays are moved to the device. Needs output="torch". target: None, one (C,D,H,W) array shared by all views, or a
        (B,C,D,H,W) array with one target per view (a target lives in box coordinates: views of different boxes want one
        each), converted as moments_batch converts it. Returns a (B, C, 2) - with a target (B, C, 3) - float64 tensor on this
        device; row b of a per-view call is, bit for bit, row b of the call that shares target[b]. A view that keeps no atom
        gives exact zeros. Without a recorded graph the call is one library call (one stream synchronisation, for the
        selection). Not part of the autograd graph unless the voxelizer was made with moments_grad=True: then, with grad mode on
        and coords, features or centers that require grad, the views are selected once, the same call records a graph, and
        backward() forms the per-(view, atom) rows (mvx_moments_backward_views) and sums them onto the shared atoms with
        mvx_views_reduce - deterministic, no atomics. A target, radii or a sigma tensor that requires grad raises ValueError.
        Not supported: what moments_batch does not support (use forward_views(...) and reduce the grids)."""
        return self._moments_views(coords, centers, channels, radii, target, num_channels, random_translation, random_rotation)

    def moments_posed_views(self, coords, centers, quaternions, translations, channels, radii, target=None, num_channels=None):
        """moments_views with one explicit rigid pose per view (forward_posed_views' arguments and records): the moments of B
        poses of ONE shared cloud - every pose's cross-correlation with a map in one call, the cloud handed over once. On a
        moments_grad voxelizer `centers`, `quaternions` and `translations` that require grad get their gradients per view
        (mvx_pose_grad_batch on the rows), next to coords and features."""
        return self._moments_views(coords, centers, channels, radii, target, num_channels, posed=(quaternions, translations))

    def _moments_views(self, coords, centers, channels, radii, target=None, num_channels=None, random_translation=0.0,
                       random_rotation=False, posed=None):
        """moments_views' call. posed: (quaternions, translations) of moments_posed_views."""
        self._sum_guard(channels, "moments_views", "moments_views / moments_posed_views", "the moments are a tensor",
                        "use forward_views(...) (forward_posed_views(...)) and reduce the grids instead")
        record = self._moments_record(radii, target)
        with torch.enable_grad() if record else torch.no_grad():
            call = self._views_call(coords, centers, channels, radii, num_channels, random_translation, random_rotation, posed,
                                    device=True, score=record, check=self._target_rule(target, per_row=True))
        return self._moments(call, target)

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
        self._score_guard(field, True)  # (the guard, then the poses' rules, then everything else)
        self._check_pose(self._pose_count(offsets), centers, quaternions, translations)
        return self._score_batch(coords, offsets, centers, channels, radii, field, num_channels, per_atom=per_atom,
                                 posed=(quaternions, translations))

    def _score_guard(self, field, shared_field_grad=False):
        """What a score call refuses before it looks at anything else. shared_field_grad: the call is one of those that, on a
        field_grad voxelizer, give a shared (C, D, H, W) field its gradient (score_batch / score_posed_batch)."""
        if self.output != "torch":
            raise ValueError("score_batch / score_posed_batch need output='torch': the scores are tensors on the voxelizer's device")
        if _is_torch(field) and field.requires_grad:
            if shared_field_grad and self.field_grad and field.dim() == 4:
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

    def _check_grid_operand(self, x, what, B, C_, per_row=True):
        """The shape rule of a field or a target: (C,D,H,W), one for all, or - per_row - (B,C,D,H,W), one per molecule or view."""
        shape, one = tuple(getattr(x, "shape", ())), self.grid_dimension(C_)
        if per_row:
            assert shape in (one, (B,) + one), f"{what} does not match dimension: {shape} vs {one} or {(B,) + one}"
        else:
            assert shape == one, f"{what} does not match dimension: {shape} vs {one}"

    def _grid_operand(self, x, C_, dtype):
        """(tensor, stride) of a field (dtype: the grid's) or a target (float32) as the library reads it: on this device,
        contiguous; stride: the elements between the grids of two molecules or views, C * D^3, or 0: one (C,D,H,W) grid for
        all. None: (None, 0)."""
        if x is None:
            return None, 0
        t = (x if _is_torch(x) else torch.as_tensor(np.asarray(x))).to(device=self.device, dtype=dtype).contiguous()
        return t, C_ * int(self.dimension) ** 3 if t.dim() == 5 else 0

    def _select_rows(self, call, wanted):
        """The selection step of a body, which only views calls take: `wanted` (the call has outputs laid out per (view, atom)
        row, or records a graph) attaches the selection to the call, for the entry and for backward()."""
        if call.views and wanted:
            with torch.no_grad():
                call.index, call.offsets = self._select(call)

    def _score_batch(self, coords, offsets, centers, channels, radii, field, num_channels=None, random_translation=0.0,
                     random_rotation=False, per_atom=False, posed=None):
        """score_batch's call. posed: (quaternions, translations) of score_posed_batch."""
        self._score_guard(field, True)
        fgrad = (_is_torch(field) and field.requires_grad and self.field_grad and self.differentiable and torch.is_grad_enabled())
        if fgrad:  # (what forward_sum cannot serve is refused now, not in backward())
            self._sum_guard(channels)
        call = self._batch_call(coords, offsets, centers, channels, radii, num_channels, random_translation, random_rotation,
                                posed, device=True, score=True,
                                check=lambda B, C_, offsets: self._check_grid_operand(field, "field", B, C_))
        return self._score(call, field, per_atom, fgrad)

    def _score(self, call, field, per_atom, fgrad=False):
        """The body of the score entries: one mvx_score_batch or mvx_score_views call, inside _ScoreFunction where the call
        records a graph or - fgrad - the shared field of a batch gets its gradient. Returns scores, with per_atom
        (scores, atom_scores): one row per atom of a batch, per (view, atom) of the selection of a views call."""
        F, stride = self._grid_operand(field, call.C, self._gdt)
        B, C_, grad = call.B, call.C, call.grad
        feat = call.channels if call.mode == "features" else None
        need_gf = grad and feat is not None and feat.requires_grad
        self._select_rows(call, per_atom or grad)
        entry = call.pick(self._lib.mvx_score_batch, self._lib.mvx_score_views)

        def run():
            n = call.rows
            scores = torch.empty(B, dtype=torch.float64, device=self.device)
            atoms = torch.empty(n, dtype=torch.float64, device=self.device) if per_atom else None
            gc = torch.empty((n, 3), dtype=torch.float64, device=self.device) if grad else None
            gf = torch.empty((n, C_), dtype=self._tfp, device=self.device) if need_gf else None
            _lib.check(entry(*call.entry_args(self), self._ptr(F), stride, self._ptr(scores), self._ptr(atoms), self._ptr(gc),
                             self._ptr(gf), self._stream()))
            return scores, atoms, gc, gf

        if not grad and not fgrad:
            scores, atoms, _, _ = run()
            return (scores, atoms) if per_atom else scores
        # (with fgrad, backward() repeats the call as forward_sum: same offsets and records, the random draws included)
        out = _ScoreFunction.apply(self, run, call, per_atom, call.coords, feat, call.centers, call.pose, field if fgrad else None)
        return out if per_atom else out[0]

    # ------------------------------------------------------------------------------------------
    # SECOND ORDER (per-atom and rigid-twist Hessians of the scores: mvx_score_hessian_batch)
    def score_hessian_batch(self, coords, offsets, centers, channels, radii, field, num_channels=None, pivots=None, per_atom=False):
        """The scores of score_batch with what a Newton step on a rigid pose needs: per molecule the gradient (B, 6) and the
        Hessian (B, 6, 6) of S_b under a twist xi = (tau, omega) about a pivot o_b, which moves the molecule's atoms in the grid
        frame (after centring, relative to the box centre) to p' = exp([omega]x) (p - o_b) + o_b + tau. One more walk of the
        atoms' boxes: the score splits by atom, so its Hessian with respect to the positions is one symmetric 3x3 block per
        atom, H_n = (sum_v e) I + kfac sum_v e d d^T over the voxels and with the terms e of the gradient walk; the admitted set
        is held fixed, as for every gradient here. The 6x6 is sum_n J_n^T H_n J_n with J_n = [I | -[r_n]x], r_n = p_n - o_b, plus
        sum_n 0.5 (g_n r_n^T + r_n g_n^T) - (g_n . r_n) I on the omega-omega block; it is symmetric to the bit.

        coords ... field, num_channels: score_batch's arguments, without random transforms - a Newton step needs the pose the
        caller knows. pivots: (B, 3) in the grid frame, or None: the box centre. Needs output="torch".
        Returns (scores (B,), twist_grad (B, 6), twist_hess (B, 6, 6)), float64 on this device; with per_atom=True also
        (atom_grad (N, 3), atom_hess (N, 6)): dS/dp_n and H_n as (xx, xy, xz, yy, yz, zz), in the grid frame. The scores are
        score_batch's bits, atom_grad those of its dS/dcoords on an unrotated call. Binary density gives zero derivatives but
        scores; an atom that reaches no voxel has exact zero rows and does not enter the sums. Deterministic, no atomics: a
        molecule's values do not depend on its batch. Plain values, NOT part of the autograd graph: inputs that require grad are
        read as values. Channel-wise radii with features raise NotImplementedError."""
        return self._score_hessian_batch(coords, offsets, centers, channels, radii, field, num_channels, pivots, per_atom)

    def score_hessian_posed_batch(self, coords, offsets, centers, quaternions, translations, channels, radii, field,
                                  num_channels=None, pivots=None, per_atom=False):
        """score_hessian_batch with one explicit rigid pose per molecule (forward_posed_batch's arguments and records).
        pivots=None: `translations` rounded to float32 and widened - the point the record maps the centre to - so that
        `apply_twist(quaternions, translations, xi)` realises the twist xi exactly."""
        self._hessian_guard(channels)
        self._check_pose(self._pose_count(offsets), centers, quaternions, translations)
        return self._score_hessian_batch(coords, offsets, centers, channels, radii, field, num_channels, pivots, per_atom,
                                         posed=(quaternions, translations))

    def _hessian_guard(self, channels):
        """What a Hessian call refuses before it looks at anything else."""
        if self.output != "torch":
            raise ValueError("score_hessian_batch / score_hessian_posed_batch need output='torch': the results are tensors on the "
                             "voxelizer's device")
        if self.is_radii_type_channel_wise and channels is not None and channels.ndim != 1:
            raise NotImplementedError("score_hessian_batch does not support channel-wise radii with features: score_posed_batch "
                                      "(score_batch) on a differentiable voxelizer gives their first-order gradients")

    def _hessian_rules(self, field, pivots):
        """For the builders' `check`: the family rules of a Hessian call, the field's shape and the pivots'."""
        def check(B, C_, offsets):
            self._check_grid_operand(field, "field", B, C_)
            if pivots is not None:
                assert tuple(pivots.shape) == (B, 3), f"pivots does not match dimension: {tuple(pivots.shape)} vs {(B, 3)}"

        return check

    def _score_hessian_batch(self, coords, offsets, centers, channels, radii, field, num_channels=None, pivots=None, per_atom=False,
                             posed=None):
        """score_hessian_batch's call. posed: (quaternions, translations) of score_hessian_posed_batch."""
        self._hessian_guard(channels)
        with torch.no_grad():  # (plain values: inputs that require grad are read as values)
            call = self._batch_call(coords, offsets, centers, channels, radii, num_channels, posed=posed, device=True,
                                    check=self._hessian_rules(field, pivots))
            return self._score_hessian(call, field, pivots, posed, per_atom)

    def _score_hessian(self, call, field, pivots, posed, per_atom, torsions=None):
        """The body of the Hessian entries, under no_grad: one mvx_score_hessian_batch or mvx_score_hessian_views call. Returns
        (scores, twist_grad, twist_hess), with per_atom also (atom_grad, atom_hess): one row per atom of a batch, per
        (view, atom) of the selection of a views call. torsions: (T, axes, moves) as _torsion_arrays gives them - then one
        mvx_score_hessian_flex_batch call, G (B, n) and H (B, n, n) for n = 6 + T, and atom_pos behind the per-atom rows."""
        F, stride = self._grid_operand(field, call.C, self._gdt)
        piv = self._hessian_pivots(pivots, posed)
        self._select_rows(call, per_atom)
        B, rows, n = call.B, call.rows, 6 if torsions is None else 6 + torsions[0]
        f64 = dict(dtype=torch.float64, device=self.device)
        scores, G, H = torch.empty(B, **f64), torch.empty((B, n), **f64), torch.empty((B, n, n), **f64)
        widths = () if not per_atom else (3, 6) if torsions is None else (3, 6, 3)  # atom_grad, atom_hess, atom_pos
        per = tuple(torch.empty((rows, w), **f64) for w in widths)
        ag, ah, ap = (per + (None, None, None))[:3]
        head = (*call.entry_args(self), self._ptr(F), stride, self._ptr(piv), self._ptr(scores), self._ptr(ag), self._ptr(ah))
        if torsions is None:
            entry = call.pick(self._lib.mvx_score_hessian_batch, self._lib.mvx_score_hessian_views)
            _lib.check(entry(*head, self._ptr(G), self._ptr(H), self._stream()))
        else:  # (the twist outputs of its own are not asked for: they are G[:, :6] and H[:, :6, :6])
            T, ax, mv = torsions
            _lib.check(self._lib.mvx_score_hessian_flex_batch(*head, None, None, T, self._ptr(ax), self._ptr(mv), self._ptr(G),
                                                              self._ptr(H), self._ptr(ap), self._stream()))
        return (scores, G, H) + per

    def score_hessian_views(self, coords, centers, channels, radii, field, num_channels=None, pivots=None, per_atom=False):
        """score_hessian_batch for B views of ONE shared cloud, without B copies of it: each view's atoms are selected on the
        device, gathered into a compact batch and walked once (mvx_score_hessian_views). The values are score_hessian_batch's,
        bit for bit, on coords[index], the gathered channels and the offsets of select_views.

        coords (N,3), centers (B,3), channels and radii as score_views, without random transforms; field (C,D,H,W), shared, or
        (B,C,D,H,W), one per view; pivots (B,3) in the grid frame, or None: the box centre. Needs output="torch".
        Returns (scores (B,), twist_grad (B, 6), twist_hess (B, 6, 6)), float64 on this device: one library call, one stream
        synchronisation (the selection). With per_atom=True the call selects first and also returns (atom_grad (total, 3),
        atom_hess (total, 6), index, offsets): the rows in selection order - row k belongs to atom index[k] of its view;
        views_reduce sums them onto the shared atoms - and (index, offsets) as select_views returns them. Plain values, NOT part
        of the autograd graph. Channel-wise radii with features raise NotImplementedError."""
        return self._score_hessian_views(coords, centers, channels, radii, field, num_channels, pivots, per_atom)

    def score_hessian_posed_views(self, coords, centers, quaternions, translations, channels, radii, field, num_channels=None,
                                  pivots=None, per_atom=False):
        """score_hessian_views with one explicit rigid pose per view (forward_posed_views' arguments and records): the scores,
        twist gradients and twist Hessians of B poses of ONE shared cloud. pivots=None: `translations` rounded to float32 and
        widened, so that `apply_twist(quaternions, translations, xi)` - or lm_step - realises the twist xi exactly."""
        self._hessian_guard(channels)
        self._check_pose(self._pose_count(None, centers), centers, quaternions, translations)
        return self._score_hessian_views(coords, centers, channels, radii, field, num_channels, pivots, per_atom,
                                         posed=(quaternions, translations))

    def _hessian_pivots(self, pivots, posed):
        """The pivots of a Hessian call as the library reads them, or None (the box centre). posed without pivots: the image of
        the centre, the translation as the record holds it."""
        piv = pivots
        if piv is None and posed is not None:
            piv = (posed[1] if _is_torch(posed[1]) else torch.as_tensor(np.asarray(posed[1], dtype=np.float64))).to(torch.float32)
        if piv is None:
            return None
        piv = piv if _is_torch(piv) else torch.as_tensor(np.asarray(piv, dtype=np.float64))
        return piv.to(device=self.device, dtype=torch.float64).contiguous()

    def _score_hessian_views(self, coords, centers, channels, radii, field, num_channels=None, pivots=None, per_atom=False,
                             posed=None):
        """score_hessian_views' call. posed: (quaternions, translations) of score_hessian_posed_views."""
        self._hessian_guard(channels)
        with torch.no_grad():  # (plain values: inputs that require grad are read as values)
            call = self._views_call(coords, centers, channels, radii, num_channels, posed=posed, device=True,
                                    check=self._hessian_rules(field, pivots))
            out = self._score_hessian(call, field, pivots, posed, per_atom)
        return out + (call.index, call.offsets) if per_atom else out

    # ------------------------------------------------------------------------------------------
    # DAMPED NEWTON REFINEMENT OF POSES (mvx_lm_step between two Hessian evaluations; nothing comes to the host in between)
    def lm_step(self, state, trial=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3):
        """One Levenberg-Marquardt bookkeeping step for the B poses of `state` (an LMState), on the device and without a host
        read (mvx_lm_step). trial: (S2, G2, H2), the evaluation at (state.q2, state.t2), or None before the first trial. Per
        pose: a trial with S2 > S becomes the state (lam *= lam_down, taken += 1, dropped = 0), any other is dropped
        (lam *= lam_up, dropped += 1); a pose with dropped >= max_dropped is finished and stays; every other pose gets
        xi = solve(-H + lam I, G) and the next trial (q2, t2) = apply_twist(q, t, xi) (a singular or non-finite system: xi = 0).
        state.q2, state.t2 and state.xi are allocated on the first call and reused. Returns state."""
        return self._lm_step(state, trial, lam_down, lam_up, max_dropped)

    def _lm_step(self, state, trial, lam_down, lam_up, max_dropped, T=None):
        """The body of lm_step and flex_lm_step (T: the torsions of a FlexLMState): the state's tensors checked against their
        shapes for n = 6 + T coordinates, the trial checked, the trial buffers made on the first call, one library call."""
        B, n, f64, ptr = int(state.q.shape[0]), 6 if T is None else 6 + T, torch.float64, self._ptr
        for name, shape, dt in ((("q", (B, 4), f64), ("t", (B, 3), f64)) + (() if T is None else (("theta", (B, T), f64),)) +
                                (("S", (B,), f64), ("G", (B, n), f64), ("H", (B, n, n), f64), ("lam", (B,), f64),
                                 ("taken", (B,), torch.int32), ("dropped", (B,), torch.int32))):
            x = getattr(state, name)
            assert _is_torch(x) and tuple(x.shape) == shape and x.dtype == dt and x.is_contiguous() and self._on_device(x), (
                f"state.{name} should be a contiguous {dt} tensor of shape {shape} on this voxelizer's device")
        if trial is not None:
            assert state.q2 is not None, f"a trial needs the trial pose of an earlier {state.METHOD}"
            S2, G2, H2 = trial
            for name, x, shape in (("S2", S2, (B,)), ("G2", G2, (B, n)), ("H2", H2, (B, n, n))):
                assert _is_torch(x) and tuple(x.shape) == shape and x.dtype == f64 and x.is_contiguous() and self._on_device(x), (
                    f"trial {name} should be a contiguous float64 tensor of shape {shape} on this voxelizer's device")
        else:
            S2 = G2 = H2 = None
        if state.q2 is None:
            for name, like in zip(state.TRIAL + (state.STEP,), state.point() + (state.G,)):
                setattr(state, name, torch.empty_like(like))
        angles, angles2 = ((), ()) if T is None else ((ptr(state.theta),), (ptr(state.theta2),))
        _lib.check(getattr(self._lib, state.ENTRY)(
            self._handle, B, *(() if T is None else (T,)), 0 if trial is None else 1, float(lam_down), float(lam_up),
            int(max_dropped), ptr(state.q), ptr(state.t), *angles, ptr(state.S), ptr(state.G), ptr(state.H), ptr(state.lam),
            ptr(state.taken), ptr(state.dropped), ptr(state.q2), ptr(state.t2), *angles2, ptr(S2), ptr(G2), ptr(H2),
            ptr(getattr(state, state.STEP)), self._stream()))
        return state

    def refine_posed_batch(self, coords, offsets, centers, quaternions, translations, channels, radii, field, num_channels=None,
                           steps=40, lam0=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3, stop_when_done=False):
        """B rigid poses refined together by damped Newton (Levenberg-Marquardt) steps that raise S_b = sum(field * grid_b):
        score_hessian_posed_batch at the start poses, then `steps` rounds of lm_step and an evaluation at the trial poses, and
        a last lm_step that decides on the last trial. Each pose has its own damping and is accepted or dropped on the device;
        nothing is read back inside the loop (stop_when_done=True reads one flag per round and stops once every pose has
        dropped max_dropped steps in a row). A finished pose keeps being evaluated where it stands.

        coords ... field, num_channels: score_hessian_posed_batch's arguments; the pose tensors are not modified. lam0: the
        first damping, a float or (B,), or None: 1e-3 * max|H_b| per pose.
        Returns (quaternions (B, 4), translations (B, 3), scores (B,), info): info["lam"], info["taken"], info["dropped"] per
        pose, info["evaluations"], info["score_history"] (rounds + 1, B): the accepted score of every pose after each round."""
        self._hessian_guard(channels)
        self._check_pose(self._pose_count(offsets), centers, quaternions, translations)
        return self._refine(lambda q, t: self.score_hessian_posed_batch(coords, offsets, centers, q, t, channels, radii, field, num_channels),
                            LMState, self.lm_step, (quaternions, translations), steps, lam0, lam_down, lam_up, max_dropped, stop_when_done)

    def refine_posed_views(self, coords, centers, quaternions, translations, channels, radii, field, num_channels=None, steps=40,
                           lam0=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3, stop_when_done=False):
        """refine_posed_batch for B poses of ONE shared cloud (score_hessian_posed_views: every evaluation selects the poses'
        atoms, one stream synchronisation each)."""
        self._hessian_guard(channels)
        self._check_pose(self._pose_count(None, centers), centers, quaternions, translations)
        return self._refine(lambda q, t: self.score_hessian_posed_views(coords, centers, q, t, channels, radii, field, num_channels),
                            LMState, self.lm_step, (quaternions, translations), steps, lam0, lam_down, lam_up, max_dropped, stop_when_done)

    def _refine(self, evaluate, State, step, start, steps, lam0, lam_down, lam_up, max_dropped, stop_when_done):
        """The loop of refine_posed_batch / refine_posed_views - State = LMState, step = lm_step, start = (q, t) - and of
        refine_flex_posed_batch - FlexLMState, flex_lm_step, (q, t, theta): evaluate(*point) -> (S, G (B, n), H (B, n, n)) at
        the start and at every trial point of the state. Returns the state's point, the scores and info."""
        assert int(steps) >= 0, "steps must be >= 0"
        with torch.no_grad():
            def own(x):  # a float64 copy on this device: the caller's poses are not modified
                x = x if _is_torch(x) else torch.as_tensor(np.asarray(x, dtype=np.float64))
                return x.detach().to(device=self.device, dtype=torch.float64).clone().contiguous()

            # (the rules of the arguments fire here, before anything is copied)
            S, G, H = evaluate(*start)
            point = [own(x) for x in start]
            B = int(point[0].shape[0])
            if lam0 is None:
                lam = (1e-3 * H.abs().reshape(B, int(G.shape[1]) ** 2).amax(dim=1) if B else
                       torch.zeros(0, dtype=torch.float64, device=self.device))
            else:
                lam = (lam0.detach().to(device=self.device, dtype=torch.float64) if _is_torch(lam0) else
                       torch.as_tensor(np.asarray(lam0, dtype=np.float64), device=self.device)).expand(B).clone()
            state = State(*point, S.clone(), G.clone(), H.clone(), lam.contiguous())
            history = torch.empty((int(steps) + 1, B), dtype=torch.float64, device=self.device)
            history[0] = state.S
            kw = dict(lam_down=lam_down, lam_up=lam_up, max_dropped=max_dropped)
            step(state, **kw)
            evaluations, rounds = 1, 0
            for r in range(int(steps)):
                trial = evaluate(*state.trial())
                evaluations += 1
                step(state, trial, **kw)
                history[r + 1] = state.S
                rounds = r + 1
                if stop_when_done and bool((state.dropped >= max_dropped).all()):
                    break
            info = dict(lam=state.lam, taken=state.taken, dropped=state.dropped, evaluations=evaluations,
                        score_history=history[:rounds + 1])
        return state.point() + (state.S, info)

    # ------------------------------------------------------------------------------------------
    # TORSION COORDINATES (rotatable bonds next to the rigid twist: mvx_apply_torsions, mvx_score_hessian_flex_batch,
    # mvx_flex_lm_step; batch form only - views cull atoms, and an axis atom may be culled)
    def _flex_guard(self, channels, what):
        if self.output != "torch":
            raise ValueError(f"{what} needs output='torch': the results are tensors on the voxelizer's device")
        if channels is not None:
            self._hessian_guard(channels)

    def _torsion_arrays(self, offsets, axes, moves, angles=None, convert=True):
        """(B, T, axes, moves, angles) as the library reads them: int32 and float64 tensors on this device, behind their shape
        rules. convert=False: the rules alone."""
        def shape(x):
            return tuple(getattr(x, "shape", ()))

        off = np.asarray(offsets, dtype=np.int64)
        B, N = off.shape[0] - 1, int(off[-1]) if off.shape[0] else 0
        assert len(shape(axes)) == 3 and shape(axes)[0] == B and shape(axes)[2] == 2, (
            f"axes does not match dimension: {shape(axes)} vs {(B, 'T', 2)}")
        T = int(shape(axes)[1])
        assert T <= 32, f"at most 32 torsions per molecule: {T}"
        assert shape(moves) == (N,), f"moves does not match dimension: {shape(moves)} vs {(N,)}"
        assert angles is None or shape(angles) == (B, T), f"angles does not match dimension: {shape(angles)} vs {(B, T)}"
        if not convert:
            return B, T, None, None, None

        def dev(x, dt):
            x = x.detach() if _is_torch(x) else torch.from_numpy(np.array(x))  # (a copy: the caller's array may be read-only)
            return x.to(device=self.device, dtype=dt).contiguous()

        return B, T, dev(axes, torch.int32), dev(moves, torch.int32), None if angles is None else dev(angles, torch.float64)

    def apply_torsions(self, coords, offsets, axes, moves, angles):
        """The conformers C(theta) of B molecules stored back to back, on the device (mvx_apply_torsions): for k = 0 .. T-1 in
        order the atoms with bit k of `moves` set are turned by angles[b, k] about the current axis from atom axes[b, k, 0] to
        atom axes[b, k, 1] (local indices), through the latter. coords (N, 3); offsets (B + 1,); axes (B, T, 2) int32, padded
        with -1; moves (N,) int32; angles (B, T) radians. Applying angles and then more angles to the result is the same as
        applying their sum. An angle of exactly 0 and an inert torsion (padding, an index outside the molecule, coincident
        axis atoms) turn nothing. Returns the new coordinates (N, 3), float64 on this device. The tree rules are not checked
        here: check_torsions.

        Outside autograd unless the voxelizer was made with torsion_grad=True (and differentiable=True). Then, with grad mode
        on and `coords` or `angles` a tensor on this device that requires grad, the call is part of the autograd graph: the
        same launch and the same bits, and backward() is mvx_apply_torsions_backward from the returned conformer and the angles
        - dL/dcoords and dL/dangles in the inputs' dtype and shape. The adjoint undoes the turns, which needs the tree rules (an
        axis atom a_k outside its set): outside them the gradients are unspecified. No double backward."""
        self._flex_guard(None, "apply_torsions")
        assert len(getattr(coords, "shape", ())) == 2 and coords.shape[1] == 3, "coords should be (N, 3)"
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        assert off[0] == 0 and off[-1] == coords.shape[0], "offsets must span coords"
        self._torsion_arrays(off, axes, moves, angles, convert=False)
        wanted = self._torsion_grad_wanted(coords, angles)  # (its refusal needs no device)
        B, T, ax, mv, th = self._torsion_arrays(off, axes, moves, angles)
        if wanted:
            tracked = lambda x: x if _is_torch(x) and x.requires_grad else None  # noqa: E731
            return _TorsionFunction.apply(self, (off, B, T, ax, mv), self._device_coords(coords), th, tracked(coords), tracked(angles))
        return self._apply_torsions(self._device_coords(coords), off, B, T, ax, mv, th)

    def _torsion_grad_wanted(self, coords, angles) -> bool:
        """Does apply_torsions record an autograd graph: a torsion_grad voxelizer, grad mode on and coords or angles a tensor
        that requires grad - on this device, or _grad_wanted raises."""
        if not self._tgrad or torch is None or not torch.is_grad_enabled():
            return False
        tracked = [x for x in (coords, angles) if _is_torch(x) and x.requires_grad]
        return bool(tracked) and self._grad_wanted(tracked[0], tracked[-1], None, None, None)

    def _apply_torsions(self, coords, off, B, T, ax, mv, th):
        """The call of apply_torsions, as plain values: coords on this device, the others as _torsion_arrays gives them."""
        with torch.no_grad():
            c = coords.detach().to(torch.float64).contiguous()
            out = torch.empty_like(c)
            _lib.check(self._lib.mvx_apply_torsions(self._handle, self._ptr(c), off.ctypes.data, B, T, self._ptr(ax), self._ptr(mv),
                                                    self._ptr(th), self._ptr(out), self._stream()))
        return out

    def apply_torsions_backward(self, conformer, offsets, axes, moves, angles, grad):
        """The adjoint of apply_torsions (mvx_apply_torsions_backward): from the conformer (N, 3) that apply_torsions returned
        for (offsets, axes, moves, angles) and grad = dL/dconformer (N, 3) to (dL/dcoords (N, 3), dL/dangles (B, T)), float64
        on this device; plain values on any output='torch' voxelizer - what backward() of a recorded apply_torsions calls. The
        turns are undone last first on a copy of the conformer while the rows are pulled back through them; nothing the caller
        passed is modified. An angle of exactly 0 has its true derivative; an inert torsion has +0.0; an atom whose row is all
        zero may have NaN coordinates. Deterministic, no atomics: two runs give the same bits and a molecule's values do not
        depend on its batch. The tree rules are assumed, not checked (check_torsions): outside them the values are
        unspecified."""
        self._flex_guard(None, "apply_torsions_backward")
        assert len(getattr(conformer, "shape", ())) == 2 and conformer.shape[1] == 3, "conformer should be (N, 3)"
        assert tuple(getattr(grad, "shape", ())) == tuple(conformer.shape), (
            f"grad does not match dimension: {tuple(getattr(grad, 'shape', ()))} vs {tuple(conformer.shape)}")
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        assert off[0] == 0 and off[-1] == conformer.shape[0], "offsets must span conformer"
        B, T, ax, mv, th = self._torsion_arrays(off, axes, moves, angles)
        return self._apply_torsions_backward(self._device_coords(conformer), off, B, T, ax, mv, th, self._device_coords(grad))

    def _apply_torsions_backward(self, conformer, off, B, T, ax, mv, th, grad):
        with torch.no_grad():
            c = conformer.detach().to(torch.float64).contiguous()
            g = grad.detach().to(torch.float64).contiguous()
            gc = torch.empty_like(c)
            ga = (torch.empty if c.shape[0] else torch.zeros)((B, T), dtype=torch.float64, device=c.device)  # (no atoms: no launch)
            _lib.check(self._lib.mvx_apply_torsions_backward(self._handle, self._ptr(c), off.ctypes.data, B, T, self._ptr(ax),
                                                             self._ptr(mv), self._ptr(th), self._ptr(g), self._ptr(gc), self._ptr(ga),
                                                             self._stream()))
        return gc, ga

    def score_hessian_flex_batch(self, coords, offsets, centers, channels, radii, field, axes, moves, num_channels=None, pivots=None,
                                 per_atom=False):
        """score_hessian_batch in the coordinates x = (tau, omega, theta_0 .. theta_{T-1}), n = 6 + T: torsion angles about
        rotatable bonds next to the rigid twist (mvx_score_hessian_flex_batch). coords is the conformer the angles are counted
        from: p_n(x) = exp([omega]x) (C(theta)_n - o_b) + o_b + tau in the grid frame, C as apply_torsions.

        coords ... field, num_channels, pivots: score_hessian_batch's arguments; axes (B, T, 2) int32 and moves (N,) int32 as
        apply_torsions takes them, checked by check_torsions on host copies. Returns (scores (B,), G (B, n), H (B, n, n)),
        float64 on this device; G[:, :6] and H[:, :6, :6] are score_hessian_batch's twist_grad and twist_hess, bit for bit;
        H is symmetric to the bit; an inert torsion has a zero entry, row and column. With per_atom=True also (atom_grad
        (N, 3), atom_hess (N, 6), atom_pos (N, 3)): the walk's rows and the grid-frame positions they belong to.
        Deterministic, no atomics; plain values outside autograd. Batch form only: views cull atoms, and an axis atom may be
        culled - repeat the cloud per pose instead. Channel-wise radii with features raise NotImplementedError."""
        self._flex_guard(channels, "score_hessian_flex_batch / score_hessian_flex_posed_batch")
        return self._score_hessian_flex(coords, offsets, centers, channels, radii, field, axes, moves, num_channels, pivots, per_atom)

    def score_hessian_flex_posed_batch(self, coords, offsets, centers, quaternions, translations, channels, radii, field, axes, moves,
                                       num_channels=None, pivots=None, per_atom=False):
        """score_hessian_flex_batch with one explicit rigid pose per molecule (score_hessian_posed_batch's arguments, records
        and default pivots: the translations rounded to float32)."""
        self._flex_guard(channels, "score_hessian_flex_batch / score_hessian_flex_posed_batch")
        self._check_pose(self._pose_count(offsets), centers, quaternions, translations)
        return self._score_hessian_flex(coords, offsets, centers, channels, radii, field, axes, moves, num_channels, pivots, per_atom,
                                        posed=(quaternions, translations))

    def _score_hessian_flex(self, coords, offsets, centers, channels, radii, field, axes, moves, num_channels=None, pivots=None,
                            per_atom=False, posed=None, checked=False):
        """The call of the two flex Hessian entries, behind their guard. checked: the tree rules were asserted already (the
        refinement loop)."""
        if not checked:  # (the torsions' own rules first: they need neither the library nor a device)
            self._torsion_arrays(offsets, axes, moves, convert=False)
            check_torsions(offsets, axes, moves)
        with torch.no_grad():  # (plain values: inputs that require grad are read as values)
            call = self._batch_call(coords, offsets, centers, channels, radii, num_channels, posed=posed, device=True,
                                    check=self._hessian_rules(field, pivots))
            _, T, ax, mv, _ = self._torsion_arrays(call.offsets, axes, moves)
            return self._score_hessian(call, field, pivots, posed, per_atom, torsions=(T, ax, mv))

    def flex_lm_step(self, state, trial=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3):
        """lm_step for the B poses of a FlexLMState, in n = 6 + T coordinates (mvx_flex_lm_step): the same decisions, damping and
        solve, x = solve(-H + lam I, G); an accepted trial also makes theta2 the state's theta, and the next trial is
        (q2, t2) = apply_twist(q, t, x[:6]), theta2 = theta + x[6:]. trial: (S2, G2 (B, n), H2 (B, n, n)) evaluated at
        (state.q2, state.t2, state.theta2), or None before the first trial. With T = 0 the values are lm_step's bits.
        Returns state."""
        B = int(state.q.shape[0])
        assert _is_torch(state.theta) and state.theta.ndim == 2 and state.theta.shape[0] == B and state.theta.shape[1] <= 32, (
            f"state.theta should be a (B, T) tensor with T <= 32")
        T = int(state.theta.shape[1])
        return self._lm_step(state, trial, lam_down, lam_up, max_dropped, T)

    def refine_flex_posed_batch(self, coords, offsets, centers, quaternions, translations, angles, channels, radii, field, axes, moves,
                                num_channels=None, steps=40, lam0=None, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3,
                                stop_when_done=False):
        """refine_posed_batch with rotatable bonds: B poses and their torsion angles refined together by damped Newton steps in
        n = 6 + T coordinates. Every evaluation is apply_torsions from the caller's reference conformer `coords` with the
        state's total angles, then score_hessian_flex_posed_batch at the trial poses; flex_lm_step decides on the device.
        angles (B, T): the start angles, counted from `coords`; the other arguments as refine_posed_batch and
        score_hessian_flex_posed_batch; nothing the caller passed is modified. Batch form only (views cull atoms).
        Returns (quaternions (B, 4), translations (B, 3), angles (B, T), scores (B,), info), info as refine_posed_batch."""
        self._flex_guard(channels, "refine_flex_posed_batch")
        self._check_pose(self._pose_count(offsets), centers, quaternions, translations)
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        self._torsion_arrays(off, axes, moves, angles, convert=False)
        check_torsions(off, axes, moves)
        _, _, ax, mv, _ = self._torsion_arrays(off, axes, moves)

        def evaluate(q, t, theta):
            conformer = self.apply_torsions(coords, off, ax, mv, theta)
            return self._score_hessian_flex(conformer, off, centers, channels, radii, field, ax, mv, num_channels, None, False,
                                            posed=(q, t), checked=True)

        return self._refine(evaluate, FlexLMState, self.flex_lm_step, (quaternions, translations, angles), steps, lam0, lam_down,
                            lam_up, max_dropped, stop_when_done)

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
        """score_views' call. posed: (quaternions, translations) of score_posed_views."""
        self._score_guard(field)
        call = self._views_call(coords, centers, channels, radii, num_channels, random_translation, random_rotation, posed,
                                device=True, score=True,
                                check=lambda B, C_, offsets: self._check_grid_operand(field, "field", B, C_))
        out = self._score(call, field, per_atom)
        return out + (call.index, call.offsets) if per_atom else out

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

    def _autograd(self, launch, ret, call):
        """Run `launch` inside _VoxelizeFunction with the call's record as the backward's spec."""
        r = call.radii
        # radii_grad: the radii as the call hands them to the library (dtype conversion / type padding recorded by autograd)
        rin = r if (self.radii_grad and _is_torch(r) and r.requires_grad) else None
        call.settings = self._grad_settings()
        sig = self.sigma_tensor
        sig = sig if (sig is not None and sig.requires_grad) else None
        rsc = call.rten if (call.rten is not None and call.rten.requires_grad) else None
        return _VoxelizeFunction.apply(self, launch, ret, call, call.coords, call.channels if call.mode == "features" else None,
                                       call.centers, rin, sig, rsc, call.pose)

    def _grad_settings(self):
        """What the backward reads from the voxelizer rather than from the call: density, sigma and radii type."""
        return (self.density_type, float(self._sigma) if self.is_density_type_gaussian else None, self.radii_type)

    def _same_settings(self, spec):
        """backward() of a recorded call: the settings it reads from the voxelizer must be the forward's."""
        now = self._grad_settings()
        if now != spec.settings:
            raise RuntimeError(
                "the voxelizer's density / sigma / radii type changed between the forward call and backward() "
                f"(forward: {spec.settings}, now: {now}); the gradients would be those of another grid. Restore the "
                "settings before backward(), or use one voxelizer per setting")

    def _backward(self, spec, c, f, grad, need_features, need_radii=False, need_sigma=False, need_rscalar=False):
        """(dL/dcoords (N,3) float64, dL/dfeatures (N,C) or None, dL/dradii shaped and typed like the call's radii or None,
        dL/dsigma and dL/d(scalar radius) as 0-dim float64 device tensors or None) for dL/dgrid = grad, on the current stream.
        spec: the forward call's _Call; c, f: its coords and features as autograd saved them."""
        self._same_settings(spec)
        g = grad.to(device=self.device, dtype=self._gdt).contiguous()
        gc = torch.empty((c.shape[0], 3), dtype=torch.float64, device=self.device)
        gf = torch.empty((c.shape[0], spec.C), dtype=self._tfp, device=self.device) if need_features else None
        r = spec.radii
        gr = torch.zeros(r.shape[0], dtype=torch.float64, device=self.device) if need_radii else None
        gs = torch.zeros(2, dtype=torch.float64, device=self.device) if (need_sigma or need_rscalar) else None  # [sigma, radius]
        gsig = gs[0] if need_sigma else None
        grs = gs[1] if need_rscalar else None
        if c.shape[0] == 0:  # no atoms: no gradient rows (the library would see null outputs); channel-wise radii get zeros
            return gc, gf, None if gr is None else gr.to(r.dtype), gsig, grs
        args = spec.batch_args(self, c, f if spec.mode == "features" else None) + (self._ptr(g), self._ptr(gc), self._ptr(gf))
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
        gp = torch.zeros((spec.B, 10), dtype=torch.float64, device=self.device)
        if c.shape[0] == 0 or spec.B == 0:
            return gp
        _lib.check(self._lib.mvx_pose_grad_batch(self._handle, self._ptr(c), self._ptr(gc), spec.offsets.ctypes.data,
                                                 C.addressof(spec.xforms), spec.B, gp.data_ptr(), self._stream()))
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


def _input_grads(vox, spec, c, index, gc, gf, cen, need_c, need_cen, need_pose, up=None, lengths=None):
    """The tail the three backward() share, from the rows to the inputs: (dL/dcoords, dL/dfeatures, dL/dcentres,
    dL/d(packed poses)) from the per-row dL/dcoords `gc` and dL/dfeatures `gf` (each or None). A batch's rows are its atoms'.
    The rows of views (`index`: their selection, as autograd saved it) are summed onto the shared atoms with mvx_views_reduce -
    no autograd index backward, no atomics - and reduced to centres and poses per view. up: the upstream of every row of a
    score call, which scales its saved rows first (the scaled feature rows live only as long as their reduction takes).
    lengths: spec.row_lengths where the caller has them."""
    scaled = (lambda g: g) if up is None else (lambda g: g * up[:, None].to(g.dtype))
    if gc is not None:
        gc = scaled(gc)
    if spec.views:
        gcoords = vox.views_reduce(gc, index, spec.offsets, spec.N) if need_c else None
        gfeat = vox.views_reduce(scaled(gf), index, spec.offsets, spec.N) if gf is not None else None
        c = c[index] if need_pose else None
        one_centre = False
    else:
        gcoords, gfeat = gc if need_c else None, None if gf is None else scaled(gf)
        one_centre = need_cen and cen.numel() == 3  # (a single-molecule call: all rows belong to the one centre)
    gcen = None
    if need_cen:
        if one_centre:
            lengths = None
        elif lengths is None:
            lengths = spec.row_lengths(gc.device)
        gcen = _center_grad(gc, cen, lengths)
    # explicit poses: the per-row gradients reduced to dL/dc, dL/dq, dL/dt per molecule (autograd splits the block)
    gpose = vox._pose_backward(spec, c, gc) if need_pose else None
    return gcoords, gfeat, gcen, gpose


if torch is not None:

    class _VoxelizeFunction(torch.autograd.Function):
        """grid = voxelize(coords, features, center, radii, sigma, scalar radius, packed poses): the forward call as it runs without autograd
        (same kernels, same bits); backward = mvx_backward_batch (mvx_backward_radii_batch with radii, mvx_backward_density_batch
        with sigma or a scalar radius) from the saved inputs and the call's record (`spec`, a _Call)."""

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
            gc, gf, gcen, gpose = _input_grads(ctx.vox, ctx.spec, c, None, gc, gf, cen, need_c, need_cen, need_pose)
            return None, None, None, None, gc, gf, gcen, gr, gsig, grs, gpose


    class _ScoreFunction(torch.autograd.Function):
        """scores (and atom_scores) = score(coords, features, centres, packed poses, field) of a batch, or of B views of one
        shared cloud (no field gradient: `field` is None): the one walk of mvx_score_batch / mvx_score_views also writes
        dS/dcoords and dS/dfeatures per row, which are saved; backward scales each row by its upstream (dL/dS of its molecule or
        view plus, with per_atom, dL/ds_n) and takes the rows to the inputs as _VoxelizeFunction does (_input_grads). No second
        walk."""

        @staticmethod
        def forward(ctx, vox, run, spec, per_atom, c, f, cen, pose, field):
            scores, atoms, gc, gf = run()
            ctx.vox, ctx.spec = vox, spec
            ctx.save_for_backward(c, cen, pose, gc, gf, spec.index)
            ctx.field_like = None if field is None else (field.dtype, field.device)
            if per_atom:
                return scores, atoms
            return (scores,)

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, gs, ga=None):
            c, cen, pose, gc, gf, index = ctx.saved_tensors
            need_c, need_f, need_cen, need_pose, need_field = ctx.needs_input_grad[4:9]
            vox, spec = ctx.vox, ctx.spec
            lengths = spec.row_lengths(c.device)
            up = _row_upstream(gs, ga, lengths, spec.rows)  # dL/ds of every row
            gcoords, gfeat, gcen, gpose = _input_grads(vox, spec, c, index, gc, gf if need_f else None, cen, need_c, need_cen,
                                                       need_pose, up, lengths)
            gfield = None
            if need_field and ctx.field_like is not None:
                # dL/dfield[c, v] = sum_n up_n w[n,c] rho_{n,c}(v): the saved call's grids summed with one float32 weight per atom
                gfield = vox._sum_call(spec, up.to(torch.float32), None, False, coords=c)
                gfield = gfield.to(dtype=ctx.field_like[0]).to(ctx.field_like[1])
            return None, None, None, None, gcoords, gfeat, gcen, gpose, gfield


    class _MomentsFunction(torch.autograd.Function):
        """moments = moments(coords, features, centres, packed poses) of a batch, or of B views of one shared cloud, on a
        moments_grad voxelizer: the forward call as it runs without autograd (same kernels, same bits; for views with the
        selection made before it); backward = mvx_moments_backward_batch / mvx_moments_backward_views from the saved inputs, the
        target as the forward read it and the call's record (`spec`: a random transform's records are reused, not redrawn),
        then the rows taken to the inputs as _VoxelizeFunction does (_input_grads)."""

        @staticmethod
        def forward(ctx, vox, run, spec, c, f, cen, pose):
            out, T = run()
            ctx.vox, ctx.spec = vox, spec
            ctx.save_for_backward(c, f, cen, pose, T, spec.index)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, gm):
            c, f, cen, pose, T, index = ctx.saved_tensors
            need_c, need_f, need_cen, need_pose = ctx.needs_input_grad[3:7]
            gc, gf = ctx.vox._moments_backward(ctx.spec, c, f, T, gm, need_f)
            return (None, None, None) + _input_grads(ctx.vox, ctx.spec, c, index, gc, gf, cen, need_c, need_cen, need_pose)


    class _TorsionFunction(torch.autograd.Function):
        """conformer = apply_torsions(coords, angles) on a torsion_grad voxelizer: the forward call as it runs without autograd
        (same launch, same bits); backward = mvx_apply_torsions_backward from the saved conformer and angles. `c`, `th`: the
        values as the library reads them; `coords`, `angles`: the caller's tensors that require grad, or None."""

        @staticmethod
        def forward(ctx, vox, spec, c, th, coords, angles):
            out = vox._apply_torsions(c, *spec, th)
            ctx.vox, ctx.spec = vox, spec
            ctx.like = tuple(None if x is None else (x.dtype, x.shape) for x in (coords, angles))
            ctx.save_for_backward(out, th)
            return out

        @staticmethod
        @torch.autograd.function.once_differentiable
        def backward(ctx, grad):
            out, th = ctx.saved_tensors
            gc, ga = ctx.vox._apply_torsions_backward(out, *ctx.spec, th, grad)
            like = lambda g, t: None if t is None else g.to(dtype=t[0]).reshape(t[1])  # noqa: E731
            return None, None, None, None, like(gc, ctx.like[0]), like(ga, ctx.like[1])


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
