"""Device helpers the tests/test_hip_*.py files share (torch is imported inside the functions, as the test files do)."""
import numpy as np


def dev(x, grad=False, dtype=None):
    """A host array as a tensor on the GPU (None and scalars pass through); `dtype` converts it there."""
    import torch

    if x is None or np.isscalar(x):
        return x
    if isinstance(x, np.ndarray):
        x = np.require(x, requirements="C")  # (as np.ascontiguousarray, but a 0-d array keeps its shape)
    t = torch.tensor(x, device="cuda", requires_grad=grad)
    return t if dtype is None else t.to(dtype)


def nan(shape, dt=None):
    import torch

    return torch.full(shape, float("nan"), dtype=dt or torch.float64, device="cuda")


def ptr(x):
    return None if x is None else x.data_ptr()


def nc(d):
    return d["C"] if d["mode"] == "types" else None


def grid_dtype(d):
    import torch

    return {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[d["kind"]]


def same_bits(a, b):
    """Two host arrays: the same shape, dtype and bytes."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
