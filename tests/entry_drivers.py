"""The driver layer tests/test_hip_dead_atoms.py and tests/test_hip_entry_fuzz.py share: a voxelizer for a row or draw d (the dicts
of tests/dead_atom_rows.py and tests/entry_fuzz_rows.py), its inputs on the device, every batch entry with the row's transform - an
explicit pose, the seeded random rotation of a row that has one, or the centring alone - and the worst error / bar of a module."""
import numpy as np

from tests import grad_reference as gr
from tests.hip_support import dev, nc
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL


def vox(d, kind=None, **kw):
    import molvoxel_amd as mv

    kind = kind or d["kind"]
    extra = {} if d["blockdim"] is None else {"blockdim": d["blockdim"]}
    if kind == "bf16":
        extra["grid_dtype"] = "bfloat16"
    kw.setdefault("sigma", d["sigma"])
    return mv.create_voxelizer(d["res"], d["D"], d["radii_type"], d["density"], library="hip", precision=64 if kind == "f64" else 32,
                               **extra, **kw)


def inputs(d, grad=False, radii_grad=False, host=False):
    """The inputs of a batch on the device (host: as numpy arrays). grad: coordinates, features, centres and poses are leaves;
    radii_grad: the radii too (a scalar radius as a one-element host tensor)."""
    import torch

    conv = (lambda x, g=False: x) if host else dev
    radii = d["radii"]
    if radii_grad and np.isscalar(radii):
        radii = torch.tensor([radii], dtype=torch.float64, requires_grad=True)
    else:
        radii = conv(radii, radii_grad)
    return dict(xyz=conv(d["xyz"], grad), cen=conv(d["cen"], grad), chan=conv(d["chan"], grad and d["mode"] == "features"), radii=radii,
                q=conv(d["q"], grad and d["posed"]), t=conv(d["t"], grad and d["posed"]))


def rot(d):
    """The seeded random rotation of a row that has one: the same quaternions on every call."""
    if "transform" in d and not d["posed"]:
        np.random.seed(d["transform"])
        return dict(random_rotation=True)
    return {}


def forward(vox, d, a, **kw):
    if d["posed"]:
        return vox.forward_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], num_channels=nc(d), **kw)
    return vox.forward_batch(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], num_channels=nc(d), **rot(d), **kw)


def score(vox, d, a, F, per_atom=False):
    if d["posed"]:
        return vox.score_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], F, num_channels=nc(d),
                                     per_atom=per_atom)
    return vox.score_batch(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], F, num_channels=nc(d), per_atom=per_atom, **rot(d))


def sum(vox, d, a, weights=None):
    if d["posed"]:
        return vox.forward_posed_sum(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], weights=weights,
                                     num_channels=nc(d))
    return vox.forward_sum(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], weights=weights, num_channels=nc(d), **rot(d))


def moments(vox, d, a, target=None):
    if d["posed"]:
        return vox.moments_posed_batch(a["xyz"], d["off"], a["cen"], a["q"], a["t"], a["chan"], a["radii"], target=target,
                                       num_channels=nc(d))
    return vox.moments_batch(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], target=target, num_channels=nc(d), **rot(d))


def spec(vox, d, a):
    """The call record as the Python layer builds it for the library (offsets, records, converted arrays)."""
    import torch

    with torch.no_grad():
        if d["posed"]:
            return vox._batch_call(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], nc(d), posed=(a["q"], a["t"]), device=True)
        if rot(d):
            return vox._batch_call(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], nc(d), 0.0, True, device=True)
        return vox._batch_call(a["xyz"], d["off"], a["cen"], a["chan"], a["radii"], nc(d), device=True)


class Worst:
    """The worst error / bar a module has seen per key, and the cases behind it; each module chooses its keys and prints them."""

    def __init__(self):
        self.worst, self.cases = {}, {}

    def note(self, key, ratio):
        self.worst[key] = max(self.worst.get(key, 0.0), float(ratio))
        self.cases[key] = self.cases.get(key, 0) + 1

    def close(self, key, d, got, ref, bound, what, exact_terms=False):
        """The gradient rule with the bars of d's precision; the worst error / bar goes into the report."""
        rel, abs_ = (GRAD64_REL, GRAD64_ABS) if (d["precision"] == 64 or exact_terms) else (GRAD_REL, GRAD_ABS)
        self.note(key, gr.close(got, ref, bound, what, rel, abs_))
