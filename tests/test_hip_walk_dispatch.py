"""Every instantiation of the three walk kernels (grad_kernel, grad_radii_kernel, score_kernel <grid type, mode, gauss,
chanwise>) run once at the smallest shape, each result against the float64 references (tests/grad_reference.py,
tests/score_reference.py): a WalkKey that reached another kernel than the one it names shows as a wrong number. (That every key
maps to its own instantiation is proven without a GPU in tests/test_walk_dispatch_host.py; a wrong grid TYPE is never tried
here - a double kernel on a float grid would read out of bounds.)

Entries: backward (forward_batch + backward()), radius backward (radii_grad=True) and score (score_batch); grid types float32,
bfloat16 and precision 64; variants features with one radius for all channels (scalar radii, or one radius per atom for the
radius walk), features with channel-wise radii, types, single; Gaussian and binary density (the radius walk is Gaussian only:
its binary result, exact zeros without a launch, is tested in tests/test_hip_grad_radii.py). Shape: D = 8 at resolution 0.5, two
molecules of 3 and 5 atoms (two workgroups of four waves); C = 33 for features (one chunk of 32 channels and a remainder of one),
3 for types, 1 for single; the 33 channel-wise radii are all distinct.

Bars: those of the existing tests of each entry (tests/test_hip_grad.py, tests/test_hip_grad_radii.py, tests/test_hip_score.py),
imported from tests/tolerance.py: GRAD_REL * bound + GRAD_ABS on float32 and bfloat16 grids, GRAD64_REL * bound + GRAD64_ABS on
float64 grids and for the scores of binary types / single (exact terms summed in another order), bound = the reference's sum of
the absolute values of the terms.

Discrimination, computed in numpy from the references of this file's data (float32 grids; `python -m tests.test_hip_walk_dispatch`
prints it): the largest |ref_a - ref_b| / (GRAD_REL * bound_a + GRAD_ABS) over the elements of an output, a and b the
references of two neighbouring instantiations:
  Gaussian against binary density   features gradients 6.0e+04 (features) and 1.1e+05 (channel-wise); atom scores 1.5e+04,
                                    1.1e+04, 3.3e+04, 4.1e+04 and scores 5.6e+03, 4.3e+03, 1.3e+04, 2.3e+04 (features, channel-wise,
                                    types, single); the coordinate gradients of binary density are exact zeros
  scalar against channel-wise radii feature gradients 2.8e+04 (Gaussian) and 3.0e+04 (binary), coordinates 1.6e+04, atom
                                    scores 1.5e+03 and 2.9e+03, scores 8.8e+02 and 1.5e+03
  radius walk, one radius per atom against channel-wise: the outputs differ in shape, (8,) against (33,)
so the result of a kernel of the other density or the other radii rule lies hundreds to ten thousands of bars away.
"""
import functools

import numpy as np
import pytest

from tests import grad_reference as gr
from tests import score_reference as sr
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

D, SIZES = 8, (3, 5)
OFF = np.array([0, 3, 8], np.int64)
VARIANTS = {  # name: (mode, C, radii type of backward and score, radii type of the radius walk)
    "features": ("features", 33, "scalar", "atom-wise"),
    "features-chanwise": ("features", 33, "channel-wise", "channel-wise"),
    "types": ("types", 3, "scalar", "atom-wise"),
    "single": ("single", 1, "scalar", "atom-wise"),
}
KINDS = ("f32", "bf16", "f64")


def _bar(kind, exact_terms=False):
    return (GRAD64_REL, GRAD64_ABS) if (kind == "f64" or exact_terms) else (GRAD_REL, GRAD_ABS)


@functools.lru_cache(maxsize=None)
def _data(variant, radii_type, kind):
    """Host arrays of one case (never modified): coordinates, channels, radii, and the upstream gradient / field in float64
    both as drawn and as the kernel reads it (rounded to the grid type)."""
    import torch

    mode, C_, _, _ = VARIANTS[variant]
    rng = np.random.default_rng(41)
    fp = np.float64 if kind == "f64" else np.float32
    N = int(OFF[-1])
    W = 0.5 * (D - 1)
    xyz = rng.uniform(-0.45 * W, 0.45 * W, (N, 3))
    chan = {"features": rng.standard_normal((N, C_)).astype(fp), "types": rng.integers(0, C_, N), "single": None}[mode]
    radii = {"scalar": 1.0, "atom-wise": rng.uniform(0.8, 1.2, N).astype(fp),
             "channel-wise": rng.permutation(np.linspace(0.7, 1.3, C_)).astype(fp)}[radii_type]
    G = rng.standard_normal((len(SIZES), C_, D, D, D))
    dt = {"f32": torch.float32, "bf16": torch.bfloat16, "f64": torch.float64}[kind]
    Gt = torch.tensor(G).to(dt)
    return dict(mode=mode, C=C_, xyz=xyz, chan=chan, radii=radii, radii_type=radii_type, G=Gt, Gref=Gt.to(torch.float64).numpy(),
                kind=kind, precision=64 if kind == "f64" else 32)


@functools.lru_cache(maxsize=None)
def _grad_reference(variant, radii_type, kind, density):
    """tests/grad_reference.py molecule by molecule: coords and features rows of the batch, dL/dradii per atom or summed over
    the batch per channel; each with its bound."""
    d = _data(variant, radii_type, kind)
    out = {}
    for b in range(len(SIZES)):
        lo, hi = int(OFF[b]), int(OFF[b + 1])
        o = gr.reference(d["xyz"][lo:hi], d["Gref"][b], d["radii"][lo:hi] if radii_type == "atom-wise" else d["radii"], radii_type,
                         w=d["chan"][lo:hi] if d["mode"] == "features" else None, mode=d["mode"],
                         types=d["chan"][lo:hi] if d["mode"] == "types" else None, blockdim=8, density=density,
                         precision=d["precision"])
        for k in ("coords", "features", "radii"):
            if k in o:
                out.setdefault(k, []).append(o[k])
    cat = lambda k: tuple(np.concatenate([x[i] for x in out[k]]) for i in (0, 1))
    res = {"coords": cat("coords")}
    if "features" in out:
        res["features"] = cat("features")
    if "radii" in out:  # channel-wise: one radius vector for the batch, the molecules' sums added
        res["radii"] = tuple(sum(x[i] for x in out["radii"]) for i in (0, 1)) if radii_type == "channel-wise" else cat("radii")
    return res


@functools.lru_cache(maxsize=None)
def _score_reference(variant, radii_type, kind, density):
    d = _data(variant, radii_type, kind)
    return sr.batch_reference(d["xyz"], OFF, d["Gref"], d["radii"], radii_type, w=d["chan"] if d["mode"] == "features" else None,
                              mode=d["mode"], types=d["chan"] if d["mode"] == "types" else None, blockdim=8, density=density,
                              precision=d["precision"])


def _close(got, ref_bound, kind, what, exact_terms=False):
    ref, bound = ref_bound
    rel, abs_ = _bar(kind, exact_terms)
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = np.abs(got - ref)
    assert np.all(err <= rel * bound + abs_), (what, float(err.max()), float((err / (rel * bound + abs_)).max()))


def _vox(kind, radii_type, density, **kw):
    import molvoxel_amd as mv

    if kind == "bf16":
        kw["grid_dtype"] = "bfloat16"
    return mv.create_voxelizer(0.5, D, radii_type, density, library="hip", precision=64 if kind == "f64" else 32, blockdim=8, **kw)


def _backward(kind, variant, density, radii_grad):
    """forward_batch + backward() under the case's upstream: (coords.grad, features.grad | None, radii.grad | None)."""
    import torch

    mode, C_, rt_plain, rt_radii = VARIANTS[variant]
    radii_type = rt_radii if radii_grad else rt_plain
    d = _data(variant, radii_type, kind)
    vox = _vox(kind, radii_type, density, differentiable=True, radii_grad=radii_grad)
    c = torch.tensor(d["xyz"], device="cuda", requires_grad=True)
    f = torch.tensor(d["chan"], device="cuda", requires_grad=mode == "features") if d["chan"] is not None else None
    r = d["radii"] if np.isscalar(d["radii"]) else torch.tensor(d["radii"], device="cuda", requires_grad=radii_grad)
    grid = vox.forward_batch(c, OFF, None, f, r, num_channels=C_ if mode == "types" else None)
    assert tuple(grid.shape) == (len(SIZES), C_, D, D, D)
    grid.backward(d["G"].to("cuda"))
    cpu = lambda t: None if t is None else t.double().cpu().numpy()
    return radii_type, cpu(c.grad), cpu(f.grad) if mode == "features" else None, cpu(r.grad) if radii_grad else None


@pytest.mark.parametrize("density", ["gaussian", "binary"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", KINDS)
def test_backward_walk(kind, variant, density):
    radii_type, gc, gf, _ = _backward(kind, variant, density, radii_grad=False)
    ref = _grad_reference(variant, radii_type, kind, density)
    if density == "binary":
        assert np.array_equal(gc, np.zeros_like(gc))
    else:
        assert np.any(ref["coords"][0]) and np.all(ref["coords"][1].max(1) > 0)  # (every atom reaches voxels)
        _close(gc, ref["coords"], kind, "dL/dcoords")
    if gf is not None:
        assert np.all(ref["features"][1] > 0)
        _close(gf, ref["features"], kind, "dL/dfeatures")


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", KINDS)
def test_radius_walk(kind, variant):
    radii_type, gc, gf, grad_r = _backward(kind, variant, "gaussian", radii_grad=True)
    ref = _grad_reference(variant, radii_type, kind, "gaussian")
    assert np.all(ref["radii"][1] > 0)
    _close(grad_r, ref["radii"], kind, "dL/dradii")
    _close(gc, ref["coords"], kind, "dL/dcoords")
    if gf is not None:
        _close(gf, ref["features"], kind, "dL/dfeatures")


@pytest.mark.parametrize("density", ["gaussian", "binary"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("kind", KINDS)
def test_score_walk(kind, variant, density):
    import torch

    mode, C_, radii_type, _ = VARIANTS[variant]
    d = _data(variant, radii_type, kind)
    vox = _vox(kind, radii_type, density)
    dev = lambda x: x if (x is None or np.isscalar(x)) else torch.tensor(x, device="cuda")
    scores, atoms = vox.score_batch(dev(d["xyz"]), OFF, None, dev(d["chan"]), dev(d["radii"]), d["G"].to("cuda"),
                                    num_channels=C_ if mode == "types" else None, per_atom=True)
    s_ref, b_ref, S_ref, Sb_ref = _score_reference(variant, radii_type, kind, density)
    assert np.all(b_ref > 0)
    exact_terms = density == "binary" and mode != "features"  # (tests/test_hip_score.py: field values times 1, in float64)
    _close(atoms.cpu().numpy(), (s_ref, b_ref), kind, "atom scores", exact_terms)
    _close(scores.cpu().numpy(), (S_ref, Sb_ref), kind, "scores", exact_terms)


def _discrimination():
    """The figures of the docstring: how far, in bars, the reference of a neighbouring instantiation lies (float32 grids)."""
    def worst(a, b, kind="f32"):
        rel, abs_ = _bar(kind)
        return float((np.abs(a[0] - b[0]) / (rel * a[1] + abs_)).max())

    for variant in VARIANTS:
        rt = VARIANTS[variant][2]
        g, b = (_grad_reference(variant, rt, "f32", dn) for dn in ("gaussian", "binary"))
        sg, sb = (_score_reference(variant, rt, "f32", dn) for dn in ("gaussian", "binary"))
        row = {k: worst(g[k], b[k]) for k in ("features",) if k in g}
        row["atom scores"], row["scores"] = worst(sg[:2], sb[:2]), worst(sg[2:], sb[2:])
        print(f"gaussian against binary, {variant}: " + ", ".join(f"{k} {v:.3g}" for k, v in row.items()))
    for dn in ("gaussian", "binary"):
        s, c = _grad_reference("features", "scalar", "f32", dn), _grad_reference("features-chanwise", "channel-wise", "f32", dn)
        ss, sc = _score_reference("features", "scalar", "f32", dn), _score_reference("features-chanwise", "channel-wise", "f32", dn)
        print(f"scalar against channel-wise radii, {dn}: features {worst(s['features'], c['features']):.3g}, coords "
              f"{worst(s['coords'], c['coords']) if dn == 'gaussian' else float('nan'):.3g}, atom scores {worst(ss[:2], sc[:2]):.3g}, "
              f"scores {worst(ss[2:], sc[2:]):.3g}")
    a, c = _grad_reference("features", "atom-wise", "f32", "gaussian"), _grad_reference("features-chanwise", "channel-wise", "f32", "gaussian")
    print("radius walk, one radius per atom against channel-wise: dL/dradii shapes", a["radii"][0].shape, c["radii"][0].shape)


if __name__ == "__main__":
    _discrimination()
