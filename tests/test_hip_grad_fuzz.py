"""Randomised sweep of the backward pass (mvx_backward_batch / mvx_backward_radii_batch) against the float64 reference
(tests/grad_reference.py, pinned on the CPU by tests/test_grad_reference.py).

Single molecules (160 seeds): grid size (test_hip_fuzz.DIMS), resolution 0.3 ... 1.0, sigma, blockdim (None, D, ones that do
not divide D), density, radii type x mode, C in 1 ... 71 (partial chunks of 32), N in 1 ... 3000, spread / cluster / shell
layouts with atoms on grid nodes at r = 2 res and one past the box face, precision 32 / 64, bfloat16 grids, radius
gradients, numpy or device centres, random transforms. Batches (40 seeds): ragged sizes with empty molecules first, last
and back to back, per-molecule centres and random transforms, D up to 128, every mode, radii type and precision.

Per-atom outputs (coordinates, features, atom-wise radii) are checked on a seeded sample of at most 32 atoms per molecule
that always holds the atoms on grid nodes and the one past the box face; sums over atoms (channel-wise radii, radii by
type, centres) against the full reference. Bars (tests/tolerance.py): 2e-5 bound + 1e-7 at precision 32, GRAD64_REL bound
+ GRAD64_ABS at precision 64. Binary density: zero coordinate and radius gradients, and with an integer upstream the
feature gradients are the sums of G over each atom's support bit for bit (the backward's support is the forward's, ties
included). The grid of every differentiable call is the plain voxelizer's bit for bit.
"""
import json
import os

import numpy as np
import pytest

from tests import grad_reference as gr
from tests.test_hip_fuzz import DIMS
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

N_SINGLE = 160
N_BATCH = 40
CHANNELS = [1, 2, 5, 8, 16, 31, 32, 33, 40, 64, 65, 71]
SAMPLE = 32

_WORST = {}  # (output kind, precision) -> worst error / bar over the sweep


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    lines = [f"{k[0]:>10s} p{k[1]}: worst error / bar {v:.3g}" for k, v in sorted(_WORST.items())]
    print("\n" + "\n".join(lines))
    path = os.environ.get("MVX_GRAD_FUZZ_REPORT")
    if path:
        with open(path, "w") as fh:
            json.dump({f"{k[0]} p{k[1]}": v for k, v in sorted(_WORST.items())}, fh, indent=1)


def _check(kind, precision, got, ref, bound, what):
    rel, abs_ = (GRAD_REL, GRAD_ABS) if precision == 32 else (GRAD64_REL, GRAD64_ABS)
    ratio = gr.close(got, ref, bound, what, rel, abs_)
    key = (kind, precision)
    _WORST[key] = max(_WORST.get(key, 0.0), ratio)


def _rotation(q):
    q0, q1, q2, q3 = (float(x) for x in q)
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


def _geometry(rng, N, D, res, style):
    """(N, 3) atoms; the first k = min(N, 5) on grid nodes (ties at r = 2 res), atom k past a box face."""
    W = res * (D - 1)
    if style == "spread":
        xyz = rng.uniform(-W / 2 - 2.0, W / 2 + 2.0, (N, 3))
    elif style == "cluster":  # dense: many atoms per voxel neighbourhood
        xyz = rng.normal(0.0, max(0.3, W / 12), (N, 3)) + rng.uniform(-W / 4, W / 4, 3)
    else:  # shells at the faces of the box: cull edge cases
        xyz = rng.uniform(-W / 2, W / 2, (N, 3))
        ax = rng.integers(0, 3, N)
        xyz[np.arange(N), ax] = rng.choice([-1.0, 1.0], N) * (W / 2 + rng.uniform(-1.2, 1.2, N))
    k = min(N, 5)
    xyz[:k] = rng.integers(0, D, (k, 3)) * res - W / 2
    if N > k:
        xyz[k] = [W / 2 + rng.uniform(0.1, 0.9) * res, rng.uniform(-W / 4, W / 4), rng.uniform(-W / 4, W / 4)]
    return xyz, list(range(min(N, k + 1)))


def _radii(rng, radii_type, N, C_, res, k):
    base_r = float(rng.choice([0.6, 1.0, 1.5, 2.2])) * max(res / 0.5, 0.6)
    if radii_type == "scalar":
        return 2 * res if rng.random() < 0.3 else base_r
    if radii_type == "atom-wise":
        r = (base_r * rng.uniform(0.6, 1.4, N)).astype(np.float64)
        r[:k] = 2 * res  # ties stay ties
        return r
    r = base_r * rng.uniform(0.6, 1.4, C_)
    r[0] = 2 * res
    return r


def _draw(seed):
    rng = np.random.default_rng(30_000 + seed)
    D = int(rng.choice(DIMS))
    res = float(rng.choice([0.3, 0.4, 0.5, 0.75, 1.0]))
    blockdim = rng.choice([None, None, 4, 5, 7, 8, 12, 16, D])
    blockdim = None if blockdim is None else int(blockdim)
    density = str(rng.choice(["gaussian", "gaussian", "binary"]))
    sigma = float(rng.choice([0.3, 0.5, 1.0]))
    mode = str(rng.choice(["features", "types", "single"]))
    radii_type = str(rng.choice(["scalar", "atom-wise", "channel-wise"]))
    if mode == "single" and radii_type == "channel-wise":
        radii_type = "atom-wise"
    C_ = 1 if mode == "single" else int(rng.choice(CHANNELS))
    if D >= 64:
        C_ = min(C_, 33)
    precision = 64 if rng.random() < 0.35 else 32
    bf16 = precision == 32 and rng.random() < 0.25
    radii_grad = radii_type != "scalar" and rng.random() < 0.5
    center = str(rng.choice(["none", "numpy", "device"]))
    transform = rng.random() < 0.25
    # sums over atoms are checked against the full reference: keep those molecules small
    sums = center == "device" or (radii_grad and radii_type == "channel-wise")
    N = int(rng.choice([1, 2, 7, 33, 64, 65, 200, 300] if sums else [1, 2, 7, 33, 64, 65, 200, 700, 3000]))
    style = str(rng.choice(["spread", "cluster", "shell"]))
    xyz, special = _geometry(rng, N, D, res, style)
    k = min(N, 5)
    cen = rng.uniform(-3, 3, 3) if center != "none" else None
    if cen is not None:
        xyz = xyz + cen
    feats = rng.random((N, C_))
    feats[rng.random((N, C_)) < 0.3] = 0.0
    feats[rng.random((N, C_)) < 0.3] *= -1.0
    types = rng.integers(0, C_, N)
    if N:
        types[0] = C_ - 1
    outside = mode == "types" and radii_type != "channel-wise" and N >= 3 and rng.random() < 0.5
    if outside:
        types[2] = C_ + 2  # beyond the channels of the call (num_channels): ignored by forward and backward
    radii = _radii(rng, radii_type, N, C_, res, k)
    sample = sorted(set(special) | set(rng.choice(N, min(N, SAMPLE - len(special)), replace=False).tolist()))
    return dict(D=D, res=res, blockdim=blockdim, density=density, sigma=sigma, mode=mode, radii_type=radii_type, C=C_,
                precision=precision, bf16=bf16, radii_grad=radii_grad, center=center, transform=transform, N=N, xyz=xyz,
                cen=cen, feats=feats, types=types, outside=outside, radii=radii, sample=sample, sums=sums,
                gseed=int(rng.integers(1 << 30)))


def _voxelizer(case, **kw):
    import molvoxel_amd as mv

    extra = {} if case["blockdim"] is None else {"blockdim": case["blockdim"]}
    return mv.create_voxelizer(case["res"], case["D"], case["radii_type"], case["density"], "hip", sigma=case["sigma"],
                               precision=case["precision"], grid_dtype="bfloat16" if case["bf16"] else None, **extra, **kw)


def _upstream(case, shape):
    """G in the grid's type (small integers for a binary density) and its float64 widening for the reference."""
    import torch

    rng = np.random.default_rng(case["gseed"])
    if case["density"] == "binary":
        G = rng.integers(-3, 4, shape).astype(np.float64)
    else:
        G = rng.standard_normal(shape)
    dt = torch.bfloat16 if case["bf16"] else (torch.float32 if case["precision"] == 32 else torch.float64)
    Gt = torch.as_tensor(G, device="cuda").to(dt)
    return Gt, Gt.double().cpu().numpy()


def _check_molecule(case, p, G64, rot, feats, types, radii, sample, gc, gf, gr_atom, full, tag):
    """Per-atom outputs of one molecule against the reference. p: kernel-frame positions; gc, gf, gr_atom: the library's
    rows for this molecule (gf / gr_atom None when not requested). Returns the full reference when `full`."""
    prec, mode, rt = case["precision"], case["mode"], case["radii_type"]
    kw = dict(w=feats, mode=mode, types=types, res=case["res"], sigma=case["sigma"], blockdim=case["blockdim"],
              density=case["density"], precision=prec, rot=rot, radii_by_type=mode == "types" and rt == "channel-wise")
    ref = gr.reference(p, G64, radii, rt, atoms=None if full else sample, **kw)
    pick = lambda x: x if not full else x[sample]  # noqa: E731
    if case["density"] == "binary":
        assert not np.any(gc), f"{tag}: binary density with coordinate gradients"
        if gr_atom is not None:
            assert not np.any(gr_atom), f"{tag}: binary density with radius gradients"
        if gf is not None:  # integer upstream: exact sums over the support, channel by channel
            want = pick(ref["features"][0])
            got = gf[sample].astype(np.float64)
            assert np.array_equal(got, want), f"{tag}: dL/dfeatures differ from the support sums in " \
                f"{int((got != want).sum())} entries, first at {np.argwhere(got != want)[:3].tolist()}"
        return ref
    gcr, bcr = ref["coords"]
    _check("coords", prec, gc[sample], pick(gcr), pick(bcr), f"{tag}: dL/dcoords")
    if gf is not None:
        gfr, bfr = ref["features"]
        _check("features", prec, gf[sample], pick(gfr), pick(bfr), f"{tag}: dL/dfeatures")
    if gr_atom is not None:
        grr, brr = ref["radii"]
        _check("radii", prec, gr_atom[sample], pick(grr), pick(brr), f"{tag}: dL/dradii")
    if mode == "types" and case["outside"]:
        out = np.flatnonzero(np.asarray(types) >= case["C"])
        assert not np.any(gc[out]), f"{tag}: an atom of a type outside the call has coordinate gradients"
        if gr_atom is not None:
            assert not np.any(gr_atom[out])
    return ref


@pytest.mark.parametrize("seed", range(N_SINGLE))
def test_random_gradient_configuration(seed):
    import torch

    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform
    from molvoxel_amd.voxelizer.hip.voxelizer import transform_on_device

    case = _draw(seed)
    D, C_, N, prec, mode, rt = case["D"], case["C"], case["N"], case["precision"], case["mode"], case["radii_type"]
    tdt = torch.float32 if prec == 32 else torch.float64
    nch = 1 if mode == "single" else C_
    vox = _voxelizer(case, differentiable=True, radii_grad=case["radii_grad"])
    plain = _voxelizer(case)

    def inputs(track):
        c = torch.tensor(case["xyz"], device="cuda", requires_grad=track)
        f = torch.tensor(case["feats"], device="cuda", dtype=tdt, requires_grad=track) if mode == "features" else None
        r = case["radii"]
        if rt != "scalar":
            r = torch.tensor(r, device="cuda", dtype=tdt, requires_grad=track and case["radii_grad"])
        cen = case["cen"]
        if case["center"] == "device":
            cen = torch.tensor(cen, device="cuda", requires_grad=track)
        return c, f, r, cen

    def call(v, c, f, r, cen):
        kw = dict(random_translation=0.7, random_rotation=True) if case["transform"] else {}
        np.random.seed(seed)
        if mode == "features":
            return v.forward_features(c, cen, f, r, **kw)
        if mode == "single":
            return v.forward_single(c, cen, r, **kw)
        t = torch.tensor(case["types"], device="cuda")
        if case["outside"]:
            return v.forward_batch(c, np.array([0, N]), None if cen is None else cen.reshape(1, 3) if torch.is_tensor(cen)
                                   else np.asarray(cen).reshape(1, 3), t, r, num_channels=C_, **kw)[0]
        return v.forward_types(c, cen, t, r, **kw)

    c, f, r, cen = inputs(True)
    grid = call(vox, c, f, r, cen)
    assert grid.grad_fn is not None and tuple(grid.shape) == (nch, D, D, D)
    with torch.no_grad():
        g0 = call(plain, *inputs(False))
    assert torch.equal(grid.detach(), g0), "the differentiable call's grid is not the plain voxelizer's"
    G, G64 = _upstream(case, (nch, D, D, D))
    grid.backward(G)

    # the positions the kernel saw: centring, then the transform drawn in the call (replayed from the same RNG state)
    moved = torch.tensor(case["xyz"], device="cuda")
    if case["cen"] is not None:
        moved = moved - torch.tensor(case["cen"], device="cuda")
    rot = None
    if case["transform"]:
        np.random.seed(seed)
        t, q = draw_forward_transform(0.7, True)
        moved = transform_on_device(moved, None, t, q)
        rot = _rotation(q)
    p = moved.cpu().numpy()
    gc = c.grad.cpu().numpy()
    gf = f.grad.double().cpu().numpy() if f is not None else None
    radii_np = case["radii"] if rt == "scalar" else np.asarray(case["radii"]).astype(np.float32 if prec == 32 else np.float64)
    per_atom_r = case["radii_grad"] and (rt == "atom-wise")
    gra = r.grad.double().cpu().numpy() if per_atom_r else None
    feats = case["feats"].astype(np.float32).astype(np.float64) if prec == 32 else case["feats"]
    tag = {k: v for k, v in case.items() if k not in ("xyz", "feats", "types", "radii", "sample", "cen")}
    ref_mol = _check_molecule(case, p, G64, rot, feats if mode == "features" else None, case["types"], radii_np,
                              case["sample"], gc, gf, gra, case["sums"], tag)
    if case["radii_grad"] and rt == "channel-wise":
        got = r.grad.double().cpu().numpy()
        if case["density"] == "binary":
            assert not np.any(got)
        else:
            want, bound = ref_mol["radii"]
            _check("radii sum", prec, got, want, bound, f"{tag}: channel-wise dL/dradii")
    if case["center"] == "device":
        got = cen.grad.cpu().numpy()
        assert np.allclose(got, -gc.sum(0), rtol=1e-12, atol=1e-12 * np.abs(gc).sum()), "centre != -sum dL/dcoords"
        if case["density"] != "binary":
            want, bound = ref_mol["center"]
            _check("center", prec, got, want, bound, f"{tag}: dL/dcenter")


def _draw_batch(seed):
    rng = np.random.default_rng(40_000 + seed)
    D = int(rng.choice([16, 24, 33, 48, 64, 96, 128]))
    res = float(rng.choice([0.3, 0.5, 0.75, 1.0]))
    blockdim = rng.choice([None, 5, 8, 12])
    blockdim = None if blockdim is None else int(blockdim)
    mode = str(rng.choice(["features", "types", "single"]))
    radii_type = str(rng.choice(["scalar", "atom-wise"] + ([] if mode == "single" else ["channel-wise"])))
    density = str(rng.choice(["gaussian", "gaussian", "binary"]))
    sigma = float(rng.choice([0.3, 0.5, 1.0]))
    C_ = 1 if mode == "single" else int(rng.choice([1, 4, 6, 16, 33, 40]))
    if D > 64:
        C_ = min(C_, 6)
    precision = 64 if rng.random() < 0.4 else 32
    bf16 = precision == 32 and rng.random() < 0.25
    radii_grad = radii_type != "scalar" and rng.random() < 0.6
    center = str(rng.choice(["numpy", "device"]))
    transform = rng.random() < 0.5
    B = int(rng.choice([3, 4, 6, 9])) if D <= 64 else int(rng.choice([3, 4]))
    sums = center == "device" or (radii_grad and radii_type == "channel-wise")
    sizes = [int(rng.choice([1, 7, 40, 300] if sums else [1, 7, 40, 300, 2000])) for _ in range(B)]
    empty = seed % 3  # empty molecules first, last, or back to back in the middle
    if empty == 0:
        sizes[0] = 0
    elif empty == 1:
        sizes[-1] = 0
    else:
        sizes[1] = sizes[2] = 0
    mols, specials = [], []
    for n in sizes:
        xyz, special = _geometry(rng, n, D, res, str(rng.choice(["spread", "cluster", "shell"])))
        mols.append(xyz)
        specials.append(special)
    centers = rng.uniform(-2, 2, (B, 3))
    mols = [m + centers[b] for b, m in enumerate(mols)]
    feats = [rng.random((n, C_)) - 0.3 for n in sizes]
    types = [rng.integers(0, C_, n) for n in sizes]
    r_atom = [_radii(rng, "atom-wise", n, C_, res, min(n, 5)) for n in sizes]
    radii = {"scalar": 1.3 * res / 0.5, "atom-wise": np.concatenate(r_atom),
             "channel-wise": _radii(rng, "channel-wise", 0, C_, res, 0)}[radii_type]
    samples = [sorted(set(s) | set(rng.choice(n, min(n, SAMPLE - len(s)), replace=False).tolist())) if n else []
               for n, s in zip(sizes, specials)]
    return dict(D=D, res=res, blockdim=blockdim, density=density, sigma=sigma, mode=mode, radii_type=radii_type, C=C_,
                precision=precision, bf16=bf16, radii_grad=radii_grad, center=center, transform=transform, sizes=sizes,
                mols=mols, centers=centers, feats=feats, types=types, r_atom=r_atom, radii=radii, samples=samples, sums=sums,
                outside=False, gseed=int(rng.integers(1 << 30)))


@pytest.mark.parametrize("seed", range(N_BATCH))
def test_random_gradient_batch(seed):
    import torch

    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform
    from molvoxel_amd.voxelizer.hip.voxelizer import transform_on_device

    case = _draw_batch(seed)
    D, C_, prec, mode, rt, sizes = case["D"], case["C"], case["precision"], case["mode"], case["radii_type"], case["sizes"]
    B = len(sizes)
    offsets = np.cumsum([0] + sizes)
    tdt = torch.float32 if prec == 32 else torch.float64
    nch = 1 if mode == "single" else C_
    vox = _voxelizer(case, differentiable=True, radii_grad=case["radii_grad"])
    plain = _voxelizer(case)
    kw = dict(random_translation=0.7, random_rotation=True) if case["transform"] else {}

    def inputs(track):
        c = torch.tensor(np.concatenate(case["mols"]), device="cuda", requires_grad=track)
        if mode == "features":
            ch = torch.tensor(np.concatenate(case["feats"]), device="cuda", dtype=tdt, requires_grad=track)
        elif mode == "types":
            ch = torch.tensor(np.concatenate(case["types"]), device="cuda")
        else:
            ch = None
        r = case["radii"]
        if rt != "scalar":
            r = torch.tensor(r, device="cuda", dtype=tdt, requires_grad=track and case["radii_grad"])
        cen = case["centers"]
        if case["center"] == "device":
            cen = torch.tensor(cen, device="cuda", requires_grad=track)
        return c, ch, r, cen

    c, ch, r, cen = inputs(True)
    np.random.seed(seed)
    grid = vox.forward_batch(c, offsets, cen, ch, r, num_channels=C_, **kw)
    assert grid.grad_fn is not None and tuple(grid.shape) == (B, nch, D, D, D)
    with torch.no_grad():
        np.random.seed(seed)
        c0, ch0, r0, cen0 = inputs(False)
        g0 = plain.forward_batch(c0, offsets, cen0, ch0, r0, num_channels=C_, **kw)
    assert torch.equal(grid.detach(), g0), "the differentiable call's grid is not the plain voxelizer's"
    G, G64 = _upstream(case, (B, nch, D, D, D))
    grid.backward(G)

    # per-molecule transforms, drawn in molecule order (empty molecules included)
    np.random.seed(seed)
    draws = [draw_forward_transform(0.7, True) if case["transform"] else (None, None) for _ in range(B)]
    gc = c.grad.cpu().numpy()
    gf = ch.grad.double().cpu().numpy() if mode == "features" else None
    fp = np.float32 if prec == 32 else np.float64
    gra = r.grad.double().cpu().numpy() if (case["radii_grad"] and rt == "atom-wise") else None
    total = None
    chan_r = np.asarray(case["radii"]).astype(fp) if rt == "channel-wise" else None
    tag = {k: v for k, v in case.items() if k in ("D", "res", "blockdim", "density", "sigma", "mode", "radii_type", "C",
                                                   "precision", "bf16", "radii_grad", "center", "transform", "sizes")}
    for b, n in enumerate(sizes):
        lo, hi = offsets[b], offsets[b + 1]
        if n == 0:
            if case["center"] == "device":
                assert not cen.grad[b].any()
            continue
        moved = torch.tensor(case["mols"][b], device="cuda") - torch.tensor(case["centers"][b], device="cuda")
        rot = None
        if case["transform"]:
            t, q = draws[b]
            moved = transform_on_device(moved, None, t, q)
            rot = _rotation(q)
        p = moved.cpu().numpy()
        radii_b = {"scalar": case["radii"], "atom-wise": np.asarray(case["r_atom"][b]).astype(fp), "channel-wise": chan_r}[rt]
        feats = case["feats"][b].astype(fp).astype(np.float64) if mode == "features" else None
        want_sum = case["radii_grad"] and rt == "channel-wise"
        ref = _check_molecule(case, p, G64[b], rot, feats, case["types"][b], radii_b, case["samples"][b], gc[lo:hi],
                              None if gf is None else gf[lo:hi], None if gra is None else gra[lo:hi], case["sums"],
                              dict(tag, molecule=b))
        if want_sum and case["density"] == "gaussian":
            g, bnd = ref["radii"]
            total = (g, bnd) if total is None else (total[0] + g, total[1] + bnd)
        if case["center"] == "device":
            got = cen.grad[b].cpu().numpy()
            assert np.allclose(got, -gc[lo:hi].sum(0), rtol=1e-12, atol=1e-12 * np.abs(gc[lo:hi]).sum()), b
            if case["density"] != "binary":
                _check("center", prec, got, ref["center"][0], ref["center"][1], f"{tag}: dL/dcenter of molecule {b}")
    if case["radii_grad"] and rt == "channel-wise":
        got = r.grad.double().cpu().numpy()
        if case["density"] == "binary":
            assert not np.any(got)
        else:
            _check("radii sum", prec, got, total[0], total[1], f"{tag}: channel-wise dL/dradii of the batch")
