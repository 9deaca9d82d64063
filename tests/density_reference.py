"""float64 reference of the sigma and scalar-radius gradients (mvx_backward_density_batch), derived from the radius gradients
of tests/grad_reference.py (imported unchanged), and the cases the GPU test (tests/test_hip_grad_density.py) runs.

The density is rho = m exp(-0.5 (d / (r sigma))^2) and the membership m (d / r <= 1, the culls) does not depend on sigma, so
sigma d rho / d sigma = r d rho / d r term by term:
  one radius per atom        dL/dsigma = sum_n gr_n r_n / sigma          (bound sum_n br_n r_n / sigma)
  channel-wise radii         dL/dsigma = sum_c gr_c r_c / sigma          (features: per channel; types: per type)
  scalar radius              the reference as atom-wise with np.full(N, r): dL/dr = sum_n gr_n, dL/dsigma = r / sigma dL/dr
The scalar form is valid only when r is exactly representable in float32: only then do the scalar and the atom-wise culls
of the reference coincide (a scalar radius culls unrounded). Scalar test radii come from SCALAR_RADII.
tests/test_density_reference.py pins dL/dsigma against central differences in sigma; the grid is smooth in sigma.
"""
import numpy as np

from tests import grad_reference as gr

SCALAR_RADII = (0.75, 1.0, 1.25, 1.5, 2.0)


def density_grads(xyz, G, radii, radii_type, *, w=None, mode="features", types=None, sigma=0.5, precision=32, **kw):
    """{"sigma": (dL/dsigma, bound)} and for scalar radii {"radius": (dL/dr, bound)} of L = <G, grid> for one molecule.
    Arguments as grad_reference.reference (xyz: the positions the kernel sees); kw: res, blockdim, density."""
    fp = np.float32 if precision == 32 else np.float64
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    N = xyz.shape[0]
    common = dict(w=w, mode=mode, types=types, sigma=sigma, precision=precision, **kw)
    out = {}
    if radii_type == "scalar":
        r = float(radii)
        assert float(np.float32(r)) == r, f"scalar radius {r} is not a float32 value: the atom-wise reference would cull otherwise"
        g, b = gr.reference(xyz, G, np.full(N, r), "atom-wise", **common)["radii"]
        out["radius"] = (float(g.sum()), float(b.sum()))
        rr = np.full(N, r)
    elif radii_type == "channel-wise" and mode == "types":
        g, b = gr.reference(xyz, G, radii, "channel-wise", radii_by_type=True, **common)["radii"]
        rr = np.asarray(radii).astype(fp).astype(np.float64)
    else:  # one radius per atom, or channel-wise features
        g, b = gr.reference(xyz, G, radii, radii_type, **common)["radii"]
        rr = np.asarray(radii).astype(fp).astype(np.float64)
    out["sigma"] = (float((g * rr).sum() / sigma), float((b * rr).sum() / sigma))
    return out


def rotation(q):
    """The linear part of the call's transform for the quaternion q (dL/dcoords = M^T dL/dp)."""
    q0, q1, q2, q3 = (float(x) for x in q)
    return np.array([[q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)],
                     [2 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2 * (q2 * q3 - q0 * q1)],
                     [2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3]])


# The GPU cases: mode, radii type, grid ("f32" | "bf16" | "f64"), D, res, sigma, blockdim, C, molecule sizes, transform.
# Every mode x radii type, every grid type, blockdim 8 and others (ones that do not divide D), resolutions and sigmas other
# than 0.5 within the ranges tests/test_hip_grad_fuzz.py sweeps, C beyond one chunk of 32 channels, ragged batches with empty
# molecules and a random transform per molecule.
CASES = [
    ("features", "scalar", "f32", 20, 0.5, 0.5, 8, 5, [22], False),
    ("features", "scalar", "bf16", 22, 0.4, 0.3, 6, 33, [17, 0, 25, 1, 9], True),
    ("features", "scalar", "f64", 18, 0.75, 1.0, None, 4, [30], True),
    ("types", "scalar", "f32", 23, 0.3, 0.5, 5, 6, [12, 40, 0], True),
    ("types", "scalar", "f64", 17, 1.0, 0.3, 7, 3, [25], False),
    ("single", "scalar", "bf16", 21, 0.5, 1.0, 8, 1, [28], False),
    ("single", "scalar", "f32", 24, 0.4, 0.5, 12, 1, [0, 19, 33], True),
    ("single", "scalar", "f64", 16, 0.5, 0.3, 5, 1, [20], False),
    ("features", "atom-wise", "f32", 20, 0.5, 0.5, 6, 40, [22], False),
    ("features", "atom-wise", "bf16", 19, 0.75, 0.5, 8, 8, [9, 31], True),
    ("features", "atom-wise", "f64", 22, 0.3, 1.0, 7, 3, [35], False),
    ("types", "atom-wise", "f32", 21, 0.5, 0.3, 8, 5, [30, 0, 11], True),
    ("single", "atom-wise", "f32", 20, 1.0, 0.5, 6, 1, [25], True),
    ("single", "atom-wise", "f64", 18, 0.4, 1.0, 8, 1, [14, 14], False),
    ("features", "channel-wise", "f32", 17, 0.5, 0.5, 6, 71, [22], False),
    ("features", "channel-wise", "bf16", 20, 0.4, 1.0, 8, 8, [17, 0, 25, 1, 9], True),
    ("features", "channel-wise", "f64", 18, 0.75, 0.3, 5, 5, [20, 13], True),
    ("types", "channel-wise", "f32", 21, 0.5, 1.0, 6, 5, [30], False),
    ("types", "channel-wise", "bf16", 22, 0.3, 0.3, 8, 4, [21, 8, 0], True),
    ("types", "channel-wise", "f64", 19, 1.0, 0.5, None, 6, [26], True),
]


def make_case(i):
    """The inputs of CASES[i] as numpy arrays: molecules in the call's frame (before centring / transform), features or types,
    radii (scalar: one of SCALAR_RADII), the upstream seed."""
    mode, rt, grid, D, res, sigma, bd, C_, sizes, transform = CASES[i]
    rng = np.random.default_rng(7000 + i)
    W = res * (D - 1)
    mols = [rng.uniform(-W * 0.3, W * 0.3, (n, 3)) for n in sizes]
    centers = rng.uniform(-2, 2, (len(sizes), 3))
    mols = [m + centers[b] for b, m in enumerate(mols)]
    feats = [rng.standard_normal((n, C_)) for n in sizes]
    types = [rng.integers(0, C_, n) for n in sizes]
    scale = res / 0.5
    if rt == "scalar":
        radii = float(rng.choice(SCALAR_RADII))  # (float32 values: the reference's condition)
    elif rt == "atom-wise":
        radii = rng.uniform(0.8, 2.0, sum(sizes)) * scale
    else:
        radii = rng.choice([0.9, 1.4, 2.0], C_) * scale
        radii[C_ - 1] = 2.3 * scale  # the largest radius (the cull's) in the last chunk
    precision = 64 if grid == "f64" else 32
    return dict(mode=mode, radii_type=rt, grid=grid, D=D, res=res, sigma=sigma, blockdim=bd, C=C_, sizes=sizes,
                transform=transform, mols=mols, centers=centers, feats=feats, types=types, radii=radii, precision=precision,
                gseed=9000 + i)


def case_reference(case, positions, G64, density="gaussian"):
    """Sums of density_grads over the molecules of a case. positions: per molecule the (n, 3) atoms as the kernel sees them
    (None for an empty molecule); G64: (B, C, D, D, D) float64. Returns {"sigma": (g, b), "radius": (g, b) | absent} and the
    number of molecules that put density on the grid (a non-zero bound)."""
    fp = np.float32 if case["precision"] == 32 else np.float64
    offsets = np.cumsum([0] + case["sizes"])
    tot = {}
    reached = 0
    for b, n in enumerate(case["sizes"]):
        if n == 0:
            continue
        rt = case["radii_type"]
        radii = case["radii"] if rt != "atom-wise" else case["radii"][offsets[b]:offsets[b + 1]]
        if rt != "scalar":
            radii = np.asarray(radii).astype(fp)
        w = case["feats"][b].astype(fp).astype(np.float64) if case["mode"] == "features" else None
        o = density_grads(positions[b], G64[b], radii, rt, w=w, mode=case["mode"], types=case["types"][b], sigma=case["sigma"],
                          precision=case["precision"], res=case["res"], blockdim=case["blockdim"], density=density)
        reached += o["sigma"][1] > 0.0
        for k, (g, bnd) in o.items():
            tot[k] = (tot[k][0] + g, tot[k][1] + bnd) if k in tot else (g, bnd)
    return tot, reached
