"""CPU self-check of the gradient reference (tests/grad_reference.py), before it judges the HIP backward:
- its per-atom densities add up to the oracles' forward grids (c_oracle at precision 32, numpy_port at precision 64), with
  identical membership, at resolutions and sigmas other than 0.5 and blockdims that do not divide D (per-block culls);
- its gradients match central finite differences of numpy_port.voxelize(precision=64) for coordinates, features,
  atom-wise radii and channel-wise radii (features and types mode), where the support does not move under +-h."""
import numpy as np
import pytest

from tests import grad_reference as gr
from tests.tolerance import GAUSS_TOL, P64_TOL, assert_gaussian


def _forward(xyz, chan, radii, radii_type, D, res, sigma, blockdim, density, precision, num_channels=None):
    from oracle import c_oracle, numpy_port

    kw = dict(radii_type=radii_type, density=density, sigma=sigma, num_channels=num_channels)
    if precision == 32:
        return c_oracle.voxelize(xyz, chan, radii, resolution=res, dimension=D, blockdim=blockdim, **kw).astype(np.float64)
    return numpy_port.voxelize(numpy_port.GridSpec(res, D, blockdim), xyz, chan, radii, precision=64, **kw)


def _case(seed, D, res, C_, N=40):
    rng = np.random.default_rng(seed)
    W = res * (D - 1)
    xyz = rng.uniform(-W / 2 - 1.0, W / 2 + 1.0, (N, 3))
    xyz[:4] = rng.integers(0, D, (4, 3)) * res - W / 2  # on grid nodes (with r = 2 res below: d2 <= T ties)
    xyz[4] = [W / 2 + 0.4 * res, 0.1, -0.2]  # past the box face
    feats = rng.standard_normal((N, C_))
    types = rng.integers(0, C_, N)
    r_atom = rng.uniform(0.7, 1.5, N) * res / 0.5
    r_atom[:4] = 2 * res
    r_chan = rng.uniform(0.7, 1.5, C_) * res / 0.5
    return rng, xyz, feats, types, r_atom, r_chan


SPLIT = [  # res, sigma, blockdim, D
    (0.3, 0.3, 5, 23), (0.5, 1.0, 6, 20), (1.0, 0.5, 7, 17), (0.3, 1.0, None, 26), (1.0, 0.3, 4, 15), (0.5, 0.5, 9, 21)]


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("density", ["gaussian", "binary"])
@pytest.mark.parametrize("res, sigma, blockdim, D", SPLIT)
def test_per_atom_densities_add_up_to_the_oracle_grid(res, sigma, blockdim, D, density, precision):
    C_ = 3
    _, xyz, feats, types, r_atom, r_chan = _case(int(res * 10 + sigma * 100 + D), D, res, C_)
    fp = np.float32 if precision == 32 else np.float64
    feats = feats.astype(fp)
    r_atom, r_chan = r_atom.astype(fp), r_chan.astype(fp)
    tol = GAUSS_TOL if precision == 32 else P64_TOL
    geo = dict(D=D, density=density, blockdim=blockdim, res=res, sigma=sigma, precision=precision)
    N = xyz.shape[0]
    for mode, radii_type, radii in [("features", "scalar", 1.1 * res / 0.5), ("features", "atom-wise", r_atom),
                                    ("features", "channel-wise", r_chan), ("types", "atom-wise", r_atom),
                                    ("types", "channel-wise", r_chan), ("single", "scalar", 0.9 * res / 0.5)]:
        chan = {"features": feats, "types": types, "single": None}[mode]
        ref = _forward(xyz, chan, radii, radii_type, D, res, sigma, blockdim, density, precision,
                       num_channels=None if mode != "types" else C_)
        got = np.zeros_like(ref)
        for n in range(N):
            if mode == "types" and radii_type == "channel-wise":
                rho = gr.atom_grid(xyz, n, np.asarray(radii)[types], "atom-wise", C_, **geo)
            else:
                rho = gr.atom_grid(xyz, n, radii, radii_type, C_, **geo)
            if mode == "features":
                got += feats[n].astype(np.float64)[:, None, None, None] * rho
            else:
                got[0 if mode == "single" else types[n]] += rho[0]
        if density == "binary" and mode != "features":
            assert np.array_equal(got, ref), (mode, radii_type)
        else:
            assert_gaussian(got, ref, tol)
    # the per-atom membership is the oracle's for one atom alone, voxel for voxel (ties on grid nodes included)
    for n in range(6):
        one = _forward(xyz[n:n + 1], None, r_atom[n:n + 1], "atom-wise", D, res, sigma, blockdim, density, precision)
        assert np.array_equal(gr.atom_grid(xyz, n, r_atom, "atom-wise", 1, **geo) != 0, one != 0), n


def _support(xyz, radii, radii_type, C_, D, res, sigma, blockdim):
    """(N, C', D, D, D) where each atom alone reaches (float64 oracle), channel by channel for channel-wise radii."""
    from oracle import numpy_port

    spec = numpy_port.GridSpec(res, D, blockdim)
    out = []
    for n in range(xyz.shape[0]):
        if radii_type == "channel-wise":
            g = numpy_port.voxelize(spec, xyz[n:n + 1], np.ones((1, C_)), radii, radii_type="channel-wise", sigma=sigma,
                                    precision=64)
        else:
            r = radii if radii_type == "scalar" else radii[n:n + 1]
            g = numpy_port.voxelize(spec, xyz[n:n + 1], None, r, radii_type=radii_type, sigma=sigma, precision=64)
        out.append(g != 0)
    return np.stack(out)


FD = [  # res, sigma, blockdim, D
    (0.3, 0.5, 7, 18), (0.5, 1.0, 6, 16), (1.0, 0.3, 5, 13), (0.5, 0.5, None, 15), (0.3, 0.3, 9, 22), (1.0, 1.0, 4, 11)]


@pytest.mark.parametrize("res, sigma, blockdim, D", FD)
def test_reference_matches_finite_differences_at_precision_64(res, sigma, blockdim, D):
    from oracle import numpy_port

    C_, N, h = 3, 6, 1e-6
    rng = np.random.default_rng(int(res * 1000 + sigma * 10 + D))
    W = res * (D - 1)
    xyz = rng.uniform(-W * 0.35, W * 0.35, (N, 3))
    feats = rng.standard_normal((N, C_))
    types = rng.integers(0, C_, N)
    r_atom = rng.uniform(0.8, 1.6, N) * res / 0.5
    r_chan = rng.uniform(0.8, 1.6, C_) * res / 0.5
    G = rng.standard_normal((C_, D, D, D))
    spec = numpy_port.GridSpec(res, D, blockdim)

    def L(x, chan, radii, radii_type):
        g = numpy_port.voxelize(spec, x, chan, radii, radii_type=radii_type, sigma=sigma, precision=64, num_channels=C_)
        return float((g * G).sum())

    kw = dict(res=res, sigma=sigma, blockdim=blockdim, precision=64)
    checked = {"coords": 0, "features": 0, "atom-wise": 0, "channel-wise": 0, "by type": 0}

    def agree(fd, an, what):
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1.0), (what, fd, an)
        checked[what] += 1

    # coordinates and features (atom-wise radii)
    ref = gr.reference(xyz, G, r_atom, "atom-wise", w=feats, **kw)
    base = _support(xyz, r_atom, "atom-wise", C_, D, res, sigma, blockdim)
    for n in range(N):
        for a in range(3):
            x = [xyz.copy(), xyz.copy()]
            x[0][n, a] += h
            x[1][n, a] -= h
            if not all(np.array_equal(_support(xi, r_atom, "atom-wise", C_, D, res, sigma, blockdim), base) for xi in x):
                continue  # the support moved: the a.e. derivative does not see the jump
            agree((L(x[0], feats, r_atom, "atom-wise") - L(x[1], feats, r_atom, "atom-wise")) / (2 * h),
                  ref["coords"][0][n, a], "coords")
        for c in range(C_):
            f = [feats.copy(), feats.copy()]
            f[0][n, c] += h
            f[1][n, c] -= h
            agree((L(xyz, f[0], r_atom, "atom-wise") - L(xyz, f[1], r_atom, "atom-wise")) / (2 * h),
                  ref["features"][0][n, c], "features")
        r = [r_atom.copy(), r_atom.copy()]
        r[0][n] += h
        r[1][n] -= h
        if all(np.array_equal(_support(xyz, ri, "atom-wise", C_, D, res, sigma, blockdim), base) for ri in r):
            agree((L(xyz, feats, r[0], "atom-wise") - L(xyz, feats, r[1], "atom-wise")) / (2 * h), ref["radii"][0][n],
                  "atom-wise")
    # channel-wise radii: features mode, and types mode (the gradient of each type's radius)
    refc = gr.reference(xyz, G, r_chan, "channel-wise", w=feats, **kw)
    reft = gr.reference(xyz, G, r_chan, "channel-wise", mode="types", types=types, radii_by_type=True, **kw)
    basec = _support(xyz, r_chan, "channel-wise", C_, D, res, sigma, blockdim)
    for c in range(C_):
        r = [r_chan.copy(), r_chan.copy()]
        r[0][c] += h
        r[1][c] -= h
        if not all(np.array_equal(_support(xyz, ri, "channel-wise", C_, D, res, sigma, blockdim), basec) for ri in r):
            continue
        agree((L(xyz, feats, r[0], "channel-wise") - L(xyz, feats, r[1], "channel-wise")) / (2 * h), refc["radii"][0][c],
              "channel-wise")
        agree((L(xyz, types, r[0], "channel-wise") - L(xyz, types, r[1], "channel-wise")) / (2 * h), reft["radii"][0][c],
              "by type")
    assert checked["coords"] >= 10 and checked["features"] == N * C_ and checked["atom-wise"] >= 3, checked
    assert checked["channel-wise"] >= 1, checked


def test_channel_wise_radii_beyond_one_chunk_match_finite_differences():
    """C = 40 channel-wise radii, the largest (the cull's) in the second chunk of 32, res 0.3 / sigma 1.0, blockdim 7."""
    from oracle import numpy_port

    res, sigma, blockdim, D, C_, N, h = 0.3, 1.0, 7, 17, 40, 4, 1e-6
    rng = np.random.default_rng(41)
    W = res * (D - 1)
    xyz = rng.uniform(-W * 0.3, W * 0.3, (N, 3))
    feats = rng.standard_normal((N, C_))
    r_chan = rng.uniform(0.5, 0.9, C_)
    r_chan[35] = 1.05
    G = rng.standard_normal((C_, D, D, D))
    spec = numpy_port.GridSpec(res, D, blockdim)
    ref = gr.reference(xyz, G, r_chan, "channel-wise", w=feats, res=res, sigma=sigma, blockdim=blockdim, precision=64)
    base = _support(xyz, r_chan, "channel-wise", C_, D, res, sigma, blockdim)
    checked = []
    for c in range(C_):
        r = [r_chan.copy(), r_chan.copy()]
        r[0][c] += h
        r[1][c] -= h
        if not all(np.array_equal(_support(xyz, ri, "channel-wise", C_, D, res, sigma, blockdim), base) for ri in r):
            continue
        L = [float((numpy_port.voxelize(spec, xyz, feats, ri, radii_type="channel-wise", sigma=sigma, precision=64) * G).sum())
             for ri in r]
        fd = (L[0] - L[1]) / (2 * h)
        assert abs(fd - ref["radii"][0][c]) <= 1e-6 * max(abs(ref["radii"][0][c]), 1.0), (c, fd, ref["radii"][0][c])
        checked.append(c)
    assert len(checked) >= 30 and 35 in checked, checked


def test_rotation_and_centre_follow_the_chain_rule():
    """rot=M gives M^T g per row with a bound that covers it; the centre is minus the sum of the rows."""
    rng = np.random.default_rng(5)
    D, C_, N = 14, 2, 8
    xyz = rng.uniform(-2, 2, (N, 3))
    G = rng.standard_normal((C_, D, D, D))
    w = rng.standard_normal((N, C_))
    M = np.linalg.qr(rng.standard_normal((3, 3)))[0]
    plain = gr.reference(xyz, G, 1.2, w=w, res=0.4, sigma=0.7)
    rot = gr.reference(xyz, G, 1.2, w=w, res=0.4, sigma=0.7, rot=M)
    assert np.allclose(rot["coords"][0], plain["coords"][0] @ M, rtol=0, atol=1e-14 * np.abs(plain["coords"][1]).max())
    assert np.all(rot["coords"][1] >= np.abs(rot["coords"][0]) * (1 - 1e-12))
    assert np.array_equal(rot["center"][0], -rot["coords"][0].sum(0))
    sub = gr.reference(xyz, G, 1.2, w=w, res=0.4, sigma=0.7, atoms=[5, 2])
    assert np.array_equal(sub["coords"][0], plain["coords"][0][[5, 2]])
    assert np.array_equal(sub["features"][0], plain["features"][0][[5, 2]])
