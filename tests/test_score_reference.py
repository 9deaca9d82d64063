"""CPU self-check of the score reference (tests/score_reference.py), before it judges mvx_score_batch: its molecule score is
sum(F * oracle_grid) in float64 on the full grid (c_oracle at precision 32, numpy_port at precision 64) under the project's
gradient rule with bound = sum over voxels of |F| * |grid terms|, and its per-atom parts are consistent."""
import numpy as np
import pytest

from tests import grad_reference as gr
from tests import score_reference as sr
from tests.tolerance import GRAD64_ABS, GRAD64_REL, GRAD_ABS, GRAD_REL

CASES = [  # res, sigma, blockdim, D
    (0.5, 0.5, None, 16), (0.3, 1.0, 5, 23), (1.0, 0.3, 7, 17), (0.5, 0.5, 9, 21)]


def _forward(xyz, chan, radii, radii_type, D, res, sigma, blockdim, density, precision, num_channels=None):
    from oracle import c_oracle, numpy_port

    kw = dict(radii_type=radii_type, density=density, sigma=sigma, num_channels=num_channels)
    if precision == 32:
        return c_oracle.voxelize(xyz, chan, radii, resolution=res, dimension=D, blockdim=blockdim, **kw).astype(np.float64)
    return numpy_port.voxelize(numpy_port.GridSpec(res, D, blockdim), xyz, chan, radii, precision=64, **kw)


@pytest.mark.parametrize("precision", [32, 64])
@pytest.mark.parametrize("density", ["gaussian", "binary"])
@pytest.mark.parametrize("res, sigma, blockdim, D", CASES)
def test_molecule_score_is_the_field_times_the_oracle_grid(res, sigma, blockdim, D, density, precision):
    C_, N = 3, 40
    rng = np.random.default_rng(int(res * 10 + sigma * 100 + D))
    fp = np.float32 if precision == 32 else np.float64
    W = res * (D - 1)
    xyz = rng.uniform(-W / 2 - 1.0, W / 2 + 1.0, (N, 3))
    xyz[0] = [W / 2 + 5.0, 0.0, 0.0]  # far outside the box
    feats = rng.standard_normal((N, C_)).astype(fp)
    types = rng.integers(0, C_, N)
    r_atom = (rng.uniform(0.7, 1.5, N) * res / 0.5).astype(fp)
    r_chan = (rng.uniform(0.7, 1.5, C_) * res / 0.5).astype(fp)
    F = rng.standard_normal((C_, D, D, D)).astype(fp).astype(np.float64)
    rel, abs_ = (GRAD_REL, GRAD_ABS) if precision == 32 else (GRAD64_REL, GRAD64_ABS)
    kw = dict(res=res, sigma=sigma, blockdim=blockdim, density=density, precision=precision)
    for mode, radii_type, radii in [("features", "scalar", 1.1 * res / 0.5), ("features", "atom-wise", r_atom),
                                    ("features", "channel-wise", r_chan), ("types", "atom-wise", r_atom),
                                    ("types", "channel-wise", r_chan), ("single", "scalar", 0.9 * res / 0.5)]:
        chan = {"features": feats, "types": types, "single": None}[mode]
        Cm = 1 if mode == "single" else C_
        Fm = F[:Cm]
        s, b, S, Sb = sr.score_reference(xyz, Fm, radii, radii_type, w=feats, mode=mode, types=types, **kw)
        grid = _forward(xyz, chan, radii, radii_type, D, res, sigma, blockdim, density, precision,
                        num_channels=None if mode != "types" else C_)
        want = float((Fm * grid).sum())
        # bound = sum over voxels of |F| * |grid terms|: the grid of |w| (one-hot weights are their own absolute values)
        gabs = grid if mode != "features" else _forward(xyz, np.abs(feats), radii, radii_type, D, res, sigma, blockdim, density,
                                                        precision)
        bound = float((np.abs(Fm) * gabs).sum())
        assert bound > 0 and abs(Sb - bound) <= 1e-4 * bound, (mode, radii_type, Sb, bound)
        assert abs(S - want) <= rel * bound + abs_, (mode, radii_type, S, want, bound)
        assert np.all(b >= np.abs(s) * (1 - 1e-12)) and s[0] == 0.0 and b[0] == 0.0
        assert S == float(s.sum()) and Sb == float(b.sum())
        if mode == "types":  # a type beyond the channels of the call scores nothing and changes nothing else
            beyond = np.where(np.arange(N) % 5 == 1, C_, types)
            s2, b2, _, _ = sr.score_reference(xyz, Fm, np.append(radii, fp(1.0)) if radii_type == "channel-wise" else radii,
                                              radii_type, mode=mode, types=beyond, **kw)
            assert np.all(s2[beyond >= C_] == 0.0) and np.all(b2[beyond >= C_] == 0.0)
            assert np.array_equal(s2[beyond < C_], s[beyond < C_])


def test_per_atom_score_is_the_field_times_the_atoms_own_grid():
    D, C_, N = 14, 4, 12
    rng = np.random.default_rng(7)
    xyz = rng.uniform(-3, 3, (N, 3))
    w = rng.standard_normal((N, C_))
    F = rng.standard_normal((C_, D, D, D))
    r_chan = rng.uniform(0.8, 1.4, C_).astype(np.float32)
    for radii_type, radii in (("scalar", 1.2), ("channel-wise", r_chan)):
        s, b, _, _ = sr.score_reference(xyz, F, radii, radii_type, w=w)
        for n in range(N):
            rho = gr.atom_grid(xyz, n, radii, radii_type, C_, D)
            t = F * rho * w[n][:, None, None, None]
            assert abs(s[n] - t.sum()) <= 1e-12 * max(1.0, b[n]) and abs(b[n] - np.abs(t).sum()) <= 1e-12 * max(1.0, b[n])


def test_batch_reference_cuts_molecules_and_fields():
    D, C_ = 12, 2
    rng = np.random.default_rng(3)
    off = np.array([0, 5, 5, 14])
    xyz = rng.uniform(-2, 2, (14, 3))
    w = rng.standard_normal((14, C_))
    r = rng.uniform(0.8, 1.3, 14).astype(np.float32)
    F = rng.standard_normal((3, C_, D, D, D))
    s, b, S, Sb = sr.batch_reference(xyz, off, F, r, "atom-wise", w=w)
    assert S[1] == 0.0 and Sb[1] == 0.0
    one = sr.score_reference(xyz[5:], F[2], r[5:], "atom-wise", w=w[5:])
    assert np.array_equal(s[5:], one[0]) and S[2] == one[2] and Sb[2] == one[3]
    shared = sr.batch_reference(xyz, off, F[0], r, "atom-wise", w=w)
    assert np.array_equal(shared[0][:5], s[:5]) and not np.array_equal(shared[0][5:], s[5:])
