"""Summed grids in parts (set_sum_parts / mvx_set_sum_parts) on the GPU, over rows of tests/sum_rows.py.

The contract for K > 1 parts of a call of B molecules: q = ceil(B / K), part g = molecules [g q, min(B, (g + 1) q)),
G = ceil(B / q) parts, S_g the grid forward_sum (parts = 1, from zero) gives for the molecules of part g alone, and the result the
float32 chain r = (accumulate ? out : +0); r = r + S_0; ...; r = r + S_{G-1}. The expected grids below are that chain in torch,
every S_g from a parts = 1 voxelizer; the comparisons are bit for bit."""
import functools

import numpy as np
import pytest

import tests.test_hip_sum as HS  # (_sum, _weights, _vox, _fresh, _dev: forward_sum on the molecules [lo, hi) of a row)
import tests.test_hip_views_sum as VS  # (the views cases)
from tests import sum_rows as R
from tests import hip_support as hip
from tests.tolerance import GRAD_ABS, GRAD_REL, assert_exact, assert_gaussian, gaussian_excess

pytestmark = pytest.mark.gpu

ROWS = ["light", "carry", "rounds", "chunks", "single", "long"]
KS = [2, 3, 5, 64]


def _ranges(B, K):
    q = -(-B // K)
    return [(g * q, min(B, (g + 1) * q)) for g in range(-(-B // q))]


@functools.lru_cache(maxsize=None)
def _parts_vox(row_id, K, **kw):
    """A voxelizer of its own per (row, K): the setting stays with the handle."""
    import molvoxel_amd as mv

    row = R.BY_ID[row_id]
    vox = mv.create_voxelizer(0.5, row.D, row.radii_type, row.density, library="hip", **dict(kw))
    vox.set_sum_parts(K)
    assert vox.sum_parts == K
    return vox


def _wk(row_id, weighted):
    return HS._weights(row_id, "atom") if weighted else None


@functools.lru_cache(maxsize=None)
def _partials(row_id, K, weighted):
    """S_g of every part (device tensors, computed once, shared, never modified): one parts = 1 forward_sum call per part."""
    d = R.make(row_id)
    return [HS._sum(HS._vox(row_id), d, _wk(row_id, weighted), lo, hi) for lo, hi in _ranges(d["B"], K)]


def _chain(row_id, K, weighted, start=None):
    import torch

    r = torch.zeros_like(_partials(row_id, K, weighted)[0]) if start is None else start.clone()
    for s in _partials(row_id, K, weighted):
        r = r + s
    return r.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _got(row_id, K, weighted):
    """The one uncut K-part call of a row as a host array (computed once, shared, never modified)."""
    return HS._sum(_parts_vox(row_id, K), R.make(row_id), _wk(row_id, weighted)).cpu().numpy()


def test_the_parts_are_the_ones_the_contract_names():
    assert _ranges(7, 3) == [(0, 3), (3, 6), (6, 7)] and _ranges(12, 5) == [(0, 3), (3, 6), (6, 9), (9, 12)]  # (G = 4 < K = 5)
    assert _ranges(7, 64) == [(b, b + 1) for b in range(7)] and _ranges(3, 2) == [(0, 2), (2, 3)]
    d = R.make("light")
    sizes = np.diff(d["off"])
    assert sizes[0] == 0 and sizes[4] == 0  # K = 64 on `light`: parts without atoms


# ---- 1. back to one part -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", ["carry", "chunks"])
def test_one_part_after_three_gives_todays_bits(row_id):
    import molvoxel_amd as mv

    d = R.make(row_id)
    row = d["row"]
    vox = mv.create_voxelizer(0.5, row.D, row.radii_type, row.density, library="hip")
    assert vox.sum_parts == 1
    vox.set_sum_parts(3)
    three = HS._sum(vox, d, _wk(row_id, True)).cpu().numpy()
    vox.set_sum_parts(1)
    assert vox.sum_parts == 1
    one = HS._sum(vox, d, _wk(row_id, True)).cpu().numpy()
    assert_exact(one, HS._sum(HS._fresh(row_id), d, _wk(row_id, True)).cpu().numpy())
    assert_exact(three, _got(row_id, 3, True))
    with pytest.raises(RuntimeError, match="sum parts must be 1 ... 64"):
        vox.set_sum_parts(65)
    assert vox.sum_parts == 1


# ---- 2. the contract ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "atom-weights"])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("row_id", ROWS)
def test_k_parts_are_the_float32_chain_of_the_parts_own_sums(row_id, K, weighted):
    d = R.make(row_id)
    if weighted and d["row"].density == "gaussian":
        w = _wk(row_id, True)
        assert (w > 0).any() and (w < 0).any()
    got = _got(row_id, K, weighted)
    assert got.shape == (d["row"].C,) + (d["row"].D,) * 3 and float(np.abs(got).max()) > 0
    assert_exact(got, _chain(row_id, K, weighted))


def test_the_bits_of_several_parts_are_not_those_of_one():
    """What the docstring and DESIGN.md say: other partial sums are rounded. (`carry`: every voxel of the box sums many atoms.)"""
    assert not np.array_equal(_got("carry", 3, True), HS._uncut("carry", "atom"))
    np.testing.assert_allclose(_got("carry", 3, False), HS._uncut("carry"), rtol=1e-5, atol=1e-6)


# ---- 3. accumulate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id, K", [("light", 3), ("chunks", 2), ("single", 5)])
def test_accumulate_starts_the_chain_from_the_grid(row_id, K):
    import torch

    d = R.make(row_id)
    row = d["row"]
    start = torch.tensor(np.random.default_rng(6).standard_normal((row.C,) + (row.D,) * 3).astype(np.float32), device="cuda")
    out = start.clone()
    ret = HS._sum(_parts_vox(row_id, K), d, _wk(row_id, True), out_grid=out, accumulate=True)
    assert ret is out
    assert_exact(out.cpu().numpy(), _chain(row_id, K, True, start))
    fresh = torch.full_like(start, float("nan"))  # (without accumulate the grid is overwritten, whatever it held)
    HS._sum(_parts_vox(row_id, K), d, _wk(row_id, True), out_grid=fresh)
    assert_exact(fresh.cpu().numpy(), _got(row_id, K, True))


# ---- 4. cuts that do not fall on part boundaries -----------------------------------------------------------------------------
@pytest.mark.parametrize("row_id, K, option, value, nchunk", [
    ("carry", 5, "chunks", 3, 3),  # parts of 3 molecules, chunks of 4
    ("light", 3, "mall_budget_kb", 1, 7),  # parts of 3 molecules, one molecule per chunk
])
def test_molecule_chunks_give_the_bits_of_the_uncut_k_part_call(row_id, K, option, value, nchunk):
    import molvoxel_amd as mv

    d = R.make(row_id)
    row = d["row"]
    vox = mv.create_voxelizer(0.5, row.D, row.radii_type, row.density, library="hip")
    vox.set_sum_parts(K)
    vox.debug_option(option, value)
    got = HS._sum(vox, d, _wk(row_id, True)).cpu().numpy()
    plan = vox.last_plan()
    assert plan["nchunk"] == nchunk, plan  # the cut really happened
    bounds = {int(d["B"] * k // nchunk) for k in range(1, nchunk)}
    assert bounds - {lo for lo, _ in _ranges(d["B"], K)}  # ... and not only on part boundaries
    assert_exact(got, _got(row_id, K, True))


# ---- 5. determinism ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", ROWS)
def test_two_runs_give_the_same_bytes(row_id):
    again = HS._sum(_parts_vox(row_id, 3), R.make(row_id), _wk(row_id, True)).cpu().numpy()
    assert again.tobytes() == _got(row_id, 3, True).tobytes()


# ---- 6. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", R.ROW_IDS)
def test_three_parts_are_the_oracles_grid_of_the_merged_cloud(row_id):
    """As tests/test_hip_sum.py compares the one-pass sum: the CPU oracle on the merged cloud, membership identical, Gaussian by
    the project's one rule, binary bit-identical (sums of small integers are exact in any order)."""
    from oracle import c_oracle

    d = R.make(row_id)
    row = d["row"]
    ref = c_oracle.voxelize(R.merged(d), R.features_of(d), d["r_atom"].astype(np.float32), resolution=R.RES, dimension=row.D, density=row.density)
    got = _got(row_id, 3, False)
    if row.density == "binary":
        assert_exact(got, ref)
    else:
        print(f"{row_id} K=3: excess {gaussian_excess(got, ref):.3g} of the bar, largest sum {float(ref.max()):.4g}")
        assert_gaussian(got, ref)
    assert float(np.abs(ref).max()) > 0


# ---- 7. views ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["features-C33-atom", "types-C8-by-type"])
def test_views_sum_in_three_parts_is_the_chain_of_the_parts_views(case_id):
    import molvoxel_amd as mv
    import torch

    c = VS._case(case_id)
    w = c["w"]
    vox3 = mv.create_voxelizer(1.0, VS.D, c["rt"], c["density"], library="hip")
    vox3.set_sum_parts(3)
    got = VS._views_sum(c, vox=vox3, weights=hip.dev(w))
    r = torch.zeros_like(got)
    for lo, hi in _ranges(VS.B, 3):
        r = r + c["vox"].forward_views_sum(hip.dev(c["xyz"]), hip.dev(c["cen"][lo:hi]), hip.dev(c["chan"]), hip.dev(c["radii"]),
                                           weights=hip.dev(w[lo:hi]), num_channels=c["nc"])
    assert float(r.abs().max()) > 0
    assert_exact(got.cpu().numpy(), r.cpu().numpy())


# ---- 8. the field gradient ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", ["light", "chunks"])
def test_the_field_gradient_in_three_parts_is_the_weighted_sum_of_the_grids(row_id):
    """field.grad of score_batch on a field_grad voxelizer with K = 3 against the float64 field gradient through forward_batch's
    grids under the same upstream: the bar of tests/test_hip_sum.py, GRAD_REL * bound + GRAD_ABS with bound = sum_b |g_b| grid_b."""
    import torch

    d = R.make(row_id)
    vox = _parts_vox(row_id, 3, differentiable=True, field_grad=True)
    field = HS._field(d, torch.float32).requires_grad_()
    g = torch.tensor(np.random.default_rng(8).standard_normal(d["B"]), device="cuda")
    a = HS._score_args(d, False)
    np.random.seed(31)
    scores = vox.score_batch(field=field, random_rotation=True, **a)
    (scores * g).sum().backward()
    np.random.seed(31)
    grids = HS._vox(row_id).forward_batch(random_rotation=True, **a)
    gd = grids.to("cpu", dtype=torch.float64).numpy()
    w = g.cpu().numpy().reshape(-1, 1, 1, 1, 1)
    ref, bound = (w * gd).sum(0), (np.abs(w) * gd).sum(0)
    err = np.abs(field.grad.to(torch.float64).cpu().numpy() - ref)
    worst = float((err / (GRAD_REL * bound + GRAD_ABS)).max())
    print(f"{row_id} K=3 field gradient: worst |got - ref| / bar = {worst:.3g}, largest bound {float(bound.max()):.4g}")
    assert float(bound.max()) > 0 and worst <= 1.0, worst
    # ... and it is not the one-pass gradient's bits: the setting really reached the backward's summed call
    one = HS._vox(row_id, differentiable=True, field_grad=True)
    f1 = field.detach().clone().requires_grad_()
    np.random.seed(31)
    (one.score_batch(field=f1, random_rotation=True, **a) * g).sum().backward()
    assert not torch.equal(f1.grad, field.grad)
