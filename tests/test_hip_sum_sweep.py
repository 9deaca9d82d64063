"""forward_sum, forward_views_sum and set_sum_parts on the GPU over the rows of tests/sum_sweep_rows.py - rows cut along z, half a
last z sub-tile (D % 8 == 4), the 1024-thread form past one round, blockdims 16 and one block - and over 48 seeded random draws.

The reference is the CPU oracle with the row's blockdim: on the merged cloud for unweighted and positively weighted calls (the
project's one Gaussian rule, binary bit for bit), and the float64 sum of one oracle grid per molecule for weights of mixed sign
(|got - ref| <= GRAD_REL * bound + GRAD_ABS, bound = sum_b |w_b| grid_b: tests/test_hip_sum.py's rule for weighted sums). The
read-in of the grid (accumulate=True, molecule chunks, parts) is held to the bits of the uncut call and to the float32 chain of
tests/test_hip_sum_parts.py. tests/test_sum_sweep_host.py shows without a GPU that every row reaches the branch it stands for."""
import functools

import numpy as np
import pytest

import tests.test_hip_sum as HS  # (_sum: forward_sum on the molecules [lo, hi) of a batch; _dev)
import tests.test_hip_sum_parts as PS  # (_ranges: the parts of the contract)
from tests import sum_sweep_rows as S
from tests import hip_support as hip
from tests.tolerance import GRAD_ABS, GRAD_REL, assert_exact, assert_gaussian, gaussian_excess

pytestmark = pytest.mark.gpu

DENSE = ["tall", "cut96", "cut132", "cut144"]  # rows whose middle molecule walks its x-list
CHUNK_ROWS = ["tall", "cut96", "cut132", "edge20", "bd16"]
PART_ROWS = ["tall", "cut96", "cut132", "cut144", "edge20", "edge12", "bd16u"]
CUTS = [(r.id, cut) for r in S.ROWS for cut in range(1, len(r.sizes))]  # every molecule boundary of every row


def _new_vox(row, blockdim="row", parts=1):
    import molvoxel_amd as mv

    bd = row.blockdim if blockdim == "row" else blockdim
    vox = mv.create_voxelizer(S.RES, row.D, row.radii_type, row.density, library="hip", blockdim=bd)
    if parts != 1:
        vox.set_sum_parts(parts)
        assert vox.sum_parts == parts
    return vox


@functools.lru_cache(maxsize=None)
def _vox(row_id, parts=1):
    """The voxelizer of a row, with the row's blockdim (one per (row, parts): the setting stays with the handle)."""
    return _new_vox(S.BY_ID[row_id], parts=parts)


@functools.lru_cache(maxsize=None)
def _weights(row_id, kind):
    """Seeded float32 weights of a row: "atom+" (sumN,) in [0.5, 1.5); "atom" (sumN,) of mixed signs; "mol" (B,) of alternating
    sign, magnitudes in [0.5, 1.5)."""
    d = S.make(row_id)
    rng = np.random.default_rng(d["row"].seed + 1000)
    if kind == "atom+":
        return rng.uniform(0.5, 1.5, d["N"]).astype(np.float32)
    if kind == "atom":
        return rng.standard_normal(d["N"]).astype(np.float32)
    return (rng.uniform(0.5, 1.5, d["B"]) * (-1.0) ** np.arange(d["B"])).astype(np.float32)


def _wk(row_id):
    """The weights of the bit-for-bit comparisons: per atom and of mixed signs where the density is Gaussian."""
    return _weights(row_id, "atom") if S.BY_ID[row_id].density == "gaussian" else None


@functools.lru_cache(maxsize=None)
def _uncut(row_id, wkind=None, lo=0, hi=None, parts=1):
    """One uncut call on the molecules [lo, hi) of a row (computed once, shared, never modified): the grid on the device."""
    return HS._sum(_vox(row_id, parts), S.make(row_id), None if wkind is None else _weights(row_id, wkind), lo, hi)


def _oracle(d, feats, lo=0, hi=None):
    """The CPU oracle's grid of the molecules [lo, hi) as ONE merged cloud, with the row's blockdim."""
    from oracle import c_oracle

    row = d["row"]
    a0, a1 = int(d["off"][lo]), int(d["off"][d["B"] if hi is None else hi])
    if a0 == a1:
        return np.zeros((row.C,) + (row.D,) * 3, np.float32)
    return c_oracle.voxelize(S.merged(d)[a0:a1], feats[a0:a1], d["r_atom"][a0:a1].astype(np.float32), resolution=S.RES, dimension=row.D,
                             density=row.density, blockdim=row.blockdim)


def _weighted_reference(d, feats, w):
    """ref = sum_b w[b] grid_b and bound = sum_b |w[b]| |grid_b| in float64, one oracle grid per molecule."""
    row = d["row"]
    ref = np.zeros((row.C,) + (row.D,) * 3, np.float64)
    bound = np.zeros_like(ref)
    for b in range(d["B"]):
        if d["off"][b + 1] > d["off"][b]:
            g = _oracle(d, feats, b, b + 1).astype(np.float64)
            ref += float(w[b]) * g
            bound += abs(float(w[b])) * np.abs(g)
    return ref, bound


def _check_bound(got, ref, bound, what):
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / (GRAD_REL * bound + GRAD_ABS)).max())
    print(f"{what}: worst |got - ref| / (GRAD_REL * bound + GRAD_ABS) = {worst:.3g}, largest bound {float(bound.max()):.4g}")
    assert float(bound.max()) > 0 and worst <= 1.0, (what, worst)


def _check_merged(got, ref, density, what):
    """Membership identical; binary bit for bit (sums of float32 terms 1 * u in atom order, as the oracle adds them); Gaussian by
    the project's one rule."""
    if density == "binary":
        assert_exact(got, ref)
        print(f"{what}: binary, bit for bit, largest sum {float(ref.max()):.4g}")
    else:
        print(f"{what}: excess {gaussian_excess(got, ref):.3g} of the bar, largest sum {float(ref.max()):.4g}")
        assert_gaussian(got, ref)
    assert float(np.abs(ref).max()) > 0


def _equal(a, b):
    import torch

    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    assert torch.equal(a, b), f"{int((a != b).sum())} voxels differ"


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", S.ROW_IDS)
def test_the_sum_is_the_oracles_grid_of_the_merged_cloud(row_id):
    d = S.make(row_id)
    row = d["row"]
    feats = S.features_of(d)
    a = _weights(row_id, "atom+")
    for wkind, f in ((None, feats), ("atom+", (feats * a[:, None]).astype(np.float32))):
        got = _uncut(row_id, wkind).cpu().numpy()
        assert got.shape == (row.C,) + (row.D,) * 3 and got.dtype == np.float32
        _check_merged(got, _oracle(d, f), row.density, f"{row_id} weights={wkind}")


@pytest.mark.parametrize("row_id", S.ROW_IDS)
def test_molecule_weights_of_mixed_sign_are_the_weighted_sum_of_the_oracles_grids(row_id):
    d = S.make(row_id)
    w = _weights(row_id, "mol")
    sizes = np.diff(d["off"])
    assert (w[sizes > 0] > 0).any() and (w[sizes > 0] < 0).any()
    ref, bound = _weighted_reference(d, S.features_of(d), w)
    _check_bound(_uncut(row_id, "mol").cpu().numpy(), ref, bound, f"{row_id} molecule weights")


# ---- 2. bit identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", S.ROW_IDS)
def test_unweighted_is_the_forward_on_the_merged_molecule_with_the_same_blockdim(row_id):
    import torch

    d = S.make(row_id)
    row = d["row"]
    vox = _vox(row_id)
    assert vox.blockdim == (row.blockdim or 8)
    m = S.merged(d)
    if row.mode == "features":
        ref = vox.forward_features(hip.dev(m), None, hip.dev(d["chan"]), hip.dev(d["radii"]))
    elif row.mode == "single":
        ref = vox.forward_single(hip.dev(m), None, hip.dev(d["radii"]))
    else:  # (forward_types refuses the one type outside [0, C): the merged molecule without that atom, which reaches no voxel)
        keep = np.arange(d["N"]) != S.R.BAD_TYPE_ATOM
        ref = vox.forward_types(hip.dev(m[keep]), None, hip.dev(d["chan"][keep]), hip.dev(d["radii"]),
                                out_grid=torch.empty((row.C,) + (row.D,) * 3, device="cuda"))
    assert float(ref.abs().max()) > 0
    _equal(_uncut(row_id), ref)


@pytest.mark.parametrize("row_id", S.ROW_IDS)
def test_two_runs_give_the_same_bytes(row_id):
    d = S.make(row_id)
    again = HS._sum(_vox(row_id), d, _wk(row_id))
    assert again.cpu().numpy().tobytes() == _uncut(row_id, "atom" if _wk(row_id) is not None else None).cpu().numpy().tobytes()


def test_one_block_is_the_blockdim_5000_grid():
    d = S.make("bd24")
    for wkind in (None, "atom+"):
        w = None if wkind is None else _weights("bd24", wkind)
        _equal(_uncut("bd24", wkind), HS._sum(_new_vox(d["row"], blockdim=5000), d, w))
    # ... and blocks of 8 cull what one block keeps: the blockdim reaches the summed call
    assert not np.array_equal(HS._sum(_new_vox(d["row"], blockdim=None), d).cpu().numpy(), _uncut("bd24").cpu().numpy())


# ---- 3. the read-in: split calls, molecule chunks ----------------------------------------------------------------------------
def test_the_cuts_pass_directly_before_and_after_every_dense_molecule():
    for row_id in DENSE:
        assert (row_id, 1) in CUTS and (row_id, 2) in CUTS and len(S.BY_ID[row_id].sizes) == 3
    assert len(CUTS) == sum(len(r.sizes) - 1 for r in S.ROWS) and {c[0] for c in CUTS} == set(S.ROW_IDS)


@pytest.mark.parametrize("row_id, cut", CUTS)
def test_a_call_split_in_two_with_accumulate_is_the_one_call(row_id, cut):
    import torch

    d = S.make(row_id)
    row = d["row"]
    w = _wk(row_id)
    vox = _vox(row_id)
    out = torch.full((row.C,) + (row.D,) * 3, float("nan"), device="cuda")  # (the first call overwrites every voxel)
    assert HS._sum(vox, d, w, 0, cut, out_grid=out) is out
    assert not bool(torch.isnan(out).any())
    HS._sum(vox, d, w, cut, d["B"], out_grid=out, accumulate=True)
    _equal(out, _uncut(row_id, None if w is None else "atom"))


@pytest.mark.parametrize("row_id", CHUNK_ROWS)
def test_one_molecule_per_chunk_gives_the_uncut_bits(row_id):
    d = S.make(row_id)
    row = d["row"]
    vox = _new_vox(row)  # (a voxelizer of its own: the option stays with the handle)
    vox.debug_option("mall_budget_kb", 1)
    got = HS._sum(vox, d, _wk(row_id))
    plan = vox.last_plan()
    assert plan["nchunk"] == d["B"], plan  # the cut really happened
    assert (plan["nw"], plan["nzc"]) == S.nw_nzc(row.D) and plan["ct"] == 32 and plan["ncc"] == -(-row.C // 32) and plan["route"] == 0, plan
    _equal(got, _uncut(row_id, None if _wk(row_id) is None else "atom"))


# ---- 4. parts ----------------------------------------------------------------------------------------------------------------
def _wkind(row_id, weighted):
    return "atom" if weighted and S.BY_ID[row_id].density == "gaussian" else ("atom+" if weighted else None)


def _chain(row_id, K, wkind, start=None):
    """The contract of set_sum_parts: r = (start | +0); r = r + S_g for every part in order, S_g the parts = 1 sum of part g."""
    import torch

    B = len(S.BY_ID[row_id].sizes)
    r = None if start is None else start.clone()
    for lo, hi in PS._ranges(B, K):
        s = _uncut(row_id, wkind, lo, hi)
        r = torch.zeros_like(s) + s if r is None else r + s
    return r


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "atom-weights"])
@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("row_id", PART_ROWS)
def test_k_parts_are_the_float32_chain_of_the_parts_own_sums(row_id, K, weighted):
    wkind = _wkind(row_id, weighted)
    got = _uncut(row_id, wkind, parts=K)
    assert float(got.abs().max()) > 0
    _equal(got, _chain(row_id, K, wkind))


@pytest.mark.parametrize("row_id", ["cut132", "edge20"])
def test_parts_with_accumulate_start_the_chain_from_the_grid(row_id):
    import torch

    d = S.make(row_id)
    row = d["row"]
    wkind = _wkind(row_id, True)
    start = torch.tensor(np.random.default_rng(6).standard_normal((row.C,) + (row.D,) * 3).astype(np.float32), device="cuda")
    out = start.clone()
    assert HS._sum(_vox(row_id, 3), d, _weights(row_id, wkind), out_grid=out, accumulate=True) is out
    _equal(out, _chain(row_id, 3, wkind, start))
    assert not torch.equal(out, start)


def test_three_parts_with_one_molecule_per_chunk_give_the_bits_of_the_uncut_three_part_call():
    d = S.make("cut96")
    vox = _new_vox(d["row"], parts=3)
    vox.debug_option("mall_budget_kb", 1)
    got = HS._sum(vox, d, _weights("cut96", "atom"))
    plan = vox.last_plan()
    assert plan["nchunk"] == 3 and (plan["nw"], plan["nzc"]) == (8, 2), plan
    _equal(got, _uncut("cut96", "atom", parts=3))


# ---- 5. views ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _views(row_id, nviews):
    """The largest molecule of a row as the shared cloud. Views: the row's own centres (they lie tens of A apart: all but the
    cloud's own select nothing), then the cloud's centre moved by seeded offsets of up to 1.5 A per axis, `nviews` in all."""
    d = S.make(row_id)
    b = int(np.argmax(np.diff(d["off"])))
    a0, a1 = int(d["off"][b]), int(d["off"][b + 1])
    rng = np.random.default_rng(d["row"].seed + 2000)
    cen = np.concatenate([d["cen"], d["cen"][b] + rng.uniform(-1.5, 1.5, (nviews - d["B"], 3))])
    xyz, chan, n = d["xyz"][a0:a1], d["chan"][a0:a1], a1 - a0
    w = (rng.uniform(0.5, 1.5, nviews) * (-1.0) ** np.arange(nviews)).astype(np.float32)
    rep = dict(coords=np.tile(xyz, (nviews, 1)), offsets=np.arange(nviews + 1, dtype=np.int64) * n, channels=np.concatenate([chan] * nviews))
    return dict(xyz=xyz, chan=chan, radii=d["radii"], cen=cen, w=w, rep=rep)


def _views_sum(vox, c, weights=None):
    return vox.forward_views_sum(hip.dev(c["xyz"]), hip.dev(c["cen"]), hip.dev(c["chan"]), c["radii"], weights=hip.dev(weights))


def _repeated_sum(vox, c, weights=None):
    r = c["rep"]
    return vox.forward_sum(hip.dev(r["coords"]), r["offsets"], hip.dev(c["cen"]), hip.dev(r["channels"]), c["radii"], weights=hip.dev(weights))


@pytest.mark.parametrize("row_id, nviews", [("edge20", 12), ("cut96", 6)])
def test_views_sum_is_forward_sum_on_the_repeated_cloud(row_id, nviews):
    row = S.BY_ID[row_id]
    assert row.mode == "features" and row.radii_type == "scalar" and max(row.sizes) == {"edge20": 60, "cut96": 1200}[row_id]
    c = _views(row_id, nviews)
    vox = _vox(row_id)
    plain = _views_sum(vox, c)
    _equal(plain, _repeated_sum(vox, c))
    weighted = _views_sum(vox, c, c["w"])
    _equal(weighted, _repeated_sum(vox, c, c["w"]))
    assert float(plain.abs().max()) > 0 and not bool((weighted == plain).all())


def test_twelve_views_in_three_molecule_chunks_give_the_uncut_bits():
    c = _views("edge20", 12)
    vox = _new_vox(S.BY_ID["edge20"])
    vox.debug_option("chunks", 3)
    got = _views_sum(vox, c, c["w"])
    plan = vox.last_plan()
    assert plan["nchunk"] == 3 and plan["ncc"] == 2 and (plan["nw"], plan["nzc"]) == (3, 1), plan
    _equal(got, _views_sum(_vox("edge20"), c, c["w"]))


# ---- 6. the random draws -----------------------------------------------------------------------------------------------------
def test_the_draws_jointly_reach_every_dimension_channel_count_and_weight_kind():
    cov = S.sweep_coverage()
    assert len(S.SWEEP_SEEDS) == 48
    assert cov["D"] == set(S.SWEEP_D) and cov["C"] == set(S.SWEEP_C) and cov["weights"] == {None, "mol", "atom+"}, cov
    assert cov["over_one_round"], cov  # a draw with a slab over 63 candidates, by slab_counts' lower bound


@pytest.mark.parametrize("seed", S.SWEEP_SEEDS)
def test_a_random_draw_is_the_oracles_sum(seed):
    import torch

    x = S.draw(seed)
    row_id = f"draw{seed}"
    d = S.make(row_id)
    row = x.row
    rng = np.random.default_rng(seed + 1)
    shape = (row.C,) + (row.D,) * 3
    feats = S.features_of(d)
    w, w_mol = None, np.ones(d["B"])
    if x.weights == "mol":
        w = rng.standard_normal(d["B"]).astype(np.float32)
        w_mol = w
    elif x.weights == "atom+":
        w = rng.uniform(0.5, 1.5, d["N"]).astype(np.float32)
        feats = (feats * w[:, None]).astype(np.float32)
    assert d["N"] != d["B"]  # (the two readings of the weights cannot be confused)
    start = rng.standard_normal(shape).astype(np.float32) if x.accumulate else None

    def call(vox, lo=0, hi=None, onto=None):
        out = None if onto is None else torch.tensor(onto, device="cuda")
        return HS._sum(vox, d, w, lo, hi, out_grid=out, accumulate=onto is not None)

    one = _new_vox(row)
    what = (f"draw {seed}: D {row.D} C {row.C} {row.mode} {row.radii_type} {row.density} blockdim {row.blockdim} sizes {list(row.sizes)} "
            f"{row.spread} weights {x.weights} K {x.K} accumulate {x.accumulate}")
    if x.K == 1:
        got = call(one, onto=start)
    else:  # the chain's own reference: the parts = 1 sums of the parts, added in float32 in part order
        got = call(_new_vox(row, parts=x.K), onto=start)
        r = torch.zeros(shape, device="cuda") if start is None else torch.tensor(start, device="cuda")
        for lo, hi in PS._ranges(d["B"], x.K):
            r = r + call(one, lo, hi)
        _equal(got, r)
    got = got.cpu().numpy()
    assert got.shape == shape
    # the oracle: one grid per molecule, summed in float64
    ref, bound = _weighted_reference(d, feats, w_mol)
    if start is not None:
        ref, bound = ref + start.astype(np.float64), bound + np.abs(start).astype(np.float64)
    if float(bound.max()) > 0:
        _check_bound(got, ref, bound, what)
    else:  # every atom outside the box or of no channel: exact zeros
        assert not got.any()
    if x.K == 1 and start is None and x.weights != "mol" and float(bound.max()) > 0:  # ... and the merged cloud itself
        _check_merged(got, _oracle(d, feats), row.density, what)
