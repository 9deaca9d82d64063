"""forward_sum / forward_posed_sum (mvx_forward_sum_batch) and the field gradients of the score calls on the GPU, over the rows of
tests/sum_rows.py: against the CPU oracle on the merged cloud, the bit identities of the contract, molecule
chunks and split calls, rotations and poses against the float64 sum of forward_batch's grids, and dL/dfield."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import sum_rows as R
from tests import hip_support as hip
from tests.abi import MVX_ERR_INVALID, last_error
from tests.tolerance import GRAD_ABS, GRAD_REL, assert_exact, assert_gaussian, gaussian_excess

pytestmark = pytest.mark.gpu

FEATURE_ROWS = [r.id for r in R.ROWS if r.mode == "features"]


@functools.lru_cache(maxsize=None)
def _vox(row_id, radii_type=None, **kw):
    import molvoxel_amd as mv

    row = R.BY_ID[row_id]
    return mv.create_voxelizer(0.5, row.D, radii_type or row.radii_type, row.density, library="hip", **dict(kw))


@functools.lru_cache(maxsize=None)
def _weights(row_id, kind):
    """Seeded weights of a row: "atom+" (sumN,) in [0.5, 1.5); "atom" (sumN,) and "mol" (B,) of mixed signs; float32."""
    d = R.make(row_id)
    rng = np.random.default_rng(d["row"].seed + 1000)
    if kind == "atom+":
        return rng.uniform(0.5, 1.5, d["N"]).astype(np.float32)
    return rng.standard_normal(d["N"] if kind == "atom" else d["B"]).astype(np.float32)


def _nc(d):
    return d["row"].C if d["row"].mode == "types" else None


def _sum(vox, d, weights=None, lo=0, hi=None, out_grid=None, accumulate=False, **kw):
    """forward_sum on the molecules [lo, hi) of a row's batch."""
    hi = d["B"] if hi is None else hi
    a0, a1 = int(d["off"][lo]), int(d["off"][hi])
    chan = None if d["chan"] is None else d["chan"][a0:a1]
    radii = d["radii"][a0:a1] if d["row"].radii_type == "atom-wise" else d["radii"]
    if weights is not None:
        weights = weights[a0:a1] if len(weights) == d["N"] else weights[lo:hi]
    return vox.forward_sum(hip.dev(d["xyz"][a0:a1]), d["off"][lo:hi + 1] - a0, hip.dev(d["cen"][lo:hi]), hip.dev(chan), hip.dev(radii),
                           weights=None if weights is None else hip.dev(weights), num_channels=_nc(d), out_grid=out_grid,
                           accumulate=accumulate, **kw)


@functools.lru_cache(maxsize=None)
def _uncut(row_id, wkind=None):
    """The one uncut call of a row (computed once, shared, never modified): the grid as a host array."""
    d = R.make(row_id)
    return _sum(_vox(row_id), d, None if wkind is None else _weights(row_id, wkind)).cpu().numpy()


# ---- 1. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", R.ROW_IDS)
def test_the_sum_is_the_oracles_grid_of_the_merged_cloud(row_id):
    """The reference is the CPU oracle on the merged cloud: positions coords_b - c_b in float64, every atom's own radius, the weights
    folded into float32 features. Membership identical; binary bit-identical; Gaussian by the project's one rule. The weighted
    leg uses positive weights, so that the rule's max(1, |ref|) is the magnitude of the sum's terms."""
    from oracle import c_oracle

    d = R.make(row_id)
    row = d["row"]
    feats = R.features_of(d)
    legs = [(None, feats)]
    if row.density == "gaussian":
        a = _weights(row_id, "atom+")
        legs.append(("atom+", (feats * a[:, None]).astype(np.float32)))
    for wkind, f in legs:
        ref = c_oracle.voxelize(R.merged(d), f, d["r_atom"].astype(np.float32), resolution=R.RES, dimension=row.D, density=row.density)
        got = _uncut(row_id, wkind)
        assert got.shape == (row.C, row.D, row.D, row.D) and got.dtype == np.float32
        if row.density == "binary":
            assert_exact(got, ref)
        else:
            print(f"{row_id} weights={wkind}: excess {gaussian_excess(got, ref):.3g} of the bar, largest sum {float(ref.max()):.4g}")
            assert_gaussian(got, ref)
        assert float(np.abs(ref).max()) > 0


# ---- 2. bit identities -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", R.ROW_IDS)
def test_unweighted_and_centred_only_is_the_forward_on_the_merged_molecule(row_id):
    import torch

    d = R.make(row_id)
    row = d["row"]
    got = _uncut(row_id)
    m = hip.dev(R.merged(d))
    vox = _vox(row_id)
    if row.mode == "features":
        ref = vox.forward_features(m, None, hip.dev(d["chan"]), hip.dev(d["radii"]))
    elif row.mode == "single":
        ref = vox.forward_single(m, None, d["radii"])
    else:
        # (forward_types refuses a negative type: the merged molecule without that atom - it reaches no voxel - and, with it, the
        # batched entry on the one merged molecule)
        keep = np.arange(d["N"]) != R.BAD_TYPE_ATOM
        ref = vox.forward_types(hip.dev(R.merged(d)[keep]), None, hip.dev(d["chan"][keep]), hip.dev(d["radii"]),
                                out_grid=torch.empty((row.C,) + (row.D,) * 3, device="cuda"))
        one = vox.forward_batch(m, np.array([0, d["N"]]), None, hip.dev(d["chan"]), hip.dev(d["radii"]), num_channels=row.C)[0]
        assert_exact(got, one.cpu().numpy())
    assert_exact(got, ref.cpu().numpy())


@pytest.mark.parametrize("row_id", FEATURE_ROWS)
def test_weighted_features_are_the_unweighted_call_on_scaled_features(row_id):
    d = R.make(row_id)
    a = _weights(row_id, "atom")
    scaled = dict(d, chan=(d["chan"] * a[:, None]).astype(np.float32))  # formed in float32
    assert_exact(_uncut(row_id, "atom"), _sum(_vox(row_id), scaled).cpu().numpy())


@pytest.mark.parametrize("row_id", ["light", "carry", "types", "single"])
def test_molecule_weights_are_their_expansion_per_atom(row_id):
    d = R.make(row_id)
    w = _weights(row_id, "mol")
    per_atom = np.repeat(w, np.diff(d["off"]))
    assert per_atom.shape == (d["N"],) and d["B"] != d["N"]
    assert_exact(_uncut(row_id, "mol"), _sum(_vox(row_id), d, per_atom).cpu().numpy())


@pytest.mark.parametrize("row_id", R.ROW_IDS)
def test_two_runs_give_the_same_bytes(row_id):
    d = R.make(row_id)
    wk = "atom" if d["row"].density == "gaussian" else None
    again = _sum(_vox(row_id), d, None if wk is None else _weights(row_id, wk)).cpu().numpy()
    assert again.tobytes() == _uncut(row_id, wk).tobytes()


# ---- 3. cuts -----------------------------------------------------------------------------------------------------------------
def _fresh(row_id):
    import molvoxel_amd as mv

    row = R.BY_ID[row_id]
    return mv.create_voxelizer(0.5, row.D, row.radii_type, row.density, library="hip")


@pytest.mark.parametrize("row_id, option, value, nchunk", [
    ("carry", "chunks", 2, 2), ("carry", "chunks", 3, 3), ("chunks", "chunks", 2, 2), ("wide", "mall_budget_kb", 1, 4),
    ("light", "mall_budget_kb", 1, 7), ("rounds", "mall_budget_kb", 1, 3), ("types", "mall_budget_kb", 1, 5),
    ("long", "mall_budget_kb", 1, 3), ("single", "mall_budget_kb", 1, 6),
    # (carry: 480 atoms x 200 B + 12 molecules x 32 slabs x 512 B = 292 608 B of pre-pass workspace)
    ("carry", "mall_budget_kb", 200, 2), ("carry", "mall_budget_kb", 120, 3),
])
def test_molecule_chunks_give_the_uncut_bits(row_id, option, value, nchunk):
    d = R.make(row_id)
    wk = "atom" if d["row"].density == "gaussian" else None
    vox = _fresh(row_id)  # (a voxelizer of its own: the option stays with the handle)
    vox.debug_option(option, value)
    got = _sum(vox, d, None if wk is None else _weights(row_id, wk)).cpu().numpy()
    plan = vox.last_plan()
    assert plan["nchunk"] == nchunk, plan  # the cut really happened
    assert plan["grouped"] == 0 and plan["ct"] == 32 and plan["ncc"] == -(-d["row"].C // 32) and plan["nw"] == R.nw_of(d["row"]) and plan["route"] == 0, plan
    assert_exact(got, _uncut(row_id, wk))


@pytest.mark.parametrize("row_id, cut", [("light", 5), ("light", 1), ("rounds", 1), ("rounds", 2), ("carry", 7), ("chunks", 4),
                                         ("wide", 3), ("types", 2), ("single", 3), ("long", 1)])
def test_a_call_split_in_two_with_accumulate_is_the_one_call(row_id, cut):
    import torch

    d = R.make(row_id)
    row = d["row"]
    wk = "atom" if row.density == "gaussian" else None
    w = None if wk is None else _weights(row_id, wk)
    vox = _vox(row_id)
    out = torch.full((row.C,) + (row.D,) * 3, float("nan"), device="cuda")  # (the first call overwrites every voxel)
    ret = _sum(vox, d, w, 0, cut, out_grid=out)
    assert ret is out
    _sum(vox, d, w, cut, d["B"], out_grid=out, accumulate=True)
    assert_exact(out.cpu().numpy(), _uncut(row_id, wk))


def test_accumulating_nothing_leaves_the_grid_untouched_and_summing_nothing_writes_zeros():
    import torch

    d = R.make("light")
    vox = _vox("light")
    rng = np.random.default_rng(1)
    start = rng.standard_normal((5, 16, 16, 16)).astype(np.float32)
    none = dict(coords=torch.empty((0, 3), dtype=torch.float64, device="cuda"), centers=None,
                channels=torch.empty((0, 5), device="cuda"), radii=1.0)
    for offsets in (np.array([0]), np.array([0, 0, 0])):  # B = 0; molecules without atoms
        out = torch.tensor(start, device="cuda")
        vox.forward_sum(offsets=offsets, out_grid=out, accumulate=True, **none)
        assert_exact(out.cpu().numpy(), start)
        vox.forward_sum(offsets=offsets, out_grid=out, **none)
        assert float(out.abs().max()) == 0.0
    # ... and a molecule that lies outside the box adds exact zeros
    o = R.OUTSIDE_MOLECULE
    out = torch.tensor(start, device="cuda")
    _sum(vox, d, None, o, o + 1, out_grid=out, accumulate=True)
    assert_exact(out.cpu().numpy(), start)
    assert float(_sum(vox, d, None, o, o + 1).abs().max()) == 0.0


def test_host_inputs_are_moved_to_the_device_and_a_foreign_grid_is_refused():
    import torch

    d = R.make("light")
    vox = _vox("light")
    got = vox.forward_sum(d["xyz"], d["off"], d["cen"], d["chan"], d["radii"], weights=_weights("light", "mol"))
    assert got.is_cuda and got.dtype == torch.float32
    assert_exact(got.cpu().numpy(), _uncut("light", "mol"))
    for bad in (torch.empty((5, 16, 16, 16)), torch.empty((5, 16, 16, 16), dtype=torch.bfloat16, device="cuda"),
                torch.empty((5, 16, 16, 32), device="cuda")[..., ::2]):
        with pytest.raises(ValueError, match="contiguous float32 tensor on this voxelizer's device"):
            vox.forward_sum(d["xyz"], d["off"], d["cen"], d["chan"], d["radii"], out_grid=bad)


def test_the_grid_is_float32_ncdhw_whatever_the_voxelizers_grid_type_and_layout():
    import torch

    d = R.make("chunks")
    vox = _vox("chunks", grid_dtype="bfloat16", grid_layout="channels_last")
    got = _sum(vox, d, _weights("chunks", "atom"))
    assert got.dtype == torch.float32 and got.is_contiguous()
    assert_exact(got.cpu().numpy(), _uncut("chunks", "atom"))


def test_the_library_names_what_it_does_not_serve():
    """The rules of mvx_forward_sum_batch that read the handle (tests/test_sum_rows_host.py has the others), through the C ABI."""
    import molvoxel_amd as mv
    import torch

    def call(vox, C_=4, rt=0, radii=None, out=None):
        xyz = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
        feat = torch.ones((3, C_), device="cuda")
        D = vox.dimension
        out = torch.empty((C_, D, D, D), device="cuda") if out is None else out
        off = np.array([0, 3], np.int64)
        rc = vox._lib.mvx_forward_sum_batch(vox._handle, 0, xyz.data_ptr(), feat.data_ptr(), None if radii is None else radii.data_ptr(),
                                            1.0, rt, off.ctypes.data, None, 1, C_, None, out.data_ptr(), 0, None)
        return rc, last_error()

    mk = lambda D, rt="scalar", **kw: mv.create_voxelizer(0.5, D, rt, "gaussian", library="hip", **kw)  # noqa: E731
    for vox, kw, words in [
        (mk(16, precision=64), {}, "precision 64"),
        (mk(16, "channel-wise"), dict(rt=2, radii=torch.ones(4, device="cuda")), "channel-wise radii with features"),
        (mk(18), {}, "no multiple of 4"),
        (mk(24, blockdim=12), {}, "per-lane ranges"),
        (mk(16), dict(out=torch.empty(4 * 16 ** 3 + 1, device="cuda")[1:]), "16-byte aligned"),
    ]:
        rc, msg = call(vox, **kw)
        assert rc == MVX_ERR_INVALID and msg.startswith("forward_sum:" if "aligned" not in words else "out") and words in msg, (rc, msg)
    rc, msg = call(mk(16))
    assert rc == 0, msg
    torch.cuda.synchronize()


# ---- 4. rotations and poses --------------------------------------------------------------------------------------------------
def _check_weighted_sum(got, grids, w, what):
    """|got - ref| <= GRAD_REL * bound + GRAD_ABS with ref = sum_b w[b] grid_b in float64 and bound = sum_b |w[b]| grid_b: the
    weights have mixed signs, so a relative bar on the result would reward cancellation."""
    g = grids.to("cpu", dtype=__import__("torch").float64).numpy()
    w = np.asarray(w, np.float64).reshape((-1,) + (1,) * (g.ndim - 1))
    ref, bound = (w * g).sum(0), (np.abs(w) * np.abs(g)).sum(0)
    err = np.abs(np.asarray(got, np.float64) - ref)
    worst = float((err / (GRAD_REL * bound + GRAD_ABS)).max())
    print(f"{what}: worst |got - ref| / (GRAD_REL * bound + GRAD_ABS) = {worst:.3g}, largest bound {float(bound.max()):.4g}")
    assert float(bound.max()) > 0 and worst <= 1.0, (what, worst)
    return ref, bound


@pytest.mark.parametrize("row_id", ["light", "carry", "types"])
def test_rotated_sums_are_the_weighted_sum_of_forward_batchs_grids(row_id):
    d = R.make(row_id)
    vox = _vox(row_id)
    w = _weights(row_id, "mol")
    a = dict(coords=hip.dev(d["xyz"]), offsets=d["off"], centers=hip.dev(d["cen"]), channels=hip.dev(d["chan"]), radii=hip.dev(d["radii"]),
             num_channels=_nc(d))
    np.random.seed(77)
    got = vox.forward_sum(weights=hip.dev(w), random_rotation=True, random_translation=0.3, **a)
    np.random.seed(77)
    grids = vox.forward_batch(random_rotation=True, random_translation=0.3, **a)
    _check_weighted_sum(got.cpu().numpy(), grids, w, f"{row_id} rotated")


@pytest.mark.parametrize("row_id", ["light", "carry", "types"])
def test_posed_sums_are_the_weighted_sum_of_forward_posed_batchs_grids(row_id):
    d = R.make(row_id)
    vox = _vox(row_id)
    w = _weights(row_id, "mol")
    a = dict(coords=hip.dev(d["xyz"]), offsets=d["off"], centers=hip.dev(d["cen"]), quaternions=hip.dev(d["q"]), translations=hip.dev(d["t"]),
             channels=hip.dev(d["chan"]), radii=hip.dev(d["radii"]), num_channels=_nc(d))
    got = vox.forward_posed_sum(weights=hip.dev(w), **a)
    grids = vox.forward_posed_batch(**a)
    _check_weighted_sum(got.cpu().numpy(), grids, w, f"{row_id} posed")
    # poses given on the host take the same route
    host = vox.forward_posed_sum(d["xyz"], d["off"], d["cen"], d["q"], d["t"], d["chan"], d["radii"], weights=w, num_channels=_nc(d))
    assert_exact(host.cpu().numpy(), got.cpu().numpy())


# ---- 5. field gradients ------------------------------------------------------------------------------------------------------
BF16_HALF_ULP = 2.0 ** -8  # rounding a value v to bfloat16 moves it by at most 2^-8 |v| <= 2^-8 bound: half of one bfloat16 ulp of bound


def _score_args(d, posed, grad=False):
    feat = d["row"].mode == "features"
    a = dict(coords=hip.dev(d["xyz"], grad), offsets=d["off"], centers=hip.dev(d["cen"], grad), channels=hip.dev(d["chan"], grad and feat),
             radii=hip.dev(d["radii"]), num_channels=_nc(d))
    if posed:
        a.update(quaternions=hip.dev(d["q"], grad), translations=hip.dev(d["t"], grad))
    return a


def _field(d, dtype, seed=5):
    import torch

    row = d["row"]
    F = np.random.default_rng(seed).standard_normal((row.C,) + (row.D,) * 3)
    return torch.tensor(F, device="cuda").to(dtype)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("posed", [False, True])
@pytest.mark.parametrize("row_id", ["light", "chunks", "types"])
def test_the_field_gradient_is_the_weighted_sum_of_the_grids(row_id, posed, dtype):
    """field.grad against the field gradient of (forward_batch(...) * field).sum(dim=(1, 2, 3, 4)) under the same upstream,
    evaluated in float64. A bfloat16 field's gradient is compared after its final rounding, with half a bfloat16 ulp of `bound`
    (2^-8 bound) added to the bar."""
    import torch

    d = R.make(row_id)
    tdt = getattr(torch, dtype)
    vox = _vox(row_id, differentiable=True, field_grad=True)
    field = _field(d, tdt).requires_grad_()
    g = torch.tensor(np.random.default_rng(8).standard_normal(d["B"]), device="cuda")
    a = _score_args(d, posed)
    np.random.seed(31)
    scores = vox.score_posed_batch(field=field, **a) if posed else vox.score_batch(field=field, random_rotation=True, **a)
    (scores * g).sum().backward()
    assert field.grad is not None and field.grad.dtype == tdt and field.grad.shape == field.shape
    np.random.seed(31)
    plain = _vox(row_id)
    grids = plain.forward_posed_batch(**a) if posed else plain.forward_batch(random_rotation=True, **a)
    f64 = field.detach().to(torch.float64).requires_grad_()
    ((grids.to(torch.float64) * f64).sum(dim=(1, 2, 3, 4)) * g).sum().backward()
    w = g.cpu().numpy()
    gd = grids.to("cpu", dtype=torch.float64).numpy()
    bound = (np.abs(w).reshape(-1, 1, 1, 1, 1) * gd).sum(0)
    err = np.abs(field.grad.to(torch.float64).cpu().numpy() - f64.grad.cpu().numpy())
    bar = GRAD_REL * bound + GRAD_ABS + (BF16_HALF_ULP * bound if dtype == "bfloat16" else 0.0)
    worst = float((err / bar).max())
    print(f"{row_id} posed={posed} {dtype}: worst |got - ref| / bar = {worst:.3g}, largest bound {float(bound.max()):.4g}")
    assert float(bound.max()) > 0 and worst <= 1.0, worst
    # the scores are those of a constant field
    np.random.seed(31)
    const = plain.score_posed_batch(field=field.detach(), **a) if posed else plain.score_batch(field=field.detach(), random_rotation=True, **a)
    assert torch.equal(const, scores.detach())


def test_a_per_atom_upstream_weights_every_atom_by_its_own_sum():
    """per_atom=True: atom n's weight is dL/dS of its molecule plus dL/ds_n. The reference takes every atom as a molecule of its own
    (the centre and pose of its molecule) through forward_posed_batch: dL/dfield = sum_n weight_n grid_n."""
    import torch

    d = R.make("light")
    vox = _vox("light", differentiable=True, field_grad=True)
    field = _field(d, torch.float32).requires_grad_()
    rng = np.random.default_rng(12)
    g, ga = torch.tensor(rng.standard_normal(d["B"]), device="cuda"), torch.tensor(rng.standard_normal(d["N"]), device="cuda")
    scores, atoms = vox.score_posed_batch(field=field, per_atom=True, **_score_args(d, True))
    ((scores * g).sum() + (atoms * ga).sum()).backward()
    lengths = np.diff(d["off"])
    rep = lambda x: np.repeat(x, lengths, axis=0)  # noqa: E731
    grids = _vox("light").forward_posed_batch(hip.dev(d["xyz"]), np.arange(d["N"] + 1), hip.dev(rep(d["cen"])), hip.dev(rep(d["q"])),
                                              hip.dev(rep(d["t"])), hip.dev(d["chan"]), d["radii"])
    w = (rep(g.cpu().numpy()) + ga.cpu().numpy()).astype(np.float32)  # (rounded to float32, as the call rounds it)
    _check_weighted_sum(field.grad.cpu().numpy(), grids, w, "light per-atom upstream")


@pytest.mark.parametrize("posed", [False, True])
@pytest.mark.parametrize("row_id", ["light", "chunks"])
def test_the_other_gradients_are_untouched_by_the_field_gradient(row_id, posed):
    import torch

    d = R.make(row_id)
    g = torch.tensor(np.random.default_rng(9).standard_normal(d["B"]), device="cuda")
    grads = []
    for fg in (False, True):
        vox = _vox(row_id, differentiable=True, field_grad=fg)
        a = _score_args(d, posed, grad=True)
        field = _field(d, torch.float32).requires_grad_(fg)
        np.random.seed(32)
        s = vox.score_posed_batch(field=field, **a) if posed else vox.score_batch(field=field, random_rotation=True, **a)
        (s * g).sum().backward()
        leaves = ["coords", "channels", "centers"] + (["quaternions", "translations"] if posed else [])
        grads.append({k: a[k].grad.clone() for k in leaves})
        assert (field.grad is not None) == fg
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k
        assert float(grads[0][k].abs().max()) > 0


def test_a_field_gradient_step_allocates_far_less_than_the_grids():
    """64 posed ligands at D = 24, C = 32: the grids would take 64 x 32 x 24^3 x 4 bytes = 113 MB; forward and backward with the
    field gradient allocate the scores, the gradient rows and ONE grid - a condition on what the call allocates."""
    import torch

    D, C_, B = 24, 32, 64
    rng = np.random.default_rng(5)
    sizes = rng.integers(20, 40, B)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(off[-1])
    cen = rng.uniform(-20, 20, (B, 3))
    xyz = np.repeat(cen, sizes, axis=0) + rng.uniform(-2.0, 2.0, (N, 3))
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    a = dict(coords=hip.dev(xyz, True), offsets=off, centers=hip.dev(cen), quaternions=hip.dev(q, True), translations=hip.dev(rng.uniform(-0.5, 0.5, (B, 3)), True),
             channels=hip.dev(rng.random((N, C_)).astype(np.float32)), radii=1.0)
    import molvoxel_amd as mv

    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip", differentiable=True, field_grad=True)
    field = torch.randn((C_, D, D, D), device="cuda", requires_grad=True)
    vox.score_posed_batch(field=field, **a).sum().backward()  # (warm: the library's workspace and torch's pools)
    field.grad = None
    for k in ("coords", "quaternions", "translations"):
        a[k].grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    scores = vox.score_posed_batch(field=field, **a)
    scores.sum().backward()
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - base
    grids = B * C_ * D ** 3 * 4
    assert float(field.grad.abs().sum()) > 0 and a["quaternions"].grad is not None
    assert used < grids, (used, grids)
