"""Gradients through moments_batch / moments_posed_batch (mvx_moments_backward_batch, moments_grad=True) on the GPU, over six rows
of tests/sum_rows.py: light (D = 16, C = 5, empty molecules), carry (C = 32, atom-wise radii), chunks (C = 33: coefficients past
the first channel chunk), wide (C = 65), types (one type outside [0, C)) and single (binary).

* Bit identities through the C entry: dL/dm = (0, 0, 1) is mvx_score_batch over the target, (0, 0.5, 0) is mvx_backward_batch with
  the grids themselves as upstream, (1, 0) without a target is mvx_backward_batch with an upstream of ones.
* General coefficients against tests/grad_reference.reference with G = a0 + a1 g + a2 t in float64 (tests/moments_grad_reference.py)
  under the project's bar |got - ref| <= GRAD_REL * bound + GRAD_ABS, bound = the reference with |a0| + |a1| |g| + |a2| |t| for G.
* Batch and chunk identities to the bit; bfloat16 and channels-last voxelizers give the float32 bits.
* Autograd end to end with the loss -NCC against the same loss built from the grids of a differentiable voxelizer.

Measured (run with -s for the figures): worst |got - ref| / (GRAD_REL * bound + GRAD_ABS) 0.0147 over all rows and legs (wide,
posed); autograd against the grid path 0.0028 (features of `light`), poses 7.5e-5.
"""
import functools

import numpy as np
import pytest

from tests import grad_reference as GR
from tests import moments_grad_reference as MG
from tests import pose_reference as PR
from tests import sum_rows as R
from tests import sum_sweep_rows as S
from tests import hip_support as hip
from tests.abi import MVX_ERR_INVALID, last_error
from tests.tolerance import GRAD_ABS, GRAD_REL

pytestmark = pytest.mark.gpu

ROW_IDS = ["light", "carry", "chunks", "wide", "types", "single"]
LEGS = ["centred", "posed", "rotated"]
SEED = 77      # the rotated leg seeds numpy's global generator, as tests/test_hip_moments.py does
SAMPLE = 96    # atoms per case that go through the float64 reference


def _make(row_id):
    """A row of tests/sum_rows.py or of tests/sum_sweep_rows.py (these carry a blockdim and a z shift of their own)."""
    return S.make(row_id) if row_id in S.BY_ID else R.make(row_id)


@functools.lru_cache(maxsize=None)
def _vox(row_id, **kw):
    return _new_vox(row_id, **kw)


def _new_vox(row_id, **kw):
    import molvoxel_amd as mv

    row = _make(row_id)["row"]
    return mv.create_voxelizer(0.5, row.D, row.radii_type, row.density, library="hip", blockdim=getattr(row, "blockdim", None), **kw)


def _args(d, lo=0, hi=None):
    """forward_batch's arguments for the molecules [lo, hi) of a row's batch."""
    row = d["row"]
    hi = d["B"] if hi is None else hi
    a0, a1 = int(d["off"][lo]), int(d["off"][hi])
    chan = None if d["chan"] is None else d["chan"][a0:a1]
    radii = d["radii"][a0:a1] if row.radii_type == "atom-wise" else d["radii"]
    return dict(coords=hip.dev(d["xyz"][a0:a1]), offsets=d["off"][lo:hi + 1] - a0, centers=hip.dev(d["cen"][lo:hi]), channels=hip.dev(chan),
                radii=hip.dev(radii), num_channels=row.C if row.mode == "types" else None)


@functools.lru_cache(maxsize=None)
def _target(row_id):
    """A seeded float32 target of mixed signs, (C, D, D, D) (never modified)."""
    row = _make(row_id)["row"]
    t = np.random.default_rng(row.seed + 5000).standard_normal((row.C,) + (row.D,) * 3).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def _dm(row_id, K):
    """Seeded dL/dm of mixed signs, different for every molecule and channel: (B, C, K) float64 (never modified)."""
    d = _make(row_id)
    g = np.random.default_rng(d["row"].seed + 9000 + K).standard_normal((d["B"], d["row"].C, K))
    g.setflags(write=False)
    return g


def _forward(vox, d, leg, lo=0, hi=None):
    """The grids of a leg: forward_batch / forward_posed_batch of the molecules [lo, hi)."""
    a = _args(d, lo, hi)
    if leg == "posed":
        return vox.forward_posed_batch(quaternions=hip.dev(d["q"][lo:hi]), translations=hip.dev(d["t"][lo:hi]), **a)
    if leg == "rotated":
        np.random.seed(SEED)
        return vox.forward_batch(random_rotation=True, random_translation=0.5, **a)
    return vox.forward_batch(**a)


def _spec(vox, d, leg, lo=0, hi=None):
    """The call record of a leg as the Python layer builds it for the library (offsets, records, converted arrays)."""
    import torch

    a = _args(d, lo, hi)
    with torch.no_grad():
        if leg == "posed":
            return vox._batch_call(a["coords"], a["offsets"], a["centers"], a["channels"], a["radii"], a["num_channels"],
                                   posed=(hip.dev(d["q"][lo:hi]), hip.dev(d["t"][lo:hi])), device=True)
        if leg == "rotated":
            np.random.seed(SEED)
            return vox._batch_call(a["coords"], a["offsets"], a["centers"], a["channels"], a["radii"], a["num_channels"], 0.5, True,
                                   device=True)
        return vox._batch_call(a["coords"], a["offsets"], a["centers"], a["channels"], a["radii"], a["num_channels"], device=True)


def _outputs(call):
    """(grad_coords, grad_features or None), full of NaN: whatever is not overwritten fails every comparison."""
    import torch

    return hip.nan((call.N, 3)), (hip.nan((call.N, call.C), torch.float32) if call.mode == "features" else None)


def _entry(vox, call, gm, target):
    """mvx_moments_backward_batch through ctypes: (grad_coords, grad_features or None)."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    g = torch.tensor(np.ascontiguousarray(gm, np.float64), device="cuda")
    assert tuple(g.shape) == (call.B, call.C, 2 if target is None else 3)
    gc, gf = _outputs(call)
    _lib.check(vox._lib.mvx_moments_backward_batch(*call.batch_args(vox), hip.ptr(target), g.data_ptr(), gc.data_ptr(), hip.ptr(gf),
                                                   vox._stream()))
    return gc, gf


def _backward_entry(vox, call, grad_out):
    from molvoxel_amd.voxelizer.hip import _lib

    gc, gf = _outputs(call)
    _lib.check(vox._lib.mvx_backward_batch(*call.batch_args(vox), grad_out.data_ptr(), gc.data_ptr(), hip.ptr(gf), vox._stream()))
    return gc, gf


def _same(a, b):
    import torch

    return (a[0] is None) == (b[0] is None) and (a[1] is None) == (b[1] is None) and all(
        x is None or (not torch.isnan(x).any() and torch.equal(x, y)) for x, y in zip(a, b))


def _const(d, K, *values):
    """dL/dm with the same K values for every molecule and channel."""
    return np.broadcast_to(np.array(values, np.float64), (d["B"], d["row"].C, K))


# ---- 1. bit identities: the plumbing, with no tolerance ------------------------------------------------------------------------
@pytest.mark.parametrize("leg", ["centred", "posed"])
@pytest.mark.parametrize("row_id", ROW_IDS)
def test_the_third_moment_alone_is_score_batch_over_the_target(row_id, leg):
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    d = _make(row_id)
    vox = _vox(row_id)
    call = _spec(vox, d, leg)
    t = hip.dev(_target(row_id))
    got = _entry(vox, call, _const(d, 3, 0.0, 0.0, 1.0), t)  # a0 = a1 = 0, a2 = 1: u = t exactly
    gc, gf = _outputs(call)
    scores = torch.empty(call.B, dtype=torch.float64, device="cuda")
    _lib.check(vox._lib.mvx_score_batch(*call.batch_args(vox), t.data_ptr(), 0, scores.data_ptr(), None, gc.data_ptr(), hip.ptr(gf),
                                        vox._stream()))
    assert _same(got, (gc, gf)), (row_id, leg)
    assert (gf if gf is not None else gc).abs().sum() > 0 or d["row"].density == "binary"


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_the_second_moment_alone_is_backward_batch_with_the_grids_as_upstream(row_id):
    d = _make(row_id)
    vox = _vox(row_id)
    call = _spec(vox, d, "posed")
    grids = _forward(vox, d, "posed")
    want = _backward_entry(vox, call, grids)  # a0 = 0, a1 = (float)(2 * 0.5) = 1, a2 = 0: u = g exactly
    assert _same(_entry(vox, call, _const(d, 2, 0.0, 0.5), None), want), row_id
    assert _same(_entry(vox, call, _const(d, 3, 0.0, 0.5, 0.0), hip.dev(_target(row_id))), want), row_id  # (0 * t + 0: finite targets)


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_the_first_moment_alone_is_backward_batch_with_an_upstream_of_ones(row_id):
    import torch

    d = _make(row_id)
    row = d["row"]
    vox = _vox(row_id)
    call = _spec(vox, d, "centred")
    ones = torch.ones((d["B"], row.C) + (row.D,) * 3, device="cuda")
    assert _same(_entry(vox, call, _const(d, 2, 1.0, 0.0), None), _backward_entry(vox, call, ones)), row_id  # u = fmaf(0, g, 1) = 1


# ---- 2. general coefficients against the float64 reference --------------------------------------------------------------------
def _pose_of(d, leg):
    """(quaternions (B, 4), translations (B, 3)) of a leg as the kernels use them."""
    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform

    B = d["B"]
    if leg == "posed":
        return d["q"], d["t"]
    if leg == "centred":
        return np.tile([1.0, 0.0, 0.0, 0.0], (B, 1)), np.zeros((B, 3))
    np.random.seed(SEED)
    drawn = [draw_forward_transform(0.5, True) for _ in range(B)]  # (translation, quaternion) per molecule, in molecule order
    return np.array([q for _, q in drawn]).reshape(B, 4), np.array([t for t, _ in drawn]).reshape(B, 3)


def _reference(d, leg, grids, gm, target, atoms, pre_rotation=False):
    """{atom: {"coords": (value, bound), "features": (value, bound)}} for the sampled atoms, molecule by molecule: the reference
    with G, and - for the bounds - with |a0| + |a1| |g| + |a2| |t| in its place. pre_rotation: dL/dp instead of dL/dcoords."""
    row = d["row"]
    q, t = _pose_of(d, leg)
    out = {}
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        mine = [a - lo for a in atoms if lo <= a < hi]
        if not mine:
            continue
        if leg == "rotated":  # (a random translation is added twice behind a random rotation: the reference's behaviour, kept)
            p = (PR.positions(d["xyz"][lo:hi], d["cen"][b], q[b], np.zeros(3)) + t[b]) + t[b]
        else:
            p = PR.positions(d["xyz"][lo:hi], d["cen"][b], q[b], t[b])
        G, Gabs = MG.upstream(grids[b], gm[b], target)
        kw = dict(mode=row.mode, density=row.density, atoms=mine, blockdim=getattr(row, "blockdim", None),
                  rot=None if (leg == "centred" or pre_rotation) else PR.rotation(q[b]))
        if row.mode == "features":
            kw["w"] = d["chan"][lo:hi]
        elif row.mode == "types":  # (a type outside [0, C) - here -1 - reaches no channel: the reference knows it as "beyond C")
            ty = d["chan"][lo:hi]
            kw["types"] = np.where((ty < 0) | (ty >= row.C), row.C, ty)
        radii = d["radii"][lo:hi] if row.radii_type == "atom-wise" else d["radii"]
        val = GR.reference(p, G, radii, row.radii_type, **kw)
        bnd = GR.reference(p, Gabs, radii, row.radii_type, **kw)
        for j, a in enumerate(mine):
            out[lo + a] = {k: (val[k][0][j], bnd[k][1][j]) for k in ("coords", "features") if k in val}
    return out


@functools.lru_cache(maxsize=None)
def _grids(row_id, leg):
    g = _forward(_vox(row_id), _make(row_id), leg).cpu().numpy()
    assert g.dtype == np.float32
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("row_id", ROW_IDS)
def test_general_coefficients_match_the_float64_reference(row_id, leg):
    d = _make(row_id)
    row = d["row"]
    vox = _vox(row_id)
    call = _spec(vox, d, leg)
    grids = _grids(row_id, leg)
    rng = np.random.default_rng(row.seed + 31)
    atoms = sorted(rng.choice(d["N"], min(d["N"], SAMPLE), replace=False).tolist())
    worst = 0.0
    for with_target in (True, False):
        K = 3 if with_target else 2
        gm = _dm(row_id, K)
        gc, gf = _entry(vox, call, gm, hip.dev(_target(row_id)) if with_target else None)
        gc = gc.cpu().numpy()
        gf = None if gf is None else gf.cpu().numpy()
        assert not np.isnan(gc).any() and (gf is None or not np.isnan(gf).any())  # fully overwritten
        ref = _reference(d, leg, grids, gm, _target(row_id) if with_target else None, atoms)
        assert len(ref) == len(atoms)
        live = 0
        for a, o in ref.items():
            worst = max(worst, GR.close(gc[a], o["coords"][0], o["coords"][1], f"{row_id} {leg} K={K} coords[{a}]", GRAD_REL, GRAD_ABS))
            if "features" in o:
                worst = max(worst, GR.close(gf[a], o["features"][0], o["features"][1], f"{row_id} {leg} K={K} features[{a}]",
                                            GRAD_REL, GRAD_ABS))
            live += bool(np.any(o["coords"][1] > 0) or ("features" in o and np.any(o["features"][1] > 0)))
        if row.density == "binary":  # the a.e. derivative: no coordinate gradient (and one channel of weight 1 has no other)
            assert (gc == 0).all()
        if row.density != "binary" or row.mode == "features":
            assert live > 0.3 * len(atoms), (row_id, leg, live)
    if row_id == "types":  # the atom of type -1 gets nothing
        assert (gc[R.BAD_TYPE_ATOM] == 0).all()
    print(f"MOMENTS_GRAD_WORST {row_id} {leg}: worst |got - ref| / (GRAD_REL * bound + GRAD_ABS) = {worst:.3g}")


# ---- 3. batch and chunk identities, to the bit ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _uncut(row_id, with_target):
    d = _make(row_id)
    vox = _vox(row_id)
    return _entry(vox, _spec(vox, d, "centred"), _dm(row_id, 3 if with_target else 2), hip.dev(_target(row_id)) if with_target else None)


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_a_molecule_alone_and_two_runs_give_the_batchs_bits(row_id):
    d = _make(row_id)
    vox = _vox(row_id)
    t = hip.dev(_target(row_id))
    whole = _uncut(row_id, True)
    assert _same(_entry(vox, _spec(vox, d, "centred"), _dm(row_id, 3), t), whole)  # two runs
    for b in range(d["B"]):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        if hi == lo:
            continue  # (no atoms: no rows, and the entry has no output to write)
        alone = _entry(vox, _spec(vox, d, "centred", b, b + 1), _dm(row_id, 3)[b:b + 1], t)
        assert _same(alone, tuple(None if x is None else x[lo:hi] for x in whole)), (row_id, b)


@pytest.mark.parametrize("row_id, option, value, nchunk", [
    ("carry", "chunks", 2, 2), ("chunks", "chunks", 2, 2),
    # a budget of 1 KB cuts after every molecule
    ("light", "mall_budget_kb", 1, 7), ("wide", "mall_budget_kb", 1, 4), ("types", "mall_budget_kb", 1, 5), ("single", "mall_budget_kb", 1, 6),
    # the entry's own bound on the grids a chunk leaves in scratch: carry's grids are 512 KiB each (two per chunk), then one per chunk
    ("carry", "mgrad_scratch_kb", 1024, 6), ("light", "mgrad_scratch_kb", 1, 7), ("chunks", "mgrad_scratch_kb", 4000, 5),
])
def test_molecule_chunks_give_the_uncut_bits(row_id, option, value, nchunk):
    d = _make(row_id)
    vox = _new_vox(row_id)  # (a voxelizer of its own: the option stays with the handle)
    vox.debug_option(option, value)
    for with_target in (True, False):
        got = _entry(vox, _spec(vox, d, "centred"), _dm(row_id, 3 if with_target else 2), hip.dev(_target(row_id)) if with_target else None)
        plan = vox.last_plan()
        assert plan["nchunk"] == nchunk, plan  # the cut really happened, and the entry reports it
        assert _same(got, _uncut(row_id, with_target)), (row_id, with_target)


def test_the_spatial_order_applies_per_chunk_and_keeps_the_bits():
    vox = _new_vox("carry")
    vox.debug_option("grad_order", 1)
    vox.debug_option("chunks", 2)
    d = _make("carry")
    assert _same(_entry(vox, _spec(vox, d, "centred"), _dm("carry", 3), hip.dev(_target("carry"))), _uncut("carry", True))
    assert vox.last_plan()["nchunk"] == 2


@pytest.mark.parametrize("row_id, kw", [("chunks", dict(grid_dtype="bfloat16")), ("wide", dict(grid_layout="channels_last")),
                                        ("types", dict(grid_dtype="bfloat16", grid_layout="channels_last"))])
def test_bfloat16_and_channels_last_voxelizers_give_the_float32_bits(row_id, kw):
    import torch

    d = _make(row_id)
    vox = _vox(row_id, **kw)
    assert vox.forward_batch(**_args(d, 0, 1)).dtype == (torch.bfloat16 if "grid_dtype" in kw else torch.float32)
    for with_target in (True, False):
        got = _entry(vox, _spec(vox, d, "centred"), _dm(row_id, 3 if with_target else 2), hip.dev(_target(row_id)) if with_target else None)
        assert _same(got, _uncut(row_id, with_target)), (row_id, with_target)
    # the handle still writes its own grid type afterwards
    assert vox.forward_batch(**_args(d, 0, 1)).dtype == (torch.bfloat16 if "grid_dtype" in kw else torch.float32)


# ---- 4. autograd end to end: the loss -NCC --------------------------------------------------------------------------------------
def _ncc_loss(m, tt):
    """-sum over molecules and channels of m2 / sqrt(m1 * sum t^2); a channel no atom reaches contributes 0 (the small constant)."""
    import torch

    return -(m[..., 2] / torch.sqrt(m[..., 1] * tt + 1e-6)).sum()


def _moments_of(grids, T):
    import torch

    g = grids.double()
    return torch.stack([g.sum((2, 3, 4)), (g * g).sum((2, 3, 4)), (g * T.double()).sum((2, 3, 4))], dim=-1)


def _upstream_of(m, tt):
    """dL/dm of the loss at the moments m, as a host array."""
    m = m.detach().clone().requires_grad_()
    _ncc_loss(m, tt).backward()
    return m.grad.cpu().numpy()


def _close(got, ref, bound, what):
    return GR.close(got.detach().cpu().numpy(), ref.detach().cpu().numpy(), bound, what, GRAD_REL, GRAD_ABS)


def test_autograd_gives_coordinate_and_feature_gradients_of_the_ncc_loss():
    import torch

    row_id = "light"
    d = _make(row_id)
    vox = _new_vox(row_id, differentiable=True, moments_grad=True)
    plain = _new_vox(row_id, differentiable=True)
    T = hip.dev(_target(row_id))
    tt = (T.double() ** 2).sum((1, 2, 3))
    a = _args(d)

    def leaves():
        return dict(a, coords=a["coords"].clone().requires_grad_(), channels=a["channels"].clone().requires_grad_())

    x = leaves()
    m = vox.moments_batch(target=T, **x)
    assert m.requires_grad and m.dtype == torch.float64 and tuple(m.shape) == (d["B"], 5, 3)
    ungraphed = plain.moments_batch(target=T, **leaves())
    assert not ungraphed.requires_grad  # without the flag the moments stay outside the graph
    assert torch.equal(m.detach(), ungraphed)  # the same call, the same bits
    with torch.no_grad():
        assert not vox.moments_batch(target=T, **x).requires_grad
    assert not vox.moments_batch(target=T, **a).requires_grad  # nothing requires grad: no graph
    _ncc_loss(m, tt).backward()
    y = leaves()
    grids = plain.forward_batch(**y)
    _ncc_loss(_moments_of(grids, T), tt).backward()
    # the bar: the float64 reference's bounds for the upstream this loss has at these moments
    gm = _upstream_of(m, tt)
    ref = _reference(d, "centred", grids.detach().cpu().numpy(), gm, _target(row_id), list(range(d["N"])))
    bc = np.stack([ref[n]["coords"][1] for n in range(d["N"])])
    bf = np.stack([ref[n]["features"][1] for n in range(d["N"])])
    assert (bc > 0).any() and (x["coords"].grad != 0).any() and (x["channels"].grad != 0).any()
    w1 = _close(x["coords"].grad, y["coords"].grad, bc, "coords")
    w2 = _close(x["channels"].grad, y["channels"].grad, bf, "features")
    print(f"MOMENTS_GRAD_AUTOGRAD light: moments path against grid path, worst ratio coords {w1:.3g}, features {w2:.3g}")
    # a second backward through the saved record of a random transform reuses the records
    np.random.seed(SEED)
    z = leaves()
    mr = vox.moments_batch(target=T, random_rotation=True, random_translation=0.5, **z)
    np.random.seed(SEED + 1)  # (backward() draws nothing)
    state = np.random.get_state()[1].copy()
    _ncc_loss(mr, tt).backward()
    assert np.array_equal(np.random.get_state()[1], state)
    call = _spec(_vox(row_id), d, "rotated")
    gc, gf = _entry(_vox(row_id), call, _upstream_of(mr, tt), T)
    assert torch.equal(z["coords"].grad, gc) and torch.equal(z["channels"].grad, gf)


def test_autograd_gives_pose_gradients_of_the_ncc_loss():
    import torch

    row_id = "chunks"
    d = _make(row_id)
    B = d["B"]
    vox = _new_vox(row_id, differentiable=True, moments_grad=True)
    plain = _new_vox(row_id, differentiable=True)
    T = hip.dev(_target(row_id))
    tt = (T.double() ** 2).sum((1, 2, 3))
    a = _args(d)

    def leaves():
        return dict(a, centers=hip.dev(d["cen"], True), quaternions=hip.dev(d["q"], True), translations=hip.dev(d["t"], True))

    x = leaves()
    m = vox.moments_posed_batch(target=T, **x)
    assert m.requires_grad
    assert torch.equal(m.detach(), plain.moments_posed_batch(target=T, **leaves()))
    _ncc_loss(m, tt).backward()
    y = leaves()
    grids = plain.forward_posed_batch(**y)
    _ncc_loss(_moments_of(grids, T), tt).backward()
    gm = _upstream_of(m, tt)
    ref = _reference(d, "posed", grids.detach().cpu().numpy(), gm, _target(row_id), list(range(d["N"])), pre_rotation=True)
    bounds = {"center": [], "quaternion": [], "translation": []}
    for b in range(B):
        lo, hi = int(d["off"][b]), int(d["off"][b + 1])
        G = np.stack([ref[n]["coords"][0] for n in range(lo, hi)])
        bd = np.stack([ref[n]["coords"][1] for n in range(lo, hi)])
        pg = PR.pose_grads(d["xyz"][lo:hi], d["cen"][b], d["q"][b], G, bd)
        for k in bounds:
            bounds[k].append(pg[k][1])
    worst = {}
    for k, name in (("center", "centers"), ("quaternion", "quaternions"), ("translation", "translations")):
        assert (x[name].grad != 0).any()
        worst[k] = _close(x[name].grad, y[name].grad, np.stack(bounds[k]), name)
    print(f"MOMENTS_GRAD_AUTOGRAD chunks posed: moments path against grid path, worst ratios {worst}")


def test_a_change_of_density_between_forward_and_backward_is_refused():
    import torch

    d = _make("light")
    vox = _new_vox("light", differentiable=True, moments_grad=True)
    a = _args(d)
    a["coords"] = a["coords"].clone().requires_grad_()
    m = vox.moments_batch(**a)
    vox.density_type = "binary"
    with pytest.raises(RuntimeError, match="changed between the forward call and backward"):
        m.sum().backward()
    assert isinstance(m, torch.Tensor)


# ---- 5. the rules of the entry that read the handle, through the C ABI ----------------------------------------------------------
def test_the_library_names_what_it_does_not_serve_and_what_it_misses():
    import molvoxel_amd as mv
    import torch

    def call(vox, C_=4, mode=0, rt=0, radii=None, target=None, gm=True, gc=True, gf=True, B=1):
        xyz = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
        feat = torch.ones((3, C_), device="cuda") if mode == 0 else torch.zeros(3, dtype=torch.int32, device="cuda")
        g = torch.ones((1, C_, 2 if target is None else 3), dtype=torch.float64, device="cuda")
        out_c, out_f = hip.nan((3, 3)), hip.nan((3, C_), torch.float32)
        off = np.array([0, 3] if B else [0], np.int64)
        rc = vox._lib.mvx_moments_backward_batch(vox._handle, mode, xyz.data_ptr(), feat.data_ptr(), hip.ptr(radii), 1.0, rt, off.ctypes.data,
                                                 None, B, C_, hip.ptr(target), g.data_ptr() if gm else None, out_c.data_ptr() if gc else None,
                                                 out_f.data_ptr() if gf else None, None)
        return rc, last_error(), out_c, out_f

    mk = lambda D, rt="scalar", **kw: mv.create_voxelizer(0.5, D, rt, "gaussian", library="hip", **kw)  # noqa: E731
    for vox, kw, words in [
        (mk(16, precision=64), {}, "precision 64"),
        (mk(16, "channel-wise"), dict(rt=2, radii=torch.ones(4, device="cuda")), "channel-wise radii with features"),
        (mk(18), {}, "no multiple of 4"),
        (mk(24, blockdim=12), {}, "per-lane ranges"),
        (mk(16), dict(target=torch.zeros(4 * 16 ** 3 + 1, device="cuda")[1:]), "16-byte aligned"),
    ]:
        rc, msg, _, _ = call(vox, gm=False, gc=False, gf=False, **kw)  # (these rules come before the entry's own)
        assert rc == MVX_ERR_INVALID and msg.startswith("moments:" if "aligned" not in words else "target") and words in msg, (rc, msg)
    vox = mk(16)
    for kw, want in [
        (dict(gm=False, mode=1, gc=False), "grad_moments must not be null"),
        (dict(mode=1, gc=False), "grad_features exists in features mode only"),
        (dict(gc=False, gf=False), "grad_coords and grad_features are both null"),
    ]:
        rc, msg, _, _ = call(vox, **kw)
        assert rc == MVX_ERR_INVALID and msg == want, (kw, rc, msg)
    assert call(vox, B=0, gm=False)[0] == 0  # no molecules: MVX_OK, and no grad_moments to miss
    rc, msg, gc, gf = call(vox)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert not torch.isnan(gc).any() and not torch.isnan(gf).any()
    assert (gf > 0).all() and torch.equal(gf, gf[0, 0].expand(3, 4))  # three atoms at the centre, dL/dm = 1: the same row thrice
    rc, msg, gc, gf = call(vox, gf=False)  # coordinates alone
    assert rc == 0 and not torch.isnan(gc).any() and torch.isnan(gf).all()
