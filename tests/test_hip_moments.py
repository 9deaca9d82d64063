"""moments_batch / moments_posed_batch (mvx_moments_batch) on the GPU: per-channel sums and norms of every molecule's grid without
the grids, over the rows of tests/sum_rows.py and six rows of tests/sum_sweep_rows.py.

The reference is always the float32 grid of forward_batch / forward_posed_batch on the same voxelizer and inputs, reduced exactly
(tests/moments_reference.moments_of); the bar is moments_reference.bound, (n - 1) 2^-53 sum|term| - the worst case of any float64
summation order of the exact terms - and nothing else. Sums of small integers (binary density with types or one channel) must be
equal. The identities of the contract are held to the bit: a molecule alone, two runs, molecule chunks, with and without a target,
bfloat16 and channels-last voxelizers.
"""
import functools

import numpy as np
import pytest

from tests import moments_reference as MR
from tests import sum_rows as R
from tests import sum_sweep_rows as S
from tests import hip_support as hip
from tests.abi import MVX_ERR_INVALID, last_error

pytestmark = pytest.mark.gpu

SWEEP_IDS = ["edge20", "edge20d", "edge12", "cut96", "bd16", "tall"]
ROW_IDS = R.ROW_IDS + SWEEP_IDS


def _make(row_id):
    """A row of tests/sum_rows.py, or a row or a draw ("draw<seed>") of tests/sum_sweep_rows.py."""
    return S.make(row_id) if (row_id in S.BY_ID or row_id.startswith("draw")) else R.make(row_id)


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


def _posed_args(d):
    a = _args(d)
    return dict(a, quaternions=hip.dev(d["q"]), translations=hip.dev(d["t"]))


@functools.lru_cache(maxsize=None)
def _target(row_id):
    """A seeded float32 target of mixed signs, (C, D, D, D) (never modified)."""
    row = _make(row_id)["row"]
    t = np.random.default_rng(row.seed + 5000).standard_normal((row.C,) + (row.D,) * 3).astype(np.float32)
    t.setflags(write=False)
    return t


SEED = 77  # the rotation legs seed numpy's global generator as tests/test_hip_sum.py does


def _call(vox, d, kind, target=None, method=True):
    """moments_* (method) or forward_* of one of the three legs: "centred", "posed", "rotated"."""
    if kind == "posed":
        fn = vox.moments_posed_batch if method else vox.forward_posed_batch
        kw = _posed_args(d)
    else:
        fn = vox.moments_batch if method else vox.forward_batch
        kw = _args(d)
        if kind == "rotated":
            np.random.seed(SEED)
            kw.update(random_rotation=True, random_translation=0.5)
    if method:
        kw["target"] = target
    return fn(**kw)


@functools.lru_cache(maxsize=None)
def _reference(row_id, kind):
    """(moments (B, C, 3), bound (B, C, 3)) of the float32 grids forward_batch / forward_posed_batch write for a row, with the row's
    target: computed once, shared, never modified. The first two moments are the reference of the call without a target."""
    d = _make(row_id)
    grids = _call(_vox(row_id), d, kind, method=False)
    row = d["row"]
    assert tuple(grids.shape) == (d["B"], row.C) + (row.D,) * 3
    m, b = MR.moments_and_bound(grids.cpu().numpy(), _target(row_id))
    m.setflags(write=False)
    b.setflags(write=False)
    return m, b


def _integers(row):
    return row.density == "binary" and row.mode in ("types", "single")


def _check(got, ref, bnd, row, what):
    import torch

    K = ref.shape[-1]
    assert got.dtype == torch.float64 and got.is_cuda and tuple(got.shape) == ref.shape, (what, got.dtype, tuple(got.shape))
    g = got.cpu().numpy()
    err = np.abs(g - ref)
    live = bnd > 0
    worst = float((err[live] / bnd[live]).max()) if live.any() else 0.0
    print(f"{what}: K = {K}, worst |got - exact| / bound = {worst:.3g}, largest moment {float(np.abs(ref).max()):.6g}")
    assert live.any(), what
    assert (err <= bnd).all(), (what, worst)  # (where the bound is 0 - no atom reaches the channel - this is equality with 0)
    if _integers(row):  # sums of small integers: voxel counts
        assert np.array_equal(g[..., :2], ref[..., :2]) and (g[..., :2] == np.round(g[..., :2])).all(), what


# ---- 1. against forward_batch's grids ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_id", ROW_IDS)
def test_moments_are_those_of_forward_batchs_grids(row_id):
    d = _make(row_id)
    row = d["row"]
    ref, bnd = _reference(row_id, "centred")
    vox = _vox(row_id)
    plain = _call(vox, d, "centred")
    _check(plain, ref[..., :2], bnd[..., :2], row, f"{row_id} without a target")
    with_t = _call(vox, d, "centred", hip.dev(_target(row_id)))
    _check(with_t, ref, bnd, row, f"{row_id} with a target")
    # molecules without atoms, or with none inside the box: exact zeros
    sizes = np.diff(d["off"])
    empty = [b for b in range(d["B"]) if sizes[b] == 0 or (row_id == "light" and b == R.OUTSIDE_MOLECULE)]
    assert (with_t[empty] == 0).all() and (plain[empty] == 0).all()
    if row_id in ("light", "edge12"):
        assert len(empty) >= 2
    assert (ref[[b for b in range(d["B"]) if b not in empty], :, 1] > 0).any()


def test_the_rows_have_molecules_that_reach_no_voxel_next_to_ones_that_do():
    one = _reference("light", "centred")[0]
    assert (one[R.OUTSIDE_MOLECULE] == 0).all() and (one[0] == 0).all() and (one[4] == 0).all() and (one[3, :, 0] > 0).all()


@pytest.mark.parametrize("row_id", R.ROW_IDS + ["edge12", "bd16"])
def test_posed_moments_are_those_of_forward_posed_batchs_grids(row_id):
    d = _make(row_id)
    ref, bnd = _reference(row_id, "posed")
    _check(_call(_vox(row_id), d, "posed", hip.dev(_target(row_id))), ref, bnd, d["row"], f"{row_id} posed")
    _check(_call(_vox(row_id), d, "posed"), ref[..., :2], bnd[..., :2], d["row"], f"{row_id} posed, no target")
    assert not np.array_equal(ref, _reference(row_id, "centred")[0])  # (the poses reach the call)


@pytest.mark.parametrize("row_id", ["light", "chunks", "types", "single", "edge20d"])
def test_rotated_moments_are_those_of_forward_batch_with_the_same_rng_state(row_id):
    d = _make(row_id)
    ref, bnd = _reference(row_id, "rotated")
    _check(_call(_vox(row_id), d, "rotated", hip.dev(_target(row_id))), ref, bnd, d["row"], f"{row_id} rotated")
    drawn = np.random.rand()
    np.random.seed(SEED)
    _vox(row_id).forward_batch(random_rotation=True, random_translation=0.5, **_args(d))
    assert np.random.rand() == drawn  # the same draws were consumed
    assert not np.array_equal(ref, _reference(row_id, "centred")[0])


# ---- 2. bit identities -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _uncut(row_id, with_target):
    return _call(_vox(row_id), _make(row_id), "centred", hip.dev(_target(row_id)) if with_target else None)


@pytest.mark.parametrize("row_id", ROW_IDS)
def test_a_molecule_alone_two_runs_and_the_target_do_not_change_the_bits(row_id):
    import torch

    d = _make(row_id)
    vox = _vox(row_id)
    t = hip.dev(_target(row_id))
    both, plain = _uncut(row_id, True), _uncut(row_id, False)
    assert torch.equal(both[..., :2], plain)  # the first two moments do not depend on the target
    assert torch.equal(_call(vox, d, "centred", t), both) and torch.equal(_call(vox, d, "centred"), plain)  # two runs
    for b in range(d["B"]):  # molecule b alone is row b of the batch
        assert torch.equal(vox.moments_batch(target=t, **_args(d, b, b + 1)), both[b:b + 1]), (row_id, b)
    if d["B"] > 2:  # ... and so is any other cut of the batch into calls
        assert torch.equal(vox.moments_batch(target=t, **_args(d, 1, d["B"])), both[1:])


@pytest.mark.parametrize("row_id, option, value, nchunk", [
    ("carry", "chunks", 2, 2), ("chunks", "chunks", 2, 2), ("tall", "mall_budget_kb", 1, 3), ("cut96", "mall_budget_kb", 1, 3),
    # one molecule per chunk (tests/test_hip_sum.py: a budget of 1 KB cuts after every molecule)
    ("light", "mall_budget_kb", 1, 7), ("wide", "mall_budget_kb", 1, 4), ("types", "mall_budget_kb", 1, 5), ("long", "mall_budget_kb", 1, 3),
    ("single", "mall_budget_kb", 1, 6), ("edge12", "mall_budget_kb", 1, 5),
])
def test_molecule_chunks_give_the_uncut_bits(row_id, option, value, nchunk):
    import torch

    d = _make(row_id)
    vox = _new_vox(row_id)  # (a voxelizer of its own: the option stays with the handle)
    vox.debug_option(option, value)
    for with_target in (True, False):
        got = _call(vox, d, "centred", hip.dev(_target(row_id)) if with_target else None)
        plan = vox.last_plan()
        assert plan["nchunk"] == nchunk, plan  # the cut really happened
        assert plan["ct"] == 32 and plan["ncc"] == -(-d["row"].C // 32) and plan["route"] == 0 and plan["grouped"] == 0, plan
        assert torch.equal(got, _uncut(row_id, with_target)), (row_id, with_target)


@pytest.mark.parametrize("row_id, kw", [("chunks", dict(grid_dtype="bfloat16")), ("wide", dict(grid_layout="channels_last")),
                                        ("types", dict(grid_dtype="bfloat16", grid_layout="channels_last"))])
def test_bfloat16_and_channels_last_voxelizers_give_the_float32_bits(row_id, kw):
    import torch

    d = _make(row_id)
    vox = _vox(row_id, **kw)
    assert vox.forward_batch(**_args(d, 0, 1)).dtype == (torch.bfloat16 if "grid_dtype" in kw else torch.float32)
    assert torch.equal(_call(vox, d, "centred", hip.dev(_target(row_id))), _uncut(row_id, True))
    assert torch.equal(_call(vox, d, "centred"), _uncut(row_id, False))


# ---- 3. many molecules -------------------------------------------------------------------------------------------------------
def test_sixty_six_thousand_molecules_cross_the_grid_limit_and_the_chunk_workspace():
    import molvoxel_amd as mv
    import torch

    B, D = 66000, 8
    rng = np.random.default_rng(66)
    sizes = rng.integers(1, 4, B)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    half = 0.5 * (D - 1) / 2
    xyz = rng.uniform(-half - 0.5, half + 0.5, (int(off[-1]), 3))
    target = rng.standard_normal((1, D, D, D)).astype(np.float32)
    vox = mv.create_voxelizer(0.5, D, "scalar", "gaussian", library="hip")
    a = dict(coords=hip.dev(xyz), offsets=off, centers=None, channels=None, radii=1.0)
    got = vox.moments_batch(target=hip.dev(target), **a)
    plan = vox.last_plan()
    assert plan["nchunk"] >= 2 and B > 65535, plan  # more molecules than one launch's grid holds
    assert got.dtype == torch.float64 and tuple(got.shape) == (B, 1, 3)
    grids = vox.forward_batch(**a)
    assert tuple(grids.shape) == (B, 1, D, D, D)
    ref, bnd = MR.moments_and_bound(grids.cpu().numpy(), target)
    err = np.abs(got.cpu().numpy() - ref)
    print(f"66 000 molecules: worst |got - exact| / bound = {float((err[bnd > 0] / bnd[bnd > 0]).max()):.3g}, {plan['nchunk']} chunks")
    assert (err <= bnd).all() and (ref[:, 0, 1] > 0).mean() > 0.9
    assert torch.equal(vox.moments_batch(**a), got[..., :2])
    # the last molecules alone: what sits behind the cut is not a function of the cut
    lo = B - 500
    tail = dict(a, coords=hip.dev(xyz[off[lo]:]), offsets=off[lo:] - off[lo])
    assert torch.equal(vox.moments_batch(target=hip.dev(target), **tail), got[lo:])


# ---- 4. what the calls refuse, and the calls without molecules or atoms ----------------------------------------------------------
def test_no_molecules_and_no_atoms():
    import torch

    vox = _vox("light")
    none = dict(coords=torch.empty((0, 3), dtype=torch.float64, device="cuda"), centers=None, channels=torch.empty((0, 5), device="cuda"),
                radii=1.0)
    t = hip.dev(_target("light"))
    for offsets, B in ((np.array([0]), 0), (np.array([0, 0, 0]), 2)):
        for target in (None, t):
            got = vox.moments_batch(offsets=offsets, target=target, **none)
            assert tuple(got.shape) == (B, 5, 2 if target is None else 3) and got.dtype == torch.float64 and (got == 0).all()


def test_a_target_of_the_wrong_shape_and_inputs_that_require_grad():
    import torch

    d = _make("light")
    vox = _vox("light")
    with pytest.raises(AssertionError, match="target does not match dimension"):
        vox.moments_posed_batch(target=torch.zeros((5, 16, 16, 8), device="cuda"), **_posed_args(d))
    with pytest.raises(AssertionError, match="target does not match dimension"):
        vox.moments_batch(target=torch.zeros((4, 16, 16, 16), device="cuda"), **_args(d))
    # a float64 host target is converted; inputs that require grad are read as values
    a = _args(d)
    a["coords"] = a["coords"].clone().requires_grad_()
    got = _vox("light", differentiable=True).moments_batch(target=_target("light").astype(np.float64), **a)
    assert not got.requires_grad and torch.equal(got, _uncut("light", True))


def test_the_library_names_what_it_does_not_serve():
    """The rules of mvx_moments_batch that read the handle (tests/test_moments_host.py has the others), through the C ABI."""
    import molvoxel_amd as mv
    import torch

    def call(vox, C_=4, rt=0, radii=None, target=None):
        xyz = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
        feat = torch.ones((3, C_), device="cuda")
        out = torch.empty((1, C_, 2 if target is None else 3), dtype=torch.float64, device="cuda")
        off = np.array([0, 3], np.int64)
        rc = vox._lib.mvx_moments_batch(vox._handle, 0, xyz.data_ptr(), feat.data_ptr(), None if radii is None else radii.data_ptr(),
                                        1.0, rt, off.ctypes.data, None, 1, C_, None if target is None else target.data_ptr(),
                                        out.data_ptr(), None)
        return rc, last_error(), out

    mk = lambda D, rt="scalar", **kw: mv.create_voxelizer(0.5, D, rt, "gaussian", library="hip", **kw)  # noqa: E731
    for vox, kw, words in [
        (mk(16, precision=64), {}, "precision 64"),
        (mk(16, "channel-wise"), dict(rt=2, radii=torch.ones(4, device="cuda")), "channel-wise radii with features"),
        (mk(18), {}, "no multiple of 4"),
        (mk(24, blockdim=12), {}, "per-lane ranges"),
        (mk(16), dict(target=torch.zeros(4 * 16 ** 3 + 1, device="cuda")[1:]), "16-byte aligned"),
    ]:
        rc, msg, _ = call(vox, **kw)
        assert rc == MVX_ERR_INVALID and msg.startswith("moments:" if "aligned" not in words else "target") and words in msg, (rc, msg)
    rc, msg, out = call(mk(16))
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert (out[0, :, 0] > 0).all() and torch.equal(out[0, :, 0], out[0, 0, 0].expand(4))  # three atoms at the centre, weight 1
