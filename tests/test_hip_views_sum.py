"""forward_views_sum / forward_posed_views_sum (mvx_forward_views_sum) on the GPU: the summed grid of B views of ONE shared cloud
against forward_sum on the cloud repeated B times (bit for bit), against forward_sum on the gathered
selection, and against the float64 sum of forward_views' grids. Clouds of 600 atoms from tests/views_rows.py, seven views of
which view 0 selects nothing, D = 16, res 1.0."""
import functools

import numpy as np
import pytest

import tests.test_hip_sum as HS  # (_check_weighted_sum: the bar of the rotated and posed sums, GRAD_REL * bound + GRAD_ABS)
from tests import views_rows as V
from tests import hip_support as hip
from tests.abi import MVX_ERR_INVALID, last_error
from tests.tolerance import assert_exact

pytestmark = pytest.mark.gpu

B, N, D = 7, 600, 16
# id: (seed, mode, C, radii_type, density)
CASES = {
    "features-C5-scalar": (11, "features", 5, "scalar", "gaussian"),  # one padded chunk
    "features-C33-atom": (12, "features", 33, "atom-wise", "gaussian"),  # two chunks
    "types-C8-by-type": (13, "types", 8, "channel-wise", "gaussian"),  # radii[types]
    "single-binary": (14, "single", 1, "scalar", "binary"),
    "single-atom": (15, "single", 1, "atom-wise", "gaussian"),
}


@functools.lru_cache(maxsize=None)
def _vox(radii_type, density, D_=D, **kw):
    import molvoxel_amd as mv

    return mv.create_voxelizer(1.0, D_, radii_type, density, library="hip", **dict(kw))


@functools.lru_cache(maxsize=None)
def _case(case_id, nviews=B):
    """The cloud and the views of a case as host arrays (never modified), with the cloud repeated once per view."""
    seed, mode, C_, rt, density = CASES[case_id]
    xyz, chan, radii = V.cloud(seed, N, mode, C_, rt)
    cen = V.centers(seed, nviews, xyz)
    rng = np.random.default_rng(seed + 7)
    q = rng.standard_normal((nviews, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    rep = dict(coords=np.tile(xyz, (nviews, 1)), offsets=np.arange(nviews + 1, dtype=np.int64) * N,
               channels=None if chan is None else np.concatenate([chan] * nviews),
               radii=np.tile(radii, nviews) if rt == "atom-wise" else radii)
    return dict(xyz=xyz, chan=chan, radii=radii, cen=cen, q=q, t=rng.uniform(-0.5, 0.5, (nviews, 3)), rep=rep, mode=mode, C=C_, rt=rt,
                density=density, nc=C_ if mode == "types" else None, w=rng.standard_normal(nviews).astype(np.float32),
                vox=_vox(rt, density))


def _views_sum(c, vox=None, **kw):
    return (vox or c["vox"]).forward_views_sum(hip.dev(c["xyz"]), hip.dev(c["cen"]), hip.dev(c["chan"]), hip.dev(c["radii"]), num_channels=c["nc"], **kw)


def _repeated_sum(c, vox=None, **kw):
    r = c["rep"]
    return (vox or c["vox"]).forward_sum(hip.dev(r["coords"]), r["offsets"], hip.dev(c["cen"]), hip.dev(r["channels"]), hip.dev(r["radii"]),
                                         num_channels=c["nc"], **kw)


@functools.lru_cache(maxsize=None)
def _plain(case_id):
    """The one plain call of a case (computed once, shared, never modified): the grid as a host array."""
    return _views_sum(_case(case_id)).cpu().numpy()


# ---- 1 - 6: bit for bit forward_sum on the cloud repeated B times ------------------------------------------------------------
@pytest.mark.parametrize("case_id", list(CASES))
def test_views_sum_is_forward_sum_on_the_repeated_cloud(case_id):
    c = _case(case_id)
    got = _plain(case_id)
    assert got.shape == (c["C"], D, D, D) and got.dtype == np.float32 and float(np.abs(got).max()) > 0
    assert_exact(got, _repeated_sum(c).cpu().numpy())


@pytest.mark.parametrize("case_id", ["features-C5-scalar", "types-C8-by-type"])
def test_random_transforms_are_drawn_per_view_as_forward_sum_draws_them(case_id):
    c = _case(case_id)
    np.random.seed(5)
    got = _views_sum(c, **V.TRANSFORM)
    np.random.seed(5)
    ref = _repeated_sum(c, **V.TRANSFORM)
    assert_exact(got.cpu().numpy(), ref.cpu().numpy())
    assert not np.array_equal(got.cpu().numpy(), _plain(case_id))  # (the transforms did something)


@pytest.mark.parametrize("case_id", ["features-C33-atom", "types-C8-by-type", "single-binary"])
def test_views_sum_is_forward_sum_on_the_gathered_selection(case_id):
    c = _case(case_id)
    vox = c["vox"]
    index, offsets = vox.select_views(hip.dev(c["xyz"]), hip.dev(c["cen"]), hip.dev(c["chan"]) if c["mode"] == "types" else None, hip.dev(c["radii"]))
    assert offsets[1] == 0 and 0 < offsets[-1] < B * N  # view 0 selects nothing; atoms are culled
    i = index.cpu().numpy()
    ref = vox.forward_sum(hip.dev(c["xyz"][i]), offsets, hip.dev(c["cen"]), None if c["chan"] is None else hip.dev(c["chan"][i]),
                          hip.dev(c["radii"][i]) if c["rt"] == "atom-wise" else hip.dev(c["radii"]), num_channels=c["nc"])
    assert_exact(_plain(case_id), ref.cpu().numpy())


@pytest.mark.parametrize("case_id", ["features-C5-scalar", "single-atom"])
def test_posed_views_sum_is_forward_posed_sum_on_the_repeated_cloud(case_id):
    c = _case(case_id)
    r = c["rep"]
    w = c["w"]
    got = c["vox"].forward_posed_views_sum(hip.dev(c["xyz"]), hip.dev(c["cen"]), hip.dev(c["q"]), hip.dev(c["t"]), hip.dev(c["chan"]), hip.dev(c["radii"]),
                                           weights=hip.dev(w))
    ref = c["vox"].forward_posed_sum(hip.dev(r["coords"]), r["offsets"], hip.dev(c["cen"]), hip.dev(c["q"]), hip.dev(c["t"]), hip.dev(r["channels"]),
                                     hip.dev(r["radii"]), weights=hip.dev(w))
    assert float(ref.abs().max()) > 0
    assert_exact(got.cpu().numpy(), ref.cpu().numpy())


@pytest.mark.parametrize("case_id", ["features-C5-scalar", "features-C33-atom", "types-C8-by-type"])
def test_view_weights_are_the_molecule_weights_of_forward_sum(case_id):
    c = _case(case_id)
    assert (c["w"][1:] > 0).any() and (c["w"][1:] < 0).any()  # mixed signs among the views that select atoms
    got = _views_sum(c, weights=hip.dev(c["w"])).cpu().numpy()
    assert_exact(got, _repeated_sum(c, weights=hip.dev(c["w"])).cpu().numpy())
    assert not np.array_equal(got, _plain(case_id))


def test_accumulate_continues_from_the_grid_as_forward_sum_does():
    import torch

    c = _case("features-C33-atom")
    start = np.random.default_rng(3).standard_normal((33, D, D, D)).astype(np.float32)
    out, ref = torch.tensor(start, device="cuda"), torch.tensor(start, device="cuda")
    ret = _views_sum(c, weights=hip.dev(c["w"]), out_grid=out, accumulate=True)
    assert ret is out
    _repeated_sum(c, weights=hip.dev(c["w"]), out_grid=ref, accumulate=True)
    assert_exact(out.cpu().numpy(), ref.cpu().numpy())
    assert not np.array_equal(out.cpu().numpy(), start)


# ---- 7. empty cases ----------------------------------------------------------------------------------------------------------
def test_no_atoms_or_no_selected_atoms_write_zeros_or_leave_an_accumulated_grid_untouched():
    import torch

    vox = _vox("scalar", "gaussian")
    start = np.random.default_rng(4).standard_normal((5, D, D, D)).astype(np.float32)
    c = _case("features-C5-scalar")
    nobody = dict(coords=torch.empty((0, 3), dtype=torch.float64, device="cuda"), centers=hip.dev(c["cen"]),
                  channels=torch.empty((0, 5), device="cuda"), radii=1.5)
    far = dict(coords=hip.dev(c["xyz"]), centers=hip.dev(c["cen"] + 1000.0), channels=hip.dev(c["chan"]), radii=1.5)
    for a in (nobody, far):
        out = torch.tensor(start, device="cuda")
        vox.forward_views_sum(out_grid=out, accumulate=True, weights=hip.dev(c["w"]), **a)
        assert_exact(out.cpu().numpy(), start)
        vox.forward_views_sum(out_grid=out, **a)
        assert float(out.abs().max()) == 0.0
        assert float(vox.forward_views_sum(**a).abs().max()) == 0.0


# ---- 8. an independent check -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", ["features-C33-atom", "types-C8-by-type", "single-atom"])
def test_views_sum_is_the_weighted_sum_of_forward_views_grids(case_id):
    c = _case(case_id)
    a = (hip.dev(c["xyz"]), hip.dev(c["cen"]), hip.dev(c["chan"]), hip.dev(c["radii"]))
    np.random.seed(9)
    got = c["vox"].forward_views_sum(*a, weights=hip.dev(c["w"]), num_channels=c["nc"], **V.TRANSFORM)
    np.random.seed(9)
    grids = c["vox"].forward_views(*a, num_channels=c["nc"], **V.TRANSFORM)
    HS._check_weighted_sum(got.cpu().numpy(), grids, c["w"], f"{case_id} views")


# ---- 9. a cut ----------------------------------------------------------------------------------------------------------------
def test_molecule_chunks_give_the_uncut_bits():
    """The "chunks" option cuts a batch of at least 4 x 3 molecules (mvx_plan.hip), so this test uses twelve views of the cloud
    instead of seven: view 0 still selects nothing."""
    import molvoxel_amd as mv

    c = _case("features-C33-atom", 12)
    uncut = _views_sum(c, weights=hip.dev(c["w"])).cpu().numpy()
    vox = mv.create_voxelizer(1.0, D, c["rt"], c["density"], library="hip")  # (a voxelizer of its own: the option stays with the handle)
    vox.debug_option("chunks", 3)
    got = _views_sum(c, vox=vox, weights=hip.dev(c["w"])).cpu().numpy()
    plan = vox.last_plan()
    assert plan["nchunk"] == 3 and plan["ncc"] == 2 and plan["ct"] == 32, plan
    assert_exact(got, uncut)
    assert_exact(uncut, _repeated_sum(c, weights=hip.dev(c["w"])).cpu().numpy())


# ---- 10. host arrays, grid types ---------------------------------------------------------------------------------------------
def test_host_arrays_are_accepted_and_the_grid_is_contiguous_float32_whatever_the_voxelizer_writes():
    import torch

    c = _case("features-C5-scalar")
    got = c["vox"].forward_views_sum(c["xyz"], c["cen"], c["chan"], c["radii"], weights=c["w"])
    assert got.is_cuda and got.dtype == torch.float32
    assert_exact(got.cpu().numpy(), _views_sum(c, weights=hip.dev(c["w"])).cpu().numpy())
    host = c["vox"].forward_posed_views_sum(c["xyz"], c["cen"], c["q"], c["t"], c["chan"], c["radii"])
    dev = c["vox"].forward_posed_views_sum(hip.dev(c["xyz"]), hip.dev(c["cen"]), hip.dev(c["q"]), hip.dev(c["t"]), hip.dev(c["chan"]), hip.dev(c["radii"]))
    assert_exact(host.cpu().numpy(), dev.cpu().numpy())
    other = _vox("scalar", "gaussian", grid_dtype="bfloat16", grid_layout="channels_last")
    got = _views_sum(c, vox=other)
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (5, D, D, D)
    assert_exact(got.cpu().numpy(), _plain("features-C5-scalar"))
    for bad in (torch.empty((5, D, D, D)), torch.empty((5, D, D, D), dtype=torch.bfloat16, device="cuda"),
                torch.empty((5, D, D, 2 * D), device="cuda")[..., ::2]):
        with pytest.raises(ValueError, match="contiguous float32 tensor on this voxelizer's device"):
            _views_sum(c, out_grid=bad)


def test_the_library_names_what_it_does_not_serve_in_forward_sums_order():
    """The rules of mvx_forward_views_sum that read the handle, through the C ABI: each call breaks two of them and the earlier
    one is reported - precision 64, channel-wise radii with features, D % 4, per-lane ranges, the alignment of out."""
    import molvoxel_amd as mv
    import torch

    def call(vox, C_=4, rt=0, radii=None, aligned=True):
        xyz = torch.zeros((3, 3), dtype=torch.float64, device="cuda")
        feat = torch.ones((3, C_), device="cuda")
        n = C_ * vox.dimension ** 3
        out = torch.empty(n + 4, device="cuda")[0 if aligned else 1:]
        import ctypes as C

        from molvoxel_amd.voxelizer.hip import _lib

        xf = (_lib.MvxXform * 1)()
        rc = vox._lib.mvx_forward_views_sum(vox._handle, 0, xyz.data_ptr(), feat.data_ptr(), None if radii is None else radii.data_ptr(),
                                            1.0, rt, 3, C_, C.addressof(xf), 1, None, out.data_ptr(), 0, None)
        return rc, last_error()

    mk = lambda D_, rt="scalar", **kw: mv.create_voxelizer(0.5, D_, rt, "gaussian", library="hip", **kw)  # noqa: E731
    ones = torch.ones(4, device="cuda")
    for vox, kw, want in [
        (mk(16, "channel-wise", precision=64), dict(rt=2, radii=ones.double()), "forward_sum: precision 64 is not supported (float32 sums only)"),
        (mk(18, "channel-wise"), dict(rt=2, radii=ones), "forward_sum: channel-wise radii with features are not supported (the grouped launch)"),
        (mk(18, blockdim=4), {}, "forward_sum: a dimension that is no multiple of 4 is not supported (run-wise write-out)"),
        (mk(24, blockdim=12), dict(aligned=False), "forward_sum: a blockdim that needs per-lane ranges is not supported"),
        (mk(16), dict(aligned=False), "out must be 16-byte aligned"),
    ]:
        rc, msg = call(vox, **kw)
        assert rc == MVX_ERR_INVALID and msg == want, (rc, msg, want)
    rc, msg = call(mk(16))
    assert rc == 0, msg
    torch.cuda.synchronize()


# ---- 11. memory --------------------------------------------------------------------------------------------------------------
def test_sixty_four_views_allocate_less_than_their_grids():
    """64 views at D = 24, C = 32: the grids forward_views would write take 64 x 32 x 24^3 x 4 bytes = 113 MB; the summed call
    allocates ONE grid - a condition on what the call allocates, after a warm call."""
    import torch

    D_, C_, nv = 24, 32, 64
    xyz, chan, _ = V.cloud(21, N, "features", C_, "scalar")
    cen = V.centers(21, nv, xyz)
    vox = _vox("scalar", "gaussian", D_)
    a = (hip.dev(xyz), hip.dev(cen), hip.dev(chan), 1.5)
    vox.forward_views_sum(*a)  # (warm: the library's workspace and torch's pools)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    got = vox.forward_views_sum(*a)
    torch.cuda.synchronize()
    used = torch.cuda.max_memory_allocated() - base
    grids = nv * C_ * D_ ** 3 * 4
    assert float(got.abs().sum()) > 0 and used < grids, (used, grids)
