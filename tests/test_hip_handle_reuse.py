"""One handle through every family of entries, back to back on one stream: forward from host and from device arrays with
centres (records travel: offsets and records are uploaded every time), the same batch without centres or transforms from device
tensors and from numpy, each twice (no records: the second call of a kind finds the offsets of the call before on the device and
skips their upload; from numpy it then takes a slot for the arrays alone), a posed forward with backward, views, scores of views
with backward, scores of a batch, the reduction of views, a transform, then the calls without records again (the first re-uploads
- the views' forward left records behind - the next two skip), and the first call again. The entries stage offsets, records
and host arrays through the same ring of pinned slots and keep device copies of them in buffers of their own; a call that
wrote another entry's buffer (the forward's cached offsets above all), or reused a slot a copy still reads, would change some
later result. Every result and gradient must equal, bit for bit, the same call made on a fresh voxelizer of its own.
On the float32 handle the entries on the summed walk run in between: forward_sum (plain; accumulating with atom weights; in two
parts under set_sum_parts(2)), forward_views_sum with view weights and moments_batch with a target - they take the forward's
workspace, its cached offsets and the views' buffers, and own the partial grids and the moments' partials.

D = 16 at 0.5 A, three molecules of 40 / 0 / 25 atoms with C = 4 features (C = 5 on the summed walk: one chunk of 32 channels,
zero padded), five views of the 150-atom cloud of tests/test_hip_score_views.py."""
import ctypes as C

import numpy as np
import pytest

from tests.test_hip_score_views import _data

pytestmark = pytest.mark.gpu

D, RES, C_ = 16, 0.5, 4
C_SUM = 5
SIZES = (40, 0, 25)


def _vox(kind):
    import molvoxel_amd as mv

    return mv.create_voxelizer(RES, D, "scalar", "gaussian", library="hip", precision=64 if kind == "f64" else 32, differentiable=True)


def _inputs(kind):
    rng = np.random.default_rng(11)
    fp = np.float64 if kind == "f64" else np.float32
    offsets = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, B = int(offsets[-1]), len(SIZES)
    half = RES * (D - 1) / 2
    cen = rng.uniform(-5.0, 5.0, (B, 3))
    xyz = np.repeat(cen, SIZES, axis=0) + rng.uniform(-0.8 * half, 0.8 * half, (N, 3))
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1)[:, None]
    cloud = _data(5, 150, 5, C_, "features", "scalar", kind)
    a = dict(offsets=offsets, xyz=xyz, cen=cen, feat=rng.standard_normal((N, C_)).astype(fp), q=q, t=rng.uniform(-0.3, 0.3, (B, 3)),
             field=rng.standard_normal((C_, D, D, D)).astype(fp), cloud=cloud, rows=rng.standard_normal((150, 3)), kind=kind)
    # the summed and moments entries (float32 only): C_SUM channels are one chunk of 32, zero padded
    a.update(feat5=rng.standard_normal((N, C_SUM)).astype(np.float32), cloud5=rng.standard_normal((150, C_SUM)).astype(np.float32),
             w_atoms=rng.uniform(0.5, 1.5, N).astype(np.float32), w_views=rng.uniform(0.5, 1.5, 5).astype(np.float32),
             grid5=rng.standard_normal((C_SUM, D, D, D)).astype(np.float32))
    return a


def _steps(a):
    """The sequence as functions of a voxelizer; each returns the tensors to compare (results first, then gradients)."""
    import torch

    from molvoxel_amd.voxelizer.hip import _lib

    def dev(x, grad=False):
        return torch.tensor(x, device="cuda", requires_grad=grad)

    off, cl = a["offsets"], a["cloud"]
    xyz, cen, feat = dev(a["xyz"]), dev(a["cen"]), dev(a["feat"])
    xyz0_host = a["xyz"] - np.repeat(a["cen"], SIZES, axis=0)  # already centred: a call without records
    xyz0 = dev(xyz0_host)
    F = dev(a["field"])

    def from_host(v):
        return (v.forward_batch(a["xyz"], off, a["cen"], a["feat"], 1.25),)

    def from_device(v):
        return (v.forward_batch(xyz, off, cen, feat, 1.25),)

    def plain_device(v):
        return (v.forward_batch(xyz0, off, None, feat, 1.25),)

    def plain_host(v):
        return (v.forward_batch(xyz0_host, off, None, a["feat"], 1.25),)

    def posed(v):
        x, f, q, t = dev(a["xyz"], True), dev(a["feat"], True), dev(a["q"], True), dev(a["t"], True)
        g = v.forward_posed_batch(x, off, cen, q, t, f, 1.25)
        (g * F).sum().backward()
        return g.detach(), x.grad, f.grad, q.grad, t.grad

    def views(v):
        return (v.forward_views(dev(cl["xyz"]), dev(cl["cen"]), dev(cl["chan"]), 1.25),)

    def score_views(v):
        x, f, c = dev(cl["xyz"], True), dev(cl["chan"], True), dev(cl["cen"], True)
        scores, atoms, index, offsets = v.score_views(x, c, f, 1.25, F, per_atom=True)
        (scores.sum() + (atoms * atoms).sum()).backward()
        return scores.detach(), atoms.detach(), index, torch.as_tensor(offsets), x.grad, f.grad, c.grad

    def score_batch(v):
        return v.score_batch(xyz, off, cen, feat, 1.25, F, per_atom=True)

    def reduce(v):
        index, offsets = v.select_views(dev(cl["xyz"]), dev(cl["cen"]), None, 1.25)
        rows = dev(a["rows"])[index]
        return (v.views_reduce(rows, index, offsets, 150),)

    def transform(v):
        xf = _lib.MvxXform()
        xf.center[:] = a["cen"][0].tolist()
        xf.quat[:] = a["q"][0].tolist()
        xf.trans[:] = a["t"][0].astype(np.float32).tolist()
        xf.flags = _lib.MVX_XF_CENTER | _lib.MVX_XF_RECENTER | _lib.MVX_XF_ROTATE | _lib.MVX_XF_TRANSLATE
        out = torch.empty_like(xyz)
        _lib.check(_lib.load().mvx_transform_coords(v._handle, xyz.data_ptr(), xyz.shape[0], C.addressof(xf), out.data_ptr(),
                                                    _lib.MVX_DEVICE, _lib.MVX_DEVICE, torch.cuda.current_stream().cuda_stream))
        return (out,)

    steps = [("forward_batch from numpy, centres", from_host), ("forward_batch from device tensors, centres", from_device),
             ("device tensors, centres, again", from_device),
             ("no records, device tensors (offsets uploaded)", plain_device),
             ("no records, device tensors again (skipped upload)", plain_device),
             ("no records, numpy (skipped upload, a slot for the arrays alone)", plain_host), ("no records, numpy again", plain_host),
             ("forward_posed_batch + backward", posed), ("forward_views", views),
             ("score_views per_atom + backward", score_views), ("score_batch", score_batch), ("views_reduce", reduce),
             ("transform on the handle", transform),
             ("no records, device tensors, after the other entries (offsets uploaded)", plain_device),
             ("no records, device tensors, after the other entries, again (skipped upload)", plain_device),
             ("no records, numpy, after the other entries (skipped upload)", plain_host),
             ("forward_batch from numpy, centres, again", from_host)]
    if a["kind"] == "f64":  # (the summed and moments entries serve float32 handles only)
        return steps

    # ---- the entries on the summed walk, in between the steps above: they use the forward's workspace, offsets cache and slots ----
    feat5, cloud5, grid5 = dev(a["feat5"]), dev(a["cloud5"]), dev(a["grid5"])
    w_atoms, w_views = dev(a["w_atoms"]), dev(a["w_views"])

    def fsum(v):
        return (v.forward_sum(xyz, off, cen, feat5, 1.25),)

    def fsum_accumulate(v):
        return (v.forward_sum(xyz, off, cen, feat5, 1.25, weights=w_atoms, out_grid=grid5.clone(), accumulate=True),)

    def fsum_parts(v):
        v.set_sum_parts(2)
        out = v.forward_sum(xyz, off, cen, feat5, 1.25)
        v.set_sum_parts(1)
        return (out,)

    def views_sum(v):
        return (v.forward_views_sum(dev(cl["xyz"]), dev(cl["cen"]), cloud5, 1.25, weights=w_views),)

    def moments(v):
        return (v.moments_batch(xyz, off, cen, feat5, 1.25, target=grid5),)

    for after, name, step in [("device tensors, centres, again", "forward_sum", fsum),
                              ("no records, numpy again", "forward_sum, accumulate with weights", fsum_accumulate),
                              ("forward_views", "forward_views_sum with weights", views_sum),
                              ("score_batch", "moments_batch with a target", moments),
                              ("transform on the handle", "forward_sum in two parts", fsum_parts)]:  # (never inside a skipped-upload pair)
        steps.insert([n for n, _ in steps].index(after) + 1, (name, step))
    return steps


def _host(x):
    return x if isinstance(x, np.ndarray) else x.detach().cpu().numpy()


@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_one_handle_through_every_entry_gives_the_bits_of_fresh_handles(kind):
    import torch

    a = _inputs(kind)
    steps = _steps(a)
    shared = _vox(kind)
    got = [[x for x in step(shared)] for _, step in steps]  # back to back: nothing is read before the last call is enqueued
    torch.cuda.synchronize()
    for (name, step), mine in zip(steps, got):
        fresh = [x for x in step(_vox(kind))]
        assert len(fresh) == len(mine), name
        for i, (x, y) in enumerate(zip(mine, fresh)):
            assert x is not None and y is not None, (name, i)
            x, y = _host(x), _host(y)
            assert x.shape == y.shape and x.dtype == y.dtype, (name, i, x.shape, y.shape)
            assert np.array_equal(x, y, equal_nan=True), (name, i, float(np.abs(x.astype(np.float64) - y.astype(np.float64)).max()))
    by_name = {name: mine for (name, _), mine in zip(steps, got)}
    assert len(by_name) == len(steps)
    summed = ("forward_sum", "forward_sum, accumulate with weights", "forward_views_sum with weights", "moments_batch with a target",
              "forward_sum in two parts")
    assert all((name in by_name) == (kind == "f32") for name in summed)
    for name in ("forward_batch from numpy, centres", "no records, device tensors again (skipped upload)",
                 "no records, numpy, after the other entries (skipped upload)", "score_views per_atom + backward") + summed * (kind == "f32"):
        assert np.abs(_host(by_name[name][0])).max() > 0, name  # (the grids, the scores and the moments are not all zero)
    if kind == "f32":  # the accumulated sum started from its grid, and the two parts are a sum of their own
        assert not np.array_equal(_host(by_name["forward_sum, accumulate with weights"][0]), _host(by_name["forward_sum"][0]))
