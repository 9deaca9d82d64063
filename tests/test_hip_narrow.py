"""voxelize_narrow_kernel (mvx_slab.hip: chunks of 1 ... 8 channels, two or four z sub-tiles per wave) beyond the one-round case.

The narrow kernel serves forward_single, forward_types with a few channels and every 32 k + r remainder launch. It runs through
mvx_slab_body.inc like every other batched kernel, with Ops::NSUB accumulator sets per wave: the staging's trips (stage_round_v),
the row filter's turns (filter_walk) and the write-out's passes (write_slab, write_ndhwc_sets) depend on NSUB, and the x-list path,
the extension line and several rounds per slab are reached only by dense geometries of 2 k or 4 k sub-tiles per row
(tests/narrow_rows.py; tests/test_narrow_rows_host.py proves the line forms and the plan on the host). Per row:

* the launch reaches the narrow kernel with the expected sub-tiles per wave (last_plan() and batch_cut_rows.narrow_sub_tiles);
* bit identity across kernels: "narrow_sub" = 2, and = 4 where the row allows it, give the bits of "narrow_sub" = 1
  (voxelize_kernel's pair walk: same candidates, same order, same arithmetic per voxel);
* reference: binary grids equal the C oracle exactly, Gaussian grids pass tests/tolerance.py assert_gaussian;
* batch decode: the molecule second of three - behind one with no atom inside the box, in front of a ten-atom one - has the bits
  of the molecule alone, and the empty molecule's grid is all zeros in a buffer pre-filled with 7.0;
* channels-last: the grid of a channels-last voxelizer equals the permuted contiguous grid bit for bit.
"""
import functools

import numpy as np
import pytest

from tests import batch_cut_rows as B
from tests import narrow_rows as R
from tests.tolerance import assert_gaussian

pytestmark = pytest.mark.gpu


def _voxelizer(row, **kw):
    import molvoxel_amd as mv

    v = mv.create_voxelizer(R.RES, row.g.D, "scalar", row.cfg.density, "hip", sigma=R.SIGMA, output="torch", **kw)
    v.debug_option("direct", 0)  # the binned route, whatever the size of the call
    return v


def _forward(v, row, xyz, chan, sizes, fill=7.0):
    """One forward_batch into a grid full of stale content."""
    cfg = row.cfg
    out = v.get_empty_grid(cfg.nch, batch_size=len(sizes))
    out.fill_(fill)
    d_chan = None if chan is None else v.asarray(chan, cfg.mode)
    got = v.forward_batch(v.asarray(np.array(xyz), "coords"), np.cumsum([0] + list(sizes)).astype(np.int64), None, d_chan, row.g.radius,
                          num_channels=cfg.nch, out_grid=out)
    assert got is out
    return got


def _assert_plan(v, row, nsub, cl=False):
    """The call took the row's plan and its narrow launch `nsub` sub-tiles per wave (None: the library's rule)."""
    p = v.last_plan()
    want = {k: row.plan[k] for k in ("route", "nw", "ct", "lane_range", "grouped")} if cl else row.plan
    assert {k: p[k] for k in want} == want, (row.id, p)
    rule = (4 if row.ct == 1 and row.g.nw % 4 == 0 else 2) if cl else row.nsub  # (channels-last: four for one channel only)
    assert B.narrow_sub_tiles(R.narrow_plan(p), 0 if nsub is None else nsub, cl) == (rule if nsub is None else nsub), (row.id, p)


@functools.lru_cache(maxsize=None)
def _alone(row):
    """The row's molecule alone under the library's own rule: (grid on the host, read-only; its channels)."""
    batch = R.make_batch(row)
    v = _voxelizer(row)
    out = _forward(v, row, batch["xyz"][1], batch["chan"][1], batch["sizes"][1:2])
    _assert_plan(v, row, None)
    grid = out[0].cpu().numpy()
    grid.setflags(write=False)
    return grid


@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_sub_tiles_per_wave_give_the_bits_of_the_pair_walk(row):
    import torch

    batch = R.make_batch(row)
    xyz, chan, sizes = batch["xyz"][1], batch["chan"][1], batch["sizes"][1:2]
    v = _voxelizer(row)
    v.debug_option("narrow_sub", 1)
    one = _forward(v, row, xyz, chan, sizes).clone()
    assert B.narrow_sub_tiles(R.narrow_plan(v.last_plan()), 1, False) == 0
    assert row.nsub in row.forced
    for nsub in row.forced:
        v.debug_option("narrow_sub", nsub)
        got = _forward(v, row, xyz, chan, sizes, fill=float(nsub))
        _assert_plan(v, row, nsub)
        assert torch.equal(got.view(torch.int32), one.view(torch.int32)), (row.id, nsub)
    assert np.array_equal(_alone(row).view(np.int32), one[0].cpu().numpy().view(np.int32)), row.id


@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_row_against_the_oracle(row):
    from oracle import c_oracle

    g, cfg = row.g, row.cfg
    batch = R.make_batch(row)
    ref = c_oracle.voxelize(batch["xyz"][1], batch["chan"][1], g.radius, resolution=R.RES, dimension=g.D, radii_type="scalar",
                            density=cfg.density, sigma=R.SIGMA, num_channels=cfg.nch)
    got = _alone(row)
    assert got.shape == ref.shape and got.dtype == ref.dtype
    if cfg.exact:
        assert np.array_equal(got, ref), row.id
    else:
        assert_gaussian(got, ref)


@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_row_second_of_three_molecules(row):
    batch = R.make_batch(row)
    v = _voxelizer(row)
    out = _forward(v, row, np.concatenate(batch["xyz"]), None if batch["chan"][1] is None else np.concatenate(batch["chan"]), batch["sizes"])
    _assert_plan(v, row, None)
    out = out.cpu().numpy()
    assert not out[0].any(), "the molecule outside the box left something behind (or stale content survived)"
    assert np.array_equal(out[1].view(np.int32), _alone(row).view(np.int32)), row.id
    assert out[2].any() and not (out[2] == 7.0).any()


@pytest.mark.parametrize("row", R.CL_ROWS, ids=R.CL_IDS)
def test_channels_last_grid_is_the_permuted_contiguous_grid(row):
    import torch

    batch = R.make_batch(row)
    v = _voxelizer(row, grid_layout="channels_last")
    out = _forward(v, row, np.concatenate(batch["xyz"]), None if batch["chan"][1] is None else np.concatenate(batch["chan"]), batch["sizes"])
    _assert_plan(v, row, None, cl=True)
    assert out.shape == (3, row.cfg.nch, row.g.D, row.g.D, row.g.D)
    assert row.cfg.nch == 1 or out.is_contiguous(memory_format=torch.channels_last_3d)
    host = out.contiguous().cpu().numpy()
    assert not host[0].any()
    assert np.array_equal(host[1].view(np.int32), _alone(row).view(np.int32)), row.id
