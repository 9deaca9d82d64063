"""Host half of tests/test_hip_batch_cuts.py: no GPU, nothing is launched.

* every row of tests/batch_cut_rows.py really is the kernel family it names (mvx_plan_call), and its forced cuts really cut;
* the Python restatement of the plan's molecule-chunk rule agrees with the library;
* the division trick of the kernels' decode (n / d == __umulhi(n, ceil(2^32 / d))) is exact for every divisor the plan can
  produce at the largest dividend each launch can pass.
"""
import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import batch_cut_rows as R


@pytest.mark.parametrize("row", R.ROWS, ids=R.ROW_IDS)
def test_row_is_the_family_it_names(row):
    batch = R.make_batch(row)
    sizes = batch["sizes"]
    p = R.host_plan(row, sizes)
    got = {k: p[k] for k in row.plan}
    assert got == row.plan, (row.id, p)
    if row.narrow >= 0:
        assert R.narrow_sub_tiles(p, row.narrow_sub, row.cl) == row.narrow, (row.id, p)
    B, total = len(sizes), int(sum(sizes))
    # uncut at the production budget, and the knobs of the GPU test cut it as it says
    assert p["nchunk"] == 1 and R.expected_nchunk(p, B, row.C, total, row.precision) == 1
    if row.precision == 32:
        assert R.expected_nchunk(p, B, row.C, total, 32, budget_kb=1) == B  # one molecule per chunk, empty ones included
        k = R.expected_nchunk(p, B, row.C, total, 32, budget_kb=R.budget_for(p, B, row.C, total, 3 if B >= 6 else 2))
        assert 2 <= k <= 3 and k < B
    for chunks in row.chunks:
        assert B >= 4 * chunks and R.expected_nchunk(p, B, row.C, total, row.precision, chunks=chunks) == chunks
    if row.precision == 64:
        assert row.chunks, "the Infinity Cache budget does not cut float64 calls: the row needs the chunks option"
    # the batch has what the families need: empty molecules first, last and in the middle, one of every size class
    if row.batch == "ragged":
        assert sizes[0] == 0 and sizes[-1] == 0 and 0 in sizes[1:-1] and set(sizes) == {0, 1, 5, 45, 300, 1200, 2200}
    assert (row.n_radii == 0) or len(set(batch["r_chan"].tolist())) == row.n_radii


def test_every_kernel_family_has_rows():
    fam = {}
    for r in R.ROWS:
        fam.setdefault(r.id.split("-")[0], []).append(r)
    assert set(fam) == {"rem", "full", "grouped", "narrow", "pair", "runs", "vec", "lanes", "types", "bf16", "cl", "f64", "xform"}
    for name, rows in fam.items():  # device-resident and host inputs each appear at least once per family group
        assert {r.device for r in rows} == {True, False}, name
    for name in ("rem", "grouped", "cl", "f64"):  # the side stream's per-chunk events / float64's "all pre-passes, one launch"
        assert any(r.chunks for r in fam[name]), name
    assert {r.precision for r in fam["f64"]} == {64} and {R.F64_DENSE, R.F64_MX} == {r.plan["route"] for r in fam["f64"]}


@pytest.mark.parametrize("case", R.BIG, ids=R.BIG_IDS)
def test_big_case_crosses_the_grid_limit(case):
    p = R.big_host_plan(case)
    assert {k: p[k] for k in case.plan} == case.plan, (case.id, p)
    assert R.big_output_bytes(case) < R.MAX_OUTPUT_BYTES
    if case.narrow >= 0:
        assert R.narrow_sub_tiles(p, 0, case.cl) == case.narrow, (case.id, p)
    per = R.GRID_Y_MAX // p["ncc"]
    sizes = R.big_sizes(case)
    assert p["nchunk"] == R.expected_nchunk(p, case.B, case.C, int(sizes.sum()), case.precision)
    cuts = R.big_cut_points(case, p)
    if case.id.endswith(("-65535", "-32767")):  # the largest batch that still is one launch for the gridDim.y limit
        assert case.B * p["ncc"] <= R.GRID_Y_MAX < (case.B + 1) * p["ncc"]
    else:
        assert case.B > per and p["nchunk"] >= 2 and cuts
    assert all(0 < c < case.B for c in cuts)


def test_the_narrow_kernel_crosses_the_grid_limit():
    """voxelize_narrow_kernel decodes blockIdx.y and b0 as every slab kernel does (mvx_slab_body.inc) but is the one whose workgroups
    have fewer waves than the slab has sub-tiles: at least two of the big cases must reach it beyond 65 535 molecules, and the
    one-sub-tile rows must not claim to."""
    narrow = [c for c in R.BIG if c.narrow > 0]
    assert len(narrow) >= 2 and all(c.B > R.GRID_Y_MAX and R.big_host_plan(c)["nchunk"] >= 2 for c in narrow)
    assert all(c.narrow == 0 for c in R.BIG if c.D == 8)


def test_chunk_rule_restated_matches_the_library():
    rng = np.random.default_rng(5)
    for _ in range(400):
        D = int(rng.choice([4, 8, 16, 31, 32, 50, 64, 96, 130]))
        C_ = int(rng.choice([1, 4, 8, 16, 32, 33, 40, 64, 65, 72, 200]))
        B = int(rng.choice([1, 16, 300, 512, 513, 4000, 21846, 32768, 65535, 65536, 100000]))
        atoms = int(rng.choice([0, 3, 50, 4000]))
        if B * atoms >= 1 << 31:
            continue
        for precision in (32, 64):
            for radii in ("scalar", "channel-wise"):
                p = _lib.plan_call(D, C_, B, total_atoms=B * atoms, max_atoms=atoms, precision=precision, radii_type=radii)
                assert p["nchunk"] == R.expected_nchunk(p, B, C_, B * atoms, precision), (D, C_, B, atoms, precision, radii, p)
    # tests/test_plan.py's rows
    p = _lib.plan_call(64, 32, 513, total_atoms=513 * 4000, max_atoms=4000)
    assert p["nchunk"] == R.expected_nchunk(p, 513, 32, 513 * 4000) == 2


MAX_SLABS = 0x7FFFFFFF - 1  # run(): "batch too large for one call" beyond this many (slab, chunk) pairs


def _exact(n, d):
    return n // d == R.umulhi(n, R.umulhi_inverse(d))


def test_division_by_multiplication_is_exact_where_the_launches_use_it():
    """ceil(2^32 / d) as a multiplier is exact while n * (d * inv - 2^32) < 2^32, which n * d < 2^32 guarantees. The kernels rely on
    it for: blockIdx.y / ncc (n <= 65 535), t / nsx, t / nzc and (t / nzc) / nsy for slab ids t < nslab (mvx_slab_body.inc, the narrow
    kernel, decode_slab), and blockIdx.x / nsx in xbin_kernel, whose grid has (molecules of the chunk) * nsx blocks - the one
    dividend that grows with the batch. Checked for every slab divisor (nsx, nsy, nzc) the plan produces over D <= 1020, contiguous and
    channels-last, and for every channel-chunk count ncc / nfull of C <= 4096 (2 ... 128, grouped launches included), at n = 0,
    d - 1, d and the largest n of each launch; d == 1 is special-cased by the kernels (no multiply)."""
    for C_ in range(1, 4097):  # what divides blockIdx.y: ncc (nfull in a call with a remainder launch), at most 65 535 pairs per launch
        for radii in ("scalar", "channel-wise"):
            p = _lib.plan_call(32, C_, 1, total_atoms=100, radii_type=radii)
            assert 1 <= p["nfull"] <= p["ncc"] <= 128
    for d in range(2, 129):
        for n in {0, d - 1, d, R.GRID_Y_MAX, R.GRID_Y_MAX - (R.GRID_Y_MAX % d) - 1, R.GRID_Y_MAX - (R.GRID_Y_MAX % d)}:
            assert _exact(n, d), (d, n)
    seen = set()
    for D in range(1, 1021):
        for C_, mode, layout in ((1, "single", 0), (4, "types", 0), (16, "features", 0), (32, "features", 0), (33, "features", 0),
                                 (4096, "features", 0), (32, "features", 1), (4096, "features", 1)):
            for aligned in (True, False):
                p = _lib.plan_call(D, C_, 1, total_atoms=100, mode=mode, out_aligned16=aligned,
                                   layout=_lib.MVX_LAYOUT_NDHWC if layout else _lib.MVX_LAYOUT_NCDHW)
                key = (p["nsx"], p["nsy"], p["nzc"], p["ncc"], p["nfull"])
                if key in seen:
                    continue
                seen.add(key)
                nsx, nsy, nzc, ncc = p["nsx"], p["nsy"], p["nzc"], p["ncc"]
                nslab = nsx * nsy * nzc
                # molecules one launch can hold: the gridDim.y limit and run()'s bound on slabs per call
                nb = min(R.GRID_Y_MAX // ncc, MAX_SLABS // (nslab * ncc))
                assert nb >= 1
                checks = [(ncc, R.GRID_Y_MAX), (p["nfull"], R.GRID_Y_MAX), (nsx, nslab - 1), (nzc, nslab - 1), (nsy, (nslab - 1) // nzc),
                          (nsx, nb * nsx - 1)]
                for d, nmax in checks:
                    if d == 1:
                        continue
                    for n in {0, d - 1, d, nmax, nmax - (nmax % d) - 1 if nmax >= d else 0, nmax - (nmax % d)}:
                        assert _exact(n, d), (D, C_, p, d, n)
                # ... and the sufficient condition itself at the xbin launch, the largest dividend there is
                assert (nb * nsx - 1) * (R.umulhi_inverse(nsx) * nsx - (1 << 32) if nsx > 1 else 0) < 1 << 32
    assert len(seen) > 500
    # the trick does break beyond its range (so the test can fail): 510 slabs per row at 40 million blocks
    assert not all(_exact(n, 510) for n in range(40_000_000 - 510, 40_000_000))
