"""What the draws of tests/entry_fuzz_rows.py reach, shown with numpy and the CPU references alone (no GPU): every value of every
axis and the cross cells that matter occur, the references put something on every draw, the planted ties are ties under the drawn
pose, and draw(seed) is a function of the seed. tests/test_hip_entry_fuzz.py therefore needs no skip."""
import functools

import numpy as np

from tests import entry_fuzz_rows as E
from tests import grad_reference as gr
from tests import score_reference as sr
from tests.sum_sweep_rows import SERVED, SWEEP_C

WALK = [E.walk_draw(s) for s in range(E.N_WALK)]
SUMMED = [E.summed_draw(s) for s in range(E.N_SUMMED)]


def _values(draws, key):
    return {d[key] for d in draws}


def _divides(d):
    return d["D"] % (8 if d["blockdim"] is None else d["blockdim"]) == 0


# ---- 1. the axes ---------------------------------------------------------------------------------------------------------------
def test_the_counts_and_the_generators_offsets():
    assert (E.N_WALK, E.N_SUMMED) == (96, 48) and len(WALK) == 96 and len(SUMMED) == 48
    assert [d["seed"] for d in WALK] == list(range(96)) and [d["seed"] for d in SUMMED] == list(range(48))


def test_every_value_of_every_walk_axis_occurs():
    assert _values(WALK, "D") == set(E.WALK_D) and max(E.WALK_D) == 48 and 5 in E.WALK_D
    assert _values(WALK, "res") == set(E.RESOLUTIONS) == {0.3, 0.4, 0.5, 0.75, 1.0}
    assert _values(WALK, "sigma") == set(E.SIGMAS) == {0.3, 0.5, 1.0}
    bds = {"D" if (d["blockdim"] == d["D"] and d["D"] not in (4, 5, 7, 8, 12, 16)) else d["blockdim"] for d in WALK}
    assert bds >= {None, 4, 5, 7, 8, 12, 16, "D"}, bds
    assert _values(WALK, "density") == {"gaussian", "binary"}
    pairs = {(d["mode"], d["radii_type"]) for d in WALK}
    assert pairs == {(m, r) for m in ("features", "types", "single") for r in ("scalar", "atom-wise", "channel-wise")} - {("single", "channel-wise")}
    assert _values(WALK, "C") == set(E.WALK_C) == {1, 2, 5, 8, 31, 32, 33, 40, 65}
    assert _values(WALK, "kind") == {"f32", "bf16", "f64"} and _values(WALK, "per_mol") == {False, True}
    assert _values(WALK, "posed") == {False, True} and _values(WALK, "B") == {1, 2, 3, 4, 5}
    assert {n for d in WALK for n in d["sizes"]} == set(E.WALK_SIZES) == {0, 1, 2, 33, 64, 65, 150, 300}
    for d in WALK:
        assert d["B"] * d["C"] * d["D"] ** 3 <= E.WALK_ELEMENTS and len(d["sizes"]) == d["B"] and d["N"] == sum(d["sizes"])
        assert all(len(s) <= E.SAMPLE and set(p) <= set(s) for s, p in zip(d["sample"], d["planted"]))
        for b in range(d["B"]):  # centres away from the origin (but the float64 tie molecules at resolution 0.3 / 0.4)
            at_origin = b in d["tie_mols"] and d["precision"] == 64 and not E.dyadic(d["res"])
            assert (not d["cen"][b].any()) if at_origin else float(np.abs(d["cen"][b]).min()) >= 10.0, (d["seed"], b)


def test_empty_molecules_fall_first_last_and_in_the_middle_in_a_fixed_share_of_the_walk_draws():
    for d in WALK:
        want = ("first", "last", "middle", "drawn")[d["seed"] % 4]
        assert d["empty"] == want
        if want == "first":
            assert d["sizes"][0] == 0 and d["B"] >= 2
        elif want == "last":
            assert d["sizes"][-1] == 0 and d["B"] >= 2
        elif want == "middle":
            assert d["sizes"][d["B"] // 2] == 0 and 0 < d["B"] // 2 < d["B"] - 1
    assert sum(d["empty"] != "drawn" for d in WALK) == 72


def test_layout_atoms_on_nodes_one_past_a_face_and_types_past_the_channels():
    past_face = 0
    for d in WALK + SUMMED:
        half = d["res"] * (d["D"] - 1) / 2
        for b, n in enumerate(d["sizes"]):
            assert len(d["planted"][b]) == min(n, 6)
            if n > 5 and b in d["tie_mols"]:  # the sixth planted atom lies 0.1 ... 0.9 voxels past the +x face in the molecule's frame
                p = E.positions_of(d)[d["planted"][b][5]]
                assert half + 0.09 * d["res"] < p[0] < half + 0.91 * d["res"], (d["seed"], b, p, half)
                past_face += 1
        for a in d["bad_types"]:
            assert d["mode"] == "types" and d["radii_type"] != "channel-wise" and d["chan"][a] >= d["C"]
        if d["mode"] == "types":
            assert int(d["chan"].min(initial=0)) >= 0
    assert past_face > 20
    assert sum(bool(d["bad_types"]) for d in WALK) >= 5 and sum(bool(d["bad_types"]) for d in SUMMED) >= 2


def test_every_value_of_every_summed_axis_occurs():
    assert _values(SUMMED, "D") == set(E.SUMMED_D) == {8, 12, 16, 20, 24, 28, 36, 44}
    assert _values(SUMMED, "res") == set(E.RESOLUTIONS) and _values(SUMMED, "sigma") == set(E.SIGMAS)
    bds = {"D" if (d["blockdim"] == d["D"] and d["D"] not in (16, 24)) else d["blockdim"] for d in SUMMED}
    assert bds >= {None, 16, 24, "D"}, bds
    assert {(d["mode"], d["radii_type"]) for d in SUMMED} == set(SERVED)
    assert _values(SUMMED, "C") == set(SWEEP_C) and _values(SUMMED, "density") == {"gaussian", "binary"}
    assert _values(SUMMED, "B") == set(range(1, 9)) and _values(SUMMED, "posed") == {False, True}
    for d in SUMMED:
        assert d["posed"] == (d["seed"] % 3 == 0) and d["clustered"] == (d["seed"] % 4 == 0)
        assert all(0 <= n <= 120 for n in d["sizes"]) and d["N"] > 0 and d["precision"] == 32
        assert not (d["mode"] == "features" and d["radii_type"] == "channel-wise")
        assert d["chan"] is None or d["mode"] == "types" or float(d["chan"].min()) >= 0.0  # (positive terms: the one Gaussian rule)


def test_the_summed_blockdims_are_the_ones_whose_plan_has_no_lane_ranges():
    from molvoxel_amd.voxelizer.hip import _lib

    for d in SUMMED:
        bd = 8 if d["blockdim"] is None else d["blockdim"]
        assert _lib.plan_call(d["D"], 32, 2, total_atoms=10, blockdim=bd)["lane_range"] == 0, (d["seed"], d["D"], bd)
        assert E.sums_supported(d["D"], d["blockdim"])
    for D in E.SUMMED_D:  # ... and the rule of the Python layer that the walk draws' field_grad uses is that plan's
        for bd in (4, 5, 7, 8, 12, 16, 24, D):
            assert E.sums_supported(D, bd) == (_lib.plan_call(D, 32, 2, total_atoms=10, blockdim=bd)["lane_range"] == 0), (D, bd)
    assert any(d["D"] == 20 and d["blockdim"] == 24 for d in SUMMED) or len(E.summed_blockdims(20)) == 4
    assert E.summed_blockdims(44) == [None, 16, 24, 44] and E.summed_blockdims(8) == [None, 16, 24, 8]


def test_the_cross_cells_occur():
    def some(draws, cond):
        return [d["seed"] for d in draws if cond(d)]

    cells = {
        "binary x types x per-molecule field": some(WALK, lambda d: d["density"] == "binary" and d["mode"] == "types" and d["per_mol"]),
        "binary x single": some(WALK, lambda d: d["density"] == "binary" and d["mode"] == "single"),
        "features x channel-wise x C > 32": some(WALK, lambda d: d["mode"] == "features" and d["radii_type"] == "channel-wise" and d["C"] > 32),
        "f64 x posed (a molecule under a general pose)": some(WALK, lambda d: d["kind"] == "f64" and d["posed"] and any(
            n and b not in d["tie_mols"] for b, n in enumerate(d["sizes"]))),
        "bf16 x random rotation": some(WALK, lambda d: d["kind"] == "bf16" and not d["posed"] and d["N"] > 0),
        "res != 0.5 x a blockdim that does not divide D": some(WALK, lambda d: d["res"] != 0.5 and not _divides(d)),
        "field gradient": some(WALK, lambda d: d["field_grad"] and d["N"] > 0),
        "field gradient x bf16": some(WALK, lambda d: d["field_grad"] and d["kind"] == "bf16" and d["N"] > 0),
        "summed: binary x types x channel-wise": some(SUMMED, lambda d: d["density"] == "binary" and d["mode"] == "types"
                                                      and d["radii_type"] == "channel-wise"),
        "summed: C = 33 or 40 with res != 0.5": some(SUMMED, lambda d: d["C"] in (33, 40) and d["res"] != 0.5),
        "summed: posed x gaussian": some(SUMMED, lambda d: d["posed"] and d["density"] == "gaussian"),
    }
    print({k: v[:6] for k, v in cells.items()})
    for k, v in cells.items():
        assert v, k


def test_general_poses_take_every_norm_and_tie_molecules_the_identity():
    norms = set()
    for d in WALK + SUMMED:
        if not d["posed"]:
            continue
        for b in range(d["B"]):
            if b in d["tie_mols"]:
                assert d["q"][b].tolist() == [1.0, 0.0, 0.0, 0.0]
                k = d["t"][b] / d["res"]
                assert np.array_equal(k, np.round(k)) and np.abs(d["t"][b]).max() <= 0.6
            else:
                norms.add(round(float(np.linalg.norm(d["q"][b])), 6))
                assert np.abs(d["t"][b]).max() <= 0.6
        assert set(d["tie_mols"]) == {b for b in range(d["B"]) if (b + d["seed"]) % 2 == 0}
    assert norms == {1.0, 0.8, 1.25}


# ---- 2. the references put something on every draw ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sampled_scores(seed):
    """score_reference.score_reference restricted to the sampled atoms of a walk draw: {molecule: (s, bound)}."""
    d = E.walk_draw(seed)
    p, F = E.positions_of(d), E.field_of(d)
    w, types = E.reference_channels(d)
    out = {}
    for b in range(d["B"]):
        lo, hi, radii = E.molecule(d, b)
        if hi == lo:
            continue
        rows = [a - lo for a in d["sample"][b]]
        W = sr.weights(hi - lo, d["C"], d["mode"], None if w is None else w[lo:hi], None if types is None else types[lo:hi])
        rt = d["radii_type"]
        if d["mode"] != "features" and rt == "channel-wise":
            radii, rt = d["r_atom"][lo:hi].astype(np.float32 if d["precision"] == 32 else np.float64), "atom-wise"
        o = gr.reference(p[lo:hi], F if F.ndim == 4 else F[b], radii, rt, w=W, mode="features", res=d["res"], sigma=d["sigma"],
                         blockdim=d["blockdim"], density=d["density"], precision=d["precision"], atoms=rows)
        gw, bw = o["features"]
        out[b] = ((W[rows] * gw).sum(1), (np.abs(W[rows]) * bw).sum(1))
    return out


def test_the_score_reference_puts_something_on_every_walk_draw():
    busy = 0
    with_atoms = [d for d in WALK if d["N"] > 0]
    for d in with_atoms:
        ref = _sampled_scores(d["seed"])
        assert any(float(b.sum()) > 0 for _, b in ref.values()), d["seed"]  # a molecule whose score bound is positive
        s = np.concatenate([v[0] for v in ref.values()])
        busy += np.count_nonzero(s) > 0.3 * s.shape[0]
    print(f"{busy} of {len(with_atoms)} walk draws have a non-zero reference score on more than 30 % of their sampled atoms")
    assert len(with_atoms) >= 90 and busy >= 0.9 * len(with_atoms)


def test_every_summed_draw_has_a_positive_second_moment():
    for d in SUMMED:
        p = E.positions_of(d)
        m1 = [float((E.oracle_grid(d, p, b).astype(np.float64) ** 2).sum(axis=(1, 2, 3)).max()) for b in range(d["B"])]
        assert max(m1) > 0, d["seed"]
        assert sum(m > 0 for m in m1) >= 0.5 * sum(n > 0 for n in d["sizes"]), (d["seed"], m1)


# ---- 3. ties --------------------------------------------------------------------------------------------------------------------
def test_the_planted_ties_are_ties_under_the_drawn_pose():
    """For every claimed atom the reference's compare dr <= 1 holds with equality on a voxel it admits, at the positions
    pose_reference gives under the drawn pose, in the draw's own precision."""
    count = {}
    for d in WALK + SUMMED:
        if not d["ties"]:
            continue
        p = E.positions_of(d)
        for a in d["ties"]:
            assert E.tie_count(d, a, p[a]) >= 1, (d["seed"], "transform" in d, a, p[a].tolist())
        key = ("walk" if "transform" in d else "summed", d["kind"], d["radii_type"], E.dyadic(d["res"]))
        count[key] = count.get(key, 0) + len(d["ties"])
    print(count)
    for kind in ("f32", "bf16", "f64"):
        for dy in (False, True):  # (f64 at resolution 0.3 / 0.4 included: the tie molecules centred on the origin)
            assert sum(v for k, v in count.items() if k[0] == "walk" and k[1] == kind and k[3] == dy) >= 5, (kind, dy, count)
    for rt in ("scalar", "atom-wise", "channel-wise"):
        assert sum(v for k, v in count.items() if k[2] == rt) >= 5, (rt, count)
    assert sum(v for k, v in count.items() if k[0] == "summed") >= 100
    # posed draws: the claimed atoms belong to tie molecules only, and a random rotation claims none
    for d in WALK:
        if not d["posed"]:
            assert not d["ties"] and not d["tie_mols"]


# ---- 4. determinism ------------------------------------------------------------------------------------------------------------
def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), k
        else:
            assert x == y, k


def test_a_draw_is_a_function_of_its_seed():
    for s in (0, 1, 2, 3, 17, 50, 95):
        _same(E.walk_draw.__wrapped__(s), E.walk_draw.__wrapped__(s))
        _same(E.walk_draw.__wrapped__(s), E.walk_draw(s))
    for s in (0, 1, 2, 3, 30, 47):
        _same(E.summed_draw.__wrapped__(s), E.summed_draw(s))
    assert not np.array_equal(E.walk_draw(0)["xyz"], E.walk_draw(1)["xyz"])
    # the field, target and dL/dm of a draw are seeded by the draw
    d = E.walk_draw(5)
    assert np.array_equal(E.field_of(d), E.field_of(d)) and E.field_of(d).shape[-4:] == (d["C"],) + (d["D"],) * 3
    s = E.summed_draw(5)
    assert E.target_of(s).dtype == np.float32 and (E.target_of(s) > 0).any() and (E.target_of(s) < 0).any()
    assert E.dm_of(s, 3).shape == (s["B"], s["C"], 3) and (E.dm_of(s, 3) > 0).any() and (E.dm_of(s, 3) < 0).any()


def test_bfloat16_fields_are_rounded_to_nearest_even_on_the_host():
    d = next(d for d in WALK if d["kind"] == "bf16")
    F = E.field_of(d)
    raw = np.random.default_rng(d["fseed"]).standard_normal(F.shape).astype(np.float32)
    assert np.array_equal(F, F.astype(np.float32)) and not (F.astype(np.float32).view(np.uint32) & 0xFFFF).any()
    assert np.all(np.abs(F - raw) <= 2.0 ** -8 * np.abs(raw)) and (F != raw).any()  # (half of one bfloat16 ulp)


def test_the_gradient_fuzz_draws_come_from_the_generators_this_module_calls():
    """_geometry and _radii stay where they were (tests/test_hip_grad_fuzz.py); a few of its draws, pinned by a checksum of their
    coordinates and radii taken before this module existed."""
    from tests import test_hip_grad_fuzz as GF

    assert E._geometry is GF._geometry and E._radii is GF._radii
    sums = [round(float(np.sum(GF._draw(s)["xyz"]) + np.sum(GF._draw(s)["radii"])), 6) for s in (0, 1, 7, 100)]
    assert sums == GRAD_FUZZ_CHECKSUMS, sums


GRAD_FUZZ_CHECKSUMS = [292.778496, 1.67148, 175.373341, 6.163678]
