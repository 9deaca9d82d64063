"""Torsion coordinates without a GPU: the numpy reference (tests/flex_reference.py) against central finite differences of a smooth
analytic score and its two conformer identities, the three C ABI entries (mvx_apply_torsions, mvx_score_hessian_flex_batch,
mvx_flex_lm_step; prototypes: tests/test_abi_header_host.py), every rejection and its order, what the Python layer and check_torsions
refuse before they need the library, torsion_tree on the 10GS ligand, the four kernels' resources read from mvx_flex.o, and the
conditions of the GPU refinement test on the numpy loop (tests/flex_rows.py).

Finite differences on the 12-atom tree (4 torsions, one branch, nesting depth 3), n = 10: the worst Hessian error is 1.5e-3 /
1.4e-4 / 1.5e-5 at h = 1e-3 / 3e-4 / 1e-4 with max |H| = 97 - the h^2 law, a factor of 100 from 1e-3 to 1e-4. The two conformer
identities hold to 0.02 of their bar 64 T 2^-53 L. np.linalg.solve's largest residual ratio on the n-dimensional systems of
flex_rows.lm_rows: 0.35 (largest condition number 5.5e3). The numpy refinement: 8 starts, score 591 ... 616 -> 639 ... 643, the
rigid refinement of the same starts ends at 633 ... 641."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import flex_reference as fr
from tests import flex_rows as X
from tests.abi import MVX_ERR_INVALID, P, call, records
from tests.fake_voxelizer import fake as _fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the reference against finite differences -------------------------------------------------------------------------------
def _analytic(rng, N, J=3):
    """A smooth score per atom, s_n(p) = sum_j a_nj sin(k_nj . p + phi_nj), with its gradient and Hessian."""
    al, kv, ph = rng.standard_normal((N, J)), 0.7 * rng.standard_normal((N, J, 3)), rng.uniform(0, 6, (N, J))

    def rows(p):
        a = np.einsum("njk,nk->nj", kv, p) + ph
        return ((al * np.sin(a)).sum(1), np.einsum("nj,njk->nk", al * np.cos(a), kv),
                -np.einsum("nj,njk,njl->nkl", al * np.sin(a), kv, kv))

    return rows


def test_the_reference_agrees_with_central_finite_differences_at_the_h2_rate():
    rng = np.random.default_rng(3)
    p0, axes, moves = fr.tree_coords(rng), fr.TREE_AXES, fr.tree_moves()
    rows = _analytic(rng, 12)
    piv = np.array([0.3, -0.2, 0.1])
    n = 10

    def S(x):
        return rows(fr.positions(fr.apply_torsions(p0, axes, moves, x[6:]), piv, x))[0].sum()

    _, g, H = rows(p0)
    G, _, Hx, _ = fr.flex(p0, g, H, piv, axes, moves)
    assert np.abs(Hx - Hx.T).max() <= 1e-13 * np.abs(Hx).max()
    assert np.array_equal(Hx[6:, 6:], Hx[6:, 6:].T) and np.array_equal(Hx[:6, 6:], Hx[6:, :6].T)
    # unrelated pairs: torsion 3 (the branch) against 1 and 2
    assert Hx[6 + 1, 6 + 3] == 0.0 and Hx[6 + 2, 6 + 3] == 0.0 and Hx[6 + 0, 6 + 3] != 0.0 and Hx[6 + 1, 6 + 2] != 0.0
    err = {}
    for h in (1e-3, 1e-4):
        E, S0 = np.eye(n) * h, S(np.zeros(n))
        Gf, Hf = np.zeros(n), np.zeros((n, n))
        for i in range(n):
            Gf[i] = (S(E[i]) - S(-E[i])) / (2 * h)
            Hf[i, i] = (S(E[i]) - 2 * S0 + S(-E[i])) / h ** 2
            for j in range(i + 1, n):
                Hf[i, j] = Hf[j, i] = (S(E[i] + E[j]) - S(E[i] - E[j]) - S(-E[i] + E[j]) + S(-E[i] - E[j])) / (4 * h * h)
        err[h] = (np.abs(Gf - G).max(), np.abs(Hf - Hx).max())
        print(f"FLEX_FD h {h:g}: gradient error {err[h][0]:.3g}, Hessian error {err[h][1]:.3g}, max |H| {np.abs(Hx).max():.3g}")
    assert 50.0 <= err[1e-3][1] / err[1e-4][1] <= 200.0, err
    assert 50.0 <= err[1e-3][0] / err[1e-4][0] <= 200.0, err
    assert err[1e-4][1] <= 1e-6 * np.abs(Hx).max()


def test_the_two_conformer_identities():
    rng = np.random.default_rng(4)
    p0, axes, moves = fr.tree_coords(rng), fr.TREE_AXES, fr.tree_moves()
    T = 4
    th, dl = rng.uniform(-2, 2, T), rng.uniform(-1, 1, T)
    bar = 64 * T * 2.0 ** -53 * fr.reach(p0, axes, moves)
    root_to_leaf = fr.apply_torsions(p0, axes, moves, th)
    leaf_to_root = fr.apply_torsions(p0, axes, moves, th, order=range(T - 1, -1, -1), frozen_axes=True)
    a = np.abs(root_to_leaf - leaf_to_root).max()
    b = np.abs(fr.apply_torsions(p0, axes, moves, th + dl) - fr.apply_torsions(root_to_leaf, axes, moves, dl)).max()
    print(f"FLEX_IDENTITIES order {a / bar:.3f}, sum {b / bar:.3f} of the bar {bar:.3g}")
    assert a <= bar and b <= bar
    assert np.array_equal(root_to_leaf[:3], p0[:3])  # (the root is in no set)
    assert np.array_equal(fr.apply_torsions(p0, axes, moves, np.zeros(T)), p0)


def test_inert_torsions_in_the_reference_give_exact_zeros():
    rng = np.random.default_rng(5)
    p0, moves = fr.tree_coords(rng), fr.tree_moves()
    rows = _analytic(rng, 12)
    _, g, H = rows(p0)
    want = fr.flex(p0, g, H, np.zeros(3), fr.TREE_AXES[:3], moves)
    for bad in ([-1, -1], [4, 12], [4, 4]):
        axes = np.concatenate([fr.TREE_AXES[:3], [bad]]).astype(np.int32)
        G, _, Hx, _ = fr.flex(p0, g, H, np.zeros(3), axes, moves)
        assert G[9] == 0.0 and not Hx[9].any() and not Hx[:, 9].any()
        assert np.array_equal(G[:9], want[0]) and np.array_equal(Hx[:9, :9], want[2])
        th = np.array([0.3, -0.2, 0.5, 1.0])
        assert np.array_equal(fr.apply_torsions(p0, axes, moves, th), fr.apply_torsions(p0, axes[:3], moves, th[:3]))


# ---- the entries against the header -------------------------------------------------------------------------------------------
def test_the_flex_entry_begins_like_the_hessian_entry():
    assert _lib.SIGNATURES["mvx_score_hessian_flex_batch"][1][:19] == _lib.SIGNATURES["mvx_score_hessian_batch"][1][:19]


# ---- rejections --------------------------------------------------------------------------------------------------------------
def _apply(handle=None, coords=P, offsets=(0, 3), B=1, T=2, axes=P, moves=P, angles=P, out=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_apply_torsions, handle, coords, None if off is None else off.ctypes.data, B, T, axes, moves, angles, out,
                None)


@pytest.mark.parametrize("kw, words", [
    (dict(B=-1), "B must be >= 0"), (dict(T=-1), "T must be 0 ... 32"), (dict(T=33), "T must be 0 ... 32"),
    (dict(offsets=None), "offsets must not be null"), (dict(offsets=(1, 3)), "offsets[0]"),
    (dict(B=2, offsets=(0, 3, 2)), "non-decreasing"), (dict(offsets=(0, 1 << 31)), "too many atoms"),
    (dict(coords=None), "coords / out"), (dict(out=None), "coords / out"),
    (dict(axes=None), "with T > 0"), (dict(moves=None), "with T > 0"), (dict(angles=None), "with T > 0"),
    (dict(), "null handle"), (dict(T=0, axes=None, moves=None, angles=None), "null handle"),
    (dict(offsets=(0, 0), coords=None, out=None, axes=None), "null handle"),
])
def test_apply_torsions_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _apply(**kw)
    assert rc == MVX_ERR_INVALID and words in msg, (rc, msg)


def test_apply_torsions_rules_fire_in_their_order():
    assert "B must be" in _apply(B=-1, T=40, offsets=None)[1]
    assert "T must be" in _apply(T=40, offsets=None, coords=None)[1]
    assert "offsets must not" in _apply(offsets=None, coords=None, axes=None)[1]
    assert "too many atoms" in _apply(offsets=(0, 1 << 31), coords=None, axes=None)[1]
    assert "coords / out" in _apply(coords=None, axes=None)[1]
    assert "with T > 0" in _apply(axes=None)[1]
    assert _apply(handle=P, offsets=(0, 0), coords=None, out=None)[0] == 0  # (no atoms: nothing to do)
    assert _apply(handle=P, B=0, offsets=None)[0] == 0


ONE = records([0])


def _flex(handle=None, mode=0, coords=P, channels=P, radii=None, radii_type=0, offsets=(0, 3), xforms=ONE, B=1, C_=4, field=P, stride=0,
          scores=P, twist_grad=P, twist_hess=P, T=2, axes=P, moves=P, flex_grad=P, flex_hess=P, atom_pos=None, flex=True):
    lib = _lib.load()
    off = None if offsets is None else np.asarray(offsets, np.int64)
    head = (handle, mode, coords, channels, radii, 1.0, radii_type, None if off is None else off.ctypes.data,
            None if xforms is None else C.addressof(xforms), B, C_, field, stride, None, scores, None, None, twist_grad, twist_hess)
    if not flex:
        return call(lib.mvx_score_hessian_batch, *head, None)
    return call(lib.mvx_score_hessian_flex_batch, *head, T, axes, moves, flex_grad, flex_hess, atom_pos, None)


HESSIAN_RULES = [dict(mode=3), dict(C_=0), dict(mode=2, C_=3), dict(stride=-1), dict(scores=None), dict(B=-1), dict(radii_type=7),
                 dict(offsets=None), dict(offsets=(1, 3)), dict(), dict(handle=P, offsets=(0, 1 << 31)), dict(handle=P, coords=None),
                 dict(handle=P, field=None), dict(handle=P, channels=None), dict(handle=P, radii_type=1),
                 # (behind the rules that read the handle once there are atoms: a batch without atoms)
                 dict(handle=P, offsets=(0, 0), radii_type=2, radii=P), dict(handle=P, offsets=(0, 0), twist_grad=None)]
ALL_BAD = dict(T=40, axes=None, moves=None, flex_grad=None)  # every rule of the entry's own broken at once


@pytest.mark.parametrize("kw", HESSIAN_RULES)
def test_the_flex_entry_rejects_what_the_hessian_entry_rejects_with_its_words_first(kw):
    want = _flex(flex=False, **kw)
    assert want[0] == MVX_ERR_INVALID, want
    assert _flex(**kw) == want
    assert _flex(**dict(kw, **ALL_BAD)) == want


def test_the_flex_rules_fire_last_in_their_order_and_before_a_device_is_touched():
    # (P stands for a handle: a batch without atoms reads it only once every rule has passed; the rule for `moves`, which needs
    # atoms, and the calls that pass are tests/test_hip_flex.py's)
    empty = dict(handle=P, offsets=(0, 0))
    for T in (-1, 33):
        rc, msg = _flex(T=T, axes=None, flex_grad=None, **empty)
        assert rc == MVX_ERR_INVALID and "T must be 0 ... 32" in msg, (rc, msg)
    rc, msg = _flex(axes=None, flex_grad=None, **empty)
    assert rc == MVX_ERR_INVALID and "axes and moves must not be null with T > 0" in msg, (rc, msg)
    for kw in (dict(), dict(moves=None), dict(T=0, axes=None, moves=None)):
        rc, msg = _flex(flex_grad=None, **dict(empty, **kw))
        assert rc == MVX_ERR_INVALID and "flex_grad must not be null" in msg, (rc, msg)
    # no molecules: nothing is needed but a legal T, and nothing is done
    none = dict(handle=P, B=0, xforms=None, scores=None, field=None, offsets=None)
    assert _flex(**dict(none, axes=None, moves=None, flex_grad=None, flex_hess=None))[0] == 0
    assert "T must be" in _flex(**dict(none, T=33))[1]
    # good arguments get as far as the handle
    for kw in (dict(), dict(flex_hess=None), dict(atom_pos=P), dict(T=0, axes=None, moves=None), dict(twist_grad=None, twist_hess=None),
               dict(T=32)):
        rc, msg = _flex(**kw)
        assert rc == MVX_ERR_INVALID and "null handle" in msg, (kw, rc, msg)


STATE = ("q", "t", "theta", "S", "G", "H", "lam", "taken", "dropped", "q2", "t2", "theta2")


def _lm(handle=None, B=2, T=3, have_trial=1, lam_down=1.0 / 3.0, lam_up=10.0, max_dropped=3, x=P, **ptrs):
    a = {k: P for k in STATE + ("S2", "G2", "H2")}
    a.update(ptrs)
    return call(_lib.load().mvx_flex_lm_step, handle, B, T, have_trial, lam_down, lam_up, max_dropped, *(a[k] for k in STATE), a["S2"],
                a["G2"], a["H2"], x, None)


@pytest.mark.parametrize("kw, words", [(dict(B=-1), "B must be >= 0"), (dict(T=-1), "T must be 0 ... 32"), (dict(T=33), "T must be 0 ... 32")]
                         + [({k: None}, "must not be null") for k in STATE]
                         + [({k: None}, "with have_trial") for k in ("S2", "G2", "H2")]
                         + [(dict(max_dropped=0), "max_dropped")]
                         + [({k: v}, "finite and > 0") for k in ("lam_down", "lam_up") for v in (0.0, -1.0, np.inf, np.nan)]
                         + [(dict(), "null handle"), (dict(B=0), "null handle"), (dict(T=0, theta=None, theta2=None), "null handle")])
def test_flex_lm_step_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _lm(**kw)
    assert rc == MVX_ERR_INVALID and words in msg, (rc, msg)


def test_flex_lm_step_rules_fire_in_lm_steps_order():
    assert "B must be" in _lm(B=-1, T=40, q=None, max_dropped=0)[1]
    assert "T must be" in _lm(T=40, q=None, max_dropped=0)[1]
    assert "q, t, S" in _lm(q=None, theta=None, S2=None, max_dropped=0)[1]
    assert "theta and theta2" in _lm(theta2=None, S2=None, max_dropped=0)[1]
    assert "with have_trial" in _lm(S2=None, max_dropped=0, lam_up=0.0)[1]
    assert "max_dropped" in _lm(max_dropped=0, lam_up=0.0)[1]
    assert "finite and > 0" in _lm(lam_up=0.0)[1]
    for kw in (dict(have_trial=0, S2=None, G2=None, H2=None), dict(x=None)):
        assert "null handle" in _lm(**kw)[1]
    none = dict(B=0, **{k: None for k in STATE + ("S2", "G2", "H2")}, x=None)
    assert _lm(handle=P, **none)[0] == 0


# ---- the Python layer --------------------------------------------------------------------------------------------------------
def _args(N=6, C_=4, B=2):
    rng = np.random.default_rng(0)
    moves = np.zeros(N, np.int32)
    moves[2] = moves[5] = 1
    return dict(coords=rng.uniform(-2, 2, (N, 3)), offsets=np.array([0, 3, 6]), centers=np.zeros((B, 3)),
                channels=rng.standard_normal((N, C_)).astype(np.float32), radii=1.0, axes=np.array([[[1, 2]], [[1, 2]]], np.int32),
                moves=moves)


def _posed(a, B=2):
    return dict(a, quaternions=np.ones((B, 4)), translations=np.zeros((B, 3)))


def test_voxelizer_has_the_methods():
    from molvoxel_amd.voxelizer.hip import voxelizer
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    par = lambda f: list(inspect.signature(f).parameters)
    assert par(Voxelizer.apply_torsions) == ["self", "coords", "offsets", "axes", "moves", "angles"]
    tail = ["channels", "radii", "field", "axes", "moves", "num_channels", "pivots", "per_atom"]
    assert par(Voxelizer.score_hessian_flex_batch) == ["self", "coords", "offsets", "centers"] + tail
    assert par(Voxelizer.score_hessian_flex_posed_batch) == ["self", "coords", "offsets", "centers", "quaternions", "translations"] + tail
    assert par(Voxelizer.flex_lm_step) == par(Voxelizer.lm_step)
    assert par(Voxelizer.refine_flex_posed_batch) == [
        "self", "coords", "offsets", "centers", "quaternions", "translations", "angles", "channels", "radii", "field", "axes", "moves",
        "num_channels", "steps", "lam0", "lam_down", "lam_up", "max_dropped", "stop_when_done"]
    p = inspect.signature(Voxelizer.refine_flex_posed_batch).parameters
    assert p["steps"].default == 40 and p["lam_down"].default == 1.0 / 3.0 and p["lam_up"].default == 10.0 and p["max_dropped"].default == 3
    assert inspect.isclass(voxelizer.FlexLMState) and callable(voxelizer.check_torsions)


def test_the_python_guards_fire_before_the_library_is_needed():
    import torch

    from molvoxel_amd.voxelizer.hip.voxelizer import FlexLMState

    F = torch.zeros((4, 16, 16, 16))
    a = _args()
    calls = (lambda v, **o: v.score_hessian_flex_batch(**{**a, 'field': F, **o}),
             lambda v, **o: v.score_hessian_flex_posed_batch(**{**_posed(a), 'field': F, **o}),
             lambda v, **o: v.refine_flex_posed_batch(**{**_posed(a), 'field': F, 'angles': np.zeros((2, 1)), **o}))
    for call in calls:
        with pytest.raises(ValueError, match="output='torch'"):
            call(_fake(output="numpy"))
        with pytest.raises(NotImplementedError, match="channel-wise radii with features"):
            call(_fake("channel-wise"), radii=np.ones(4, np.float32))
        with pytest.raises(AssertionError, match="axes does not match dimension"):
            call(_fake(), axes=np.zeros((3, 1, 2), np.int32))
        with pytest.raises(AssertionError, match="moves does not match dimension"):
            call(_fake(), moves=np.zeros(5, np.int32))
        with pytest.raises(AssertionError, match="at most 32 torsions"):
            call(_fake(), axes=np.full((2, 33, 2), -1, np.int32))
        with pytest.raises(AssertionError, match="molecule 1, torsion 0: the axis atom a"):
            call(_fake(), moves=np.array([0, 0, 1, 0, 1, 1], np.int32))
    for call in calls[:1]:  # (the posed forms pack their poses on the device in front of these)
        with pytest.raises(AssertionError, match="field does not match dimension"):
            call(_fake(), field=torch.zeros((3, 16, 16, 16)))
        with pytest.raises(AssertionError, match="pivots does not match dimension"):
            call(_fake(), pivots=np.zeros((3, 3)))
    for call in calls[1:]:
        with pytest.raises(AssertionError, match="quaternions does not match dimension"):
            call(_fake(), quaternions=np.ones((2, 3)))
    with pytest.raises(AssertionError, match="angles does not match dimension"):
        calls[2](_fake(), angles=np.zeros((2, 2)))
    with pytest.raises(ValueError, match="output='torch'"):
        _fake(output="numpy").apply_torsions(a["coords"], a["offsets"], a["axes"], a["moves"], np.zeros((2, 1)))
    with pytest.raises(AssertionError, match="angles does not match dimension"):
        _fake().apply_torsions(a["coords"], a["offsets"], a["axes"], a["moves"], np.zeros((2, 3)))
    with pytest.raises(AssertionError, match="offsets must span coords"):
        _fake().apply_torsions(a["coords"], np.array([0, 3, 5]), a["axes"], a["moves"], np.zeros((2, 1)))
    f64 = dict(dtype=torch.float64)
    st = FlexLMState(torch.zeros((3, 4), **f64), torch.zeros((3, 3), **f64), torch.zeros((3, 2), **f64), torch.zeros(3, **f64),
                     torch.zeros((3, 8), **f64), torch.zeros((3, 8, 8), **f64), torch.ones(3, **f64))
    assert st.taken.dtype == torch.int32 and st.q2 is None and st.theta2 is None and st.x is None
    with pytest.raises(AssertionError, match="state.q should be"):  # (host tensors: not on the voxelizer's device)
        _fake().flex_lm_step(st)


def test_check_torsions_names_the_first_torsion_that_breaks_each_tree_rule():
    from molvoxel_amd.voxelizer.hip.voxelizer import check_torsions

    off = np.array([0, 0, 12])
    axes = np.full((2, 5, 2), -1, np.int32)
    axes[1, :4] = fr.TREE_AXES
    good = fr.tree_moves()
    check_torsions(off, axes, good)  # (padding and a molecule without atoms are fine)
    import torch

    check_torsions(off, torch.tensor(axes), torch.tensor(good))

    def broken(words, ax=None, mv=None, **sets):
        m = good.copy() if mv is None else mv
        with pytest.raises(AssertionError, match=words):
            check_torsions(off, axes if ax is None else ax, m)

    def with_sets(*sets):
        return fr.tree_moves(12, sets)

    s = [list(x) for x in fr.TREE_SETS]
    broken("molecule 1, torsion 1: the axis atom b = 5 must turn", mv=with_sets(s[0], s[1][1:], s[2], s[3]))
    broken("molecule 1, torsion 3: the axis atom a = 4 must not turn", mv=with_sets(s[0], s[1], s[2], s[3] + [4]))
    broken("molecule 1, torsion 3: its set overlaps the set of torsion 1", mv=with_sets(s[0], s[1], s[2], s[3] + [8]))
    swapped = axes.copy()
    swapped[1, [0, 1]] = swapped[1, [1, 0]]
    broken("molecule 1, torsion 1: contains the set of torsion 0.*parents come before children", ax=swapped,
           mv=with_sets(s[1], s[0], s[2], s[3]))
    same = axes.copy()
    same[1, 4] = same[1, 2]
    broken("molecule 1, torsion 4: the same set as torsion 2", ax=same, mv=with_sets(s[0], s[1], s[2], s[3], s[2]))
    outside = axes.copy()
    outside[1, 2] = (2, 7)  # (a_2 = 2 is not in the set of torsion 0 around it)
    broken("molecule 1, torsion 2: both axis atoms must lie in the set of torsion 0", ax=outside)
    with pytest.raises(AssertionError, match="moves does not match dimension"):
        check_torsions(off, axes, good[:11])
    with pytest.raises(AssertionError, match="axes does not match dimension"):
        check_torsions(off, axes[:1], good)


def test_torsion_tree_on_the_10gs_ligand():
    from molvoxel_amd.etc.mol import BondType, Molecule, read_sdf, torsion_tree
    from molvoxel_amd.voxelizer.hip.voxelizer import check_torsions

    mol = read_sdf(os.path.join(ROOT, "tests", "golden", "10gs", "10gs_ligand.sdf"))[0]
    axes, moves = torsion_tree(mol)
    T, N = axes.shape[0], mol.num_atoms
    assert axes.dtype == np.int32 and moves.dtype == np.int32 and moves.shape == (N,) and 0 < T <= 32
    check_torsions(np.array([0, N]), axes[None], moves)
    bonds = {frozenset(map(int, b)): int(t) for b, t in zip(mol.bonds, mol.bond_types)}
    degree = np.bincount(mol.bonds.reshape(-1), minlength=N)
    for k, (a, b) in enumerate(axes):
        assert bonds[frozenset((int(a), int(b)))] == BondType.SINGLE and degree[a] >= 2 and degree[b] >= 2
        # acyclic: no other bond joins the set and the rest
        inside = fr.bits(moves, k)
        crossing = [tuple(x) for x in mol.bonds if inside[x[0]] != inside[x[1]]]
        assert len(crossing) == 1 and set(crossing[0]) == {int(a), int(b)}, (k, crossing)
    # ... and every bond that qualifies was cut: single bonds with further neighbours at both ends that are bridges of the bond
    # graph, found here by a depth-first search of its own (a tree edge (p, v) is a bridge iff low[v] > disc[p])
    nbrs = [[] for _ in range(N)]
    for j, (a, b) in enumerate(mol.bonds):
        nbrs[int(a)].append((int(b), j))
        nbrs[int(b)].append((int(a), j))
    disc, low, bridges, clock = [-1] * N, [0] * N, set(), [0]

    def visit(v, by):
        disc[v] = low[v] = clock[0]
        clock[0] += 1
        for w, j in nbrs[v]:
            if j == by:
                continue
            if disc[w] < 0:
                visit(w, j)
                low[v] = min(low[v], low[w])
                if low[w] > disc[v]:
                    bridges.add(j)
            else:
                low[v] = min(low[v], disc[w])

    for v in range(N):
        if disc[v] < 0:
            visit(v, -1)
    want = {frozenset(map(int, mol.bonds[j])) for j in bridges
            if int(mol.bond_types[j]) == BondType.SINGLE and degree[mol.bonds[j, 0]] >= 2 and degree[mol.bonds[j, 1]] >= 2}
    assert {frozenset(map(int, ax)) for ax in axes} == want and T == len(want) == 15
    assert (moves == 0).sum() >= 1  # (the root fragment is in no set)
    other_root = torsion_tree(mol, root=int(axes[-1, 1]))
    assert other_root[0].shape == axes.shape and other_root[1][int(axes[-1, 1])] == 0
    chain = Molecule(np.arange(105.0).reshape(35, 3), ["C"] * 35, [(i, i + 1) for i in range(34)], [1] * 34)
    assert torsion_tree(chain, root=0)[0].shape == (32, 2)
    longer = Molecule(np.arange(108.0).reshape(36, 3), ["C"] * 36, [(i, i + 1) for i in range(35)], [1] * 35)
    with pytest.raises(ValueError, match="more than 32"):
        torsion_tree(longer, root=0)


# ---- kernel resources -----------------------------------------------------------------------------------------------------------
def test_the_flex_kernels_use_no_scratch_and_spill_nothing():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_flex.o")
    assert obj in regs.KERNEL_OBJECTS
    assert os.path.exists(obj), "mvx_flex.o not built (make -C molvoxel_amd/csrc)"
    res = regs.kernel_resources(obj)
    assert sorted(res) == ["flex_assemble_kernel", "flex_lm_step_kernel", "flex_subset_kernel", "torsion_apply_kernel"], sorted(res)
    for name, r in res.items():
        print(f"{name}: {r}")
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (name, r)
    assert res["flex_lm_step_kernel"]["lds"] <= 38 * 39 * 8 + 38 * 8, res["flex_lm_step_kernel"]  # the system and x


# ---- what the GPU tests rest on ----------------------------------------------------------------------------------------------------
def test_the_lm_rows_mix_every_kind_and_numpy_solves_them_to_rounding():
    from tests import lm_rows as R

    for T in X.LM_T:
        st, trial = X.lm_reference_state(T)
        assert {R.kind_of(X.LM_B, b) for b in range(X.LM_B)} == set(R.KINDS)
        got = fr.step(st, trial, R.LAM_DOWN, R.LAM_UP, R.MAX_DROPPED)
        for b in range(X.LM_B):
            k = R.kind_of(X.LM_B, b)
            assert got[b] == {"accepted": "accept", "unnormalised": "accept", "finished": None}.get(k, "drop"), (T, b, k, got[b])
            stays = k in R.FAILS or k in ("finished", "dropped_last")
            assert stays == (not st.x[b].any()), (T, b, k)
            if k == "omega_zero":
                assert not st.x[b, 3:6].any() and np.array_equal(st.q2[b], st.q[b]) and st.x[b, 6:].all()
            if got[b] == "accept":
                assert np.array_equal(st.theta[b], X.lm_rows(T)[0]["theta2"][b])
    worst, cond = X.lm_numpy_residual()
    print(f"FLEX_LM_NUMPY_RESIDUAL np.linalg.solve: worst residual ratio {worst:.3f}, largest condition number {cond:.3g}")
    assert cond < 1e8 and 0.0 < worst < 8.0


def test_the_reference_step_with_no_torsions_is_lm_references_step():
    from tests import lm_reference as lm
    from tests import lm_rows as R

    B = 65
    a, trial = R.reference_state(B)
    s = R.rows(B)[0]
    b = fr.State(s["q"], s["t"], np.zeros((B, 0)), s["S"], s["G"], s["H"], s["lam"], s["taken"], s["dropped"])
    b.q2, b.t2, b.theta2 = s["q2"].copy(), s["t2"].copy(), np.zeros((B, 0))
    assert lm.step(a, trial, R.LAM_DOWN, R.LAM_UP, R.MAX_DROPPED) == fr.step(b, trial, R.LAM_DOWN, R.LAM_UP, R.MAX_DROPPED)
    for name, other in (("q", "q"), ("t", "t"), ("S", "S"), ("G", "G"), ("H", "H"), ("lam", "lam"), ("taken", "taken"),
                        ("dropped", "dropped"), ("q2", "q2"), ("t2", "t2"), ("xi", "x")):
        assert np.array_equal(getattr(a, name), getattr(b, other), equal_nan=True), name


def test_the_cpu_refinement_meets_the_conditions_of_the_gpu_test():
    st, hist, rigid, rhist = X.cpu_refinement()
    q0, t0, th0 = X.refine_starts()
    assert tuple(hist.shape) == (X.REFINE_ROUNDS + 1, X.REFINE_POSES) and th0.shape == (8, 4)
    assert (np.abs(np.degrees(th0)) >= 10.0).all() and (np.abs(np.degrees(th0)) <= 15.0).all()
    X.refine_conditions(hist, st.S, rigid.S)
    print(f"FLEX_CPU_REFINE taken {st.taken.tolist()} (rigid {rigid.taken.tolist()}); score {hist[0].min():.1f} ... {hist[0].max():.1f} -> "
          f"{st.S.min():.1f} ... {st.S.max():.1f}, rigid -> {rigid.S.min():.1f} ... {rigid.S.max():.1f}")
