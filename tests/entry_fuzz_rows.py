"""Seeded draws of the entry fuzz (tests/test_hip_entry_fuzz.py on the GPU, tests/test_entry_fuzz_host.py without one): the score,
pose, sum and moments entries over the parameter space of the gradient fuzz - resolution 0.3 ... 1.0, sigma 0.3 ... 1.0, blockdims
that do not divide D, dimensions that are no multiple of the sub-tile edges, spread / cluster / shell layouts with atoms on grid
nodes at r = 2 res and one atom past a box face. Needs neither torch nor a GPU; the arrays of a draw are never modified.

walk_draw(seed), seed in range(N_WALK): one batch for score_batch / score_posed_batch, mvx_pose_grad_batch and
forward_posed_batch. summed_draw(seed), seed in range(N_SUMMED): one batch for forward_batch, forward_sum, moments_batch and the
moments gradient (and their posed variants in every third draw). The layouts and radii are tests/test_hip_grad_fuzz.py's
_geometry and _radii, called as they stand.

Ties under a pose. A molecule's first min(n, 5) atoms lie on grid nodes of its own frame with a radius of 2 res. In a posed walk
draw the molecules b with (b + seed) % 2 == 0 - the `tie_mols` - keep them on nodes: identity quaternion, a translation k res per
axis (k in {-1, 0, 1}, 0 where res > 0.6), and coordinates x = c + (node - float32(t)), so that pose_reference.positions gives the
node back. The centres are multiples of 1/8, so for the resolutions 0.5, 0.75 and 1.0 every step of that is exact. At precision 32
the reference compares float32(sqrt(d2)) / r32 with 1, which absorbs the last-place errors of the other resolutions; at precision
64 with resolution 0.3 or 0.4 nothing absorbs them, and those tie molecules are centred on the origin with a zero translation
(their atoms ARE the nodes - or, since axis[i] - axis[i +- 2] is 2 res only to the last place there, the float64 number that is
2 res from the neighbouring node, which lies within two units in the last place of the node). The nodes of a tie molecule are
redrawn (at most 64 times) until tie_voxels() - the reference's own compare - finds equality. The other molecules of a posed draw get |q| in {1, 0.8, 1.25} and t up to +-0.6, and the draws with a
random rotation cannot keep an atom on a node: their planted atoms are ordinary atoms of the sample. `ties` lists the atoms (global
indices) whose tie is claimed: those of tie molecules that have a radius of 2 res (atom-wise always, channel-wise through channel
or type 0, scalar where the scalar is 2 res). In a summed draw every molecule of a centred draw claims its ties (precision 32
absorbs the centring), and a posed summed draw has tie molecules as above.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import grad_reference as gr
from tests import pose_reference as pr
from tests.sum_sweep_rows import SERVED, SWEEP_C
from tests.test_hip_fuzz import DIMS
from tests.test_hip_grad_fuzz import _geometry, _radii

N_WALK, N_SUMMED = 96, 48
WALK_OFFSET, SUMMED_OFFSET = 50_000, 60_000
SAMPLE = 32  # atoms per molecule that go through the per-atom checks

RESOLUTIONS = [0.3, 0.4, 0.5, 0.75, 1.0]
SIGMAS = [0.3, 0.5, 1.0]
NORMS = [1.0, 0.8, 1.25]
CEN = np.array([30.0, -20.0, 12.0])

WALK_D = [d for d in DIMS if d <= 48]
WALK_BLOCKDIMS = [None, None, 4, 5, 7, 8, 12, 16, "D"]
WALK_C = [1, 2, 5, 8, 31, 32, 33, 40, 65]
WALK_KINDS = ["f32", "bf16", "f64"]
WALK_SIZES = [0, 1, 2, 33, 64, 65, 150, 300]
WALK_ELEMENTS = 8_000_000  # B * C * D^3: the per-molecule upstream of the bit identity and the posed grids stay this small
BAD_TYPE_ATOM = 6          # this atom of a molecule of seven or more gets a type past the channels

SUMMED_D = [8, 12, 16, 20, 24, 28, 36, 44]
SUMMED_BLOCKDIMS = [None, 16, 24, "D"]
SUMMED_ELEMENTS = 8_000_000


def dyadic(res):
    return res in (0.5, 0.75, 1.0)


def sums_supported(D, blockdim):
    """Do forward_sum and moments_batch serve this (dimension, blockdim)? Voxelizer._sum_guard's rule, which
    tests/test_sum_rows_host.py holds equal to mvx_plan's lane_range."""
    bd = 8 if blockdim is None else blockdim
    return D % 4 == 0 and (-(-D // bd) == 1 or bd % 8 == 0)


def tie_voxels(p, r, D, res, blockdim, precision, rc=None, form="atom"):
    """How many voxels the reference admits for an atom at p (3,) of radius r with dr == 1 exactly: grad_reference.atom_density's
    window and admission, and its compare dr = fp(sqrt(d2)) / fp(r) <= 1 restated on that window."""
    geo = gr.Geometry(D, res, blockdim, 0.5, "binary", precision)
    ev = gr.atom_density(geo, np.asarray(p, np.float64), [r], float(r) if rc is None else rc, form)
    if ev is None:
        return 0
    _, _, d2, rho = ev
    dr = np.sqrt(d2).astype(geo.fp) / geo.fp(r)
    return int(((dr == 1.0) & (rho[0] > 0)).sum())


def _poses(rng, B, seed, res, D, precision, sizes, posed):
    """Centres (multiples of 1/8 around CEN), quaternions, translations and the tie molecules of a batch."""
    cen = CEN + rng.integers(-16, 17, (B, 3)) / 8.0
    q = rng.standard_normal((B, 4))
    q *= (np.array(NORMS)[rng.integers(0, 3, B)] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    k = rng.integers(-1, 2, (B, 3)) if res <= 0.6 else np.zeros((B, 3), np.int64)
    tie_mols = [b for b in range(B) if (b + seed) % 2 == 0] if posed else []
    for b in tie_mols:
        q[b] = [1.0, 0.0, 0.0, 0.0]
        t[b] = k[b] * res
        if precision == 64 and not dyadic(res):
            cen[b], t[b] = 0.0, 0.0
    return cen, q, t, tie_mols


def _place(rng, rel, k, c, q, t, D, res, blockdim, precision, tie):
    """World coordinates of a molecule whose frame positions are rel (n, 3). tie: the first k rows are nodes that the pose must
    give back - x = c + (node - float32(t)) under the identity quaternion, the nodes redrawn until the reference sees the tie."""
    if not tie:
        # (general pose: the frame positions are taken as the world positions around the centre; the kernel poses them)
        return rel + c
    t32 = t.astype(np.float32).astype(np.float64)
    axis = gr.axis(D, res)
    x = c + (rel - t32)

    def tied(a):
        p = pr.positions(x[a:a + 1], c, q, t)[0]
        return tie_voxels(p, 2 * res, D, res, blockdim, precision) > 0

    for a in range(k):
        for _ in range(64):
            if tied(a):
                break
            i, j, l = (int(v) for v in rng.integers(0, D, 3))
            xs = [axis[i]]
            if precision == 64 and not dyadic(res):
                # float64 at resolution 0.3 / 0.4: axis[i] - axis[i +- 2] is 2 res only to the last place or two; the x that IS 2 res
                # from a neighbour's node, where float64 has one
                xs += [axis[n] + s * 2 * res for n, s in ((i - 2, 1.0), (i + 2, -1.0)) if 0 <= n < D]
            for px in xs:
                rel[a] = [px, axis[j], axis[l]]
                x[a] = c + (rel[a] - t32)
                if tied(a):
                    break
    return x


def _channels(rng, mode, radii_type, sizes, C_, fp, bad_types, signed=True):
    """(chan, bad): feature rows with zeros (of mixed signs if `signed`) | types with C - 1 first and - radii type permitting, in molecules of
    seven atoms or more - one type past the channels | None; bad: the global indices of those atoms."""
    N = int(sum(sizes))
    off = np.concatenate([[0], np.cumsum(sizes)])
    if mode == "features":
        f = rng.random((N, C_))
        f[rng.random((N, C_)) < 0.3] = 0.0
        if signed:
            f[rng.random((N, C_)) < 0.3] *= -1.0
        return f.astype(fp), []
    if mode == "single":
        return None, []
    ty = rng.integers(0, C_, N)
    bad = []
    for b, n in enumerate(sizes):
        if n:
            ty[off[b]] = C_ - 1
        if radii_type == "channel-wise":
            ty[off[b]:off[b] + min(n, 5)] = 0  # (radii[0] = 2 res: the planted atoms keep their tie)
        elif bad_types and n > BAD_TYPE_ATOM:
            ty[off[b] + BAD_TYPE_ATOM] = C_ + 2
            bad.append(int(off[b]) + BAD_TYPE_ATOM)
    return ty, bad


def _radii_of(rng, radii_type, sizes, C_, res, fp):
    """(radii as the call takes them, r_atom (N,) float64 or None for channel-wise features)."""
    N = int(sum(sizes))
    if radii_type == "scalar":
        r = float(_radii(rng, "scalar", 0, C_, res, 0))
        return r, np.full(N, float(fp(r)))
    if radii_type == "atom-wise":
        parts = [_radii(rng, "atom-wise", n, C_, res, min(n, 5)) for n in sizes]
        r = (np.concatenate(parts) if parts else np.zeros(0)).astype(fp)
        return r, r.astype(np.float64)
    return np.asarray(_radii(rng, "channel-wise", 0, C_, res, 0)).astype(fp), None


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _shrink(C_, choices, per_channel, limit):
    """The largest channel count of `choices` not above C_ whose grids stay under `limit` elements."""
    for c in sorted((x for x in choices if x <= C_), reverse=True):
        if c * per_channel <= limit:
            return c
    return min(choices)


@functools.lru_cache(maxsize=None)
def walk_draw(seed: int) -> dict:
    rng = np.random.default_rng(WALK_OFFSET + seed)
    D = int(rng.choice(WALK_D))
    res = float(rng.choice(RESOLUTIONS))
    sigma = float(rng.choice(SIGMAS))
    blockdim = WALK_BLOCKDIMS[int(rng.integers(len(WALK_BLOCKDIMS)))]
    blockdim = D if blockdim == "D" else blockdim
    density = str(rng.choice(["gaussian", "gaussian", "binary"]))
    mode = str(rng.choice(["features", "types", "single"]))
    radii_type = str(rng.choice(["scalar", "atom-wise", "channel-wise"]))
    if mode == "single" and radii_type == "channel-wise":
        radii_type = "atom-wise"
    C_ = 1 if mode == "single" else int(rng.choice(WALK_C))
    kind = str(rng.choice(WALK_KINDS))
    precision = 64 if kind == "f64" else 32
    fp = np.float64 if kind == "f64" else np.float32
    per_mol = bool(rng.integers(2))
    transform = "posed" if rng.integers(2) else int(rng.integers(1 << 20))
    B = int(rng.integers(1, 6))
    empty = seed % 4  # an empty molecule first, last, in the middle, or wherever the sizes put one
    B = max(B, (2, 2, 3, 1)[empty])
    sizes = [int(rng.choice(WALK_SIZES)) for _ in range(B)]
    if empty < 3:
        sizes[(0, B - 1, B // 2)[empty]] = 0
    C_ = _shrink(C_, WALK_C, B * D ** 3, WALK_ELEMENTS)
    posed = transform == "posed"
    cen, q, t, tie_mols = _poses(rng, B, seed, res, D, precision, sizes, posed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    mols, planted = [], []
    for b, n in enumerate(sizes):
        rel, special = _geometry(rng, n, D, res, str(rng.choice(["spread", "cluster", "shell"])))
        mols.append(_place(rng, rel, min(n, 5), cen[b], q[b], t[b], D, res, blockdim, precision, b in tie_mols))
        planted.append([int(off[b]) + a for a in special])
    xyz = np.concatenate(mols).reshape(-1, 3)
    chan, bad = _channels(rng, mode, radii_type, sizes, C_, fp, bool(rng.integers(2)))
    radii, r_atom = _radii_of(rng, radii_type, sizes, C_, res, fp)
    if mode == "types" and radii_type == "channel-wise":
        r_atom = radii[chan].astype(np.float64)
    sample = []
    for b, n in enumerate(sizes):
        keep = set(planted[b]) | {a for a in bad if off[b] <= a < off[b + 1]}
        rest = rng.choice(n, min(n, SAMPLE - len(keep)), replace=False) if n else []
        sample.append(sorted(keep | {int(off[b]) + int(a) for a in rest}))
    # whose tie is claimed: the node atoms of the tie molecules that have a radius of 2 res
    has_tie_radius = radii_type != "scalar" or radii == 2 * res
    ties = [a for b in tie_mols for a in planted[b][:min(sizes[b], 5)]] if has_tie_radius else []
    field_grad = (not per_mol and kind != "f64" and sums_supported(D, blockdim)
                  and not (mode == "features" and radii_type == "channel-wise"))
    return _freeze(dict(seed=seed, D=D, res=res, sigma=sigma, blockdim=blockdim, density=density, mode=mode, radii_type=radii_type,
                        C=C_, kind=kind, precision=precision, per_mol=per_mol, transform=transform, posed=posed, B=B, N=int(off[-1]),
                        sizes=tuple(sizes), empty=("first", "last", "middle", "drawn")[empty], off=off, cen=cen, q=q, t=t, xyz=xyz,
                        chan=chan, radii=radii, r_atom=r_atom, tie_mols=tuple(tie_mols), planted=planted, ties=tuple(ties),
                        bad_types=tuple(bad), sample=sample, field_grad=field_grad, fseed=int(rng.integers(1 << 30))))


def summed_blockdims(D):
    """The blockdims of SUMMED_BLOCKDIMS the summed kernels serve at dimension D: those whose plan has lane_range == 0
    (molvoxel_amd.voxelizer.hip._lib.plan_call, as tests/test_sum_rows_host.py queries it)."""
    from molvoxel_amd.voxelizer.hip import _lib

    out = []
    for bd in SUMMED_BLOCKDIMS:
        v = D if bd == "D" else bd
        if _lib.plan_call(D, 32, 2, total_atoms=10, blockdim=8 if v is None else v)["lane_range"] == 0:
            out.append(v)
    return out


@functools.lru_cache(maxsize=None)
def summed_draw(seed: int) -> dict:
    rng = np.random.default_rng(SUMMED_OFFSET + seed)
    D = int(rng.choice(SUMMED_D))
    res = float(rng.choice(RESOLUTIONS))
    sigma = float(rng.choice(SIGMAS))
    served = summed_blockdims(D)
    blockdim = served[int(rng.integers(len(served)))]
    mode, radii_type = SERVED[int(rng.integers(len(SERVED)))]
    C_ = 1 if mode == "single" else int(rng.choice(SWEEP_C))
    density = ("gaussian", "binary")[int(rng.integers(2))]
    B = int(rng.integers(1, 9))
    sizes = [int(n) for n in rng.integers(0, 121, B)]
    if sum(sizes) == 0:
        sizes[-1] = 7
    C_ = _shrink(C_, SWEEP_C, B * D ** 3, SUMMED_ELEMENTS)
    posed = seed % 3 == 0
    clustered = seed % 4 == 0
    cen, q, t, tie_mols = _poses(rng, B, seed, res, D, 32, sizes, posed)
    if not posed:
        tie_mols = list(range(B))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    mols, planted = [], []
    for b, n in enumerate(sizes):
        rel, special = _geometry(rng, n, D, res, "cluster" if clustered else str(rng.choice(["spread", "shell"])))
        tie = posed and b in tie_mols
        mols.append(_place(rng, rel, min(n, 5), cen[b], q[b], t[b], D, res, blockdim, 32, tie))
        planted.append([int(off[b]) + a for a in special])
    xyz = np.concatenate(mols).reshape(-1, 3)
    chan, bad = _channels(rng, mode, radii_type, sizes, C_, np.float32, bool(rng.integers(2)), signed=False)
    radii, r_atom = _radii_of(rng, radii_type, sizes, C_, res, np.float32)
    if mode == "types" and radii_type == "channel-wise":
        r_atom = radii[chan].astype(np.float64)
    has_tie_radius = radii_type != "scalar" or radii == 2 * res
    ties = [a for b in tie_mols for a in planted[b][:min(sizes[b], 5)]] if has_tie_radius else []
    sample = sorted({a for p in planted for a in p} | set(bad) | set(rng.choice(int(off[-1]), min(int(off[-1]), 64), replace=False).tolist()))
    return _freeze(dict(seed=seed, D=D, res=res, sigma=sigma, blockdim=blockdim, density=density, mode=mode, radii_type=radii_type,
                        C=C_, kind="f32", precision=32, posed=posed, clustered=clustered, B=B, N=int(off[-1]), sizes=tuple(sizes),
                        off=off, cen=cen, q=q, t=t, xyz=xyz, chan=chan, radii=radii, r_atom=r_atom, tie_mols=tuple(tie_mols),
                        planted=planted, ties=tuple(ties), bad_types=tuple(bad), sample=sample, tseed=int(rng.integers(1 << 30)),
                        gseed=int(rng.integers(1 << 30))))


def field_of(d: dict) -> np.ndarray:
    """The seeded field of a walk draw as the kernel reads it, widened to float64: (C, D, D, D) shared or (B, C, D, D, D), standard
    normal values rounded to the grid's type (bfloat16: round to nearest even on the float32 bits)."""
    shape = ((d["B"],) if d["per_mol"] else ()) + (d["C"],) + (d["D"],) * 3
    F = np.random.default_rng(d["fseed"]).standard_normal(shape)
    if d["kind"] == "f64":
        return F
    F = F.astype(np.float32)
    if d["kind"] == "bf16":
        u = F.view(np.uint32)
        u = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
        F = u.view(np.float32)
    return F.astype(np.float64)


def target_of(d: dict) -> np.ndarray:
    """The seeded float32 target of a summed draw, of mixed signs: (C, D, D, D)."""
    return np.random.default_rng(d["tseed"]).standard_normal((d["C"],) + (d["D"],) * 3).astype(np.float32)


def dm_of(d: dict, K: int) -> np.ndarray:
    """Seeded dL/dm of mixed signs, different for every molecule and channel: (B, C, K) float64."""
    return np.random.default_rng(d["gseed"] + K).standard_normal((d["B"], d["C"], K))


# ---- what the kernels see, and the channels as the references take them ----------------------------------------------------------
def quaternions_of(d: dict) -> np.ndarray:
    """(B, 4): the poses of a posed draw, or the quaternions score_batch / forward_batch draw with random_rotation under
    np.random.seed(transform), molecule by molecule (walk draws); the identity for a centred summed draw."""
    if d["posed"]:
        return d["q"]
    if "transform" not in d:
        return np.tile([1.0, 0.0, 0.0, 0.0], (d["B"], 1))
    from molvoxel_amd.voxelizer.hip.transform import draw_forward_transform

    state = np.random.get_state()
    np.random.seed(d["transform"])
    out = np.array([draw_forward_transform(0.0, True)[1] for _ in range(d["B"])]).reshape(d["B"], 4)
    np.random.set_state(state)
    return out


def positions_of(d: dict) -> np.ndarray:
    """(N, 3) float64: the atoms as the kernels see them (pose_reference.batch_positions)."""
    t = d["t"] if d["posed"] else np.zeros((d["B"], 3))
    return pr.batch_positions(d["xyz"], d["off"], d["cen"], quaternions_of(d), t)


def reference_channels(d: dict):
    """(w, types) for the references: float64 feature rows, or the types with everything past the channels named C."""
    if d["mode"] == "features":
        return d["chan"].astype(np.float64), None
    if d["mode"] == "types":
        return None, np.where(d["chan"] >= d["C"], d["C"], d["chan"])
    return None, None


def features_of(d: dict) -> np.ndarray:
    """The weight rows w[n, c] of every atom as features in the call's float type: the feature row, onehot(type) (zeros for a type
    past the channels), or 1 - the form in which the oracles take every mode, a type past the channels included."""
    fp = np.float64 if d["precision"] == 64 else np.float32
    if d["mode"] == "features":
        return d["chan"]
    if d["mode"] == "single":
        return np.ones((d["N"], 1), fp)
    w = np.zeros((d["N"], d["C"]), fp)
    ok = d["chan"] < d["C"]
    w[np.nonzero(ok)[0], d["chan"][ok]] = 1.0
    return w


def oracle_grid(d: dict, p: np.ndarray, b: int) -> np.ndarray:
    """The oracle's grid (C, D, D, D) of molecule b at the positions p (N, 3): oracle/c_oracle, or oracle/numpy_port at precision
    64, with the draw's resolution, sigma and blockdim; one-hot features with each atom's own radius stand for types."""
    from oracle import c_oracle, numpy_port

    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    fp = np.float64 if d["precision"] == 64 else np.float32
    if hi == lo:
        return np.zeros((d["C"],) + (d["D"],) * 3, fp)
    chan = None if d["mode"] == "single" else features_of(d)[lo:hi]
    if d["radii_type"] == "scalar":
        radii, rt = d["radii"], "scalar"
    elif d["radii_type"] == "channel-wise" and d["mode"] == "features":
        radii, rt = d["radii"], "channel-wise"
    else:
        radii, rt = d["r_atom"][lo:hi].astype(fp), "atom-wise"
    if d["precision"] == 32:
        return c_oracle.voxelize(p[lo:hi], chan, radii, resolution=d["res"], dimension=d["D"], blockdim=d["blockdim"], radii_type=rt,
                                 density=d["density"], sigma=d["sigma"])
    spec = numpy_port.GridSpec(d["res"], d["D"], d["blockdim"])
    return numpy_port.voxelize(spec, p[lo:hi], chan, radii, radii_type=rt, density=d["density"], sigma=d["sigma"], precision=64)


def molecule(d: dict, b: int):
    """(lo, hi, radii of molecule b as the references take them)."""
    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    return lo, hi, (d["radii"][lo:hi] if d["radii_type"] == "atom-wise" else d["radii"])


def tie_count(d: dict, a: int, p: np.ndarray) -> int:
    """tie_voxels for atom a (global index) of a draw at its position p under the pose, with the atom's own 2 res radius and the
    cull of its radii type."""
    r = 2 * d["res"]
    if d["radii_type"] == "scalar":
        return tie_voxels(p, r, d["D"], d["res"], d["blockdim"], d["precision"], rc=float(d["radii"]), form="scalar")
    if d["radii_type"] == "channel-wise" and d["mode"] == "features":
        fp = np.float32 if d["precision"] == 32 else np.float64
        rc = float(np.asarray(d["radii"]).astype(fp).max())
        return tie_voxels(p, r, d["D"], d["res"], d["blockdim"], d["precision"], rc=rc, form="chan32" if d["precision"] == 32 else "scalar")
    return tie_voxels(p, r, d["D"], d["res"], d["blockdim"], d["precision"])
