"""Batches with atoms that reach no voxel (tests/test_hip_dead_atoms.py on the GPU, tests/test_dead_atoms_host.py without one).
Needs neither torch nor a GPU; the arrays of a row are never modified.

A dead atom passes no compare of the reference's rule: a NaN, infinite or astronomically large coordinate (DEAD_COORDS, with an
ordinary radius), an atom-wise radius that is zero, negative, NaN or infinite on an atom well inside the box (DEAD_RADII), or a
type outside [0, C) (dead_types(C); types mode with scalar or atom-wise radii - radii by type would be indexed by it). A row is a
small clean batch plus such atoms spliced in: dirty(row) and clean(row) are the two batches in the form of
tests/entry_fuzz_rows.py's draws (so the helpers of tests/test_hip_entry_fuzz.py take them), live(row) is the mask over the dirty
atoms that maps one onto the other: dirty arrays[live] are the clean arrays. Both have the same B molecules, so per-molecule
outputs compare row by row.

The clean batch: live sizes LIVE = (70, 0, 300, 0, 40). Molecule 1 has no atoms in either batch; molecule 3 has none in the clean
batch and ALL_DEAD = 7 dead atoms in the dirty one (n > 0 and nothing kept), between live molecules. Placements of the dead atoms:
  scattered  dirty positions 0, 63, 64 and last of molecule 0, 0, 255, 256 and last of molecule 2 (the wave chunk, the four-wave
             stride of pose_grad_kernel and the thread stride of density_sum_kernel), first and last of molecule 4;
  tail       the same atoms after the last live atom of their molecule: every live atom keeps the lane it has in the clean call
             of a per-molecule reduction;
  call_tail  all of them - molecule 3's too, which is then empty - after the last live atom of molecule 4: the same for a
             call-wide reduction.
The kinds that apply to a row go round its 17 slots in order, so each occurs at least once (there are at most 14).

cloud(row), for the view entries: ONE shared cloud of 300 live atoms wider than the box with dead atoms at 0, 63, 64, 255, 256,
last and a few more, under B = 3 poses; dirty / clean / live as above with the key "N" instead of offsets.
"""
from __future__ import annotations

import functools

import numpy as np

from tests.entry_fuzz_rows import CEN, NORMS, WALK_ELEMENTS, _freeze

NAN, INF = float("nan"), float("inf")
DEAD_COORDS = {"x nan": [NAN, 0.0, 0.0], "y nan": [0.0, NAN, 0.0], "x inf": [INF, 1.0, -1.0], "x -inf y nan": [-INF, NAN, 2.0],
               "1e300": [1e300] * 3, "3e38": [3e38, -3e38, 0.5], "1e20": [1e20, 0.0, 0.0]}
DEAD_RADII = {"r 0": 0.0, "r -1": -1.0, "r nan": NAN, "r inf": INF}
LIVE = (70, 0, 300, 0, 40)
ALL_DEAD, ALL_DEAD_MOL, EMPTY_MOL, LAST_MOL = 7, 3, 1, 4
SLOTS = {0: (0, 63, 64, -1), 2: (0, 255, 256, -1), 4: (0, -1)}  # dirty positions of the scattered placement; -1: the last atom
PLACEMENTS = ("scattered", "tail", "call_tail")
GEOMETRIES = {"d16": dict(D=16, res=0.5, blockdim=None, sigma=0.5), "d20": dict(D=20, res=0.4, blockdim=5, sigma=0.3)}

# id: mode, radii type, C, grid kind, placement, pose ("posed" | "centred" | the seed of a random rotation), density, geometry
ROWS = {
    "feat-scalar-f32-scattered-posed": ("features", "scalar", 5, "f32", "scattered", "posed", "gaussian", "d16"),
    "feat-atom-bf16-tail-posed": ("features", "atom-wise", 33, "bf16", "tail", "posed", "gaussian", "d16"),
    "feat-chan-f64-call_tail-posed": ("features", "channel-wise", 5, "f64", "call_tail", "posed", "gaussian", "d16"),
    "feat-chan-f32-scattered-centred": ("features", "channel-wise", 5, "f32", "scattered", "centred", "gaussian", "d16"),
    "types-scalar-f32-scattered-rot": ("types", "scalar", 5, "f32", "scattered", 4242, "gaussian", "d16"),
    "types-atom-f32-tail-posed": ("types", "atom-wise", 33, "f32", "tail", "posed", "gaussian", "d16"),
    "types-atom-f64-scattered-posed": ("types", "atom-wise", 5, "f64", "scattered", "posed", "gaussian", "d16"),
    "types-bytype-bf16-scattered-posed": ("types", "channel-wise", 5, "bf16", "scattered", "posed", "gaussian", "d16"),
    "types-bytype-f32-call_tail-centred": ("types", "channel-wise", 5, "f32", "call_tail", "centred", "gaussian", "d16"),
    "single-atom-f64-scattered-posed": ("single", "atom-wise", 1, "f64", "scattered", "posed", "gaussian", "d16"),
    "single-scalar-f32-call_tail-centred": ("single", "scalar", 1, "f32", "call_tail", "centred", "gaussian", "d16"),
    "feat-atom-f32-scattered-centred": ("features", "atom-wise", 33, "f32", "scattered", "centred", "gaussian", "d16"),
    "feat-atom-f32-call_tail-posed": ("features", "atom-wise", 5, "f32", "call_tail", "posed", "gaussian", "d16"),
    "feat-scalar-f32-tail-centred": ("features", "scalar", 33, "f32", "tail", "centred", "gaussian", "d16"),
    "types-atom-f32-scattered-binary": ("types", "atom-wise", 5, "f32", "scattered", "posed", "binary", "d16"),
    "feat-atom-f32-scattered-d20": ("features", "atom-wise", 5, "f32", "scattered", "posed", "gaussian", "d20"),
    "types-scalar-f64-tail-d20": ("types", "scalar", 5, "f64", "tail", 77, "gaussian", "d20"),
}
ROW_IDS = list(ROWS)


def dead_types(C_):
    return {"type -1": -1, "type C": C_, "type C + 2": C_ + 2}


def kinds_of(mode, radii_type, C_):
    """The names of the dead kinds that apply to a mode and radii type, in the order the slots take them."""
    out = list(DEAD_COORDS)
    if radii_type == "atom-wise":
        out += list(DEAD_RADII)
    if mode == "types" and radii_type in ("scalar", "atom-wise"):
        out += list(dead_types(C_))
    return out


def _live_channels(rng, mode, n, C_, fp):
    if mode == "features":
        f = rng.random((n, C_)) + 0.05
        f[rng.random((n, C_)) < 0.3] = 0.0
        f[rng.random((n, C_)) < 0.3] *= -1.0
        if n:
            f[0] = np.abs(f[0]) + 0.05  # (every channel has a live atom)
        return f.astype(fp)
    if mode == "types":
        ty = rng.integers(0, C_, n)
        ty[:min(n, C_)] = np.arange(min(n, C_))
        return ty
    return None


def _dead_atom(rng, kind, mode, radii_type, C_, fp, res, near):
    """(xyz (3,), channel row | type | None, atom-wise radius | None) of one dead atom of `kind`; `near`: a point well inside the
    box of the atom's molecule (its centre), around which the atoms with a dead radius or type sit."""
    xyz = near + rng.uniform(-0.3, 0.3, 3)
    chan = None
    if mode == "features":
        chan = (rng.random(C_) + 0.5).astype(fp)
    elif mode == "types":
        chan = int(rng.integers(0, C_))
    radius = fp(rng.uniform(1.6, 3.0) * res) if radii_type == "atom-wise" else None
    if kind in DEAD_COORDS:
        xyz = np.array(DEAD_COORDS[kind])
    elif kind in DEAD_RADII:
        radius = fp(DEAD_RADII[kind])
    else:
        chan = dead_types(C_)[kind]
    return xyz, chan, radius


def _stack(rows, mode, radii_type, C_, fp):
    """Arrays (xyz, chan, radii) of a list of (xyz, chan, radius) atoms."""
    n = len(rows)
    xyz = np.array([r[0] for r in rows], np.float64).reshape(n, 3)
    chan = None
    if mode == "features":
        chan = np.array([r[1] for r in rows], fp).reshape(n, C_)
    elif mode == "types":
        chan = np.array([r[1] for r in rows], np.int64).reshape(n)
    radii = np.array([r[2] for r in rows], fp).reshape(n) if radii_type == "atom-wise" else None
    return xyz, chan, radii


def _splice(nl, slots):
    """Mask over nl + len(slots) atoms, True where a live atom stands; slots: dirty positions of the dead ones (-1: last)."""
    n = nl + len(slots)
    m = np.ones(n, bool)
    m[[s % n for s in slots]] = False
    assert int(m.sum()) == nl
    return m


@functools.lru_cache(maxsize=None)
def row(row_id: str) -> dict:
    mode, radii_type, C_, kind, placement, pose, density, geometry = ROWS[row_id]
    g = GEOMETRIES[geometry]
    D, res = g["D"], g["res"]
    rng = np.random.default_rng(70_000 + ROW_IDS.index(row_id))
    fp = np.float64 if kind == "f64" else np.float32
    B = len(LIVE)
    assert B * C_ * D ** 3 <= WALK_ELEMENTS
    half = res * (D - 1) / 2.0
    posed = pose == "posed"
    cen = CEN + rng.integers(-16, 17, (B, 3)) / 8.0
    q = rng.standard_normal((B, 4))
    norms = np.array([NORMS[b % 3] for b in range(B)])
    q *= (norms / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    if not posed:
        q, t, norms = np.tile([1.0, 0.0, 0.0, 0.0], (B, 1)), np.zeros((B, 3)), np.ones(B)
    if radii_type == "scalar":
        radii = float(np.float32(2.0 * res))  # (a float32 value: tests/density_reference.py's scalar-radius reference needs one)
    elif radii_type == "channel-wise":
        radii = (rng.uniform(1.6, 3.0, C_) * res).astype(fp)
    kinds = kinds_of(mode, radii_type, C_)
    live_parts, dead_parts, names, turn = [], [], [], 0
    for b, nl in enumerate(LIVE):
        ext = 0.45 * half / norms[b] ** 2  # the posed atoms stay in the box, and no atom reaches its outermost voxels
        xyz = cen[b] + rng.uniform(-ext, ext, (nl, 3))
        r = (rng.uniform(1.6, 3.0, nl) * res).astype(fp) if radii_type == "atom-wise" else None
        live_parts.append((xyz, _live_channels(rng, mode, nl, C_, fp), r))
        nd = len(SLOTS[b]) if b in SLOTS else (ALL_DEAD if b == ALL_DEAD_MOL else 0)
        mine = [kinds[(turn + i) % len(kinds)] for i in range(nd)]
        turn += nd
        dead_parts.append(_stack([_dead_atom(rng, k, mode, radii_type, C_, fp, res, cen[b]) for k in mine], mode, radii_type, C_, fp))
        names.append(mine)

    def cat(parts, i):
        return None if parts[0][i] is None else np.concatenate([p[i] for p in parts])

    mols, masks, dead_names = [], [], []
    for b, nl in enumerate(LIVE):
        if placement == "call_tail":
            mine = dead_parts if b == LAST_MOL else []
            dead = tuple(cat(mine, i) for i in range(3)) if mine else _stack([], mode, radii_type, C_, fp)
            my_names = [k for m in range(B) for k in names[m]] if b == LAST_MOL else []
        else:
            dead, my_names = dead_parts[b], names[b]
        nd = dead[0].shape[0]
        if placement == "scattered" and b in SLOTS:
            mask = _splice(nl, SLOTS[b])
        else:
            mask = np.concatenate([np.ones(nl, bool), np.zeros(nd, bool)])
        parts = []
        for i in range(3):
            if live_parts[b][i] is None:
                parts.append(None)
                continue
            a = np.empty((nl + nd,) + live_parts[b][i].shape[1:], live_parts[b][i].dtype)
            a[mask], a[~mask] = live_parts[b][i], dead[i]
            parts.append(a)
        mols.append(tuple(parts))
        masks.append(mask)
        dead_names.append(my_names)
    live_mask = np.concatenate(masks)
    sizes = tuple(int(m.shape[0]) for m in masks)
    kind_of = np.full(live_mask.shape[0], "", dtype=object)
    kind_of[~live_mask] = [k for m in dead_names for k in m]
    return _freeze(dict(id=row_id, mode=mode, radii_type=radii_type, C=C_, kind=kind, precision=64 if kind == "f64" else 32,
                        placement=placement, pose=pose, posed=posed, density=density, B=B, cen=cen, q=q, t=t, live=live_mask,
                        sizes=sizes, xyz=cat(mols, 0), chan=cat(mols, 1),
                        radii=cat(mols, 2) if radii_type == "atom-wise" else radii, dead_kind=kind_of,
                        fseed=90_000 + ROW_IDS.index(row_id), per_mol=ROW_IDS.index(row_id) % 4 == 1, **g))


def live(r: dict) -> np.ndarray:
    """(N_dirty,) bool: True for the atoms of the clean batch, in its order."""
    return r["live"]


def _draw(r, keep):
    sizes = tuple(int(keep[lo:lo + n].sum()) for lo, n in zip(np.concatenate([[0], np.cumsum(r["sizes"])]), r["sizes"]))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    atomwise = r["radii_type"] == "atom-wise"
    radii = r["radii"][keep] if atomwise else r["radii"]
    chan = None if r["chan"] is None else r["chan"][keep]
    N = int(off[-1])
    if atomwise:
        r_atom = radii.astype(np.float64)
    elif r["radii_type"] == "scalar":
        r_atom = np.full(N, float(np.float32(radii) if r["precision"] == 32 else radii))
    else:
        r_atom = radii[chan].astype(np.float64) if r["mode"] == "types" else None
    d = dict(seed=r["id"], D=r["D"], res=r["res"], sigma=r["sigma"], blockdim=r["blockdim"], density=r["density"], mode=r["mode"],
             radii_type=r["radii_type"], C=r["C"], kind=r["kind"], precision=r["precision"], per_mol=r["per_mol"], posed=r["posed"],
             B=r["B"], N=N, sizes=sizes, off=off, cen=r["cen"], q=r["q"], t=r["t"], xyz=r["xyz"][keep], chan=chan, radii=radii,
             r_atom=r_atom, tie_mols=(), ties=(), bad_types=(), fseed=r["fseed"], placement=r["placement"],
             sample=[list(range(int(off[b]), int(off[b + 1]))) for b in range(r["B"])])
    if r["pose"] != "centred":
        d["transform"] = r["pose"]
    return _freeze(d)


def dirty(r: dict) -> dict:
    """The batch with the dead atoms, as a draw of tests/entry_fuzz_rows.py."""
    return _draw(r, np.ones(r["live"].shape[0], bool))


def clean(r: dict) -> dict:
    """The same batch with the dead atoms deleted and the offsets moved up."""
    return _draw(r, r["live"])


def weights_of(d: dict) -> np.ndarray:
    """The weight rows w[n, c] of every atom: the feature row, onehot(type) (zeros for a type outside [0, C)), or 1 - the form in
    which the oracles take every mode."""
    fp = np.float64 if d["precision"] == 64 else np.float32
    if d["mode"] == "features":
        return d["chan"]
    if d["mode"] == "single":
        return np.ones((d["N"], 1), fp)
    w = np.zeros((d["N"], d["C"]), fp)
    ok = (d["chan"] >= 0) & (d["chan"] < d["C"])
    w[np.nonzero(ok)[0], d["chan"][ok]] = 1.0
    return w


def positions_of(d: dict) -> np.ndarray:
    """(N, 3) float64: the atoms as the kernels see them; non-finite where a dead coordinate makes them so."""
    from tests import entry_fuzz_rows as E

    with np.errstate(all="ignore"):
        return E.positions_of(d)


def oracle_grid(d: dict, p: np.ndarray, b: int, xyz=None, w=None, r_atom=None) -> np.ndarray:
    """The oracle's grid (C, D, D, D) of molecule b at the positions p (oracle/c_oracle, or oracle/numpy_port at precision 64);
    xyz / w / r_atom: replacements for the molecule's positions, weight rows and per-atom radii (the mutated references)."""
    from oracle import c_oracle, numpy_port

    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    fp = np.float64 if d["precision"] == 64 else np.float32
    if hi == lo:
        return np.zeros((d["C"],) + (d["D"],) * 3, fp)
    pos = p[lo:hi] if xyz is None else xyz
    chan = weights_of(d)[lo:hi] if w is None else w
    if d["mode"] == "single":
        chan = None
    if r_atom is not None:
        radii, rt = r_atom.astype(fp), "atom-wise"
    elif d["radii_type"] == "scalar":
        radii, rt = d["radii"], "scalar"
    elif d["radii_type"] == "channel-wise" and d["mode"] == "features":
        radii, rt = d["radii"], "channel-wise"
    else:
        radii, rt = d["r_atom"][lo:hi].astype(fp), "atom-wise"
    with np.errstate(all="ignore"):
        if d["precision"] == 32:
            return c_oracle.voxelize(pos, chan, radii, resolution=d["res"], dimension=d["D"], blockdim=d["blockdim"], radii_type=rt,
                                     density=d["density"], sigma=d["sigma"])
        spec = numpy_port.GridSpec(d["res"], d["D"], d["blockdim"])
        return numpy_port.voxelize(spec, pos, chan, radii, radii_type=rt, density=d["density"], sigma=d["sigma"], precision=64)


# ---- one shared cloud under B poses ------------------------------------------------------------------------------------------------
CLOUD_LIVE, CLOUD_VIEWS = 300, 3
CLOUD_SLOTS = (0, 1, 63, 64, 100, 101, 102, 200, 201, 255, 256, 257, 300, -2, -1)
# id: mode, radii type, C, grid kind
CLOUDS = {"cloud-feat-scalar": ("features", "scalar", 5, "f32"), "cloud-types-atom": ("types", "atom-wise", 5, "f32"),
          "cloud-feat-chan-f64": ("features", "channel-wise", 5, "f64"), "cloud-single-atom-bf16": ("single", "atom-wise", 1, "bf16")}
CLOUD_IDS = list(CLOUDS)


@functools.lru_cache(maxsize=None)
def cloud(cloud_id: str) -> dict:
    """A shared cloud wider than the box (so the cull keeps some live atoms and drops some) with dead atoms at CLOUD_SLOTS, and
    three poses whose centres lie inside it. dirty_cloud / clean_cloud give the two clouds."""
    mode, radii_type, C_, kind = CLOUDS[cloud_id]
    g = GEOMETRIES["d16"]
    rng = np.random.default_rng(80_000 + CLOUD_IDS.index(cloud_id))
    fp = np.float64 if kind == "f64" else np.float32
    B, nl = CLOUD_VIEWS, CLOUD_LIVE
    cen = CEN + rng.integers(-16, 17, (B, 3)) / 8.0
    q = rng.standard_normal((B, 4))
    q *= (np.array(NORMS) / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    radii = 2.0 * g["res"] if radii_type == "scalar" else (rng.uniform(1.6, 3.0, C_) * g["res"]).astype(fp)
    xyz = CEN + rng.uniform(-6.0, 6.0, (nl, 3))
    lr = (rng.uniform(1.6, 3.0, nl) * g["res"]).astype(fp) if radii_type == "atom-wise" else None
    live_part = (xyz, _live_channels(rng, mode, nl, C_, fp), lr)
    kinds = kinds_of(mode, radii_type, C_)
    names = [kinds[i % len(kinds)] for i in range(len(CLOUD_SLOTS))]
    dead = _stack([_dead_atom(rng, k, mode, radii_type, C_, fp, g["res"], CEN) for k in names], mode, radii_type, C_, fp)
    mask = _splice(nl, CLOUD_SLOTS)
    parts = []
    for i in range(3):
        if live_part[i] is None:
            parts.append(None)
            continue
        a = np.empty((mask.shape[0],) + live_part[i].shape[1:], live_part[i].dtype)
        a[mask], a[~mask] = live_part[i], dead[i]
        parts.append(a)
    kind_of = np.full(mask.shape[0], "", dtype=object)
    kind_of[~mask] = names
    return _freeze(dict(id=cloud_id, mode=mode, radii_type=radii_type, C=C_, kind=kind, precision=64 if kind == "f64" else 32,
                        density="gaussian", B=B, cen=cen, q=q, t=t, live=mask, xyz=parts[0], chan=parts[1],
                        radii=parts[2] if radii_type == "atom-wise" else radii, dead_kind=kind_of,
                        fseed=95_000 + CLOUD_IDS.index(cloud_id), **g))


def _cloud(c, keep):
    atomwise = c["radii_type"] == "atom-wise"
    d = {k: c[k] for k in ("id", "mode", "radii_type", "C", "kind", "precision", "density", "B", "cen", "q", "t", "D", "res", "sigma",
                           "blockdim", "fseed")}
    d.update(seed=c["id"], per_mol=False, posed=True, xyz=c["xyz"][keep], chan=None if c["chan"] is None else c["chan"][keep], radii=c["radii"][keep] if atomwise else c["radii"],
             N=int(keep.sum()))
    return _freeze(d)


def dirty_cloud(c: dict) -> dict:
    return _cloud(c, np.ones(c["live"].shape[0], bool))


def clean_cloud(c: dict) -> dict:
    return _cloud(c, c["live"])


def repeated(c: dict) -> dict:
    """The batch of B copies of a cloud (dirty_cloud / clean_cloud) under its B poses, as a posed draw."""
    B, N = c["B"], c["N"]
    rep = lambda x: None if x is None else np.concatenate([x] * B)  # noqa: E731
    atomwise = c["radii_type"] == "atom-wise"
    d = dict(c, xyz=rep(c["xyz"]), chan=rep(c["chan"]), radii=rep(c["radii"]) if atomwise else c["radii"], N=B * N,
             sizes=(N,) * B, off=np.arange(B + 1, dtype=np.int64) * N, transform="posed", tie_mols=(),
             ties=(), bad_types=(), sample=[list(range(b * N, (b + 1) * N)) for b in range(B)])
    return _freeze(d)


def view_source(c: dict) -> str:
    """The radii source name of tests/views_reference.py for a cloud."""
    if c["radii_type"] == "channel-wise":
        return "by-type" if c["mode"] == "types" else "channel-features"
    return c["radii_type"]
