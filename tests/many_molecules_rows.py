"""Shapes and case builders of tests/test_hip_many_molecules.py (GPU) and tests/test_many_molecules_host.py (host): the
differentiable entries (mvx_backward_batch, mvx_backward_radii_batch, mvx_backward_density_batch, mvx_score_batch,
mvx_pose_grad_batch) and the device-pose path of the forward on batches of many molecules.

What only does real work when B is large: pose_resolve_kernel (one thread per record, workgroups of 64: the partly filled last
workgroup and the early return for plain records), find_molecule (a binary search over the offsets, through runs of empty
molecules), the address of a molecule's upstream gradient or field, the per-molecule reductions (score_reduce_kernel,
pose_grad_kernel: 4 waves, stride 256) and the spatial order ("grad_order" 1). Every row names a batch that is built here from
a seed, so that the host module can hold the references to conditions (the sample touches what it claims, the reference is
non-zero there) without a GPU, and the GPU module reads the same arrays.

Sections: A the ladder batch (B = 203 = 3 x 64 + 11), B tiny totals under the spatial order, C B = 70 001, D upstream
gradients and fields past 2^31 and 2^32 elements, E posed forward calls cut into several launches.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass

import numpy as np

from tests import batch_cut_rows as R
from tests import grad_reference as gr
from tests import pose_reference as pr
from tests import score_reference as sr

CEN = np.array([30.0, -20.0, 12.0])
NORMS = np.array([1.0, 0.8, 1.25])
RES = 0.5

# ---- A. the ladder batch ------------------------------------------------------------------------------------------------------------
B_LADDER = 203  # 3 * 64 + 11: pose_resolve_kernel runs four workgroups, the last holds 11 records
D_LADDER = 12
LADDER = [0, 1, 63, 64, 65, 0, 0, 255, 256, 257, 5, 300, 511, 512, 513, 2, 0]
THIN_LADDER = [0, 1, 2, 5, 63, 64, 65, 0, 0, 7]  # call-wide sums: the reference reads every atom
CUTS = (0, 1, 3, 64, 65, 130, 203)  # the six pieces of the bit comparison (sizes 1 and 2 among them)
FIXED_MOLECULES = (63, 64, 65, 127, 128, 191, 192)
ATOM_MARKS = (63, 64, 65, 255, 256, 257, 511, 512)  # atoms of a long molecule that are always in the sample
MAX_WHOLE = 65  # molecules up to this size are sampled whole


def ladder_sizes(ladder, B=B_LADDER) -> tuple:
    """sizes[b] = ladder[b % len(ladder)], the last molecule forced empty."""
    sizes = [int(ladder[b % len(ladder)]) for b in range(B)]
    sizes[-1] = 0
    return tuple(sizes)


def empty_runs(sizes) -> list:
    """[first, last] of every maximal run of molecules without atoms."""
    runs, b, B = [], 0, len(sizes)
    while b < B:
        if sizes[b] == 0:
            e = b
            while e + 1 < B and sizes[e + 1] == 0:
                e += 1
            runs.append((b, e))
            b = e + 1
        else:
            b += 1
    return runs


def whole_molecules(sizes) -> list:
    """The first molecule of every distinct non-zero size: molecule scores and pose rows need all atoms of a molecule."""
    seen, out = set(), []
    for b, n in enumerate(sizes):
        if n > 0 and n not in seen:
            seen.add(n)
            out.append(b)
    return out


def sample_molecules(sizes) -> list:
    """Every index next to a run of empties, FIXED_MOLECULES, the first and last non-empty molecule, one of every size."""
    B = len(sizes)
    picks = set(FIXED_MOLECULES) | set(whole_molecules(sizes))
    for lo, hi in empty_runs(sizes):
        picks |= {lo - 1, hi + 1}
    full = [b for b in range(B) if sizes[b] > 0]
    picks |= {full[0], full[-1]}
    return sorted(b for b in picks if 0 <= b < B and sizes[b] > 0)


def sample_atoms(n: int) -> np.ndarray:
    """Atoms of a molecule of n atoms (indices inside the molecule): all of them up to MAX_WHOLE, otherwise the first three,
    the last three and ATOM_MARKS where present."""
    if n <= MAX_WHOLE:
        return np.arange(n, dtype=np.int64)
    picks = {0, 1, 2, n - 3, n - 2, n - 1} | {a for a in ATOM_MARKS if a < n}
    return np.array(sorted(picks), dtype=np.int64)


@dataclass(frozen=True)
class Row:
    id: str
    entry: str  # backward | backward_radii | score | pose | forward | density
    mode: str
    C: int
    radii: str
    density: str = "gaussian"
    kind: str = "f32"  # f32 | bf16 | f64: the grid type (upstream gradient, field)
    transform: str = "pose"  # pose | rotation | none
    per_mol: bool = True  # score: a field per molecule (else one shared field)
    beyond: bool = False  # types mode: one type past the channels of the call
    device_pose: bool = True  # forward: the poses as a device block (else numpy arrays)
    ladder: str = "ladder"  # ladder | thin


ROWS = [
    Row("backward-feat33-scalar-f32-pose", "backward", "features", 33, "scalar"),
    Row("backward-feat33-chan-bf16-rot", "backward", "features", 33, "channel-wise", kind="bf16", transform="rotation"),
    Row("backward-types5-atom-f64-pose", "backward", "types", 5, "atom-wise", kind="f64", beyond=True),
    Row("backward-single-scalar-binary-f32-none", "backward", "single", 1, "scalar", density="binary", transform="none"),
    Row("radii-feat5-atom-f32-pose", "backward_radii", "features", 5, "atom-wise"),
    Row("score-shared-feat33-chan-f32-pose", "score", "features", 33, "channel-wise", per_mol=False),
    Row("score-permol-types5-atom-binary-bf16-rot", "score", "types", 5, "atom-wise", density="binary", kind="bf16",
        transform="rotation", beyond=True),
    Row("score-permol-single-scalar-f64-pose", "score", "single", 1, "scalar", kind="f64"),
    Row("pose-feat4-scalar-f32", "pose", "features", 4, "scalar"),
    Row("pose-feat4-scalar-f64", "pose", "features", 4, "scalar", kind="f64"),
    Row("forward-feat33-device-pose", "forward", "features", 33, "scalar"),
    Row("forward-feat33-numpy-pose", "forward", "features", 33, "scalar", device_pose=False),
    Row("forward-types4-device-pose", "forward", "types", 4, "scalar"),
    Row("forward-types4-numpy-pose", "forward", "types", 4, "scalar", device_pose=False),
]
# call-wide sums (dL/dsigma, dL/d(scalar radius), channel-wise dL/dradii) on the thin ladder
SUM_ROWS = [
    Row("sums-feat4-scalar-sigma-f32", "density", "features", 4, "scalar", ladder="thin"),
    Row("sums-feat33-chan-sigma-f64", "density", "features", 33, "channel-wise", kind="f64", ladder="thin"),
    Row("sums-types5-bytype-f32", "backward_radii", "types", 5, "channel-wise", ladder="thin"),
]
ROW_IDS = [r.id for r in ROWS]
SUM_IDS = [r.id for r in SUM_ROWS]
GRAD_ROWS = [r for r in ROWS if r.entry != "forward"]
GRAD_IDS = [r.id for r in GRAD_ROWS]
FORWARD_ROWS = [r for r in ROWS if r.entry == "forward"]
FORWARD_IDS = [r.id for r in FORWARD_ROWS]
assert len(set(ROW_IDS + SUM_IDS)) == len(ROW_IDS) + len(SUM_IDS)


# ---- records -------------------------------------------------------------------------------------------------------------------------
# mvx_xform (include/mvx.h) as a numpy record: 70 001 records are filled with array operations, not one ctypes store each
XF = np.dtype({"names": ["center", "quat", "trans", "flags", "center_ptr"], "formats": [("<f8", 3), ("<f8", 4), ("<f4", 3), "<u4", "<u8"],
               "offsets": [0, 24, 56, 68, 72], "itemsize": 80})
XF_CENTER, XF_ROTATE, XF_TRANSLATE, XF_POSE_PTR, XF_TRANSLATE_ONCE = 1, 2, 4, 32, 64


def records(d, lo, hi, how, pose_ptr=0, plain_every=0):
    """The records of molecules [lo, hi). how "pose": MVX_XF_POSE_PTR records pointing at rows lo ... of the packed (B, 10)
    poses at device address pose_ptr (row 0 of the batch); "resolved": the plain records pose_to_record writes for them
    (CENTER | ROTATE | TRANSLATE | TRANSLATE_ONCE, the translation rounded to float32); "rotation": CENTER | ROTATE from the
    host centre and quaternion. plain_every = k: every k-th molecule of the batch (b % k == k - 1) gets a "rotation" record
    whatever `how` says (a mixed array)."""
    xf = np.zeros(hi - lo, XF)
    b = np.arange(lo, hi)
    plain = np.zeros(hi - lo, bool) if not plain_every else (b % plain_every == plain_every - 1)
    if how == "rotation":
        plain[:] = True
    xf["center"], xf["quat"] = d["cen"][lo:hi], d["q"][lo:hi]
    xf["flags"] = XF_CENTER | XF_ROTATE
    if how == "resolved":
        xf["trans"][~plain] = d["t"][lo:hi][~plain].astype(np.float32)
        xf["flags"][~plain] = XF_CENTER | XF_ROTATE | XF_TRANSLATE | XF_TRANSLATE_ONCE
    elif how == "pose":
        assert pose_ptr
        xf["center"][~plain], xf["quat"][~plain] = 0.0, 0.0
        xf["flags"][~plain] = XF_POSE_PTR
        xf["center_ptr"][~plain] = (pose_ptr + 80 * b)[~plain].astype(np.uint64)
    return xf


def seed_of(name: str) -> int:
    return zlib.crc32(name.encode())


def precision_of(kind: str) -> int:
    return 64 if kind == "f64" else 32


def make_batch(seed, sizes, D, C_, mode, radii_type, kind="f32", transform="pose", beyond=False, spread=0.4) -> dict:
    """One batch (host arrays, never modified): offsets, centres around CEN, atoms uniform within +-spread W of their centre, the
    first atom of every molecule of two or more atoms far outside the box, poses with |q| cycling through NORMS (transform
    "pose"), unit quaternions and no translation ("rotation") or coordinates already centred ("none"). Channels, coordinates and
    radii are random per molecule: a row computed from another molecule's data cannot pass. `xyz` is what the call is given."""
    rng = np.random.default_rng(seed)
    fp = np.float64 if kind == "f64" else np.float32
    sizes = np.asarray(sizes, np.int64)
    B, N = len(sizes), int(sizes.sum())
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    mol = np.repeat(np.arange(B), sizes)
    W = RES * (D - 1)
    cen = CEN + rng.normal(0.0, 0.4, (B, 3))
    xyz = cen[mol] + rng.uniform(-spread * W, spread * W, (N, 3))
    outside = off[:-1][sizes >= 2]
    xyz[outside] += [100.0, -80.0, 90.0]  # (far outside under every pose: |q|^2 >= 0.64)
    q = rng.standard_normal((B, 4))
    norms = NORMS[np.arange(B) % 3] if transform == "pose" else np.ones(B)
    q *= (norms / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3)) if transform == "pose" else np.zeros((B, 3))
    if transform == "none":
        xyz = xyz - cen[mol]
        cen, q = np.zeros((B, 3)), np.tile([1.0, 0.0, 0.0, 0.0], (B, 1))
    types = rng.integers(0, C_ + (1 if beyond else 0), N)  # (beyond: type C_ lies past the channels of the call)
    chan = {"features": rng.standard_normal((N, C_)).astype(fp), "types": types, "single": None}[mode]
    radii = {"scalar": 1.25, "atom-wise": rng.uniform(1.0, 1.5, N).astype(fp), "channel-wise": rng.uniform(1.0, 1.5, C_).astype(fp)}[radii_type]
    return dict(off=off, cen=cen, xyz=xyz, q=q, t=t, chan=chan, radii=radii, B=B, N=N, outside=outside, mode=mode, C=C_, D=D,
                radii_type=radii_type, kind=kind, transform=transform, sizes=sizes, seed=seed)


@functools.lru_cache(maxsize=None)
def row_batch(row: Row) -> dict:
    sizes = ladder_sizes(LADDER if row.ladder == "ladder" else THIN_LADDER)
    return make_batch(seed_of(row.id), sizes, D_LADDER, row.C, row.mode, row.radii, row.kind, row.transform, row.beyond)


def positions(d, lo=0, hi=None) -> np.ndarray:
    """The atoms of molecules [lo, hi) as the kernels see them (tests/pose_reference.py; "none": the coordinates themselves)."""
    hi = d["B"] if hi is None else hi
    a0, a1 = int(d["off"][lo]), int(d["off"][hi])
    if d["transform"] == "none":
        return d["xyz"][a0:a1].copy()
    return pr.batch_positions(d["xyz"][a0:a1], d["off"][lo:hi + 1] - a0, d["cen"][lo:hi], d["q"][lo:hi], d["t"][lo:hi])


def as_read(x, kind: str) -> np.ndarray:
    """A float64 array rounded to the grid type `kind` and widened again: what the kernel reads of an upstream or a field."""
    if kind == "f64":
        return np.asarray(x, np.float64)
    if kind == "f32":
        return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    import torch

    return torch.as_tensor(np.asarray(x, np.float64)).to(torch.bfloat16).to(torch.float64).numpy()


def field_of(d, b, shared=False) -> np.ndarray:
    """(C, D, D, D) float64: molecule b's upstream gradient or field in the batch's grid type, widened (b is ignored for the one
    shared field). Drawn per molecule from (seed, b): a sample of molecules does not need the other 200 fields."""
    rng = np.random.default_rng([d["seed"], 0 if shared else b + 1])
    return as_read(rng.standard_normal((d["C"],) + (d["D"],) * 3), d["kind"])


def all_fields(d, shared=False) -> np.ndarray:
    """(B, C, D, D, D), or (C, D, D, D) shared: field_of stacked for the device."""
    if shared:
        return field_of(d, 0, True)
    return np.stack([field_of(d, b) for b in range(d["B"])])


def _molecule(d, b):
    lo, hi = int(d["off"][b]), int(d["off"][b + 1])
    radii = d["radii"][lo:hi] if d["radii_type"] == "atom-wise" else d["radii"]
    chan = None if d["chan"] is None else d["chan"][lo:hi]
    return lo, hi, radii, chan


def grad_rows(d, b, G, density, atoms=None, by_type=False) -> dict:
    """grad_reference.reference of molecule b for the upstream G on the atoms `atoms` (inside the molecule; None: all). The
    coordinate rows are dL/dcoords = M^T dL/dp (M scales by |q|^2); "p" holds dL/dp for the pose chain rule."""
    lo, hi, radii, chan = _molecule(d, b)
    p = positions(d, b, b + 1)
    M = None if d["transform"] == "none" else pr.rotation(d["q"][b])
    o = gr.reference(p, G, radii, d["radii_type"], w=chan if d["mode"] == "features" else None, mode=d["mode"],
                     types=chan if d["mode"] == "types" else None, density=density, precision=precision_of(d["kind"]),
                     atoms=atoms, radii_by_type=by_type)
    gp, bp = o["coords"]
    o["p"] = (gp, bp)
    if M is not None:
        o["coords"] = (gp @ M, bp @ np.abs(M))
    return o


def score_rows(d, b, F, density, atoms=None):
    """score_reference of molecule b on the atoms `atoms` (an atom's score depends on nothing but the atom): (s, bound, S, its
    bound); S is the molecule's score only with atoms=None."""
    lo, hi, radii, chan = _molecule(d, b)
    p = positions(d, b, b + 1)
    sel = np.arange(hi - lo) if atoms is None else np.asarray(atoms, np.int64)
    r = radii[sel] if d["radii_type"] == "atom-wise" else radii
    return sr.score_reference(p[sel], F, r, d["radii_type"], w=chan[sel] if d["mode"] == "features" else None, mode=d["mode"],
                              types=chan[sel] if d["mode"] == "types" else None, density=density,
                              precision=precision_of(d["kind"]))


def pose_rows(d, b, G, density="gaussian") -> dict:
    """pose_reference.pose_grads of molecule b (all atoms) for the upstream G."""
    lo, hi, _, _ = _molecule(d, b)
    o = grad_rows(d, b, G, density)
    return pr.pose_grads(d["xyz"][lo:hi], d["cen"][b], d["q"][b], *o["p"])


@functools.lru_cache(maxsize=None)
def row_reference(row: Row) -> dict:
    """The float64 reference of a ladder row on its sample, computed once and shared by the host and the GPU module:
    {"atoms": {b: (atom indices inside b, reference dict)}, "whole": {b: ...}} per entry."""
    d = row_batch(row)
    sizes = d["sizes"]
    shared = row.entry == "score" and not row.per_mol
    out = {"atoms": {}, "whole": {}}
    whole = whole_molecules(sizes) if row.entry in ("score", "pose") else []
    for b in sample_molecules(sizes):
        G = field_of(d, b, shared)
        sel = sample_atoms(int(sizes[b]))
        if row.entry == "pose":
            continue
        if row.entry == "score":
            if b in whole:
                continue
            out["atoms"][b] = (sel, score_rows(d, b, G, row.density, sel))
        else:
            out["atoms"][b] = (sel, grad_rows(d, b, G, row.density, sel))
    for b in whole:
        G = field_of(d, b, shared)
        if row.entry == "score":
            s = score_rows(d, b, G, row.density)
            out["whole"][b] = s
            out["atoms"][b] = (np.arange(int(sizes[b])), s)
        else:
            out["whole"][b] = pose_rows(d, b, G, row.density)
    return out


@functools.lru_cache(maxsize=None)
def sum_reference(row: Row) -> dict:
    """The call-wide sums of a thin-ladder row over every atom of the call, as (value, bound) pairs: "sigma" and "radius"
    (scalar radii: tests/density_reference.py), "radii" (channel-wise: (C,)) and "sigma" from it by density_reference's identity
    sigma dL/dsigma = sum_c r_c dL/dr_c."""
    from tests import density_reference as dr

    d = row_batch(row)
    fp = np.float64 if row.kind == "f64" else np.float32
    tot = {}

    def add(k, g, b):
        tot[k] = (tot[k][0] + g, tot[k][1] + b) if k in tot else (g, b)

    for b in range(d["B"]):
        if d["sizes"][b] == 0:
            continue
        G = field_of(d, b)
        if row.radii == "scalar":
            lo, hi, radii, chan = _molecule(d, b)
            o = dr.density_grads(positions(d, b, b + 1), G, radii, "scalar", w=chan if row.mode == "features" else None,
                                 mode=row.mode, types=chan if row.mode == "types" else None, precision=precision_of(row.kind))
            for k, (g, bnd) in o.items():
                add(k, g, bnd)
        else:
            g, bnd = grad_rows(d, b, G, row.density, by_type=row.mode == "types")["radii"]
            add("radii", g, bnd)
    if "radii" in tot and row.entry == "density":
        rr = np.asarray(d["radii"]).astype(fp).astype(np.float64)
        tot["sigma"] = (float((tot["radii"][0] * rr).sum() / 0.5), float((tot["radii"][1] * rr).sum() / 0.5))
    return tot


# ---- B. tiny totals under the spatial order --------------------------------------------------------------------------------------
TINY_TOTALS = (1, 2, 3, 4, 5, 31, 32, 33)


def tiny_sizes(total: int) -> tuple:
    """Three molecules, the middle one empty."""
    first = total // 2
    return (first, 0, total - first)


@functools.lru_cache(maxsize=None)
def tiny_batch(total: int) -> dict:
    return make_batch(seed_of(f"tiny-{total}"), tiny_sizes(total), D_LADDER, 33, "features", "scalar", "f32", "pose")


# ---- C. past the block-count edges -------------------------------------------------------------------------------------------------
HUGE_B, HUGE_D, HUGE_C = 70001, 8, 4
HUGE_PICKS = (0, 1, 63, 64, 65534, 65535, 65536, 70000)
HUGE_WINDOWS = ((0, 64), (65472, 65600), (69937, 70001))


def huge_sizes() -> np.ndarray:
    return R.big_sizes(R.Big("many-molecules", HUGE_D, HUGE_C, HUGE_B, mode="types"))


def huge_molecules(sizes) -> list:
    """HUGE_PICKS and their nearest non-empty neighbours."""
    B, picks = len(sizes), set()
    for b in HUGE_PICKS:
        picks.add(b)
        for step in (-1, 1):
            n = b + step
            while 0 <= n < B and sizes[n] == 0:
                n += step
            if 0 <= n < B:
                picks.add(n)
    return sorted(picks)


@functools.lru_cache(maxsize=None)
def huge_batch(transform: str) -> dict:
    return make_batch(seed_of(f"huge-{transform}"), huge_sizes(), HUGE_D, HUGE_C, "types", "scalar", "f32", transform)


def huge_bytes() -> dict:
    """Bytes of every device array of section C's calls."""
    N = int(huge_sizes().sum())
    return dict(upstream=HUGE_B * HUGE_C * HUGE_D**3 * 4, coords=N * 24, grad_coords=N * 24, types=N * 4, poses=HUGE_B * 80,
                records=HUGE_B * 80, scores=HUGE_B * 8, pose_rows=HUGE_B * 80)


# ---- D. upstream gradients and fields past 2^31 and 2^32 elements -----------------------------------------------------------------
@dataclass(frozen=True)
class Wide:
    id: str
    kind: str
    B: int
    C: int = 32
    D: int = 64
    atoms: int = 6
    picks: tuple = (0, 127, 128, 255, 256)


WIDE = [Wide("bfloat16-B513", "bf16", 513, picks=(0, 127, 128, 255, 256, 511, 512)), Wide("float32-B257", "f32", 257)]
WIDE_IDS = [w.id for w in WIDE]


@functools.lru_cache(maxsize=None)
def wide_batch(case: Wide) -> dict:
    """Six atoms per molecule within +-0.2 W of the centre: under |q|^2 = 1.5625 and the translation they stay inside the box
    (0.2 * 31.5 * 1.5625 * sqrt(3) + 0.6 * sqrt(3) < 15.75 + 1.25 per axis holds with room), the first one far outside."""
    return make_batch(seed_of(case.id), (case.atoms,) * case.B, case.D, case.C, "features", "scalar", case.kind, "pose", spread=0.2)


# ---- E. posed forward calls cut into several launches -------------------------------------------------------------------------------
CUT_ROWS = [R.Row("posed-rem-C33", 32, 33, dict(R.WIDE, ncc=2, nfull=1, ct_rem=1), chunks=(3,)),
            R.Row("posed-narrow-types-C4", 32, 4, dict(route=R.BINNED, ct=4, ncc=1, nw=4), mode="types", chunks=(3,))]
CUT_IDS = [r.id for r in CUT_ROWS]
CUT_NCHUNKS = (2, 3, 16)
CUT_ORACLE_MOLECULES = (1, R.DENSE, 14)
VIEWS_ATOMS, VIEWS_POSES, VIEWS_NCHUNKS = 2200, 16, (2, 16)


@functools.lru_cache(maxsize=None)
def cut_batch(row_id: str) -> dict:
    """The 16 ragged molecules of tests/batch_cut_rows.py under explicit poses: the molecule's atoms around its centre (the
    pose's c), |q| cycling through NORMS, translations within +-0.6."""
    row = CUT_ROWS[CUT_IDS.index(row_id)]
    batch = R.make_batch(row)
    rng = np.random.default_rng(seed_of(row_id))
    sizes = np.asarray(batch["sizes"], np.int64)
    B = len(sizes)
    cen = CEN + batch["centers"]
    xyz = np.concatenate([c + cen[b] for b, c in enumerate(batch["coords"])])
    q = rng.standard_normal((B, 4))
    q *= (NORMS[np.arange(B) % 3] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    chan = {"features": np.concatenate(batch["feats"]), "types": np.concatenate(batch["types"]).astype(np.int64)}[row.mode]
    mol = np.repeat(np.arange(B), sizes)
    return dict(off=batch["offsets"], cen=cen, xyz=xyz, mirror=2.0 * cen[mol] - xyz, q=q, t=t, chan=chan, radii=R.SCALAR_RADIUS,
                B=B, N=int(sizes.sum()), sizes=sizes, mode=row.mode, C=row.C, D=row.D, transform="pose")


def cut_budgets(row) -> dict:
    """{nchunk: "mall_budget_kb" value} for CUT_NCHUNKS on the row's batch."""
    sizes = R.RAGGED_SIZES
    p = R.host_plan(row, sizes)
    return {n: R.budget_for(p, len(sizes), row.C, int(sum(sizes)), n) for n in CUT_NCHUNKS}


@functools.lru_cache(maxsize=None)
def views_cloud() -> dict:
    """One cloud of VIEWS_ATOMS atoms wider than the box and VIEWS_POSES poses whose centres lie inside it."""
    rng = np.random.default_rng(seed_of("posed-views"))
    N, B = VIEWS_ATOMS, VIEWS_POSES
    xyz = CEN + rng.uniform(-10.0, 10.0, (N, 3))
    cen = CEN + rng.uniform(-3.0, 3.0, (B, 3))
    q = rng.standard_normal((B, 4))
    q *= (NORMS[np.arange(B) % 3] / np.linalg.norm(q, axis=1))[:, None]
    t = rng.uniform(-0.6, 0.6, (B, 3))
    return dict(xyz=xyz, cen=cen, q=q, t=t, chan=rng.standard_normal((N, 33)).astype(np.float32), N=N, B=B, C=33, D=32)
