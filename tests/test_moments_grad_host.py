"""Host half of tests/test_hip_moments_grad.py: no GPU, nothing is launched.

* the C ABI entry mvx_moments_backward_batch: its rejections and their order
  up to the rules that read the handle (those need a real one: tests/test_hip_moments_grad.py);
* the constructor option moments_grad and what a moments call on such a voxelizer refuses before the library is needed;
* the registers of the eight moments_grad_kernel instantiations read from mvx_moments_grad.o, against grad_kernel's for the same key;
* the composition the GPU tests use as their reference: the float64 upstream G = a0 + a1 g + a2 t fed to
  tests/grad_reference.reference equals finite differences of the exact moments (tests/moments_reference.moments_of).
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import grad_reference as GR
from tests import moments_grad_reference as MG
from tests import moments_reference as MR
from tests.abi import MVX_ERR_INVALID, P, call, declarations, records
from tests.fake_voxelizer import fake as _fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 31
POSE = _lib.MVX_XF_POSE_PTR
ENTRY = "mvx_moments_backward_batch"


# ---- the C ABI entry ---------------------------------------------------------------------------------------------------------
def test_the_entry_begins_like_moments_batch_and_keeps_its_pointee_types():
    # the first eleven are mvx_moments_batch's, so that one _Call.batch_args serves both
    assert _lib.SIGNATURES[ENTRY][1][:12] == _lib.SIGNATURES["mvx_moments_batch"][1][:12]
    types = {name: text for text, name in declarations()[ENTRY][1]}
    assert types["target"] == "const float *" and types["grad_moments"] == "const double *"
    assert types["grad_coords"] == "double *" and types["grad_features"] == "mvx_real *"


BAD_POSE = records([POSE | _lib.MVX_XF_ROTATE])


def _backward(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, offsets=(0, 3), xforms=None, B=1, C_=4, target=None, gm=P, gc=P,
              gf=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    return call(_lib.load().mvx_moments_backward_batch, h, mode, coords, channels, radii, 1.0, rt, None if off is None else off.ctypes.data,
                None if xforms is None else C.addressof(xforms), B, C_, target, gm, gc, gf, None)


M_MODE = "bad mode (0 features, 1 types, 2 single)"
M_C = "C must be > 0"
M_SINGLE = "single mode has one channel (C = 1)"
M_B = "B must be >= 0"
M_RTYPE = "bad radii_type"
M_CHANWISE = "Channel-Wise Radii Type is not supported"
M_OFFNULL = "offsets must not be null"
M_OFF0 = "offsets[0] must be 0"
M_OFFDEC = "offsets must be non-decreasing"
M_HANDLE = "null handle"
M_POSE = "a MVX_XF_POSE_PTR record must have every other flag bit clear and a non-null center_ptr"
M_MANY = "too many atoms"
M_COORDS = "coords must not be null"
M_CHANNELS = "channels must not be null"
M_RADII = "radii array required"


def test_the_entry_reports_the_earlier_of_two_mistakes():
    """mvx_moments_batch's chain, in its order; every call breaks two rules that follow each other and must report the earlier one.
    The entry's own rules (grad_moments, grad_features, both outputs) sit behind the rules that read the handle, so with no
    handle - and with a made-up one - a call that breaks them too still reports the shared rule. Nothing touches a device."""
    own = dict(gm=None, gc=None, gf=None)  # breaks "grad_moments must not be null" and "... both null" as well
    rows = [
        (dict(mode=3, C_=0), M_MODE),
        (dict(mode=-1, C_=0), M_MODE),
        (dict(C_=0, B=-1), M_C),
        (dict(mode=2, C_=3, B=-1), M_SINGLE),
        (dict(B=-1, rt=7), M_B),
        (dict(rt=7, offsets=None), M_RTYPE),
        (dict(mode=2, C_=1, rt=2, radii=P, offsets=None), M_CHANWISE),
        (dict(offsets=None), M_OFFNULL),
        (dict(offsets=(1, 3)), M_OFF0),
        (dict(B=2, offsets=(0, 3, 2)), M_OFFDEC),
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE, offsets=(0, BIG)), M_POSE),
        (dict(h=P, offsets=(0, BIG), coords=None), M_MANY),
        (dict(h=P, coords=None, channels=None), M_COORDS),
        (dict(h=P, channels=None, rt=1), M_CHANNELS),
        (dict(h=P, rt=1), M_RADII),
    ]
    for kw, want in rows:
        for extra in ({}, own):
            rc, msg = _backward(**dict(kw, **extra))
            assert rc == MVX_ERR_INVALID and msg == want, (kw, extra, rc, msg, want)
    # grad_features outside features mode is the entry's own rule too: it does not jump the queue as it does in mvx_backward_batch
    rc, msg = _backward(mode=1, gf=P)
    assert rc == MVX_ERR_INVALID and msg == M_HANDLE, (rc, msg)


def test_no_molecules_get_as_far_as_the_handle():
    for kw in (dict(B=0, offsets=(0,), coords=None, channels=None, gm=None, gc=None, gf=None), dict(target=P), dict(B=0, offsets=(0,))):
        rc, msg = _backward(**kw)
        assert rc == MVX_ERR_INVALID and msg == M_HANDLE, (kw, rc, msg)


# ---- the constructor option and the guards of a recorded call ------------------------------------------------------------------
def test_moments_grad_is_a_constructor_option_that_needs_differentiable():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    init = inspect.signature(Voxelizer.__init__).parameters
    assert init["moments_grad"].default is False
    with pytest.raises(ValueError, match="moments_grad=True needs differentiable=True"):
        Voxelizer(0.5, 16, moments_grad=True)  # (raised before anything touches a device)
    assert Voxelizer._mgrad is False


def _args(N=6, C_=4):
    rng = np.random.default_rng(0)
    return dict(coords=rng.uniform(-2, 2, (N, 3)), offsets=np.array([0, 2, N]), centers=None,
                channels=rng.standard_normal((N, C_)).astype(np.float32), radii=1.0)


def test_a_fake_voxelizer_without_the_new_attribute_still_runs_the_guards():
    v = _fake(precision=64)
    assert "_mgrad" not in vars(v) and v._mgrad is False  # (the class-level default)
    with pytest.raises(NotImplementedError, match="moments_batch does not support .*precision 64"):
        v.moments_batch(**_args())
    with pytest.raises(AssertionError, match="target does not match dimension"):
        _fake().moments_batch(target=np.zeros((3, 16, 16, 16), np.float32), **_args())
    with pytest.raises(AssertionError, match="offsets must span coords"):
        _fake().moments_batch(**dict(_args(), offsets=np.array([0, 2, 5])))


def test_a_target_radii_or_sigma_that_require_grad_are_refused():
    import torch

    a = _args()
    t = torch.zeros((4, 16, 16, 16), requires_grad=True)
    on = dict(differentiable=True, _mgrad=True)
    with pytest.raises(ValueError, match="moments_grad gives no gradient with respect to the target"):
        _fake(**on).moments_batch(target=t, **a)
    posed = dict(a, quaternions=np.ones((2, 4)), translations=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="moments_grad gives no gradient with respect to the target"):
        _fake(**on).moments_posed_batch(target=t, **posed)
    r = torch.ones(6, requires_grad=True)
    with pytest.raises(ValueError, match="moments_grad gives no gradient with respect to radii"):
        _fake("atom-wise", **on).moments_batch(**dict(a, radii=r))
    with pytest.raises(ValueError, match="moments_grad gives no gradient with respect to radii"):
        _fake(radii_grad=True, **on).moments_batch(**dict(a, radii=torch.ones(1, requires_grad=True)))  # (a scalar-radius tensor)
    s = torch.tensor(0.5, requires_grad=True)
    with pytest.raises(ValueError, match="moments_grad gives no gradient with respect to sigma"):
        _fake(sigma_grad=True, _sigma_src=(s, s._version, 0.5), **on).moments_batch(**a)
    # the unsupported configurations are named first, as without the option
    with pytest.raises(NotImplementedError, match="moments_batch does not support .*no multiple of 4"):
        _fake(dimension=18, **on).moments_batch(target=t, **a)
    # with grad mode off the option changes nothing: the values are read, and the next rule fires
    with torch.no_grad():
        with pytest.raises(AssertionError, match="target does not match dimension"):
            _fake(**on).moments_batch(target=torch.zeros((3, 16, 16, 16), requires_grad=True), **a)


# ---- kernel resources --------------------------------------------------------------------------------------------------------
# <mode (0 features, 1 types / single), gaussian, target>: VGPRs of the shipped build (tools/regs.py). One group of loads - with a
# target 64 in flight - costs two registers more than 32 and stays where grad_kernel<float, 0, true, false> (176) is: two waves per SIMD.
SHIPPED_VGPR = {(0, False, False): 162, (0, False, True): 180, (0, True, False): 206, (0, True, True): 208,
                (1, False, False): 16, (1, False, True): 16, (1, True, False): 26, (1, True, True): 26}
VGPR_SLACK = 6


def test_moments_grad_kernels_keep_grad_kernels_resources():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_moments_grad.o")
    grad = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_grad.o")
    if not (os.path.exists(obj) and os.path.exists(grad)):
        pytest.skip("mvx_moments_grad.o / mvx_grad.o not built")
    assert obj in regs.KERNEL_OBJECTS
    res = regs.kernel_resources(obj)
    base = regs.kernel_resources(grad)
    ks = {k: v for k, v in res.items() if k.startswith("moments_grad_kernel<")}
    tf = ("true", "false")
    assert sorted(ks) == sorted(f"moments_grad_kernel<{m}, {g}, {t}>" for m in (0, 1) for g in tf for t in tf), sorted(ks)
    for name, r in ks.items():
        m = re.match(r"moments_grad_kernel<(\d), (true|false), (true|false)>", name)
        key = (int(m.group(1)), m.group(2) == "true", m.group(3) == "true")
        twin = base[f"grad_kernel<float, {key[0]}, {m.group(2)}, false>"]
        assert r["vspill"] == 0 and r["scratch"] <= twin["scratch"] and r["lds"] == 0, (name, r, twin)
        assert r["vgpr"] <= SHIPPED_VGPR[key] + VGPR_SLACK, (name, r)
        assert r["vgpr"] <= 256, (name, r)  # two waves per SIMD, as grad_kernel's features walk
    coef = res["moments_coef_kernel"]
    assert coef["vspill"] == 0 and coef["sspill"] == 0 and coef["scratch"] == 0 and coef["lds"] == 0, coef


# ---- the reference composition itself ----------------------------------------------------------------------------------------
D, C_, N, RADIUS, H = 8, 2, 4, 1.0, 2.0 ** -12


def _fd_case(seed):
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-1.2, 1.2, (N, 3))
    w = rng.uniform(0.25, 1.0, (N, C_))
    t = rng.standard_normal((C_, D, D, D)).astype(np.float32)
    gm = rng.integers(-16, 17, (C_, 3)) / 8.0  # (float32 values: the coefficients are exact)
    gm[gm == 0] = 0.375
    return xyz, w, t, gm


def _grid32(xyz, w):
    """The float32 grid of the molecule: the float64 densities of tests/grad_reference (precision 64: smooth in the coordinates),
    weighted, summed and rounded once."""
    g = np.zeros((C_, D, D, D))
    for n in range(N):
        g += w[n][:, None, None, None] * GR.atom_grid(xyz, n, RADIUS, "scalar", C_, D, precision=64)
    return g.astype(np.float32)


def _loss(xyz, w, t, gm):
    """(L, noise): L = sum_c sum_k gm[c, k] m[c, k] from the exact moments of the float32 grid, and what the one rounding of the grid
    can move it by: 2^-24 (|G0| sum|g| + 2 |G1| sum g^2 + |G2| sum|g t|), first order, with one per cent on top."""
    g = _grid32(xyz, w)
    L = float((gm * MR.moments_of(g, t)).sum())
    g64, t64 = np.abs(g.astype(np.float64)), np.abs(t.astype(np.float64))
    s = [g64.sum((1, 2, 3)), 2.0 * (g64 * g64).sum((1, 2, 3)), (g64 * t64).sum((1, 2, 3))]
    return L, 1.01 * 2.0 ** -24 * float(sum((np.abs(gm[:, k]) * s[k]).sum() for k in range(3)))


def _margin(xyz):
    """The least distance between a voxel centre and the surface of an atom's sphere: a finite difference is a derivative only
    while no voxel crosses it (the kernels' gradient is the a.e. one: the jump at the truncation radius is ignored)."""
    ax = GR.axis(D)
    grid = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 3)
    return min(float(np.abs(np.linalg.norm(grid - p, axis=1) - RADIUS).min()) for p in xyz)


@pytest.mark.parametrize("seed", [6, 12, 18])
def test_the_upstream_fed_to_the_gradient_reference_is_the_derivative_of_the_exact_moments(seed):
    """Central differences with steps h and 2h. Their error: the rounding of the grid, at most noise / h per difference, and the
    truncation K h^2, of which the two steps show 3 K h^2 = |FD(2h) - FD(h)| up to 1.5 noise / h. The bar
    2 noise / h + |FD(2h) - FD(h)| therefore holds three times the truncation error and leaves the rest to the noise."""
    xyz, w, t, gm = _fd_case(seed)
    assert _margin(xyz) > 3 * H, _margin(xyz)  # (steps of up to 2 H; the seeds were chosen so)
    g = _grid32(xyz, w)
    G, Gabs = MG.upstream(g, gm, t)
    a0, a1, a2 = MG.coefficients(gm)
    assert np.array_equal(a0, gm[:, 0]) and np.array_equal(a1, 2 * gm[:, 1]) and np.array_equal(a2, gm[:, 2])
    assert (Gabs >= np.abs(G)).all() and (Gabs > np.abs(G)).any()  # (mixed signs: cancellation inside u happens)
    ref = GR.reference(xyz, G, RADIUS, "scalar", w=w, precision=64)
    _, noise = _loss(xyz, w, t, gm)

    def fd(bump, step):
        return (_loss(*bump(+step), t, gm)[0] - _loss(*bump(-step), t, gm)[0]) / (2 * step)

    checked = 0
    for n in range(N):
        for a in range(3):
            def bump(s, n=n, a=a):
                x = xyz.copy()
                x[n, a] += s
                return x, w
            d1, d2 = fd(bump, H), fd(bump, 2 * H)
            tol = 2 * noise / H + abs(d2 - d1)
            want = ref["coords"][0][n, a]
            assert abs(d1 - want) <= tol, (seed, n, a, d1, want, tol)
            checked += tol < 0.05 * np.abs(ref["coords"][0]).max()
        for c in range(C_):
            def bump(s, n=n, c=c):
                v = w.copy()
                v[n, c] += s
                return xyz, v
            d1, d2 = fd(bump, 2.0 ** -6), fd(bump, 2.0 ** -5)  # (quadratic in w: no truncation, a larger step against the noise)
            tol = 2 * noise / 2.0 ** -6 + abs(d2 - d1)
            want = ref["features"][0][n, c]
            assert abs(d1 - want) <= tol, (seed, n, c, d1, want, tol)
            checked += tol < 0.05 * np.abs(ref["features"][0]).max()
    assert checked >= 0.8 * N * (3 + C_), checked  # the bar is far below the gradients themselves: the check is not vacuous
    # without a target: the first two moments alone
    G2, _ = MG.upstream(g, gm[:, :2], None)
    assert np.array_equal(G2, a0[:, None, None, None] + a1[:, None, None, None] * g.astype(np.float64))
