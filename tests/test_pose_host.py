"""Explicit rigid poses without a GPU: what mvx_pose_grad_batch rejects before it touches a device, the ctypes table against
the header, the flag values, the public signatures of the three posed methods, the numpy restatement (tests/pose_reference.py)
against finite differences of a smooth float64 loss, and the register use of the pose kernels read from mvx_pose.o."""
import ctypes as C
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import pose_reference as pr
from tests.abi import MVX_ERR_INVALID, P, call, header_text, last_error, records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pose_grad(handle=None, coords=P, grad_coords=P, offsets=(0, 3), xforms="pose", B=1, grad_pose=P):
    off = None if offsets is None else np.asarray(offsets, np.int64)
    if isinstance(xforms, str):
        xforms = records([_lib.MVX_XF_POSE_PTR] * max(B, 1))
    return call(_lib.load().mvx_pose_grad_batch, handle, coords, grad_coords, None if off is None else off.ctypes.data,
                None if xforms is None else C.addressof(xforms), B, grad_pose, None)


@pytest.mark.parametrize("kw, words", [
    (dict(), "null handle"),
    (dict(B=-1), "B must be"),
    (dict(coords=None), "coords / grad_coords"),
    (dict(grad_coords=None), "coords / grad_coords"),
    (dict(grad_pose=None), "grad_pose"),
    (dict(xforms=None), "xforms"),
    (dict(offsets=None), "offsets"),
    (dict(offsets=(1, 3)), "offsets[0]"),
    (dict(offsets=(0, 5, 3), B=2), "non-decreasing"),
    (dict(xforms=records([0])), "MVX_XF_POSE_PTR"),
    (dict(xforms=records([_lib.MVX_XF_CENTER | _lib.MVX_XF_ROTATE])), "MVX_XF_POSE_PTR"),
    (dict(xforms=records([_lib.MVX_XF_POSE_PTR, _lib.MVX_XF_CENTER_PTR]), offsets=(0, 2, 3), B=2), "MVX_XF_POSE_PTR"),
    (dict(xforms=records([_lib.MVX_XF_POSE_PTR | _lib.MVX_XF_CENTER])), "other flag bit"),
    (dict(xforms=records([_lib.MVX_XF_POSE_PTR], ptr=None)), "center_ptr"),
])
def test_pose_grad_rejects_bad_arguments_before_touching_a_device(kw, words):
    rc, msg = _pose_grad(**kw)
    assert rc == MVX_ERR_INVALID, (rc, msg)
    assert words in msg, msg


def test_pose_grad_without_atoms_accepts_null_arrays_up_to_the_handle():
    # (no atoms: coords and grad_coords may be null; the handle is looked at last)
    rc, msg = _pose_grad(coords=None, grad_coords=None, offsets=(0, 0))
    assert rc == MVX_ERR_INVALID and "null handle" in msg, (rc, msg)


@pytest.mark.parametrize("entry", ["forward", "views", "backward", "transform"])
def test_entries_reject_a_pose_record_with_other_flag_bits(entry):
    lib = _lib.load()
    bad = records([_lib.MVX_XF_POSE_PTR | _lib.MVX_XF_ROTATE])
    off = np.array([0, 3], np.int64)
    x = C.addressof(bad)  # (the handle is any non-null pointer: the records are checked before it is used)
    if entry == "forward":
        rc = lib.mvx_forward_single_batch(P, P, None, 1.0, 0, off.ctypes.data, x, 1, P, 1, 1, None)
    elif entry == "views":
        rc = lib.mvx_forward_views(P, 2, P, None, None, 1.0, 0, 3, 1, x, 1, P, 1, 1, None)
    elif entry == "backward":
        rc = lib.mvx_backward_batch(P, 2, P, None, None, 1.0, 0, off.ctypes.data, x, 1, 1, P, P, None, None)
    else:
        rc = lib.mvx_transform_coords(P, P, 3, x, P, 1, 1, None)
    assert rc == MVX_ERR_INVALID and "other flag bit" in last_error()


def test_flag_values_match_the_header():
    for name, value in (("MVX_XF_POSE_PTR", 32), ("MVX_XF_TRANSLATE_ONCE", 64)):
        assert int(re.search(name + r" = (\d+)", header_text()).group(1)) == value == getattr(_lib, name)


def test_header_compiles_as_c99_with_the_pose_prototype(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    src = tmp_path / "pose.c"
    src.write_text(
        '#include <stdio.h>\n#include "mvx.h"\n'
        "int main(void) {\n"
        "  double pose[10] = {0, 0, 0, 1, 0, 0, 0, 0, 0, 0}, xyz[3] = {0, 0, 0}, g[3] = {0, 0, 0}, out[10];\n"
        "  int64_t off[2] = {0, 1};\n"
        "  mvx_xform xf = {{0, 0, 0}, {1, 0, 0, 0}, {0, 0, 0}, MVX_XF_POSE_PTR, NULL};\n"
        "  xf.center_ptr = pose;\n"
        '  printf("%d %d\\n", mvx_pose_grad_batch(NULL, xyz, g, off, &xf, 1, out, NULL), (int)sizeof(mvx_xform));\n'
        "  return 0;\n}\n")
    exe = tmp_path / "pose"
    libdir = os.path.dirname(_lib.LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), str(src),
                           "-L", libdir, "-lmvx_hip", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    assert subprocess.check_output([str(exe)]).decode().split() == [str(MVX_ERR_INVALID), "80"]


def test_voxelizer_has_the_posed_methods():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    bat = inspect.signature(Voxelizer.forward_posed_batch).parameters
    assert list(bat) == ["self", "coords", "offsets", "centers", "quaternions", "translations", "channels", "radii", "num_channels",
                         "out_grid"]
    vws = inspect.signature(Voxelizer.forward_posed_views).parameters
    assert list(vws) == ["self", "coords", "centers", "quaternions", "translations", "channels", "radii", "num_channels", "out_grid"]
    sel = inspect.signature(Voxelizer.select_posed_views).parameters
    assert list(sel) == ["self", "coords", "centers", "quaternions", "translations", "channels", "radii"]
    assert bat["num_channels"].default is None and bat["out_grid"].default is None
    assert vws["num_channels"].default is None and vws["out_grid"].default is None
    assert sel["channels"].default is None and sel["radii"].default is None


def test_pose_shape_errors_are_assertion_errors():
    from molvoxel_amd.voxelizer.hip.voxelizer import Voxelizer

    pack = Voxelizer._pack_pose
    q, t, c = np.zeros((2, 4)), np.zeros((2, 3)), np.zeros((2, 3))
    for bad in ((c, np.zeros((2, 3)), t), (c, q, np.zeros((3, 3))), (np.zeros((2, 4)), q, t), (c, np.zeros(4), t)):
        with pytest.raises(AssertionError, match="does not match dimension"):
            pack(None, 2, *bad, False)
    block = pack(None, 2, None, q + 1.0, t + np.float32(0.1), False)  # (host coordinates: a numpy block; centers None: c = 0)
    assert block.dtype == np.float64 and block.shape == (2, 10) and block.flags.c_contiguous
    assert np.array_equal(block[:, :3], 0 * c) and np.array_equal(block[:, 3:7], q + 1.0)
    assert np.array_equal(block[:, 7:], np.full((2, 3), float(np.float32(0.1))))


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def _cloud(seed, N=40):
    rng = np.random.default_rng(seed)
    c = np.array([30.0, -20.0, 12.0]) + rng.normal(0, 0.5, 3)
    xyz = c + rng.uniform(-3, 3, (N, 3))
    return rng, xyz, c


def test_positions_are_the_sandwich_product_with_the_translation_added_once():
    rng, xyz, c = _cloud(0)
    q = rng.standard_normal(4)
    q *= 1.25 / np.linalg.norm(q)
    t = np.array([0.1, -0.7, 1.3])  # (no float32 values)
    t32 = t.astype(np.float32).astype(np.float64)
    p = pr.positions(xyz, c, q, t)
    assert np.allclose(p, (xyz - c) @ pr.rotation(q).T + t32, rtol=0, atol=1e-13)
    assert np.abs(p - ((xyz - c) @ pr.rotation(q).T + t)).max() > 1e-9  # the rounding of t is visible
    assert np.array_equal(pr.positions(xyz, c, q, t32), p)
    assert np.allclose(pr.rotation(q) @ pr.rotation(q).T, 1.25 ** 4 * np.eye(3), atol=1e-13)
    assert np.array_equal(pr.positions(xyz, None, q, t), pr.positions(xyz, np.zeros(3), q, t))
    off = np.array([0, 15, 15, 40])
    qs, ts, cs = np.stack([q, 2 * q, -q]), np.stack([t, 0 * t, -t]), np.stack([c, c + 1, c - 1])
    bp = pr.batch_positions(xyz, off, cs, qs, ts)
    assert np.array_equal(bp[15:], pr.positions(xyz[15:], cs[2], qs[2], ts[2]))
    assert np.array_equal(pr.view_positions(xyz, cs, qs, ts)[1], pr.positions(xyz, cs[1], qs[1], ts[1]))


@pytest.mark.parametrize("norm", [1.0, 0.8, 1.25])
def test_chain_rule_against_finite_differences_of_a_smooth_loss(norm):
    rng, xyz, c = _cloud(int(norm * 100))
    q = rng.standard_normal(4)
    q *= norm / np.linalg.norm(q)
    t = rng.uniform(-1, 1, 3)
    A = rng.standard_normal((xyz.shape[0], 3))

    def loss(c_, q_, t_):  # L = sum_n a_n . sin(p_n) + |p_n|^2 / 7, smooth in the pose (the translation unrounded)
        p = pr.positions(xyz, c_, q_, t_, round_translation=False)
        return float((A * np.sin(p)).sum() + (p * p).sum() / 7.0)

    p = pr.positions(xyz, c, q, t, round_translation=False)
    G = A * np.cos(p) + 2.0 * p / 7.0
    got = pr.pose_grads(xyz, c, q, G, np.abs(G))
    h = 1e-6
    for name, x0, slot in (("center", c, 0), ("quaternion", q, 1), ("translation", t, 2)):
        val, bound = got[name]
        assert np.all(bound >= np.abs(val) - 1e-12)
        for k in range(x0.shape[0]):
            args = [[c.copy(), q.copy(), t.copy()] for _ in range(2)]
            args[0][slot][k] += h
            args[1][slot][k] -= h
            fd = (loss(*args[0]) - loss(*args[1])) / (2 * h)
            assert abs(fd - val[k]) <= 1e-7 * max(1.0, float(bound[k])), (name, k, fd, val[k])
    # the same three from dL/dcoords = M^T dL/dp, the form the device reduction takes
    again = pr.from_coords_grad(xyz, c, q, G @ pr.rotation(q))
    for name in got:
        assert np.allclose(again[name][0], got[name][0], rtol=1e-12, atol=1e-12 * float(np.max(again[name][1]))), name


def test_pose_kernels_use_no_scratch():
    from tools import regs

    obj = os.path.join(ROOT, "molvoxel_amd", "csrc", "mvx_pose.o")
    if not os.path.exists(obj):
        pytest.skip("mvx_pose.o not built")
    res = regs.kernel_resources(obj)
    assert {"pose_grad_kernel", "pose_resolve_kernel"} <= set(res), sorted(res)
    for k, r in res.items():
        assert r["scratch"] == 0 and r["vspill"] == 0 and r["sspill"] == 0, (k, r)
    assert res["pose_grad_kernel"]["vgpr"] <= 128 and res["pose_grad_kernel"]["lds"] == 4 * 12 * 8, res["pose_grad_kernel"]
