"""The C ABI as the tests see it, in one place (host only, no torch): include/mvx.h parsed once, the one rule by which a ctypes
type matches a header type, the one pin of the version, the parameter names the tests pin, the status codes read from the header,
and the scaffolding of a call that is refused before it touches a device. tests/test_abi_header_host.py checks every declared
function against molvoxel_amd/voxelizer/hip/_lib.SIGNATURES with it; the *_host.py files import P, records, MVX_ERR_INVALID and
call from here for their rejection tables."""
import ctypes as C
import functools
import os
import re

from molvoxel_amd.voxelizer.hip import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mvx.h")
VERSION = 140  # the one pin: lib.mvx_version(), the header's #define and this agree (tests/test_abi_header_host.py)


@functools.lru_cache(maxsize=None)
def header_text():
    """include/mvx.h without its comments."""
    with open(HEADER) as fh:
        text = fh.read()
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


@functools.lru_cache(maxsize=None)
def declarations():
    """name -> (return type, [(type text, parameter name), ...]) in header order, for every function the header declares."""
    out = {}
    for res, name, body in re.findall(r"^([A-Za-z_][\w ]*?[ *]+)(mvx_\w+)\(([^;{}()]*)\);", header_text(), re.M):
        params = []
        for p in (" ".join(body.split()).split(",") if body.strip() != "void" else []):
            m = re.fullmatch(r"(.*?)(\w+)", p.strip())
            params.append((m.group(1).strip(), m.group(2)))
        out[name] = (" ".join(res.split()), params)
    return out


def header_version():
    return int(re.search(r"#define MVX_VERSION (\d+)", header_text()).group(1))


def _status(name):
    return int(re.search(r"\b%s = (-?\d+)" % name, header_text()).group(1))


MVX_ERR_INVALID = _status("MVX_ERR_INVALID")
MVX_ERR_ALLOC = _status("MVX_ERR_ALLOC")

_SCALAR = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
_POINTEE = {"mvx_config": C.POINTER(_lib.MvxConfig), "mvx_plan": C.POINTER(_lib.MvxPlan), "mvx_plan_query": C.POINTER(_lib.MvxPlanQuery),
            "mvx_handle *": C.POINTER(_lib.Handle), "void *": C.POINTER(C.c_void_p), "int": C.POINTER(C.c_int),
            "float": C.POINTER(C.c_float), "int32_t": C.POINTER(C.c_int32), "char": C.c_char_p}
RETURN = {"int": C.c_int, "const char *": C.c_char_p}


def matches(type_text, ctype):
    """The one rule: a scalar is matched by exactly its ctypes type, a pointer by c_void_p or by the typed pointer to its pointee."""
    t = type_text.strip()
    if not t.endswith("*"):
        return _SCALAR.get(t) is ctype
    pointee = re.sub(r"\bconst\b", "", t[:-1]).strip()
    return ctype is C.c_void_p or _POINTEE.get(pointee) is ctype


# ---- the parameter names the tests pin, entry by entry -----------------------------------------------------------------------
_VIEWS_HEAD = ["h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "N", "C", "xforms", "B", "index", "offsets_host",
               "target", "target_view_stride"]
HESS_HEAD = ["h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "offsets", "xforms", "B", "C", "field",
             "field_mol_stride", "pivots", "scores", "atom_grad", "atom_hess", "twist_grad", "twist_hess"]
PINNED_NAMES = {
    "mvx_score_batch": [
        "h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "offsets", "xforms", "B", "C", "field",
        "field_mol_stride", "scores", "atom_scores", "grad_coords", "grad_features", "stream"],
    "mvx_score_views": ["h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "N", "C", "xforms", "B", "index",
                        "offsets_host", "field", "field_view_stride", "scores", "atom_scores", "grad_coords", "grad_features",
                        "stream"],
    "mvx_views_reduce": ["h", "index", "offsets_host", "B", "N", "rows", "width", "row_type", "out", "stream"],
    "mvx_moments_views": _VIEWS_HEAD + ["moments", "stream"],
    "mvx_moments_backward_views": _VIEWS_HEAD + ["grad_moments", "grad_coords_rows", "grad_features_rows", "stream"],
    "mvx_apply_torsions": ["h", "coords", "offsets", "B", "T", "axes", "moves", "angles", "out", "stream"],
    "mvx_score_hessian_flex_batch": HESS_HEAD + ["T", "axes", "moves", "flex_grad", "flex_hess", "atom_pos", "stream"],
    "mvx_flex_lm_step": ["h", "B", "T", "have_trial", "lam_down", "lam_up", "max_dropped", "q", "t", "theta", "S", "G", "H", "lam",
                         "taken", "dropped", "q2", "t2", "theta2", "S2", "G2", "H2", "x", "stream"],
    "mvx_forward_views_sum": ["h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "N", "C", "xforms", "B",
                              "view_weights", "out", "accumulate", "stream"],
    "mvx_set_sum_parts": ["h", "parts"],
    "mvx_apply_torsions_backward": ["h", "conformer", "offsets", "B", "T", "axes", "moves", "angles", "grad_out", "grad_coords",
                                    "grad_angles", "stream"],
    "mvx_forward_sum_batch": [
        "h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "offsets", "xforms", "B", "C", "atom_weights",
        "out", "accumulate", "stream"],
    "mvx_moments_backward_batch": [
        "h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "offsets", "xforms", "B", "C", "target", "grad_moments",
        "grad_coords", "grad_features", "stream"],
    "mvx_moments_batch": [
        "h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "offsets", "xforms", "B", "C", "target", "moments",
        "stream"],
    "mvx_score_hessian_views": ["h", "mode", "coords", "channels", "radii", "radius_scalar", "radii_type", "N", "C", "xforms", "B",
                                "index", "offsets_host", "field", "field_view_stride", "pivots", "scores", "atom_grad", "atom_hess",
                                "twist_grad", "twist_hess", "stream"],
    "mvx_lm_step": ["h", "B", "have_trial", "lam_down", "lam_up", "max_dropped", "q", "t", "S", "G", "H", "lam", "taken", "dropped",
                    "q2", "t2", "S2", "G2", "H2", "xi", "stream"],
    "mvx_score_hessian_batch": HESS_HEAD + ["stream"],
}

# ---- a call that is refused before it touches a device -----------------------------------------------------------------------
P = 16  # any non-null pointer: nothing behind it is read before the checks are through


def records(flags, ptr=P):
    xfs = (_lib.MvxXform * len(flags))()
    for b, f in enumerate(flags):
        xfs[b].flags = f
        xfs[b].center_ptr = ptr
    return xfs


def last_error():
    return (_lib.load().mvx_last_error() or b"").decode()


def call(fn, *args):
    """(rc, message) of one library call."""
    rc = fn(*args)
    return rc, last_error()
