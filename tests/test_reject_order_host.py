"""The ORDER in which the C ABI entries apply their rejection rules, without a GPU. The other host tests break one rule per call;
here every call breaks two rules that follow each other in an entry's chain of checks and must report the earlier one, so a
change that reorders the checks of an entry changes a message below. Each entry's table walks its rules in the order the
library applies them; the last row of a table breaks the last rule alone. Texts are compared in full.

Arguments: P stands for any non-null pointer (nothing behind it is read before the checks are through). The backward, score,
views and pose entries look at the handle last and get None; where a rule sits behind the handle rule (the records of explicit
poses, the backward's atom count and null arrays) the handle is P in a call that still fails, so P is never dereferenced. The
forward entries look at the handle first and always get P with arguments that fail.

Pairs left out because one argument set cannot break both rules are named where they would stand."""
import ctypes as C

import numpy as np

from molvoxel_amd.voxelizer.hip import _lib
from tests.abi import MVX_ERR_INVALID, P, call, records

BIG = 1 << 31
POSE = _lib.MVX_XF_POSE_PTR
ONE, TWO = records([0]), records([0, 0])
BAD_POSE = records([POSE | _lib.MVX_XF_ROTATE])  # breaks the pose-record rule
BAD_POSE2 = records([POSE, POSE | _lib.MVX_XF_ROTATE])
GOOD_POSE = records([POSE])

M_HANDLE = "null handle"
M_RTYPE = "bad radii_type"
M_KIND = "bad memory kind"
M_CHANWISE = "Channel-Wise Radii Type is not supported"
M_OFF0 = "offsets[0] must be 0"
M_OFFDEC = "offsets must be non-decreasing"
M_COORDS = "coords must not be null"
M_RADII = "radii array required"
M_CHANNELS = "channels must not be null"
M_MANY = "too many atoms"
M_POSE = "a MVX_XF_POSE_PTR record must have every other flag bit clear and a non-null center_ptr"
M_OFFNULL_IDX = "offsets_host must not be null with an index"
M_MANY_IDX = "too many atoms: offsets[B] must stay below 2^31"


def _addr(x):
    return None if x is None else C.addressof(x)


def _off(offsets):
    """(array kept alive, its address) of host offsets, or (None, None)."""
    if offsets is None:
        return None, None
    a = np.asarray(offsets, np.int64)
    return a, a.ctypes.data


def _check(fn, rows):
    for kw, want in rows:
        rc, msg = fn(**kw)
        assert rc == MVX_ERR_INVALID and msg == want, (kw, rc, msg, want)


# ---- forward: run() -> validate(); the handle is looked at first --------------------------------------------------------------
def _fwd(entry="features", h=P, coords=P, channels=P, radii=None, rt=0, offsets=(0, 3), xforms=None, B=1, C_=4, out=P, ik=1,
         ok=1):
    lib = _lib.load()
    keep, off = _off(offsets)
    if entry == "single":
        return call(lib.mvx_forward_single_batch, h, coords, radii, 1.0, rt, off, _addr(xforms), B, out, ik, ok, None)
    return call(lib.mvx_forward_features_batch, h, coords, channels, radii, 1.0, rt, off, _addr(xforms), B, C_, out, ik, ok, None)


M_FWD_BC = "B must be >= 0 and C > 0"
M_FWD_NULL = "offsets/out must not be null"


def test_forward_features_batch_reports_the_earlier_of_two_mistakes():
    _check(_fwd, [
        (dict(h=None, B=-1), M_HANDLE),
        (dict(C_=0, out=None), M_FWD_BC),
        (dict(B=-1, offsets=None), M_FWD_BC),
        (dict(out=None, rt=7), M_FWD_NULL),
        # ("bad radii_type", "Channel-Wise ..."): the second needs single mode, which this entry does not have
        (dict(rt=7, ik=5), M_RTYPE),
        (dict(rt=-1, ok=5), M_RTYPE),
        (dict(ik=5, offsets=(1, 3)), M_KIND),
        (dict(offsets=(1, 0)), M_OFF0),
        (dict(B=2, offsets=(0, 3, 2), coords=None), M_OFFDEC),
        (dict(coords=None, rt=1), M_COORDS),
        (dict(rt=1, channels=None), M_RADII),
        (dict(rt=2, channels=None), M_RADII),
        (dict(channels=None, offsets=(0, BIG)), M_CHANNELS),
        (dict(offsets=(0, BIG), xforms=BAD_POSE), M_MANY),
        (dict(xforms=BAD_POSE), M_POSE),
    ])


def test_forward_single_batch_reports_the_earlier_of_two_mistakes():
    # (C is 1 here: only B < 0 breaks the first shape rule; "channels must not be null" does not apply to single mode)
    _check(lambda **kw: _fwd(entry="single", **kw), [
        (dict(h=None, B=-1), M_HANDLE),
        (dict(B=-1, out=None), M_FWD_BC),
        (dict(out=None, rt=7), M_FWD_NULL),
        # ("bad radii_type", "Channel-Wise ..."): one radii_type cannot be out of range and channel-wise
        (dict(offsets=None, rt=2, radii=P), M_FWD_NULL),
        (dict(rt=7, ik=5), M_RTYPE),
        (dict(rt=2, radii=P, ik=5), M_CHANWISE),
        (dict(ik=5, offsets=(1, 3)), M_KIND),
        (dict(offsets=(1, 0)), M_OFF0),
        (dict(B=2, offsets=(0, 3, 2), coords=None), M_OFFDEC),
        (dict(coords=None, rt=1), M_COORDS),
        (dict(rt=1, offsets=(0, BIG)), M_RADII),
        (dict(offsets=(0, BIG), xforms=BAD_POSE), M_MANY),
        (dict(xforms=BAD_POSE), M_POSE),
    ])


# ---- views: validate_views(), then the entry's own rules, then the handle, then the records ---------------------------------
M_MODE_V = "bad mode"
M_BNC = "B and N must be >= 0 and C > 0"
M_XF_V = "xforms must not be null (a view of the whole cloud is a record with flags = 0)"
M_SINGLE_V = "single mode has one channel"
M_TYPES_V = "types must not be null"


def _views_chain(own_first_kw, with_in_kind=True):
    """The rules every views entry shares, in order. own_first_kw: what breaks the entry's first own rule."""
    rows = [(dict(mode=3, rt=7), M_MODE_V)]
    if with_in_kind:
        rows += [(dict(rt=7, ik=5), M_RTYPE), (dict(ik=5, B=-1), M_KIND), (dict(ik=-1, N=-1), M_KIND)]
    else:  # (the entry takes device arrays only: no memory kind to get wrong)
        rows += [(dict(rt=7, B=-1), M_RTYPE)]
    rows += [
        (dict(C_=0, xforms=None), M_BNC),
        (dict(N=-1, xforms=None), M_BNC),
        (dict(xforms=None, mode=2, rt=2, radii=P), M_XF_V),
        (dict(mode=2, rt=2, radii=P, C_=3), M_CHANWISE),
        (dict(mode=2, C_=3, coords=None), M_SINGLE_V),
        (dict(coords=None, rt=1), M_COORDS),
        (dict(rt=1, mode=1, channels=None), M_RADII),
        (dict(mode=1, channels=None, N=BIG), M_TYPES_V),
        (dict(N=BIG, **own_first_kw), M_MANY),
    ]
    return rows


def _select(h=None, coords=P, channels=P, radii=None, rt=0, mode=0, N=3, C_=4, xforms=ONE, B=1, index=P, cap=8, offsets_out=P,
            ik=1):
    return call(_lib.load().mvx_select_views, h, coords, channels, radii, 1.0, rt, mode, N, C_, _addr(xforms), B, index, cap,
                offsets_out, ik, None)


def test_select_views_reports_the_earlier_of_two_mistakes():
    m_off, m_idx = "offsets_out_host must not be null", "index_out must not be null"
    _check(_select, _views_chain(dict(offsets_out=None)) + [
        (dict(offsets_out=None, cap=-1), m_off),
        (dict(offsets_out=None, index=None), m_off),
        (dict(cap=-1, xforms=BAD_POSE), m_idx),
        (dict(index=None), m_idx),  # (and a null handle)
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE), M_POSE),
    ])


def _fviews(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, N=3, C_=4, xforms=ONE, B=1, out=P, ik=1, ok=1):
    return call(_lib.load().mvx_forward_views, h, mode, coords, channels, radii, 1.0, rt, N, C_, _addr(xforms), B, out, ik, ok, None)


def test_forward_views_reports_the_earlier_of_two_mistakes():
    m_out = "out must not be null"
    _check(_fviews, _views_chain(dict(ok=5)) + [
        (dict(ok=5, out=None), M_KIND),
        (dict(out=None, channels=None), m_out),
        (dict(channels=None), M_CHANNELS),  # (and a null handle)
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE), M_POSE),
    ])


M_GF = "grad_features exists in features mode only"
M_SCORES = "scores must not be null"
M_NEED_INDEX = ("atom_scores, grad_coords and grad_features need an index: their rows are laid out in selection order "
                "(mvx_select_views)")
M_FIELD_V = "field must not be null"
M_STRIDE_V = "field_view_stride must be 0 (one shared field) or C * D^3 (one field per view)"


def _sviews(h=None, mode=0, coords=P, channels=P, radii=None, rt=0, N=3, C_=4, xforms=ONE, B=1, index=None, offsets=None, field=P,
            stride=0, scores=P, atom_scores=None, gc=None, gf=None):
    keep, off = _off(offsets)
    return call(_lib.load().mvx_score_views, h, mode, coords, channels, radii, 1.0, rt, N, C_, _addr(xforms), B, index, off, field,
                stride, scores, atom_scores, gc, gf, None)


def test_score_views_reports_the_earlier_of_two_mistakes():
    sel = dict(index=P, offsets=(0, 2))
    _check(_sviews, _views_chain(dict(scores=None), with_in_kind=False) + [
        (dict(N=BIG, mode=1, gf=P, **sel), M_MANY),
        (dict(mode=1, gf=P, stride=-1, **sel), M_GF),
        (dict(stride=-1, scores=None), M_STRIDE_V),
        (dict(scores=None, atom_scores=P), M_SCORES),
        (dict(scores=None, index=P), M_SCORES),
        # ("need an index", the offsets rules): the first needs a null index, the others a non-null one
        (dict(gc=P, channels=None), M_NEED_INDEX),
        (dict(atom_scores=P, field=None), M_NEED_INDEX),
        # (null offsets cannot also hold wrong values: "offsets_host must not be null" is paired with the rules behind the offsets)
        (dict(index=P, channels=None), M_OFFNULL_IDX),
        (dict(index=P, offsets=(1, 0)), M_OFF0),
        (dict(index=P, B=2, xforms=TWO, offsets=(0, 1 << 32, BIG)), M_OFFDEC),
        (dict(index=P, offsets=(0, BIG), channels=None), M_MANY_IDX),
        (dict(channels=None, field=None), M_CHANNELS),
        (dict(channels=None, field=None, **sel), M_CHANNELS),
        (dict(field=None), M_FIELD_V),  # (and a null handle)
        (dict(field=None, **sel), M_FIELD_V),
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE), M_POSE),
    ])


# ---- backward family and mvx_score_batch: one chain with a kind-specific middle; the handle comes after the offsets ---------
M_MODE_B = "bad mode (0 features, 1 types, 2 single)"
M_C = "C must be > 0"
M_SINGLE_B = "single mode has one channel (C = 1)"
M_B = "B must be >= 0"
M_OFFNULL = "offsets must not be null"


def _bwd(entry="plain", h=None, mode=0, coords=P, channels=P, radii=None, rt=0, offsets=(0, 3), xforms=None, B=1, C_=4, g=P, gc=P,
         gf=None, gr=P, gsig=None, grs=None, stride=0, scores=P, atoms=None):
    lib = _lib.load()
    keep, off = _off(offsets)
    head = (h, mode, coords, channels, radii, 1.0, rt, off, _addr(xforms), B, C_, g)
    if entry == "plain":
        return call(lib.mvx_backward_batch, *head, gc, gf, None)
    if entry == "radii":
        return call(lib.mvx_backward_radii_batch, *head, gc, gf, gr, None)
    if entry == "density":
        return call(lib.mvx_backward_density_batch, *head, gc, gf, gr, gsig, grs, None)
    return call(lib.mvx_score_batch, *head, stride, scores, atoms, gc, gf, None)


def _backward_chain(entry, ok, middle, first_mid_kw, last_mid_kw, last_mid_msg, chanwise_shadowed, m_grid):
    """ok: arguments that pass the entry's own rules; middle: the rows of those rules (the first breaks its first rule together
    with nothing else); first_mid_kw / last_mid_kw: what breaks the first / last of them."""
    call = lambda **kw: _bwd(entry=entry, **dict(ok, **kw))  # noqa: E731
    rows = [
        (dict(mode=3, gf=P), M_MODE_B),
        (dict(mode=-1, C_=0), M_MODE_B),
        (dict(mode=1, gf=P, C_=0), M_GF),
        (dict(mode=2, C_=0), M_C),
        (dict(mode=2, C_=3, **first_mid_kw), M_SINGLE_B),
    ] + middle + [
        (dict(B=-1, **last_mid_kw), last_mid_msg),
        (dict(B=-1, rt=7), M_B),
        # ("bad radii_type", "Channel-Wise ..."): one radii_type cannot be out of range and channel-wise
        (dict(rt=7, offsets=None), M_RTYPE),
    ]
    if not chanwise_shadowed:
        rows += [(dict(B=-1, mode=2, C_=1, rt=2, radii=P), M_B), (dict(mode=2, C_=1, rt=2, radii=P, offsets=None), M_CHANWISE)]
    # (else: the entry's own radii_type rules have already refused channel-wise radii in single mode)
    rows += [
        # (null offsets cannot also hold wrong values: the rule is paired with the handle rule behind the offsets)
        (dict(offsets=None), M_OFFNULL),
        (dict(offsets=(1, 0)), M_OFF0),
        (dict(B=2, offsets=(0, 3, 2)), M_OFFDEC),  # (and a null handle)
        (dict(xforms=BAD_POSE), M_HANDLE),
        (dict(h=P, xforms=BAD_POSE, offsets=(0, BIG)), M_POSE),
        (dict(h=P, offsets=(0, BIG), coords=None), M_MANY),
        (dict(h=P, coords=None, channels=None), m_grid),
        (dict(h=P, g=None, channels=None), m_grid),
        (dict(h=P, channels=None, rt=1, radii=None), M_CHANNELS),
        (dict(h=P, rt=1, radii=None), M_RADII),
    ]
    _check(call, rows)


M_GRID = "coords / grad_out must not be null"


def test_backward_batch_reports_the_earlier_of_two_mistakes():
    m_both = "grad_coords and grad_features are both null"
    none = dict(gc=None, gf=None)
    _backward_chain("plain", {}, [], none, none, m_both, False, M_GRID)


def test_backward_radii_batch_reports_the_earlier_of_two_mistakes():
    m_null = "grad_radii must not be null"
    m_scalar = "radii_type: scalar radii have no radius array for grad_radii (atom-wise or channel-wise radii only)"
    m_chan = "radii_type: channel-wise radii are not supported in single mode (no grad_radii)"
    _backward_chain("radii", dict(rt=1, radii=P), [
        (dict(gr=None, rt=0), m_null),
        (dict(gr=None, rt=2, mode=2, C_=1), m_null),
        # (scalar rule, channel-wise rule): one radii_type cannot be both
        (dict(rt=0, B=-1), m_scalar),
    ], dict(gr=None), dict(rt=2, mode=2, C_=1), m_chan, True, M_GRID)


def test_backward_density_batch_reports_the_earlier_of_two_mistakes():
    m_all = "grad_sigma, grad_radius_scalar and grad_radii are all null"
    m_rs = "radii_type: grad_radius_scalar exists with scalar radii only"
    m_scalar = "radii_type: scalar radii have no radius array for grad_radii (grad_radius_scalar gives dL/dr)"
    m_chan = "radii_type: channel-wise radii are not supported in single mode"
    none = dict(gr=None, gsig=None, grs=None)
    _backward_chain("density", dict(rt=1, radii=P, gsig=P), [
        # ("all null", the radii_type rules of grad_radius_scalar / grad_radii): those need one of the outputs non-null
        (dict(B=-1, **none), m_all),
        (dict(mode=2, C_=1, rt=2, **none), m_all),
        # (grad_radius_scalar rule, grad_radii rule): one radii_type cannot be scalar and not scalar
        (dict(grs=P, rt=2, mode=2, C_=1), m_rs),
        (dict(grs=P, rt=1, B=-1), m_rs),
        (dict(gr=P, rt=0, B=-1), m_scalar),
    ], none, dict(rt=2, mode=2, C_=1), m_chan, True, M_GRID)


def test_score_batch_reports_the_earlier_of_two_mistakes():
    m_stride = "field_mol_stride must be 0 (one shared field) or C * D^3 (one field per molecule)"
    _backward_chain("score", {}, [
        (dict(stride=-1, scores=None), m_stride),
        # ("scores must not be null", "B must be >= 0"): the first applies to B > 0 only
        (dict(scores=None, rt=7), M_SCORES),
    ], dict(stride=-1), dict(stride=-1), m_stride, False, "coords / field must not be null")


# ---- mvx_pose_grad_batch --------------------------------------------------------------------------------------------------
def _pose(h=None, coords=P, gcoords=P, offsets=(0, 3), xforms=GOOD_POSE, B=1, gp=P):
    keep, off = _off(offsets)
    return call(_lib.load().mvx_pose_grad_batch, h, coords, gcoords, off, _addr(xforms), B, gp, None)


def test_pose_grad_batch_reports_the_earlier_of_two_mistakes():
    m_coords = "coords / grad_coords must not be null"
    m_every = "every record must be a MVX_XF_POSE_PTR record"
    _check(_pose, [
        # ("B must be >= 0", the null-pointer rules): those apply to B > 0 only; with the handle rule instead
        (dict(B=-1), M_B),
        (dict(gp=None, xforms=None), "grad_pose must not be null"),
        (dict(xforms=None, offsets=None), "xforms must not be null"),
        # (null offsets cannot also hold wrong values: paired with the record rule behind the offsets)
        (dict(offsets=None, xforms=ONE), M_OFFNULL),
        (dict(offsets=(1, 0)), M_OFF0),
        (dict(B=2, xforms=BAD_POSE2, offsets=(0, 3, 2), coords=None), M_OFFDEC),
        (dict(coords=None, xforms=ONE), m_coords),
        (dict(gcoords=None, xforms=ONE), m_coords),
        (dict(B=2, offsets=(0, 2, 3), xforms=records([0, POSE | _lib.MVX_XF_ROTATE])), m_every),
        (dict(xforms=BAD_POSE), M_POSE),  # (and a null handle)
        (dict(), M_HANDLE),
    ])


# ---- mvx_views_reduce -------------------------------------------------------------------------------------------------------
def _reduce(h=None, index=P, offsets=(0, 2, 3), B=2, N=4, rows=P, width=3, row_type=1, out=P):
    keep, off = _off(offsets)
    return call(_lib.load().mvx_views_reduce, h, index, off, B, N, rows, width, row_type, out, None)


def test_views_reduce_reports_the_earlier_of_two_mistakes():
    m_width = "width must be > 0 (and at most 65535 * 32)"
    _check(_reduce, [
        (dict(B=-1, width=0), "B and N must be >= 0"),
        (dict(N=-1, width=0), "B and N must be >= 0"),
        (dict(width=0, row_type=2), m_width),
        (dict(width=65535 * 32 + 1, row_type=2), m_width),
        (dict(row_type=2, N=BIG), "bad row_type"),
        (dict(N=BIG, offsets=None), M_MANY),
        # (null offsets cannot also hold wrong values, nor a total: paired with the rule for `out`)
        (dict(offsets=None, out=None), M_OFFNULL_IDX),
        (dict(offsets=(1, 0, 0)), M_OFF0),
        (dict(offsets=(0, 1 << 32, BIG)), M_OFFDEC),
        (dict(offsets=(0, 2, BIG), index=None), M_MANY_IDX),
        (dict(index=None, out=None), "index / rows must not be null"),
        (dict(rows=None, out=None), "index / rows must not be null"),
        (dict(out=None), "out must not be null"),  # (and a null handle)
        (dict(), M_HANDLE),
    ])


# ---- mvx_transform_coords: one rule for every null argument, then the record -----------------------------------------------
def _xform(h=P, coords=P, N=3, xform=ONE, out=P):
    return call(_lib.load().mvx_transform_coords, h, coords, N, _addr(xform), out, 1, 1, None)


def test_transform_coords_reports_the_earlier_of_two_mistakes():
    _check(_xform, [
        (dict(h=None, xform=BAD_POSE), "null argument"),
        (dict(coords=None, xform=BAD_POSE), "null argument"),
        (dict(out=None, xform=BAD_POSE), "null argument"),
        (dict(xform=None), "null argument"),
        (dict(xform=BAD_POSE), M_POSE),
        (dict(xform=BAD_POSE, N=0), M_POSE),
    ])

