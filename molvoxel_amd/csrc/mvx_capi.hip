// mvx_capi.hip — host side of libmvx_hip.so: the C ABI declared in include/mvx.h.
//
// Owns per-handle device workspace (atom records, ranges, metadata, staging for host-resident
// arguments) and a small ring of pinned host slots so that calls with device-resident data are
// fully asynchronous on the caller's stream (no hidden device synchronisation). There is no CPU
// fallback in this library: without a usable HIP device mvx_create fails.
#include "mvx_grad.h"
#include "mvx_flex.h"
#include "mvx_hess.h"
#include "mvx_internal.h"
#include "mvx_lm.h"
#include "mvx_moments.h"
#include "mvx_plan.h"
#include "mvx_pose.h"
#include "mvx_sum.h"
#include "mvx_torsion_grad.h"
#include "mvx_views.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

using namespace mvx;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

// How an entry ends a chain of rules that each give the text of what they found wrong, or null.
int reject(const char *bad) { return bad ? fail(MVX_ERR_INVALID, bad) : MVX_OK; }

int fail_hip(hipError_t e, const char *what) {
    g_err = std::string(what) + ": " + hipGetErrorString(e);
    return MVX_ERR_HIP;
}

#define HIP_TRY(expr)                                  \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return fail_hip(_e, #expr); \
    } while (0)


// Device memory, pinned memory and events are freed by their owners' destructors (mvx_destroy); no owner can be copied.
struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

struct DevBuf : NoCopy {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
};

struct PinnedSlot : NoCopy {
    char *p = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool in_flight = false;
    ~PinnedSlot() {
        if (p) (void)hipHostFree(p);
        if (done) (void)hipEventDestroy(done);
    }
};

constexpr int NSLOTS = 4;

} // namespace

// What the binned pipeline's pre-pass writes and its voxelize launches read. Two sets exist so that, with
// mvx_set_overlap, the pre-pass of call k+1 can fill one set on the side stream while call k's voxelize launches
// still read the other.
struct Workspace : NoCopy {
    DevBuf rec, wbuf, xp, xlist, slist, meta, aux;
    std::vector<char> meta_last; // host copy of the offsets the device meta buffer holds
    bool meta_valid = false;
    hipEvent_t ev_pre = nullptr; // pre-pass into this set finished (side stream)
    hipEvent_t ev_vox = nullptr; // the launches reading this set finished (caller's stream)
    bool vox_recorded = false;
    ~Workspace() {
        if (ev_pre) (void)hipEventDestroy(ev_pre);
        if (ev_vox) (void)hipEventDestroy(ev_vox);
    }
};

struct mvx_handle : NoCopy {
    mvx_config cfg;
    Geom g;
    float sigma32;
    int device;
    Workspace ws[2];
    int cur = 0;         // the set the last binned call used
    bool overlap = false; // mvx_set_overlap
    DevBuf xf_buf, in_coords, in_chan, in_radii, out_stage, diag;
    PinnedSlot slots[NSLOTS];
    int next_slot = 0;
    std::vector<hipEvent_t> ev; // 2 * MVX_PROFILE_RING events, created on first use
    int ev_count = 0;           // timed launches recorded since the last read
    bool profiling = false;
    // test / measurement switches (mvx_debug_set_option): waves per slab, channels per workgroup, forced routes, molecule
    // chunks with the pre-pass on a side stream ("chunks": off by default - on cfg-2 x 64 the cross-stream waits and the
    // extra launch boundaries cost more than the 50 us of pre-pass they hide: 0.454 ms per step on one stream, 0.476 with 2
    // chunks, 0.513 with 4), Infinity Cache budget
    PlanKnobs knobs;
    // Stream hand-over: every call reuses the handle's workspace, ordered by the caller's stream. When a call arrives
    // on another stream than the previous one, the new stream first waits for everything the old stream holds
    // (event recorded on the old stream at that moment), so back-to-back calls on different streams never race.
    hipStream_t last_stream = nullptr;
    bool used = false;
    hipEvent_t ev_switch = nullptr;
    hipStream_t side = nullptr;
    hipEvent_t ev_in = nullptr;
    std::vector<hipEvent_t> ev_pre;
    // the backward pass (mvx_backward_batch) keeps buffers of its own: it never writes a workspace set that an overlapped
    // pre-pass (mvx_set_overlap) on the side stream may be filling, nor one that voxelize launches may still read
    DevBuf grad_rec, grad_xp, grad_meta, grad_aux, grad_sort;
    DevBuf pose_meta;  // mvx_pose_grad_batch: the call's offsets and records
    DevBuf grad_rpart; // radius gradients: per-atom / per-(channel, atom) partials of channel-wise radii and their stage sums
    DevBuf score_atoms; // mvx_score_batch without atom_scores: the per-atom scores its reduction reads, 8 bytes per atom
    DevBuf hess_rows;   // mvx_score_hessian_batch: [s_n | g_n | H_n], 8 + 24 + 48 bytes per atom; rows handed out are not used
    // mvx_score_hessian_flex_batch: [subset sums, B * T * 36 doubles | twist_grad, B * 6 | twist_hess, B * 36] (the twist values
    // only where the caller passed null for them); mvx_apply_torsions and mvx_apply_torsions_backward: the call's offsets
    DevBuf flex_ws, flex_off;
    DevBuf torsion_pos; // mvx_apply_torsions_backward: the positions the sweep turns back, 24 bytes per atom
    // "grad_order" option: 0 atoms in the caller's order (the default), 1 in spatial order, XCD by XCD. The spatial order cuts
    // the gradient kernel's memory traffic five-fold at cfg-2 x 256 but not its time (-2 %), and its sort costs small batches
    // more than it saves (profiles/r05_grad.txt)
    int grad_order = 0;
    // views of a shared cloud (mvx_select_views / mvx_forward_views): the views' transforms, per-(view, tile) counts and bases,
    // offsets, max channel radius, and - mvx_forward_views - the selected indices and the gathered rows handed to run()
    DevBuf view_xf, view_counts, view_base, view_off, view_aux, view_index, view_coords, view_chan, view_radii;
    DevBuf view_red_off; // mvx_views_reduce: the call's offsets
    DevBuf view_w;       // mvx_forward_views_sum: the view weights expanded to one per selected atom
    // mvx_set_sum_parts: K > 1 cuts the molecules of every summed call into parts with a partial grid each (G * C * D^3 floats)
    int sum_parts = 1;
    DevBuf sum_part_grids;
    DevBuf moments_part; // mvx_moments_batch: the slab partials of one molecule chunk
    // mvx_moments_backward_batch: the float32 NCDHW grids of the largest molecule chunk, and the call's (B, C, 3) coefficients
    DevBuf mgrad_grids, mgrad_coef;
    double mgrad_scratch = MOMENTS_GRAD_SCRATCH; // "mgrad_scratch_kb" option: bytes of grids a chunk of that call may hold
    int32_t layout = MVX_LAYOUT_NCDHW; // mvx_set_grid_layout
    mvx_plan last_plan{}; // the plan of the last forward call, debug options applied (mvx_debug_last_plan)
    bool has_plan = false;
    int narrow_sub = 0; // "narrow_sub" option: sub-tiles per wave of narrow chunks (1: voxelize_kernel; 2 | 4: voxelize_narrow_kernel; 0: the rule)
    int dbg = 0; // diagnostic builds (-DMVX_DIAG) only

    ~mvx_handle() { // (the buffers, slots and workspace sets free themselves)
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_pre) (void)hipEventDestroy(e);
        if (ev_in) (void)hipEventDestroy(ev_in);
        if (ev_switch) (void)hipEventDestroy(ev_switch);
        if (side) (void)hipStreamDestroy(side);
    }
};

namespace {

struct DeviceGuard {
    int prev = -1;
    bool switched = false;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        err = hipGetDevice(&prev);
        if (err == hipSuccess && prev != dev) {
            err = hipSetDevice(dev);
            switched = (err == hipSuccess);
        }
    }
    ~DeviceGuard() {
        if (switched) (void)hipSetDevice(prev);
    }
};

int ensure(DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return MVX_OK;
    if (b.p) HIP_TRY(hipFree(b.p)); // synchronises: nothing in flight may still use the old buffer
    b.p = nullptr;
    b.cap = 0;
    size_t want = bytes + bytes / 4 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        g_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return MVX_ERR_ALLOC;
    }
    b.cap = want;
    return MVX_OK;
}

int acquire_slot(mvx_handle *h, size_t bytes, PinnedSlot **out) {
    PinnedSlot &s = h->slots[h->next_slot];
    h->next_slot = (h->next_slot + 1) % NSLOTS;
    if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (s.in_flight) {
        HIP_TRY(hipEventSynchronize(s.done));
        s.in_flight = false;
    }
    if (bytes > s.cap) {
        if (s.p) HIP_TRY(hipHostFree(s.p));
        s.p = nullptr;
        s.cap = 0;
        size_t want = bytes + bytes / 4 + 4096;
        HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&s.p), want, hipHostMallocDefault));
        s.cap = want;
    }
    *out = &s;
    return MVX_OK;
}

// Every call that acquired a slot ends with this: a later call must not overwrite pinned memory that a copy still reads.
int release_slot(PinnedSlot *slot, hipStream_t s) {
    if (!slot) return MVX_OK;
    HIP_TRY(hipEventRecord(slot->done, s));
    slot->in_flight = true;
    return MVX_OK;
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

void make_geom(mvx_handle *h) {
    const mvx_config &c = h->cfg;
    Geom g;
    g.res = c.resolution;
    const double width = c.resolution * (double)(c.dimension - 1); // base/voxelizer.py:28
    g.half = width / 2.0;                                          // base/voxelizer.py:33
    g.D = c.dimension;
    g.bd = c.blockdim > 0 ? c.blockdim : 8;                        // numpy/voxelizer.py:38
    g.nb = (g.D + g.bd - 1) / g.bd;                                // numpy/voxelizer.py:44
    g.bd_inv = g.bd > 1 ? (uint32_t)((0x100000000ull + (uint64_t)g.bd - 1) / (uint64_t)g.bd) : 0u;
    g.inv_res = 1.0 / g.res;
    g.inv_pitch = 1.0 / ((double)g.bd * g.res);
    h->g = g;
    h->sigma32 = (float)c.sigma;
}

// One call as every entry describes it; the entries fill it from their arguments, nothing below them takes those loose.
struct Call {
    int mode;
    const double *coords;
    const void *channels; // float features (sumN, C) | int32 types (sumN) | null
    const void *radii; // float, or double for a precision-64 handle (like features and out)
    double radius_scalar;
    int radii_type;
    const int64_t *offsets; // batches: B + 1 host entries; views of one cloud: null
    int64_t N;              // views: the atoms of the shared cloud
    const mvx_xform *xforms;
    int B, C;
    hipStream_t stream;
    int in_kind; // MVX_HOST | MVX_DEVICE: where coords, channels, radii and the memory behind the records' pointers live
};

// The Call of an entry that takes a batch (B molecules behind host offsets), and of one that takes B views of one cloud of N atoms.
Call batch_call(int mode, const double *coords, const void *channels, const void *radii, double radius_scalar, int radii_type,
                const int64_t *offsets, const mvx_xform *xforms, int B, int C, void *stream, int in_kind = MVX_DEVICE) {
    return {mode, coords, channels, radii, radius_scalar, radii_type, offsets, 0, xforms, B, C, reinterpret_cast<hipStream_t>(stream), in_kind};
}

Call views_call(int mode, const double *coords, const void *channels, const void *radii, double radius_scalar, int radii_type, int64_t N,
                const mvx_xform *xforms, int B, int C, void *stream, int in_kind = MVX_DEVICE) {
    return {mode, coords, channels, radii, radius_scalar, radii_type, nullptr, N, xforms, B, C, reinterpret_cast<hipStream_t>(stream), in_kind};
}

struct RunArgs : Call {
    void *out;
    int out_kind;
    // the arrays were produced on the caller's stream a moment ago (the gathered rows of mvx_forward_views): the pre-pass must
    // not run ahead of them on the side stream, so cross-call overlap (mvx_set_overlap) does not apply to this call
    bool no_overlap = false;
    // `out` takes float32 NCDHW grids whatever the handle's grid type and layout (the chunk scratch of mvx_moments_backward_batch)
    bool f32_plain = false;
};

// mvx_forward_sum_batch: what a forward call that sums its molecules into ONE (C, D, D, D) float32 grid brings next to its RunArgs
struct SumCall {
    const float *atom_weights; // (sumN,) device, or null
    bool accumulate;           // the sums start from the values in `out`
    // mvx_moments_batch: the same plan, pre-pass and walk, but per molecule, and `out` takes (B, C, K) float64 moments instead of a grid
    bool moments = false;
    const float *target = nullptr; // (C, D, D, D) device, or null (K = 2)
    int64_t target_stride = 0;     // elements between the targets of two molecules: 0 (one for all) or C * D^3 (mvx_moments_views)
};

// Orders this call after the previous call's work when the caller switched streams (see mvx_handle::last_stream).
int adopt_stream(mvx_handle *h, hipStream_t s) {
    if (h->used && h->last_stream != s) {
        if (!h->ev_switch) HIP_TRY(hipEventCreateWithFlags(&h->ev_switch, hipEventDisableTiming));
        // (the previous stream is alive by contract - mvx.h: "a stream must stay alive until the next call on the handle
        // has returned". If recording on it fails all the same, the error is reported once, the sticky HIP error is
        // cleared and the handle moves on to the new stream behind a device-wide synchronisation: one caller mistake
        // must not wedge the handle for good.)
        hipError_t e = hipEventRecord(h->ev_switch, h->last_stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(s, h->ev_switch, 0);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();
            h->last_stream = s;
            return fail_hip(e, "stream hand-over (was the previous call's stream destroyed?)");
        }
    }
    h->last_stream = s;
    h->used = true;
    return MVX_OK;
}

// How every call that touches the device begins: the handle's device current while it lives, the call ordered on its stream.
struct CallScope {
    DeviceGuard guard;
    int rc; // not MVX_OK: what the entry returns
    CallScope(mvx_handle *h, hipStream_t s)
        : guard(h->device), rc(guard.err != hipSuccess ? fail_hip(guard.err, "hipSetDevice") : adopt_stream(h, s)) {}
};

// Explicit poses (MVX_XF_POSE_PTR): the other flag bits of such a record are clear and its pointer is set.
const char *check_pose_records(const mvx_xform *xf, int n) {
    for (int i = 0; xf && i < n; ++i)
        if ((xf[i].flags & MVX_XF_POSE_PTR) && (xf[i].flags != MVX_XF_POSE_PTR || !xf[i].center_ptr))
            return "a MVX_XF_POSE_PTR record must have every other flag bit clear and a non-null center_ptr";
    return nullptr;
}

bool has_pose_records(const mvx_xform *xf, int n) {
    for (int i = 0; xf && i < n; ++i)
        if (xf[i].flags & MVX_XF_POSE_PTR) return true;
    return false;
}

// All atoms of a call and its largest molecule.
struct Extent {
    int64_t total = 0, max_atoms = 0;
};

// ---- the rules that more than one entry applies, each stated once: the text of the first broken one, or null. The entries
// compose them around rules of their own, whose places differ (tests/test_reject_order_host.py pins every entry's order) ----
// An atom count (of a batch, a cloud or a selection) that does not fit; each entry reports it where it always did.
const char *too_many_atoms(int64_t n) { return n >= (int64_t)1 << 31 ? "too many atoms" : nullptr; }

const char *bad_mode(int mode) { return mode < MODE_FEATURES || mode > MODE_SINGLE ? "bad mode (0 features, 1 types, 2 single)" : nullptr; }

const char *bad_channel_count(const Call &c) {
    if (c.C <= 0) return "C must be > 0";
    return c.mode == MODE_SINGLE && c.C != 1 ? "single mode has one channel (C = 1)" : nullptr;
}

const char *bad_radii_type(const Call &c) {
    if (c.radii_type < MVX_RADII_SCALAR || c.radii_type > MVX_RADII_CHANNEL) return "bad radii_type";
    return c.radii_type == MVX_RADII_CHANNEL && c.mode == MODE_SINGLE ? "Channel-Wise Radii Type is not supported" : nullptr; // numpy/voxelizer.py:443
}

// The rules for host offsets (B + 1 entries; B <= 0: nothing to check).
const char *check_offsets(const int64_t *offsets, int B, Extent &e) {
    if (B <= 0) return nullptr;
    if (!offsets) return "offsets must not be null";
    if (offsets[0] != 0) return "offsets[0] must be 0";
    for (int b = 0; b < B; ++b) {
        if (offsets[b + 1] < offsets[b]) return "offsets must be non-decreasing";
        e.max_atoms = std::max(e.max_atoms, offsets[b + 1] - offsets[b]);
    }
    e.total = offsets[B];
    return nullptr;
}

// ---- 1. what the library checks itself (shapes are the Python layer's job) -----------------------------------------
int validate(const mvx_handle *h, const RunArgs &r, Extent &e) {
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (r.B < 0 || r.C <= 0) return fail(MVX_ERR_INVALID, "B must be >= 0 and C > 0");
    if (r.B == 0) return MVX_OK;
    if (!r.offsets || !r.out) return fail(MVX_ERR_INVALID, "offsets/out must not be null");
    if (const char *bad = bad_radii_type(r)) return fail(MVX_ERR_INVALID, bad);
    if ((r.in_kind != MVX_HOST && r.in_kind != MVX_DEVICE) || (r.out_kind != MVX_HOST && r.out_kind != MVX_DEVICE))
        return fail(MVX_ERR_INVALID, "bad memory kind");
    if (const char *bad = check_offsets(r.offsets, r.B, e)) return fail(MVX_ERR_INVALID, bad);
    if (e.total > 0 && !r.coords) return fail(MVX_ERR_INVALID, "coords must not be null");
    // (an empty molecule comes with empty, possibly null, per-atom arrays)
    if (!r.radii && (r.radii_type == MVX_RADII_CHANNEL || (r.radii_type == MVX_RADII_ATOM && e.total > 0)))
        return fail(MVX_ERR_INVALID, "radii array required");
    if (e.total > 0 && r.mode != MODE_SINGLE && !r.channels) return fail(MVX_ERR_INVALID, "channels must not be null");
    if (const char *bad = too_many_atoms(e.total)) return fail(MVX_ERR_INVALID, bad);
    return reject(check_pose_records(r.xforms, r.B));
}

// The chain that the summed, moments, backward and score entries share, from the number of molecules to the records.
// `after_B`: what the entry found wrong with an argument of its own whose rule sits behind "B must be >= 0" (null: nothing).
const char *check_batch(const mvx_handle *h, const Call &c, const char *after_B, Extent &e) {
    if (c.B < 0) return "B must be >= 0";
    if (after_B) return after_B;
    if (const char *bad = bad_radii_type(c)) return bad;
    if (const char *bad = check_offsets(c.offsets, c.B, e)) return bad;
    if (!h) return "null handle";
    return check_pose_records(c.xforms, c.B); // (the first rule that reads the records)
}

// ... and behind it: the atom count, then what a call with atoms must bring. `with_coords`: an array of the entry's own that
// shares `coords_text` with the coordinates (the backward's grad_out, the score's field), or the coordinates again.
const char *check_atoms(const Call &c, const Extent &e, const void *with_coords, const char *coords_text) {
    if (e.total == 0) return nullptr;
    if (const char *bad = too_many_atoms(e.total)) return bad;
    if (!c.coords || !with_coords) return coords_text;
    if (c.mode != MODE_SINGLE && !c.channels) return "channels must not be null";
    return !c.radii && c.radii_type != MVX_RADII_SCALAR ? "radii array required" : nullptr;
}

// ---- 2. inputs and metadata on the device ---------------------------------------------------------------------------
// With host-resident inputs a centre given by pointer (MVX_XF_CENTER_PTR) is a host pointer: fold it into center[]; a pose
// (MVX_XF_POSE_PTR) likewise: the record becomes the plain one pose_resolve_kernel writes for device poses.
void resolve_host_centers(mvx_xform *xf, int n) {
    for (int i = 0; i < n; ++i) {
        if (xf[i].flags & MVX_XF_POSE_PTR) {
            double pose[10];
            std::memcpy(pose, xf[i].center_ptr, sizeof(pose));
            pose_to_record(pose, xf[i]);
            continue;
        }
        if (xf[i].flags & MVX_XF_CENTER_PTR) {
            if (xf[i].center_ptr) std::memcpy(xf[i].center, xf[i].center_ptr, 3 * sizeof(double));
            xf[i].flags &= ~(uint32_t)MVX_XF_CENTER_PTR;
            xf[i].center_ptr = nullptr;
        }
    }
}

// A call's inputs as the kernels read them: offsets and records (stage_meta), the caller's arrays or copies (upload_arrays).
struct DeviceInputs {
    const int64_t *offsets = nullptr;
    const mvx_xform *xforms = nullptr;
    const double *coords = nullptr;
    const void *channels = nullptr;
    const void *radii = nullptr;
    PinnedSlot *slot = nullptr; // holds the host copies until release_slot
    char *rest = nullptr;       // the slot's bytes behind offsets and records: stage_meta's `extra`
    DeviceInputs() = default;
    explicit DeviceInputs(const Call &c) : coords(c.coords), channels(c.channels), radii(c.radii) {} // the caller's arrays
};

// Offsets (c.offsets, B + 1) and / or records (c.xforms, B) through one pinned slot into `dst` as [offsets, padded to 16 bytes |
// records] by one async copy. `resolve`: what the records point at is folded into them (host memory: before they travel; device
// poses: by pose_resolve_kernel on the device copy). The caller ends with release_slot(in.slot).
int stage_meta(mvx_handle *h, DevBuf &dst, const Call &c, bool resolve, size_t extra, DeviceInputs &in) {
    const size_t off_used = c.offsets ? (size_t)(c.B + 1) * sizeof(int64_t) : 0;
    const size_t off_bytes = align_up(off_used, 16);
    const size_t xf_bytes = c.xforms ? (size_t)c.B * sizeof(mvx_xform) : 0;
    int rc;
    if ((rc = ensure(dst, off_bytes + xf_bytes))) return rc;
    if ((rc = acquire_slot(h, off_bytes + xf_bytes + extra, &in.slot))) return rc;
    char *pin = in.slot->p;
    if (c.offsets) std::memcpy(pin, c.offsets, off_used);
    if (c.xforms) {
        std::memcpy(pin + off_bytes, c.xforms, xf_bytes);
        if (resolve && c.in_kind == MVX_HOST) resolve_host_centers(reinterpret_cast<mvx_xform *>(pin + off_bytes), c.B);
    }
    HIP_TRY(hipMemcpyAsync(dst.p, pin, off_bytes + xf_bytes, hipMemcpyHostToDevice, c.stream));
    mvx_xform *d_xf = reinterpret_cast<mvx_xform *>((char *)dst.p + off_bytes);
    if (resolve && c.in_kind != MVX_HOST && has_pose_records(c.xforms, c.B)) // the device copy becomes plain records
        HIP_TRY(launch_pose_resolve(d_xf, c.B, c.stream));
    in.offsets = c.offsets ? reinterpret_cast<const int64_t *>(dst.p) : nullptr;
    in.xforms = c.xforms ? d_xf : nullptr;
    in.rest = pin + off_bytes + xf_bytes;
    return MVX_OK;
}

// Bytes of a call's arrays for `atoms` atoms (a selection of views reads no feature rows); in a slot each is padded to 16.
struct ArrayBytes {
    size_t coords, chan, radii;
    size_t padded() const { return align_up(coords, 16) + align_up(chan, 16) + align_up(radii, 16); }
};

ArrayBytes array_bytes(const Call &c, int64_t atoms, size_t esz, bool with_features = true) {
    const size_t chan_elem = c.mode == MODE_FEATURES ? (with_features ? (size_t)c.C * esz : 0) : (c.mode == MODE_TYPES ? sizeof(int32_t) : 0);
    const size_t rad_count = c.radii_type == MVX_RADII_ATOM ? (size_t)atoms : (c.radii_type == MVX_RADII_CHANNEL ? (size_t)c.C : 0);
    return {(size_t)atoms * 3 * sizeof(double), (size_t)atoms * chan_elem, rad_count * esz};
}

// One host array into `dst` through its part of a pinned slot (memcpy, async H2D); `dev` then points at the device copy.
template <typename T>
int upload(DevBuf &dst, const T *src, size_t bytes, char *staging, hipStream_t s, const T *&dev) {
    if (bytes == 0 || !src) return MVX_OK;
    if (int e = ensure(dst, bytes)) return e;
    std::memcpy(staging, src, bytes);
    HIP_TRY(hipMemcpyAsync(dst.p, staging, bytes, hipMemcpyHostToDevice, s));
    dev = static_cast<const T *>(dst.p);
    return MVX_OK;
}

// The host arrays `in` points at through in.rest into the handle's input buffers (forward and views): `in` gets the copies.
int upload_arrays(mvx_handle *h, const ArrayBytes &n, hipStream_t s, DeviceInputs &in) {
    int rc;
    char *staging = in.rest;
    if ((rc = upload(h->in_coords, in.coords, n.coords, staging, s, in.coords))) return rc;
    staging += align_up(n.coords, 16);
    if ((rc = upload(h->in_chan, in.channels, n.chan, staging, s, in.channels))) return rc;
    return upload(h->in_radii, in.radii, n.radii, staging + align_up(n.chan, 16), s, in.radii);
}

// Host-resident arrays go through one pinned slot (a single memcpy each, then async H2D on the caller's stream);
// device-resident arrays are used where they are. Offsets and transforms always come from the host.
int stage_inputs(mvx_handle *h, Workspace &w, const RunArgs &r, int64_t total, size_t esz, hipStream_t s, DeviceInputs &in) {
    const bool host_in = (r.in_kind == MVX_HOST);
    const ArrayBytes nb = array_bytes(r, total, esz);
    const size_t extra = host_in ? nb.padded() : 0;
    const size_t meta_used = (size_t)(r.B + 1) * sizeof(int64_t);
    int rc;
    const void *meta_before = w.meta.p;
    if ((rc = ensure(w.meta, align_up(meta_used, 16) + (r.xforms ? (size_t)r.B * sizeof(mvx_xform) : 0)))) return rc;
    if (w.meta.p != meta_before) w.meta_valid = false;
    // offsets (+ transforms) go to the device only when they differ from what the last call left there
    // (same-shaped batches, the common case in a training loop, skip a 5 us copy kernel)
    const bool meta_same = !r.xforms && w.meta_valid && w.meta_last.size() == meta_used &&
                           std::memcmp(w.meta_last.data(), r.offsets, meta_used) == 0;
    // a pinned slot (and the event that releases it: a barrier packet on the stream, ~6 us of idle GPU) only when
    // something is staged through it
    in = DeviceInputs(r);
    if (!meta_same) {
        Call c = r;
        c.stream = s; // (with mvx_set_overlap: the side stream)
        if ((rc = stage_meta(h, w.meta, c, true, extra, in))) return rc;
        w.meta_last.assign(reinterpret_cast<const char *>(r.offsets), reinterpret_cast<const char *>(r.offsets) + meta_used);
        w.meta_valid = !r.xforms; // (a later call on another stream waits for this stream first: adopt_stream)
    } else if (host_in) {
        if ((rc = acquire_slot(h, extra, &in.slot))) return rc;
        in.rest = in.slot->p;
    }
    in.offsets = reinterpret_cast<const int64_t *>(w.meta.p); // (the last call's, without records, where they are the same)
    return host_in ? upload_arrays(h, nb, s, in) : MVX_OK;
}

// ---- 3. how the call is executed: plan_call (mvx_plan.hip) ---------------------------------------------------------
inline uint32_t umulhi_inverse(int d) { // n / d == __umulhi(n, inv) for the slab ids used (n * d < 2^32); d == 1 is special-cased by the kernel
    return d == 1 ? 0xffffffffu : (uint32_t)((0x100000000ull + (uint64_t)d - 1) / (uint64_t)d);
}

// ---- 4. launches bracketed by profiling events when mvx_set_profiling is on ----------------------------------------
template <typename Launch>
int timed_launch(mvx_handle *h, hipStream_t s, Launch &&launch) {
    const bool timed = h->profiling && h->ev_count < MVX_PROFILE_RING;
    if (timed) set_launch_events(h->ev[2 * h->ev_count], h->ev[2 * h->ev_count + 1]);
    const hipError_t e = launch();
    if (timed) {
        if (launch_events_pending()) { // nothing was launched (an empty job): keep the pair well defined
            set_launch_events(nullptr, nullptr);
            HIP_TRY(hipEventRecord(h->ev[2 * h->ev_count], s));
            HIP_TRY(hipEventRecord(h->ev[2 * h->ev_count + 1], s));
        }
        ++h->ev_count;
    }
    HIP_TRY(e);
    return MVX_OK;
}

// The pre-pass arguments of a call that do not point into its buffers (forward and backward share them: the backward's
// records are the forward's): the inputs as `in` holds them, no workspace pointers, no packed weights, the transform is none,
// the launch covers atoms [0, total).
PrepArgs prep_args(const mvx_handle *h, const Call &c, int64_t total, const DeviceInputs &in) {
    const bool f64 = (h->cfg.precision == 64);
    PrepArgs pa;
    std::memset(&pa, 0, sizeof(pa));
    pa.mode = c.mode;
    pa.precision = f64 ? 64 : 32;
    pa.total = total;
    pa.B = c.B;
    pa.C = c.C;
    pa.radius_scalar = c.radius_scalar;
    pa.T_scalar = -1.0;
    if (c.radii_type == MVX_RADII_SCALAR && !f64)
        scalar_radius_constants(c.radius_scalar, h->sigma32, h->cfg.density == MVX_GAUSSIAN, &pa.T_scalar, &pa.k_scalar);
    if (c.radii_type == MVX_RADII_SCALAR) pa.radii_src = RAD_SCALAR;
    else if (c.radii_type == MVX_RADII_ATOM) pa.radii_src = RAD_ATOM;
    else pa.radii_src = (c.mode == MODE_FEATURES) ? RAD_CHANNEL_FEATURES : RAD_CHANNEL_BY_TYPE;
    pa.density = h->cfg.density;
    pa.sigma32 = h->sigma32;
    pa.sigma64 = h->cfg.sigma;
    pa.g = h->g;
    pa.coords = in.coords;
    pa.radii = in.radii;
    pa.types = c.mode == MODE_TYPES ? static_cast<const int32_t *>(in.channels) : nullptr;
    pa.offsets = in.offsets;
    pa.xforms = in.xforms;
    return pa;
}

// Channel-wise features, float64 tables (float64 grids and every backward): [max radius | C thresholds | C coefficients].
constexpr size_t CHAN_TC_OFF = 16;
inline size_t chan_kc_off(int C) { return CHAN_TC_OFF + align_up((size_t)C * sizeof(double), 16); }

// What the voxelize launches of a binned forward call are (Forward::make_plan settles it, Forward::launch_binned switches on it):
// B grids by voxelize_kernel and its kin, by the grouped launch of channel-wise features, float64 grids in one launch; one summed
// grid, one in parts (mvx_set_sum_parts), or no grid at all but every molecule's moments.
enum Walk { WALK_GRIDS, WALK_GROUPED, WALK_F64, WALK_SUM, WALK_SUM_PARTS, WALK_MOMENTS };

// One forward call: what the steps of run() hand to each other, and the steps themselves in the order run() takes them.
struct Forward {
    mvx_handle *h;
    const RunArgs &r;
    const Extent ext;
    const SumCall *const sum; // not null: one summed float32 NCDHW grid (mvx_forward_sum_batch) instead of B grids
    const bool f64 = h->cfg.precision == 64, bf16 = !sum && !r.f32_plain && h->cfg.grid_type == MVX_GRID_BF16, gauss = h->cfg.density == MVX_GAUSSIAN;
    const bool chanwise = r.radii_type == MVX_RADII_CHANNEL && r.mode == MODE_FEATURES;
    const size_t esz = f64 ? sizeof(double) : sizeof(float); // element size of features, radii and the grid (but bfloat16 grids: 2)
    // make_plan:
    bool ndhwc = false, overlap = false, side_stream = false, dev_pose = false, by_value = false;
    size_t out_bytes = 0;
    void *d_out = nullptr;
    mvx_plan plan{};
    Walk walk = WALK_GRIDS;
    Workspace *w = nullptr;
    // order_prepass: the pre-pass's stream - the caller's (s), or the side stream
    hipStream_t s = r.stream, pre = s;
    DeviceInputs in;   // run(): the caller's arrays, or stage_inputs
    size_t nslabs = 0; // size_workspace
    // chan_tables:
    void *d_rmax = nullptr; // (channel-wise features: the tables chan_aux_kernel / chan_aux64_kernel write)
    double *d_Tc = nullptr;
    float *d_kc = nullptr;
    ChanGroups *d_groups = nullptr;
    int32_t *d_chan_slot = nullptr;
    // kernel_args:
    PrepArgs pa{};
    VoxArgs va{};
    bool lr_blocks = false, lane_range = false;
    Forward(mvx_handle *h_, const RunArgs &r_, const Extent &e, const SumCall *sum_ = nullptr) : h(h_), r(r_), ext(e), sum(sum_) {}
    hipStream_t staging_stream() const { return overlap ? pre : s; }
    size_t g_D3() const { return (size_t)h->g.D * h->g.D * h->g.D; }
    // ---- how this call is executed: one pure function of its shape (mvx_plan.hip, pinned by tests/test_plan.py) ----
    int make_plan() {
        const Geom &g = h->g;
        const size_t D = (size_t)g.D;
        if (bf16 && (reinterpret_cast<uintptr_t>(r.out) & 1u)) return fail(MVX_ERR_INVALID, "a bfloat16 grid must be 2-byte aligned");
        out_bytes = (size_t)(sum ? 1 : r.B) * r.C * D * D * D * (bf16 ? sizeof(uint16_t) : esz);
        d_out = r.out;
        if (r.out_kind == MVX_HOST) {
            if (int rc = ensure(h->out_stage, out_bytes)) return rc;
            d_out = h->out_stage.p;
        }
        mvx_plan_query q{};
        q.dimension = g.D;
        q.blockdim = g.bd;
        q.precision = f64 ? 64 : 32;
        q.mode = r.mode;
        q.radii_type = r.radii_type;
        q.B = r.B;
        q.C = r.C;
        // (a bfloat16 grid's vector store is 8 bytes: mvx_plan_call_grid)
        // channels-last grids (C > 1; one channel IS the contiguous layout): 16-byte channel runs for either element type
        ndhwc = !sum && !r.f32_plain && h->layout == MVX_LAYOUT_NDHWC && !f64 && r.C > 1;
        q.out_aligned16 = (reinterpret_cast<uintptr_t>(d_out) & ((bf16 && !ndhwc) ? 7u : 15u)) == 0 ? 1 : 0;
        q.total_atoms = ext.total;
        q.max_atoms = ext.max_atoms;
        plan = plan_call(q, h->knobs, ndhwc ? MVX_LAYOUT_NDHWC : MVX_LAYOUT_NCDHW, bf16 ? 2 : 4);
        if (sum) {
            // The summed grid: the binned pipeline with chunks of 32 channels on the matrix-core walk whatever C is - the plan of
            // a features call of ceil(C / 32) whole chunks (no remainder launch, no one-launch route) - over weight rows zero
            // padded to whole chunks. Feature rows that already are that wide and carry no per-atom weight are read in place.
            PlanKnobs k = h->knobs;
            k.direct_mode = 0;
            k.max_ct = 32;
            q.mode = MODE_FEATURES;
            if (q.radii_type == MVX_RADII_CHANNEL) q.radii_type = MVX_RADII_ATOM; // (radii[types]: one radius per atom, no grouped launch)
            q.C = (r.C + 31) / 32 * 32;
            if (sum->moments) q.out_aligned16 = 1; // (no grid is written: the plan of an aligned one, whatever `moments` points at)
            plan = plan_call(q, k, MVX_LAYOUT_NCDHW, 4);
            if (r.mode != MODE_FEATURES || q.C != r.C || sum->atom_weights) plan.weights_in_place = 0;
        }
        h->last_plan = plan;
        h->has_plan = true;
        walk = sum ? (sum->moments ? WALK_MOMENTS : (h->sum_parts > 1 ? WALK_SUM_PARTS : WALK_SUM))
                   : (f64 ? WALK_F64 : (plan.grouped ? WALK_GROUPED : WALK_GRIDS));
        const bool forced_pipeline = h->knobs.pipeline > 1 && r.B >= 4 * h->knobs.pipeline;
        // Cross-call overlap (mvx_set_overlap): this call's pre-pass fills the other workspace set on the side stream,
        // under the previous call's voxelize launches. Device-resident inputs and outputs only.
        // Batches only (mvx.h: "the batched three-launch path"): a per-molecule call hands over arrays its Python layer may
        // have converted on the caller's stream a moment ago, which the side stream would not wait for.
        overlap = !sum && h->overlap && !r.no_overlap && plan.route != MVX_ROUTE_DIRECT && r.B > 1 && plan.nchunk == 1 && !forced_pipeline &&
                  r.in_kind == MVX_DEVICE && r.out_kind == MVX_DEVICE;
        if (overlap) h->cur ^= 1;
        w = &h->ws[h->cur];
        // (the side stream only serves the "chunks" test option and mvx_set_overlap; chunks cut for the cache, or for the
        // gridDim.y limit, run their launches back to back on the caller's stream)
        side_stream = forced_pipeline || overlap;
        // (a device-resident pose is read on the device: its record is staged and resolved there, never passed by value)
        dev_pose = r.in_kind == MVX_DEVICE && has_pose_records(r.xforms, r.B);
        by_value = (r.B == 1 && r.in_kind == MVX_DEVICE && plan.nchunk == 1 && !dev_pose); // one molecule of device arrays
        return MVX_OK;
    }
    // ---- the pre-pass's stream and, with cross-call overlap, what it waits for before it refills its workspace set ----
    int order_prepass() {
        if (side_stream) {
            if (!h->side) {
                // lowest priority: the pre-pass should take the slots the voxelize launch leaves, not compete
                int lo = 0, hi = 0;
                HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
                HIP_TRY(hipStreamCreateWithPriority(&h->side, hipStreamNonBlocking, lo));
            }
            if (!h->ev_in) HIP_TRY(hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming));
            pre = h->side;
        }
        if (overlap) {
            if (!w->ev_pre) HIP_TRY(hipEventCreateWithFlags(&w->ev_pre, hipEventDisableTiming));
            if (!w->ev_vox) HIP_TRY(hipEventCreateWithFlags(&w->ev_vox, hipEventDisableTiming));
            // this set was last read by the call before the previous one: its launches must have drained. (Nothing makes
            // the side stream wait for the caller's stream otherwise: that is the caller's promise about the inputs.)
            if (w->vox_recorded) {
                HIP_TRY(hipStreamWaitEvent(pre, w->ev_vox, 0));
            } else { // first use of the set: order behind everything the caller's stream holds so far
                HIP_TRY(hipEventRecord(h->ev_in, s));
                HIP_TRY(hipStreamWaitEvent(pre, h->ev_in, 0));
            }
        }
        return MVX_OK;
    }
    // ---- workspace of the binned pipeline ----
    int size_workspace() {
        const size_t n_alloc = (size_t)std::max<int64_t>(ext.total, 1);
        nslabs = (size_t)r.B * ((size_t)plan.nsx * plan.nsy * plan.nzc);
        if (nslabs * (size_t)plan.ncc + 1 > (size_t)0x7fffffff) return fail(MVX_ERR_INVALID, "batch too large for one call");
        if (plan.route == MVX_ROUTE_DIRECT) return MVX_OK;
        int rc;
        if ((rc = ensure(w->rec, n_alloc * sizeof(AtomRec)))) return rc;
        if (!plan.weights_in_place && (rc = ensure(w->wbuf, n_alloc * (size_t)plan.cpad * esz))) return rc;
        if ((rc = ensure(w->xp, n_alloc * sizeof(uint2)))) return rc;
        // x-lists: packed regions, (sum(N) + 2*B) * nsx entries; slab lines: primary + extension entries per slab
        // (+ 64 B: a wave reads its eight entries of an overflowing slab's list as one group, up to seven past the list's end)
        if ((rc = ensure(w->xlist, ((size_t)ext.total + 2 * (size_t)r.B) * plan.nsx * sizeof(uint2) + 64))) return rc;
        return ensure(w->slist, nslabs * (SLAB_LINE_ENTRIES + SLAB_EXT_ENTRIES) * sizeof(uint2));
    }
    // ---- channel-wise features: the per-channel tables of this call ----
    int chan_tables() {
        if (!chanwise) return MVX_OK;
        DevBuf &aux = w->aux;
        if (f64) {
            if (int rc = ensure(aux, chan_kc_off(r.C) + (size_t)r.C * sizeof(double))) return rc;
            d_rmax = aux.p;
            d_Tc = reinterpret_cast<double *>((char *)aux.p + CHAN_TC_OFF);
            d_kc = reinterpret_cast<float *>((char *)aux.p + chan_kc_off(r.C)); // (double coefficients behind a float pointer)
            HIP_TRY(launch_chan_aux64(static_cast<const double *>(in.radii), r.C, h->cfg.density, h->cfg.sigma,
                                      static_cast<double *>(d_rmax), d_Tc, reinterpret_cast<double *>(d_kc), staging_stream()));
        } else { // [max radius | one ChanGroups per chunk of 32 channels | the channels' radius slots (int32 x C)]
            const size_t slot_off = 16 + (size_t)plan.ncc * sizeof(ChanGroups);
            if (int rc = ensure(aux, slot_off + (size_t)r.C * sizeof(int32_t))) return rc;
            d_rmax = aux.p;
            d_groups = reinterpret_cast<ChanGroups *>((char *)aux.p + 16);
            d_chan_slot = reinterpret_cast<int32_t *>((char *)aux.p + slot_off);
            HIP_TRY(launch_chan_aux(static_cast<const float *>(in.radii), r.C, h->cfg.density, h->sigma32, static_cast<float *>(d_rmax),
                                    d_groups, d_chan_slot, staging_stream()));
        }
        return MVX_OK;
    }
    // ---- kernel arguments ----
    void kernel_args() {
        const Geom &g = h->g;
        const bool direct_w = plan.weights_in_place != 0;
        uint2 *d_slist = reinterpret_cast<uint2 *>(w->slist.p);
        pa = prep_args(h, r, ext.total, in);
        pa.features = (r.mode == MODE_FEATURES) ? in.channels : nullptr;
        pa.Cpad = plan.cpad;
        if (by_value && r.xforms) pa.xf_one = r.xforms[0];
        pa.chan_aux = d_rmax;
        pa.rec = reinterpret_cast<AtomRec *>(w->rec.p);
        pa.wbuf = direct_w ? nullptr : w->wbuf.p;
        pa.xp = reinterpret_cast<uint2 *>(w->xp.p);
        va.rec = reinterpret_cast<const unsigned *>(w->rec.p);
        va.w = reinterpret_cast<const unsigned *>(direct_w ? in.channels : w->wbuf.p);
        va.slist = d_slist;
        va.slist_ext = d_slist ? d_slist + nslabs * SLAB_LINE_ENTRIES : nullptr; // extension lines live behind the primary lines
        va.Tc = d_Tc;
        va.kc = d_kc;
        if (walk == WALK_GROUPED) {
            // channels grouped by radius (chan_aux_kernel): chunks of 32 channels on the matrix-core path, one
            // threshold test and one density per radius slot and candidate, feature rows read in place
            va.Tc = reinterpret_cast<const double *>(d_groups);
            va.kc = reinterpret_cast<const float *>(d_chan_slot);
        }
        va.out = d_out;
        va.bf16 = bf16 ? 1 : 0;
        va.ndhwc = ndhwc ? 1 : 0;
        va.narrow_sub = h->narrow_sub;
        va.p.res = g.res;
        va.p.half = g.half;
        va.p.D = g.D;
        va.p.C = r.C;
        va.p.B = r.B;
        va.p.nsx = plan.nsx;
        va.p.nsy = plan.nsy;
        va.p.nzc = plan.nzc;
        va.p.ncc = plan.ncc;
        va.p.nsy_inv = umulhi_inverse(plan.nsy);
        va.p.nzc_inv = umulhi_inverse(plan.nzc);
        va.p.nsx_inv = umulhi_inverse(plan.nsx);
        va.p.ncc_inv = umulhi_inverse(plan.ncc);
        va.p.b0 = 0;
        va.p.c0 = 0;
        va.p.NW = plan.nw;
        va.p.nslab = (uint32_t)(plan.nsx * plan.nsy * plan.nzc);
        va.p.w_stride = plan.grouped ? r.C : plan.cpad;
        va.p.dcap = 0; // (set by the launchers that keep a table behind the rows / tile region)
        va.p.vec_store = plan.vec_store;
        va.p.xcd_ranges = plan.xcd_ranges;
        va.p.pace = plan.pace;
        va.p.sigma = h->cfg.sigma;
#ifdef MVX_DIAG
        va.p.dbg = h->dbg;
#endif
        // float32 grids whose rows are not whole 16-byte quads need the run-wise write-out (store_runs): compiled into the
        // per-lane-range kernels, voxelize_runs_kernel (the matrix-core walk of 32-channel chunks) and voxelize_pair_runs_kernel
        // (the candidate-pair walk of narrow chunks), nowhere else
        lr_blocks = plan.lane_range != 0;
        lane_range = lr_blocks || (!f64 && !ndhwc && !va.p.vec_store); // (channels-last: both store forms live in every kernel)
    }
    // ---- the whole call in one launch (voxelize_pair_kernel): no workspace, no pre-pass ----
    int launch_direct() {
        DirectArgs da;
        da.pa = pa;
        da.pa.rec = nullptr;
#ifdef MVX_DIAG // stamps of every workgroup (8 x 8 B each), read back with mvx_debug_read_records
        if (int rc = ensure(w->rec, nslabs * (size_t)plan.ncc * 64)) return rc;
        da.pa.rec = reinterpret_cast<AtomRec *>(w->rec.p);
        HIP_TRY(hipMemsetAsync(w->rec.p, 0, nslabs * (size_t)plan.ncc * 64, s)); // (slots filled by atomicMax need a zero start)
#endif
        da.pa.wbuf = nullptr;
        da.pa.xp = nullptr;
        da.pa.chan_aux = nullptr;
        da.N = ext.total;
        if (r.B == 1) { // one molecule: extent and transform by value, no metadata on the device
            da.pa.offsets = nullptr;
            da.pa.xforms = dev_pose ? in.xforms : nullptr;
            std::memset(&da.pa.xf_one, 0, sizeof(da.pa.xf_one));
            if (r.xforms && !dev_pose) {
                da.pa.xf_one = r.xforms[0];
                if (r.in_kind == MVX_HOST) resolve_host_centers(&da.pa.xf_one, 1);
            }
        }
        return timed_launch(h, s, [&] { return launch_voxelize_direct(da, va.p, ext.max_atoms, d_out, bf16, ndhwc, plan.ct, gauss, lr_blocks, s); });
    }
    // ---- the binned pipeline: pre-pass (prep + x-binning) and voxelize launches, chunk by chunk where the plan cuts the batch ----
    int launch_binned() {
        const int nchunk = plan.nchunk, ct = plan.ct;
        uint2 *xlist = reinterpret_cast<uint2 *>(w->xlist.p), *slist = reinterpret_cast<uint2 *>(w->slist.p);
        int rc;
        if (side_stream && !overlap) {
            while ((int)h->ev_pre.size() < nchunk) {
                hipEvent_t e = nullptr;
                HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                h->ev_pre.push_back(e);
            }
            // inputs (and the workspace, still read by the previous call's launches) are ready once `s` gets here
            HIP_TRY(hipEventRecord(h->ev_in, s));
            HIP_TRY(hipStreamWaitEvent(pre, h->ev_in, 0));
        }
        auto chunk_begin = [&](int k) { return (int)((int64_t)r.B * k / nchunk); };
        auto prepass = [&](int k) -> int {
            const int b0 = chunk_begin(k), b1 = chunk_begin(k + 1);
            pa.first = r.offsets[b0];
            pa.total = r.offsets[b1];
            HIP_TRY(launch_prep(pa, pre));
            if (sum && sum->atom_weights) // u[n, c] = fl32(a_n * w[n, c]): the packed rows of this chunk's atoms, scaled in place
                HIP_TRY(launch_scale_rows(static_cast<float *>(pa.wbuf), sum->atom_weights, pa.first, pa.total, pa.Cpad, pre));
            HIP_TRY(launch_xbin(pa.xp, in.offsets, ext.total, b0, b1 - b0, ext.max_atoms, plan.nsx, plan.nsy, plan.nzc, plan.nw, xlist, slist,
                                slist + nslabs * SLAB_LINE_ENTRIES, pre));
            if (side_stream) HIP_TRY(hipEventRecord(overlap ? w->ev_pre : h->ev_pre[k], pre));
            return MVX_OK;
        };
        const bool interleave = !side_stream && !f64 && nchunk > 1; // chunk by chunk: pre-pass, then its voxelize launch
        // a summed call in parts (mvx_set_sum_parts): parts of q molecules of the CALL, whatever the molecule chunks are; the
        // partial grids start from zero, every chunk's launch adds to those of the parts it meets, one reduction ends the call
        const int part_q = (int)(((int64_t)r.B + h->sum_parts - 1) / h->sum_parts), part_G = (int)(((int64_t)r.B + part_q - 1) / part_q);
        const size_t grid_voxels = (size_t)r.C * g_D3();
        float *part_grids = nullptr;
        if (walk == WALK_SUM_PARTS) {
            if ((rc = ensure(h->sum_part_grids, (size_t)part_G * grid_voxels * sizeof(float)))) return rc;
            part_grids = static_cast<float *>(h->sum_part_grids.p);
            HIP_TRY(hipMemsetAsync(part_grids, 0, (size_t)part_G * grid_voxels * sizeof(float), s));
        }
        if (walk == WALK_MOMENTS) { // the partials of the largest molecule chunk
            int nb_max = 0;
            for (int k = 0; k < nchunk; ++k) nb_max = std::max(nb_max, chunk_begin(k + 1) - chunk_begin(k));
            if ((rc = ensure(h->moments_part, moments_part_doubles(va.p, nb_max, sum->target ? 3 : 2) * sizeof(double)))) return rc;
        }
        double *moments_part = static_cast<double *>(h->moments_part.p);
        for (int k = 0; k < nchunk && !interleave; ++k)
            if ((rc = prepass(k))) return rc;
        for (int k = 0; k < nchunk; ++k) {
            const int b0 = chunk_begin(k), nb = chunk_begin(k + 1) - b0;
            if (interleave && (rc = prepass(k))) return rc;
            if (side_stream) HIP_TRY(hipStreamWaitEvent(s, overlap ? w->ev_pre : h->ev_pre[k], 0));
            va.p.b0 = walk == WALK_F64 ? 0 : b0;
            rc = MVX_OK;
            switch (walk) {
            case WALK_F64: // float64 grids: one launch over the whole batch, behind the pre-pass of every chunk
                if (k == nchunk - 1) rc = timed_launch(h, s, [&] { return launch_voxelize64(va, ct, gauss, chanwise, lr_blocks, s); });
                break;
            case WALK_MOMENTS: // one walk and one finish per molecule chunk: the partials are the chunk's
                rc = timed_launch(h, s, [&] { return launch_moments(va, nb, gauss, sum->target, sum->target_stride, moments_part, static_cast<double *>(d_out), s); });
                break;
            case WALK_SUM_PARTS: // one launch per molecule chunk over the parts that meet it
                rc = timed_launch(h, s, [&] { return launch_voxelize_sum_parts(va, nb, gauss, part_grids, part_q, s); });
                break;
            case WALK_SUM: // one launch per molecule chunk; chunk k > 0 continues the sums chunk k - 1 wrote
                rc = timed_launch(h, s, [&] { return launch_voxelize_sum(va, nb, gauss, sum->accumulate || k > 0, s); });
                break;
            case WALK_GROUPED: // (the groups and radius slots travel in va.Tc / va.kc: kernel_args)
                rc = timed_launch(h, s, [&] { return launch_voxelize_grouped(va, nb, gauss, lane_range, s); });
                break;
            case WALK_GRIDS:
                va.p.ncc = plan.nfull;
                va.p.ncc_inv = umulhi_inverse(plan.nfull); // (the main launch of a call with a remainder launch has nfull, not ncc, chunks per molecule)
                va.p.c0 = 0;
                // the bracket holds voxelize_kernel alone (what rocprofv3 reports under that name)
                rc = timed_launch(h, s, [&] { return launch_voxelize(va, nb, ct, gauss, lr_blocks, s); });
                if (!rc && plan.ct_rem) { // the remainder channels [nfull * ct, C) with a narrower kernel
                    va.p.ncc = 1;
                    va.p.c0 = plan.nfull * ct;
                    rc = timed_launch(h, s, [&] { return launch_voxelize(va, nb, plan.ct_rem, gauss, lr_blocks, s); });
                }
                break;
            }
            if (rc) return rc;
        }
        if (walk == WALK_SUM_PARTS) HIP_TRY(launch_sum_parts_reduce(part_grids, static_cast<float *>(d_out), grid_voxels, part_G, sum->accumulate, s));
        if (overlap) { // the next call but one refills this set
            HIP_TRY(hipEventRecord(w->ev_vox, s));
            w->vox_recorded = true;
        } else {
            w->vox_recorded = false; // (its reads are ordered on the caller's stream only)
        }
        return MVX_OK;
    }
    // ---- how both routes end: the slot may be reused once the stream gets here; a host grid is copied back and waited for ----
    int finish() {
        if (int rc = release_slot(in.slot, s)) return rc;
        if (r.out_kind == MVX_HOST) {
            HIP_TRY(hipMemcpyAsync(r.out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        return MVX_OK;
    }
};

// The steps of a forward call that passed its checks and has molecules; sum: the call writes one summed grid (SumCall).
int run_checked(mvx_handle *h, const RunArgs &r, const Extent &ext, const SumCall *sum) {
    int rc;
    CallScope scope(h, r.stream);
    if (scope.rc) return scope.rc;
    Forward f(h, r, ext, sum); // (each step reads what the steps before it set: see the members' comments)
    if ((rc = f.make_plan())) return rc;
    if ((rc = f.order_prepass())) return rc;
    if (f.by_value) f.in = DeviceInputs(r); // nothing to stage: extent and transform travel with the launches
    else if ((rc = stage_inputs(h, *f.w, r, f.ext.total, f.esz, f.staging_stream(), f.in))) return rc;
    if ((rc = f.size_workspace())) return rc;
    if ((rc = f.chan_tables())) return rc;
    f.kernel_args();
    if ((rc = f.plan.route == MVX_ROUTE_DIRECT ? f.launch_direct() : f.launch_binned())) return rc;
    return f.finish();
}

int run(mvx_handle *h, const RunArgs &r) {
    Extent ext;
    int rc = validate(h, r, ext);
    if (rc || r.B == 0) return rc;
    return run_checked(h, r, ext, nullptr);
}

// What the summed kernel and the moments kernel on its walk do not serve, each named, and the alignment of what the kernel reads or
// writes 16 bytes at a time (the grid; the target of the moments): the rules of these calls that read the handle.
int sum_config(const mvx_handle *h, const Call &c, bool moments, const void *aligned) {
    const std::string who = moments ? "moments" : "forward_sum";
    if (h->cfg.precision == 64)
        return fail(MVX_ERR_INVALID, moments ? "moments: precision 64 is not supported (moments of float32 grids only)"
                                             : "forward_sum: precision 64 is not supported (float32 sums only)");
    if (c.radii_type == MVX_RADII_CHANNEL && c.mode == MODE_FEATURES)
        return fail(MVX_ERR_INVALID, who + ": channel-wise radii with features are not supported (the grouped launch)");
    if (h->g.D % 4 != 0) return fail(MVX_ERR_INVALID, who + ": a dimension that is no multiple of 4 is not supported (run-wise write-out)");
    mvx_plan_query q{};
    q.dimension = h->g.D;
    q.blockdim = h->g.bd;
    q.precision = 32;
    q.C = c.C;
    if (plan_call(q, PlanKnobs{}).lane_range) return fail(MVX_ERR_INVALID, who + ": a blockdim that needs per-lane ranges is not supported");
    if (reinterpret_cast<uintptr_t>(aligned) & 15u) return fail(MVX_ERR_INVALID, moments ? "target must be 16-byte aligned" : "out must be 16-byte aligned");
    return MVX_OK;
}

// The checks of a summed or moments call: the shared ones in the backward entries' order (before_B / after_B: what the entry found
// wrong with its own arguments, on either side of "B must be >= 0"), then what the kernel does not serve. mvx_moments_backward_batch
// applies mvx_moments_batch's through here too.
int check_summed(const mvx_handle *h, const Call &c, bool moments, const void *aligned, const char *before_B, const char *after_B,
                 Extent &e) {
    const char *bad = bad_mode(c.mode);
    if (!bad) bad = bad_channel_count(c);
    if (!bad) bad = before_B;
    if (!bad) bad = check_batch(h, c, after_B, e);
    if (!bad) bad = check_atoms(c, e, c.coords, "coords must not be null");
    if (bad) return fail(MVX_ERR_INVALID, bad);
    return sum_config(h, c, moments, aligned);
}

// ---- mvx_forward_sum_batch (r.out: the grid) and mvx_moments_batch (sc.moments; r.out: the moments): the checks, the calls
// without atoms, then the forward's steps with the SumCall ----
int run_summed(mvx_handle *h, const RunArgs &r, const SumCall &sc, const char *before_B, const char *after_B) {
    Extent e;
    if (int rc = check_summed(h, r, sc.moments, sc.moments ? static_cast<const void *>(sc.target) : r.out, before_B, after_B, e)) return rc;
    if (e.total == 0) { // no atoms: every moment is zero (no molecules: there are none); a grid of zeros, or - accumulating - as it was
        const size_t bytes = sc.moments ? (size_t)r.B * r.C * (sc.target ? 3 : 2) * sizeof(double)
                                        : (sc.accumulate ? 0 : (size_t)r.C * h->g.D * h->g.D * h->g.D * sizeof(float));
        if (bytes == 0) return MVX_OK;
        CallScope scope(h, r.stream);
        if (scope.rc) return scope.rc;
        HIP_TRY(hipMemsetAsync(r.out, 0, bytes, r.stream));
        return MVX_OK;
    }
    return run_checked(h, r, e, &sc);
}

} // namespace

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int mvx_version(void) { return MVX_VERSION; }

const char *mvx_last_error(void) { return g_err.c_str(); }

int mvx_device_count(int *count) {
    if (!count) return fail(MVX_ERR_INVALID, "null count");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail_hip(e, "hipGetDeviceCount");
    }
    *count = n;
    return MVX_OK;
}

int mvx_create(const mvx_config *cfg, mvx_handle **out) {
    if (!cfg || !out) return fail(MVX_ERR_INVALID, "null argument");
    *out = nullptr;
    if (!(cfg->resolution > 0.0)) return fail(MVX_ERR_INVALID, "resolution must be > 0");
    if (cfg->dimension < 1 || cfg->dimension > 1020) return fail(MVX_ERR_INVALID, "dimension must be in [1, 1020]");
    if (cfg->density != MVX_GAUSSIAN && cfg->density != MVX_BINARY) return fail(MVX_ERR_INVALID, "bad density");
    if (cfg->density == MVX_GAUSSIAN && !(cfg->sigma > 0.0)) return fail(MVX_ERR_INVALID, "sigma must be > 0");
    if (cfg->precision != 0 && cfg->precision != 32 && cfg->precision != 64)
        return fail(MVX_ERR_INVALID, "precision must be 32 or 64"); // numpy/voxelizer.py:33
    if (cfg->grid_type != MVX_GRID_REAL && cfg->grid_type != MVX_GRID_BF16) return fail(MVX_ERR_INVALID, "unknown grid_type");
    if (cfg->grid_type == MVX_GRID_BF16 && cfg->precision == 64)
        return fail(MVX_ERR_INVALID, "a bfloat16 grid needs precision 32 (float32 arithmetic, rounded as it is stored)");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_err = std::string("no usable HIP device (libmvx_hip has no CPU fallback): ") +
                (e != hipSuccess ? hipGetErrorString(e) : "device count is 0");
        return MVX_ERR_NO_DEVICE;
    }
    if (cfg->device < 0 || cfg->device >= n) return fail(MVX_ERR_INVALID, "device ordinal out of range");
    mvx_handle *h = new (std::nothrow) mvx_handle();
    if (!h) return fail(MVX_ERR_ALLOC, "out of host memory");
    h->cfg = *cfg;
    h->device = cfg->device;
    make_geom(h);
    DeviceGuard guard(h->device);
    if (guard.err != hipSuccess) {
        delete h;
        return fail_hip(guard.err, "hipSetDevice");
    }
    *out = h;
    return MVX_OK;
}

int mvx_destroy(mvx_handle *h) {
    if (!h) return MVX_OK;
    DeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    delete h; // (buffers, slots, events and the side stream: freed by their owners)
    return MVX_OK;
}

int mvx_set_density(mvx_handle *h, int32_t density, double sigma) {
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (density != MVX_GAUSSIAN && density != MVX_BINARY) return fail(MVX_ERR_INVALID, "bad density");
    if (density == MVX_GAUSSIAN && !(sigma > 0.0)) return fail(MVX_ERR_INVALID, "sigma must be > 0");
    h->cfg.density = density;
    if (density == MVX_GAUSSIAN) {
        h->cfg.sigma = sigma;
        h->sigma32 = (float)sigma;
    }
    return MVX_OK;
}

int mvx_set_grid_layout(mvx_handle *h, int32_t layout) {
    if (layout != MVX_LAYOUT_NCDHW && layout != MVX_LAYOUT_NDHWC) return fail(MVX_ERR_INVALID, "unknown grid layout");
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (layout == MVX_LAYOUT_NDHWC && h->cfg.precision == 64)
        return fail(MVX_ERR_INVALID, "a channels-last grid needs precision 32");
    h->layout = layout;
    return MVX_OK;
}

int mvx_set_overlap(mvx_handle *h, int32_t enable) {
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    h->overlap = enable != 0;
    return MVX_OK;
}

int mvx_forward_features_batch(mvx_handle *h, const double *coords, const void *features, const void *radii,
                               double radius_scalar, int32_t radii_type, const int64_t *offsets,
                               const mvx_xform *xforms, int32_t B, int32_t C, void *out, int32_t in_kind,
                               int32_t out_kind, void *stream) {
    return run(h, {batch_call(MODE_FEATURES, coords, features, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream, in_kind), out, out_kind});
}

int mvx_forward_types_batch(mvx_handle *h, const double *coords, const int32_t *types, const void *radii,
                            double radius_scalar, int32_t radii_type, const int64_t *offsets,
                            const mvx_xform *xforms, int32_t B, int32_t C, void *out, int32_t in_kind,
                            int32_t out_kind, void *stream) {
    return run(h, {batch_call(MODE_TYPES, coords, types, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream, in_kind), out, out_kind});
}

int mvx_forward_single_batch(mvx_handle *h, const double *coords, const void *radii, double radius_scalar,
                             int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B,
                             void *out, int32_t in_kind, int32_t out_kind, void *stream) {
    return run(h, {batch_call(MODE_SINGLE, coords, nullptr, radii, radius_scalar, radii_type, offsets, xforms, B, 1, stream, in_kind), out, out_kind});
}

int mvx_forward_features(mvx_handle *h, const double *coords, const void *features, const void *radii,
                         double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xform,
                         void *out, int32_t in_kind, int32_t out_kind, void *stream) {
    const int64_t off[2] = {0, N};
    return mvx_forward_features_batch(h, coords, features, radii, radius_scalar, radii_type, off, xform, 1, C, out,
                                      in_kind, out_kind, stream);
}

int mvx_forward_types(mvx_handle *h, const double *coords, const int32_t *types, const void *radii,
                      double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xform,
                      void *out, int32_t in_kind, int32_t out_kind, void *stream) {
    const int64_t off[2] = {0, N};
    return mvx_forward_types_batch(h, coords, types, radii, radius_scalar, radii_type, off, xform, 1, C, out,
                                   in_kind, out_kind, stream);
}

int mvx_forward_single(mvx_handle *h, const double *coords, const void *radii, double radius_scalar,
                       int32_t radii_type, int64_t N, const mvx_xform *xform, void *out, int32_t in_kind,
                       int32_t out_kind, void *stream) {
    const int64_t off[2] = {0, N};
    return mvx_forward_single_batch(h, coords, radii, radius_scalar, radii_type, off, xform, 1, out, in_kind,
                                    out_kind, stream);
}

int mvx_forward_sum_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                          double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B,
                          int32_t C, const float *atom_weights, float *out, int32_t accumulate, void *stream) {
    const char *own = !out ? "out must not be null" : ((accumulate != 0 && accumulate != 1) ? "accumulate must be 0 or 1" : nullptr);
    return run_summed(h, {batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream), out, MVX_DEVICE},
                      SumCall{atom_weights, accumulate != 0}, own, nullptr);
}

int mvx_moments_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii, double radius_scalar,
                      int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B, int32_t C, const float *target,
                      double *moments, void *stream) {
    return run_summed(h, {batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream), moments, MVX_DEVICE},
                      SumCall{nullptr, false, true, target}, nullptr, (!moments && B > 0) ? "moments must not be null" : nullptr);
}

// ---- views of one shared cloud (mvx_views.hip) ----------------------------------------------------------------------------
namespace {

// A views call has N atoms, B views and no offsets. What its entries reject before any device is touched. `own`: what the entry
// found wrong with its own arguments (null: nothing);
// the handle is looked at last, so every other rule can be checked without a device.
int validate_views(const mvx_handle *h, const Call &v, const char *own) {
    if (v.mode != MODE_FEATURES && v.mode != MODE_TYPES && v.mode != MODE_SINGLE) return fail(MVX_ERR_INVALID, "bad mode");
    if (v.radii_type < MVX_RADII_SCALAR || v.radii_type > MVX_RADII_CHANNEL) return fail(MVX_ERR_INVALID, "bad radii_type");
    if (v.in_kind != MVX_HOST && v.in_kind != MVX_DEVICE) return fail(MVX_ERR_INVALID, "bad memory kind");
    if (v.B < 0 || v.N < 0 || v.C <= 0) return fail(MVX_ERR_INVALID, "B and N must be >= 0 and C > 0");
    if (v.B > 0 && !v.xforms)
        return fail(MVX_ERR_INVALID, "xforms must not be null (a view of the whole cloud is a record with flags = 0)");
    if (v.radii_type == MVX_RADII_CHANNEL && v.mode == MODE_SINGLE)
        return fail(MVX_ERR_INVALID, "Channel-Wise Radii Type is not supported"); // numpy/voxelizer.py:443
    if (v.mode == MODE_SINGLE && v.C != 1) return fail(MVX_ERR_INVALID, "single mode has one channel");
    if (v.N > 0 && !v.coords) return fail(MVX_ERR_INVALID, "coords must not be null");
    if (!v.radii && (v.radii_type == MVX_RADII_CHANNEL || (v.radii_type == MVX_RADII_ATOM && v.N > 0)))
        return fail(MVX_ERR_INVALID, "radii array required");
    if (v.N > 0 && v.mode == MODE_TYPES && !v.channels) return fail(MVX_ERR_INVALID, "types must not be null");
    if (const char *bad = too_many_atoms(v.N)) return fail(MVX_ERR_INVALID, bad);
    if (own) return fail(MVX_ERR_INVALID, own);
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    return reject(check_pose_records(v.xforms, v.B)); // (the first rule that reads the records)
}

// the cloud and the views' transforms as device arrays
struct ViewInputs : DeviceInputs {
    explicit ViewInputs(const Call &v) : DeviceInputs(v) {}
    std::vector<mvx_xform> xforms_host; // the records as run() gets them (host centres folded in)
};

// Host-resident arrays are uploaded once - the cloud, not B copies of it - through a pinned slot; `select_only`: the feature
// rows are not needed (the selection reads coordinates, types and radii).
int stage_views(mvx_handle *h, const Call &v, bool select_only, ViewInputs &in) {
    const bool host_in = v.in_kind == MVX_HOST;
    const ArrayBytes nb = array_bytes(v, v.N, h->cfg.precision == 64 ? sizeof(double) : sizeof(float), !select_only);
    in.xforms_host.assign(v.xforms, v.xforms + v.B);
    if (host_in) resolve_host_centers(in.xforms_host.data(), v.B);
    Call records = v;
    records.xforms = in.xforms_host.data(); // (host poses: folded in just now)
    int rc;
    if ((rc = stage_meta(h, h->view_xf, records, !host_in, host_in ? nb.padded() : 0, in))) return rc;
    if (host_in && (rc = upload_arrays(h, nb, v.stream, in))) return rc;
    return release_slot(in.slot, v.stream);
}

// Count, scan, one copy of the offsets to the host (THE synchronisation of a views call), fill. `index` / `capacity`: the
// caller's buffer, or null: the handle's own (mvx_forward_views), grown to fit. Returns MVX_ERR_INVALID with the offsets filled
// in when the caller's buffer is too small.
int select_views(mvx_handle *h, const Call &v, const ViewInputs &in, int64_t *index, int64_t capacity, bool own_index,
                 int64_t *offsets_host) {
    hipStream_t s = v.stream; // (N > 0: the entries answer a cloud without atoms themselves)
    const int64_t ntiles64 = (v.N + VIEW_TILE - 1) / VIEW_TILE;
    const bool views_in_x = v.B >= ntiles64;
    if (std::min<int64_t>(v.B, ntiles64) > 65535 || (int64_t)v.B * ntiles64 >= (int64_t)1 << 31)
        return fail(MVX_ERR_INVALID, "too many (view, tile) pairs for one launch");
    ViewArgs a;
    a.pa = prep_args(h, v, v.N, in);
    a.ntiles = (int32_t)ntiles64;
    a.views_in_x = views_in_x ? 1 : 0;
    int rc;
    if (a.pa.radii_src == RAD_CHANNEL_FEATURES) {
        if ((rc = ensure(h->view_aux, 16))) return rc;
        HIP_TRY(launch_view_rmax(in.radii, v.C, a.pa.precision, h->view_aux.p, s));
        a.pa.chan_aux = h->view_aux.p;
    }
    const size_t M = (size_t)v.B * (size_t)ntiles64;
    const size_t off_bytes = (size_t)(v.B + 1) * sizeof(int64_t);
    if ((rc = ensure(h->view_counts, M * sizeof(int32_t)))) return rc;
    if ((rc = ensure(h->view_base, M * sizeof(int64_t)))) return rc;
    if ((rc = ensure(h->view_off, off_bytes))) return rc;
    PinnedSlot *slot = nullptr; // (device to host, waited for below: nothing to release)
    if ((rc = acquire_slot(h, off_bytes, &slot))) return rc;
    HIP_TRY(launch_view_count(a, static_cast<int32_t *>(h->view_counts.p), s));
    HIP_TRY(launch_view_scan(static_cast<const int32_t *>(h->view_counts.p), v.B, a.ntiles, static_cast<int64_t *>(h->view_base.p),
                             static_cast<int64_t *>(h->view_off.p), s));
    HIP_TRY(hipMemcpyAsync(slot->p, h->view_off.p, off_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    std::memcpy(offsets_host, slot->p, off_bytes);
    const int64_t total = offsets_host[v.B];
    if (own_index) {
        if ((rc = ensure(h->view_index, (size_t)total * sizeof(int64_t)))) return rc;
        index = static_cast<int64_t *>(h->view_index.p);
    } else if (capacity < total || (total > 0 && !index)) {
        return fail(MVX_ERR_INVALID, "index_capacity is smaller than offsets[B]: size the buffer from offsets_out_host and call again");
    }
    if (total > 0) HIP_TRY(launch_view_fill(a, static_cast<const int64_t *>(h->view_base.p), index, s));
    return MVX_OK;
}

inline int gather_width(size_t row_bytes, const void *a, const void *b) {
    const uintptr_t bits = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | (uintptr_t)row_bytes;
    return (bits & 15u) == 0 ? 16 : ((bits & 7u) == 0 ? 8 : 4);
}

// The compact batch of a selection: the rows of the cloud (device arrays) that `index` names, gathered by one launch into the
// handle's view_* buffers for `batch` - coordinates, feature rows or types, atom-wise radii (other radii stay where they are).
int gather_views(mvx_handle *h, const Call &cloud, const int64_t *index, int64_t total, Call &batch) {
    const size_t esz = h->cfg.precision == 64 ? sizeof(double) : sizeof(float);
    GatherArgs g{};
    g.index = index;
    g.total = total;
    auto add = [&](DevBuf &dst, const void *src, size_t row_bytes) -> int {
        if (int e = ensure(dst, (size_t)total * row_bytes)) return e;
        const int i = g.narr++;
        g.src[i] = static_cast<const char *>(src);
        g.dst[i] = static_cast<char *>(dst.p);
        g.row_bytes[i] = (int32_t)row_bytes;
        g.width[i] = gather_width(row_bytes, src, dst.p);
        return MVX_OK;
    };
    int rc;
    if ((rc = add(h->view_coords, cloud.coords, 3 * sizeof(double)))) return rc;
    batch.coords = static_cast<const double *>(h->view_coords.p);
    batch.channels = cloud.channels;
    if (cloud.mode != MODE_SINGLE) {
        if ((size_t)cloud.C * esz > (size_t)1 << 30) return fail(MVX_ERR_INVALID, "too many channels");
        if ((rc = add(h->view_chan, cloud.channels, cloud.mode == MODE_FEATURES ? (size_t)cloud.C * esz : sizeof(int32_t)))) return rc;
        batch.channels = h->view_chan.p;
    }
    batch.radii = cloud.radii; // (scalar: unused; channel-wise: the C radii as they are)
    if (cloud.radii_type == MVX_RADII_ATOM) {
        if ((rc = add(h->view_radii, cloud.radii, esz))) return rc;
        batch.radii = h->view_radii.p;
    }
    HIP_TRY(launch_view_gather(g, cloud.stream));
    return MVX_OK;
}

// The views of a call as a batch of B molecules: the Call that run(), run_summed() or backward_impl() takes, with the host offsets
// and records it points at. As constructed: B molecules without atoms (what a cloud of no atoms is); compact_views fills it.
struct ViewBatch : Call {
    std::vector<int64_t> own_offsets; // B + 1
    std::vector<mvx_xform> records;   // as stage_views left them (host centres and poses folded in)
    explicit ViewBatch(const Call &v) : Call(v), own_offsets((size_t)v.B + 1, 0) { offsets = own_offsets.data(); }
};

// The compact batch of the views `v` (B > 0) of a cloud, on the device: scope, staging and selection - or the caller's `index`
// with its host offsets `index_offsets` (mvx_score_views), and nothing staged -, "too many atoms", gather. A cloud without atoms
// leaves `b` as constructed, whatever the caller's selection says, and touches no device. `features`: the call after it reads the
// feature rows of a host-resident cloud. Synchronises the stream once (select_views; not with the caller's index).
int compact_views(mvx_handle *h, const Call &v, bool features, const int64_t *index, const int64_t *index_offsets, ViewBatch &b) {
    if (v.N == 0) return MVX_OK;
    CallScope scope(h, v.stream);
    int rc = scope.rc;
    if (rc) return rc;
    Call cloud = v; // ... as device arrays
    if (index) {
        b.offsets = index_offsets;
    } else {
        ViewInputs in(v);
        if ((rc = stage_views(h, v, !features, in))) return rc;
        if ((rc = select_views(h, v, in, nullptr, 0, true, b.own_offsets.data()))) return rc;
        index = static_cast<const int64_t *>(h->view_index.p);
        cloud.coords = in.coords;
        cloud.channels = in.channels;
        cloud.radii = in.radii;
        b.records.swap(in.xforms_host);
        b.xforms = b.records.data();
    }
    const int64_t total = b.offsets[v.B];
    if (const char *bad = too_many_atoms(total)) return fail(MVX_ERR_INVALID, bad);
    b.in_kind = MVX_DEVICE;
    return gather_views(h, cloud, index, total, b);
}

} // namespace

int mvx_select_views(mvx_handle *h, const double *coords, const int32_t *types, const void *radii, double radius_scalar,
                     int32_t radii_type, int32_t mode, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                     int64_t *index_out, int64_t index_capacity, int64_t *offsets_out_host, int32_t in_kind, void *stream) {
    const Call v = views_call(mode, coords, types, radii, radius_scalar, radii_type, N, xforms, B, C, stream, in_kind);
    const char *own = !offsets_out_host ? "offsets_out_host must not be null"
                      : (index_capacity < 0 || (index_capacity > 0 && !index_out)) ? "index_out must not be null" : nullptr;
    if (int rc = validate_views(h, v, own)) return rc;
    if (B == 0 || N == 0) {
        std::fill(offsets_out_host, offsets_out_host + B + 1, (int64_t)0);
        return MVX_OK;
    }
    CallScope scope(h, v.stream);
    if (scope.rc) return scope.rc;
    ViewInputs in(v);
    if (int rc = stage_views(h, v, true, in)) return rc;
    return select_views(h, v, in, index_out, index_capacity, false, offsets_out_host);
}

int mvx_forward_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                      double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                      void *out, int32_t in_kind, int32_t out_kind, void *stream) {
    const Call v = views_call(mode, coords, channels, radii, radius_scalar, radii_type, N, xforms, B, C, stream, in_kind);
    const char *own = (out_kind != MVX_HOST && out_kind != MVX_DEVICE) ? "bad memory kind"
                      : (B > 0 && !out) ? "out must not be null"
                      : (B > 0 && N > 0 && mode != MODE_SINGLE && !channels) ? "channels must not be null" : nullptr;
    if (int rc = validate_views(h, v, own)) return rc;
    if (B == 0) return MVX_OK;
    ViewBatch batch(v); // (N == 0: B molecules without atoms, zero grids)
    if (int rc = compact_views(h, v, true, nullptr, nullptr, batch)) return rc;
    return run(h, {batch, out, out_kind, N > 0}); // (a compact batch does not overlap its pre-pass: RunArgs::no_overlap)
}

// The summed grid of B views: mvx_forward_views' selection and gather, then run_summed on the compact batch in place of run(). What
// reads the handle (sum_config) is checked before a device is touched; run_summed checks the batch again, to no effect.
int mvx_forward_views_sum(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                          double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                          const float *view_weights, float *out, int32_t accumulate, void *stream) {
    const Call v = views_call(mode, coords, channels, radii, radius_scalar, radii_type, N, xforms, B, C, stream);
    const char *own = (accumulate != 0 && accumulate != 1) ? "accumulate must be 0 or 1"
                      : (B > 0 && !out) ? "out must not be null"
                      : (B > 0 && N > 0 && mode != MODE_SINGLE && !channels) ? "channels must not be null" : nullptr;
    if (int rc = validate_views(h, v, own)) return rc;
    if (B == 0) return MVX_OK;
    if (int rc = sum_config(h, v, false, out)) return rc;
    ViewBatch batch(v); // (N == 0: B views without atoms, zeros or nothing)
    SumCall sc{nullptr, accumulate != 0};
    int rc = compact_views(h, v, true, nullptr, nullptr, batch);
    if (rc) return rc;
    const int64_t total = batch.offsets[B];
    if (view_weights && total > 0) { // one weight per selected atom, from the offsets select_views left on the device
        CallScope scope(h, v.stream);
        if (scope.rc) return scope.rc;
        if ((rc = ensure(h->view_w, (size_t)total * sizeof(float)))) return rc;
        HIP_TRY(launch_view_weights(static_cast<float *>(h->view_w.p), view_weights, static_cast<const int64_t *>(h->view_off.p), B, total, v.stream));
        sc.atom_weights = static_cast<const float *>(h->view_w.p);
    }
    return run_summed(h, {batch, out, MVX_DEVICE}, sc, nullptr, nullptr); // (a summed call never overlaps its pre-pass: Forward::make_plan)
}

int mvx_set_sum_parts(mvx_handle *h, int32_t parts) {
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (parts < 1 || parts > SUM_PARTS_MAX) return fail(MVX_ERR_INVALID, "sum parts must be 1 ... 64");
    h->sum_parts = parts;
    return MVX_OK;
}

// mvx_backward_batch (BWD_PLAIN), mvx_backward_radii_batch (BWD_RADII: grad_radii as well) and mvx_backward_density_batch
// (BWD_DENSITY: grad_sigma / grad_rscalar / grad_radii, each or NULL); mvx_score_batch (BWD_SCORE: `grad_out` is the constant
// field, ScoreCall its stride and the score outputs; grad_coords and grad_features each or NULL); mvx_moments_backward_batch
// (BWD_MOMENTS, one Backward per molecule chunk: `grad_out` is the chunk's float32 grids in handle-owned scratch, `moments` its
// coefficients and the target); mvx_score_hessian_batch (BWD_HESS: mvx_score_batch's field, stride and scores in ScoreCall, its own
// outputs and the pivots in HessCall; no grad_coords and no grad_features)
enum BackwardKind { BWD_PLAIN, BWD_RADII, BWD_DENSITY, BWD_SCORE, BWD_MOMENTS, BWD_HESS };

struct ScoreCall {
    int64_t mol_stride;  // 0 (one field for all molecules) or C * D^3
    double *scores;      // (B,)
    double *atom_scores; // (total,) or null: handle-owned workspace
};

struct HessCall {
    const double *pivots;                 // (B, 3) device or null: the origin
    double *atom_grad, *atom_hess;        // (total, 3), (total, 6), each or null: handle-owned workspace
    double *twist_grad, *twist_hess;      // (B, 6), (B, 36), each or null
};

// mvx_score_hessian_flex_batch next to its HessCall (`on`: the call is that entry)
struct FlexCall {
    bool on;
    int32_t T;
    const int32_t *axes, *moves; // (B, T, 2), (total,)
    double *flex_grad, *flex_hess; // (B, n), (B, n, n) or null, n = 6 + T
    double *atom_pos;              // (total, 3) or null
};

// What a backward call reads next to its Call and where its results go (outputs a kind does not have are null).
struct GradOut {
    BackwardKind kind;
    const void *grad_out; // dL/dgrid; BWD_SCORE: the field
    double *grad_coords;
    void *grad_features;
    double *grad_radii, *grad_sigma, *grad_rscalar;
    ScoreCall score; // BWD_SCORE only
    MomentsArgs moments{}; // BWD_MOMENTS only
    HessCall hess{};       // BWD_HESS only
    FlexCall flex{};       // BWD_HESS only: mvx_score_hessian_flex_batch
    bool scoring() const { return kind == BWD_SCORE || kind == BWD_HESS; } // walks a constant field: ScoreCall is filled
};

namespace {

// The stride between the fields or targets of two molecules or views: 0 (one for all) or C * D^3. Its sign is judged without the
// handle, stride_fits against it; one text per argument name.
const char *const BAD_FIELD_MOL_STRIDE = "field_mol_stride must be 0 (one shared field) or C * D^3 (one field per molecule)";
const char *const BAD_FIELD_VIEW_STRIDE = "field_view_stride must be 0 (one shared field) or C * D^3 (one field per view)";
const char *const BAD_TARGET_STRIDE = "target_view_stride must be 0 (one shared target) or C * D^3 (one target per view)";
bool stride_fits(const mvx_handle *h, int32_t C, int64_t stride) {
    return stride == 0 || (uint64_t)stride == (uint64_t)C * (uint64_t)h->g.D * (uint64_t)h->g.D * (uint64_t)h->g.D;
}

// ---- what is checked before any device is touched, up to the first rule that needs the atom count ----
int check_backward(const mvx_handle *h, const Call &c, const GradOut &o, Extent &e) {
    if (const char *bad = bad_mode(c.mode)) return fail(MVX_ERR_INVALID, bad);
    if (o.grad_features && c.mode != MODE_FEATURES) return fail(MVX_ERR_INVALID, "grad_features exists in features mode only");
    if (const char *bad = bad_channel_count(c)) return fail(MVX_ERR_INVALID, bad);
    if (o.kind == BWD_RADII) { // (grad_coords and grad_features may both be null: grad_radii is an output)
        if (!o.grad_radii) return fail(MVX_ERR_INVALID, "grad_radii must not be null");
        if (c.radii_type == MVX_RADII_SCALAR)
            return fail(MVX_ERR_INVALID, "radii_type: scalar radii have no radius array for grad_radii (atom-wise or channel-wise radii only)");
        if (c.radii_type == MVX_RADII_CHANNEL && c.mode == MODE_SINGLE)
            return fail(MVX_ERR_INVALID, "radii_type: channel-wise radii are not supported in single mode (no grad_radii)");
    } else if (o.kind == BWD_DENSITY) { // (grad_coords and grad_features may both be null here too)
        if (!o.grad_sigma && !o.grad_rscalar && !o.grad_radii)
            return fail(MVX_ERR_INVALID, "grad_sigma, grad_radius_scalar and grad_radii are all null");
        if (o.grad_rscalar && c.radii_type != MVX_RADII_SCALAR)
            return fail(MVX_ERR_INVALID, "radii_type: grad_radius_scalar exists with scalar radii only");
        if (o.grad_radii && c.radii_type == MVX_RADII_SCALAR)
            return fail(MVX_ERR_INVALID, "radii_type: scalar radii have no radius array for grad_radii (grad_radius_scalar gives dL/dr)");
        if (c.radii_type == MVX_RADII_CHANNEL && c.mode == MODE_SINGLE)
            return fail(MVX_ERR_INVALID, "radii_type: channel-wise radii are not supported in single mode");
    } else if (o.scoring()) { // (grad_coords, grad_features and atom_scores may all be null: scores alone)
        if (o.score.mol_stride < 0) return fail(MVX_ERR_INVALID, BAD_FIELD_MOL_STRIDE);
        if (c.B > 0 && !o.score.scores) return fail(MVX_ERR_INVALID, "scores must not be null");
    } else if (!o.grad_coords && !o.grad_features) {
        return fail(MVX_ERR_INVALID, "grad_coords and grad_features are both null");
    }
    return reject(check_batch(h, c, nullptr, e));
}

// ---- ... and, behind check_atoms, what a call with atoms must bring that reads the handle ----
int check_backward_grid(const mvx_handle *h, const Call &c, const GradOut &o) {
    const size_t gsz = h->cfg.grid_type == MVX_GRID_BF16 ? 2 : (h->cfg.precision == 64 ? 8 : 4);
    const size_t D = (size_t)h->g.D;
    if (D * D * D * gsz >= ((size_t)1 << 32)) return fail(MVX_ERR_INVALID, "one channel of the grid must stay below 4 GiB");
    if (o.scoring() && !stride_fits(h, c.C, o.score.mol_stride)) return fail(MVX_ERR_INVALID, BAD_FIELD_MOL_STRIDE);
    return MVX_OK;
}

// ---- the two rules of the Hessian entries (`form`: "batch" | "views", for the names in the text), behind every rule of the score
// entry of that form ----
int check_hessian(const Call &c, const GradOut &o, const char *form) {
    if (c.radii_type == MVX_RADII_CHANNEL && c.mode == MODE_FEATURES)
        return fail(MVX_ERR_INVALID, std::string("radii_type: channel-wise radii in features mode are not supported by mvx_score_hessian_") +
                                         form + " (mvx_score_" + form + " gives their first-order gradients)");
    if (o.hess.twist_hess && !o.hess.twist_grad) return fail(MVX_ERR_INVALID, "twist_hess needs twist_grad");
    return MVX_OK;
}

// ---- ... and the three of mvx_score_hessian_flex_batch behind them (`atoms`: the call has any) ----
int check_flex(const Call &c, const GradOut &o, bool atoms) {
    if (!o.flex.on) return MVX_OK;
    if (o.flex.T < 0 || o.flex.T > FLEX_MAX_T) return fail(MVX_ERR_INVALID, "T must be 0 ... 32");
    // (a batch without atoms has no masks: its moves may be null)
    if (o.flex.T > 0 && c.B > 0 && (!o.flex.axes || (atoms && !o.flex.moves)))
        return fail(MVX_ERR_INVALID, "axes and moves must not be null with T > 0");
    if (c.B > 0 && !o.flex.flex_grad) return fail(MVX_ERR_INVALID, "flex_grad must not be null");
    return MVX_OK;
}

// zeros for `nradii` radius gradients, for sigma and for a scalar radius, where the call has these outputs
int zero_density_grads(const GradOut &o, size_t nradii, hipStream_t s) {
    if (o.grad_radii && nradii) HIP_TRY(hipMemsetAsync(o.grad_radii, 0, nradii * sizeof(double), s));
    if (o.grad_sigma) HIP_TRY(hipMemsetAsync(o.grad_sigma, 0, sizeof(double), s));
    if (o.grad_rscalar) HIP_TRY(hipMemsetAsync(o.grad_rscalar, 0, sizeof(double), s));
    return MVX_OK;
}

// ---- no atoms: no gradient rows; channel-wise radii still get their C zeros, sigma and a scalar radius their zero ----
int backward_no_atoms(const Call &c, const GradOut &o) {
    if (int rc = zero_density_grads(o, c.radii_type == MVX_RADII_CHANNEL ? (size_t)c.C : 0, c.stream)) return rc;
    if (o.scoring()) HIP_TRY(hipMemsetAsync(o.score.scores, 0, (size_t)c.B * sizeof(double), c.stream)); // (every molecule scores 0)
    if (o.hess.twist_grad) HIP_TRY(hipMemsetAsync(o.hess.twist_grad, 0, (size_t)c.B * 6 * sizeof(double), c.stream));
    if (o.hess.twist_hess) HIP_TRY(hipMemsetAsync(o.hess.twist_hess, 0, (size_t)c.B * 36 * sizeof(double), c.stream));
    if (o.flex.on) { // (no atoms: every torsion is inert)
        const size_t n = 6 + (size_t)o.flex.T;
        HIP_TRY(hipMemsetAsync(o.flex.flex_grad, 0, (size_t)c.B * n * sizeof(double), c.stream));
        if (o.flex.flex_hess) HIP_TRY(hipMemsetAsync(o.flex.flex_hess, 0, (size_t)c.B * n * n * sizeof(double), c.stream));
    }
    return MVX_OK;
}

// One backward call with atoms, once it is on the device: what its steps share, the staging, and one step per BackwardKind.
struct Backward {
    mvx_handle *h;
    const Call &c;
    const GradOut &o;
    const int64_t total;
    const hipStream_t s = c.stream;
    const bool f64 = h->cfg.precision == 64;
    // which instantiation every walk of this call takes; key.chanwise: channel-wise radii for features, with their tables
    // (the scratch grids of the moments walk are float32 whatever the handle's grid type)
    const WalkKey key{o.kind == BWD_MOMENTS ? 0 : (h->cfg.grid_type == MVX_GRID_BF16 ? 1 : (f64 ? 2 : 0)), c.mode, h->cfg.density == MVX_GAUSSIAN,
                      c.radii_type == MVX_RADII_CHANNEL && c.mode == MODE_FEATURES};
    void *d_kc = nullptr; // channel-wise features: the per-channel coefficients (ga.kc)
    DeviceInputs in{c};   // the caller's arrays; stage(): the device copy of offsets and records, the slot they went through
    GradArgs ga;
    Backward(mvx_handle *h_, const Call &c_, const GradOut &o_, int64_t total_) : h(h_), c(c_), o(o_), total(total_) {}
    // ---- staging, channel-wise tables and the forward's pre-pass: the records of every atom, bit for bit ----
    int stage() {
        int rc; // (offsets and records through a pinned slot, as the forward stages them; the poses are device memory)
        if ((rc = stage_meta(h, h->grad_meta, c, true, 0, in))) return rc;
        if ((rc = ensure(h->grad_rec, (size_t)total * sizeof(AtomRec)))) return rc;
        if ((rc = ensure(h->grad_xp, (size_t)total * sizeof(uint2)))) return rc;
        void *d_rmax = nullptr;
        double *d_Tc = nullptr;
        if (key.chanwise) {
            if ((rc = ensure(h->grad_aux, chan_kc_off(c.C) + (size_t)c.C * sizeof(double)))) return rc;
            d_rmax = h->grad_aux.p;
            d_Tc = reinterpret_cast<double *>((char *)h->grad_aux.p + CHAN_TC_OFF);
            d_kc = (char *)h->grad_aux.p + chan_kc_off(c.C);
            HIP_TRY(launch_grad_chan(c.radii, c.C, f64, key.gauss, h->sigma32, h->cfg.sigma, d_rmax, d_Tc, d_kc, s));
        }
        PrepArgs pa = prep_args(h, c, total, in); // (no packed weights: the gradient kernel reads the feature rows in place)
        pa.Cpad = c.C;
        pa.chan_aux = d_rmax;
        pa.rec = reinterpret_cast<AtomRec *>(h->grad_rec.p);
        pa.wbuf = nullptr;
        pa.xp = reinterpret_cast<uint2 *>(h->grad_xp.p);
        HIP_TRY(launch_prep(pa, s));

        // "grad_order" 1: neighbouring atoms in neighbouring waves of one XCD, so that the rows of G they read meet in its L2
        // (the order decides which wave runs an atom, never what the atom's gradients are)
        ga.order = nullptr;
        ga.xcd_span = 0;
        if (h->grad_order) {
            const size_t ob = grad_order_bytes(total, c.B, h->g.D);
            if ((rc = ensure(h->grad_sort, ob))) return rc;
            HIP_TRY(launch_grad_order(pa.rec, in.offsets, c.B, total, h->g.D, h->grad_sort.p, h->grad_sort.cap, &ga.order, s));
            ga.xcd_span = (int32_t)(((total + 3) / 4 + 7) / 8);
        }
        ga.rec = pa.rec;
        ga.w = c.mode == MODE_FEATURES ? c.channels : nullptr;
        ga.g = o.grad_out;
        ga.offsets = in.offsets;
        ga.xforms = in.xforms;
        ga.Tc = d_Tc;
        ga.kc = d_kc;
        ga.grad_coords = o.grad_coords;
        ga.grad_w = o.grad_features;
        ga.total = total;
        ga.B = c.B;
        ga.C = c.C;
        ga.D = h->g.D;
        ga.res = h->g.res;
        ga.half = h->g.half;
        return MVX_OK;
    }

    int plain() { // BWD_PLAIN
        HIP_TRY(launch_grad(ga, key, s));
        return MVX_OK;
    }
    // BWD_SCORE: one walk over the field: the per-atom scores (the caller's array, or workspace), dS/dcoords and dS/dfeatures
    // where asked for; then every molecule's atoms summed in a fixed order
    int score() {
        ScoreArgs sa;
        sa.atom_scores = o.score.atom_scores;
        sa.mol_stride = o.score.mol_stride;
        if (!sa.atom_scores) {
            if (int rc = ensure(h->score_atoms, (size_t)total * sizeof(double))) return rc;
            sa.atom_scores = reinterpret_cast<double *>(h->score_atoms.p);
        }
        HIP_TRY(launch_score(ga, sa, key, s));
        HIP_TRY(launch_score_reduce(sa.atom_scores, in.offsets, c.B, o.score.scores, s));
        return MVX_OK;
    }
    // BWD_HESS: one walk over the field writes s_n, g_n and H_n of every atom (the caller's arrays, or workspace), then every
    // molecule's atoms are summed in a fixed order: the scores as mvx_score_batch sums them, and the twist gradient and Hessian
    int hess() {
        if (int rc = ensure(h->hess_rows, (size_t)total * 10 * sizeof(double))) return rc;
        double *ws = reinterpret_cast<double *>(h->hess_rows.p);
        HessArgs ha;
        ha.atom_scores = ws;
        ha.atom_grad = o.hess.atom_grad ? o.hess.atom_grad : ws + (size_t)total;
        ha.atom_hess = o.hess.atom_hess ? o.hess.atom_hess : ws + (size_t)total * 4;
        ha.mol_stride = o.score.mol_stride;
        HIP_TRY(launch_score_hess(ga, ha, key, s));
        HIP_TRY(launch_score_reduce(ha.atom_scores, in.offsets, c.B, o.score.scores, s));
        double *tg = o.hess.twist_grad, *th = o.hess.twist_hess;
        double *subset = nullptr;
        if (o.flex.on) { // the twist values are the first six rows and columns: workspace where the caller wants none
            const size_t nsub = (size_t)c.B * (size_t)o.flex.T * FLEX_SUBSET;
            if (int rc = ensure(h->flex_ws, (nsub + (size_t)c.B * 42) * sizeof(double))) return rc;
            subset = reinterpret_cast<double *>(h->flex_ws.p);
            if (!tg) tg = subset + nsub;
            if (!th) th = subset + nsub + (size_t)c.B * 6;
        }
        if (tg) HIP_TRY(launch_twist_reduce(ga.rec, ha.atom_grad, ha.atom_hess, in.offsets, o.hess.pivots, c.B, tg, th, s));
        if (o.flex.on) {
            FlexArgs fa{ga.rec, ha.atom_grad, ha.atom_hess, in.offsets, o.hess.pivots, o.flex.axes, o.flex.moves, tg, th, subset,
                        o.flex.flex_grad, o.flex.flex_hess, o.flex.atom_pos, total, c.B, o.flex.T};
            HIP_TRY(launch_flex(fa, s));
        }
        return MVX_OK;
    }
    // BWD_MOMENTS: the walk over the chunk's grids with the upstream formed from them, the coefficients and the target
    int moments() {
        HIP_TRY(launch_moments_grad(ga, o.moments, key, s));
        return MVX_OK;
    }
    // binary density: zero radius and sigma gradients (the a.e. derivative), the walk for the other outputs only
    int binary() {
        if (int rc = zero_density_grads(o, (size_t)(c.radii_type == MVX_RADII_CHANNEL ? c.C : total), s)) return rc;
        return (o.grad_coords || o.grad_features) ? plain() : MVX_OK;
    }
    // bytes of the radius partials, one per atom or per (channel, atom), in front of the stage sums in grad_rpart
    size_t part_bytes() const { return align_up((key.chanwise ? (size_t)c.C * (size_t)total : (size_t)total) * sizeof(double), 256); }
    // BWD_DENSITY: the radius walk with its partials kept per atom (or per channel and atom) in grad_rpart, whatever the radii
    // type: [partials | channel-wise: stage sums of grad_radii_reduce, C doubles for a grad_radii nobody asked for | the chunk
    // sums of all atoms]. One walk feeds grad_radii, grad_sigma and grad_rscalar.
    int density() {
        if (!key.gauss) return binary();
        const bool by_channel = c.radii_type == MVX_RADII_CHANNEL;
        const size_t rstage_bytes = by_channel ? align_up((grad_radii_stage_doubles(total, c.C) + (size_t)c.C) * sizeof(double), 256) : 0;
        if (int rc = ensure(h->grad_rpart, part_bytes() + rstage_bytes + grad_density_stage_doubles(total) * sizeof(double))) return rc;
        RadiiArgs ra;
        ra.radii = c.radii;
        ra.grad_radii = nullptr;
        ra.part = reinterpret_cast<double *>(h->grad_rpart.p);
        double *rstage = reinterpret_cast<double *>((char *)h->grad_rpart.p + part_bytes());
        double *dstage = reinterpret_cast<double *>((char *)h->grad_rpart.p + part_bytes() + rstage_bytes);
        // sigma and the scalar radius as the forward used them
        const double sigma = f64 ? h->cfg.sigma : (double)h->sigma32;
        const double rsc = f64 ? c.radius_scalar : (double)(float)c.radius_scalar;
        HIP_TRY(launch_grad_radii(ga, ra, key, s));
        if (by_channel && (o.grad_radii || key.chanwise)) { // (features: grad_sigma needs the stage sums of this reduction)
            double *gr = o.grad_radii ? o.grad_radii : rstage + grad_radii_stage_doubles(total, c.C);
            HIP_TRY(launch_grad_radii_reduce(ra.part, key.chanwise ? nullptr : static_cast<const int32_t *>(c.channels), c.radii,
                                             key.chanwise ? d_kc : nullptr, f64, total, c.C, rstage, gr, s));
        }
        if (key.chanwise) {
            if (o.grad_sigma) HIP_TRY(launch_grad_density_chan(rstage, total, c.C, d_kc, f64, sigma, o.grad_sigma, s));
        } else if (o.grad_sigma || o.grad_rscalar || !by_channel) {
            HIP_TRY(launch_grad_density_sum(ra.part, total, c.radii, f64, by_channel ? nullptr : o.grad_radii, rsc, sigma, dstage,
                                            o.grad_sigma, o.grad_rscalar, s));
        }
        return MVX_OK;
    }
    // BWD_RADII: radius partials straight into grad_radii (one radius per atom), or per atom / per (channel, atom) into
    // grad_rpart and reduced over all atoms of the call in a fixed order (channel-wise radii: one radius vector for the batch)
    int radii() {
        if (!key.gauss) return binary();
        RadiiArgs ra;
        ra.radii = c.radii;
        ra.grad_radii = o.grad_radii;
        ra.part = nullptr;
        double *stage = nullptr;
        if (c.radii_type == MVX_RADII_CHANNEL) {
            if (int rc = ensure(h->grad_rpart, part_bytes() + grad_radii_stage_doubles(total, c.C) * sizeof(double))) return rc;
            ra.part = reinterpret_cast<double *>(h->grad_rpart.p);
            stage = reinterpret_cast<double *>((char *)h->grad_rpart.p + part_bytes());
        }
        HIP_TRY(launch_grad_radii(ga, ra, key, s));
        if (c.radii_type == MVX_RADII_CHANNEL)
            HIP_TRY(launch_grad_radii_reduce(ra.part, key.chanwise ? nullptr : static_cast<const int32_t *>(c.channels), c.radii,
                                             key.chanwise ? d_kc : nullptr, f64, total, c.C, stage, o.grad_radii, s));
        return MVX_OK;
    }
};

int backward_impl(mvx_handle *h, const Call &c, const GradOut &o) {
    Extent e;
    int rc = check_backward(h, c, o, e);
    if (rc) return rc;
    const bool radii_by_channel = o.grad_radii && c.radii_type == MVX_RADII_CHANNEL;
    if (e.total == 0 && !radii_by_channel && o.kind != BWD_DENSITY && o.kind != BWD_HESS && !(o.kind == BWD_SCORE && c.B > 0)) return MVX_OK;
    if ((rc = reject(check_atoms(c, e, o.grad_out, o.scoring() ? "coords / field must not be null" : "coords / grad_out must not be null")))) return rc;
    if (e.total > 0 && (rc = check_backward_grid(h, c, o))) return rc;
    if (o.kind == BWD_HESS) { // its own rules, behind every rule of mvx_score_batch
        if ((rc = check_hessian(c, o, "batch"))) return rc;
        if ((rc = check_flex(c, o, e.total > 0))) return rc;
        if (c.B == 0) return MVX_OK;
    }
    CallScope scope(h, c.stream);
    if (scope.rc) return scope.rc;
    if (e.total == 0) return backward_no_atoms(c, o);
    Backward b(h, c, o, e.total);
    if ((rc = b.stage())) return rc;
    switch (o.kind) {
    case BWD_PLAIN: rc = b.plain(); break;
    case BWD_SCORE: rc = b.score(); break;
    case BWD_RADII: rc = b.radii(); break;
    case BWD_DENSITY: rc = b.density(); break;
    case BWD_MOMENTS: rc = b.moments(); break; // (not reached: moments_backward runs its chunks itself)
    case BWD_HESS: rc = b.hess(); break;
    }
    return rc ? rc : release_slot(b.in.slot, c.stream);
}

// ---- mvx_moments_backward_batch behind its checks, with atoms: the molecule chunks the forward cuts, one after the other. Per chunk
// the forward as a call of its own into the float32 NCDHW scratch (rebased offsets: a molecule's bits do not depend on its
// batch), then the backward's pre-pass and the moments walk over the chunk's atoms. The scratch holds the largest chunk. With one
// target per molecule (target_stride = C * D^3: mvx_moments_backward_views) the target base moves with the chunk, as the
// coefficients' does: the walk's molecule index is chunk-relative. ----
int moments_backward(mvx_handle *h, const Call &c, const Extent &e, const float *target, int64_t target_stride, const double *grad_moments,
                     double *grad_coords, void *grad_features) {
    CallScope scope(h, c.stream);
    if (scope.rc) return scope.rc;
    int rc;
    // the cut: the plan of the forward call that would write all B float32 grids
    RunArgs whole{c, nullptr, MVX_DEVICE};
    whole.no_overlap = whole.f32_plain = true;
    Forward cut(h, whole, e);
    if ((rc = cut.make_plan())) return rc;
    mvx_plan plan = cut.plan;
    // ... and further, until the grids of a chunk fit the scratch bound (the forward's cut counts pre-pass bytes, not grids)
    const size_t D3 = (size_t)h->g.D * h->g.D * h->g.D, K = target ? 3 : 2;
    const double mol_bytes = (double)c.C * (double)D3 * sizeof(float);
    const int64_t fit = std::max<int64_t>(1, (int64_t)(h->mgrad_scratch / mol_bytes));
    plan.nchunk = (int32_t)std::max<int64_t>(plan.nchunk, (c.B + fit - 1) / fit);
    const int nchunk = plan.nchunk;
    auto chunk_begin = [&](int k) { return (int)((int64_t)c.B * k / nchunk); }; // (Forward::launch_binned's)
    int nb_max = 0;
    for (int k = 0; k < nchunk; ++k) nb_max = std::max(nb_max, chunk_begin(k + 1) - chunk_begin(k));
    if ((rc = ensure(h->mgrad_grids, (size_t)nb_max * c.C * D3 * sizeof(float)))) return rc;
    if ((rc = ensure(h->mgrad_coef, (size_t)c.B * c.C * 3 * sizeof(float)))) return rc;
    float *coef = static_cast<float *>(h->mgrad_coef.p);
    HIP_TRY(launch_moments_coef(grad_moments, (int64_t)c.B * c.C, (int32_t)K, coef, c.stream));
    const bool profiling = h->profiling; // (the chunks' forward launches are no timed launches of the caller's)
    h->profiling = false;
    const size_t chan_elem = c.mode == MODE_FEATURES ? (size_t)c.C * sizeof(float) : (c.mode == MODE_TYPES ? sizeof(int32_t) : 0);
    std::vector<int64_t> off;
    for (int k = 0; k < nchunk && !rc; ++k) {
        const int b0 = chunk_begin(k), nb = chunk_begin(k + 1) - b0;
        const int64_t a0 = c.offsets[b0], n = c.offsets[b0 + nb] - a0;
        if (n == 0) continue; // (no atoms: no gradient rows)
        Call sub = c;
        Extent se;
        off.assign(c.offsets + b0, c.offsets + b0 + nb + 1);
        for (int64_t &v : off) v -= a0;
        for (int b = 0; b < nb; ++b) se.max_atoms = std::max(se.max_atoms, off[b + 1] - off[b]);
        se.total = n;
        sub.offsets = off.data();
        sub.B = nb;
        sub.coords = c.coords + 3 * a0;
        sub.channels = c.channels ? static_cast<const char *>(c.channels) + (size_t)a0 * chan_elem : nullptr;
        sub.radii = (c.radii && c.radii_type == MVX_RADII_ATOM) ? static_cast<const char *>(c.radii) + (size_t)a0 * sizeof(float) : c.radii;
        sub.xforms = c.xforms ? c.xforms + b0 : nullptr;
        RunArgs fwd{sub, h->mgrad_grids.p, MVX_DEVICE};
        fwd.no_overlap = fwd.f32_plain = true;
        if ((rc = run_checked(h, fwd, se, nullptr))) break;
        GradOut o{BWD_MOMENTS, h->mgrad_grids.p, grad_coords ? grad_coords + 3 * a0 : nullptr,
                  grad_features ? static_cast<float *>(grad_features) + (size_t)a0 * c.C : nullptr, nullptr, nullptr, nullptr, {},
                  {coef + (size_t)b0 * c.C * 3, target ? target + (size_t)b0 * (size_t)target_stride : nullptr, target_stride}};
        Backward b(h, sub, o, n);
        if ((rc = b.stage())) break;
        if ((rc = b.moments())) break;
        rc = release_slot(b.in.slot, c.stream);
    }
    h->profiling = profiling;
    h->last_plan = plan; // (mvx_debug_last_plan: the cut of this call, not the plan of its last chunk)
    h->has_plan = true;
    return rc;
}

// what is wrong with the offsets of a selection handed back by the caller (B + 1 entries), or null
const char *bad_view_offsets(const int64_t *offsets, int32_t B, Extent &e) {
    if (!offsets) return "offsets_host must not be null with an index";
    if (const char *bad = check_offsets(offsets, B, e)) return bad;
    return too_many_atoms(e.total) ? "too many atoms: offsets[B] must stay below 2^31" : nullptr;
}

// what the views entries say when an output laid out per (view, atom) row comes without the selection that orders the rows
const char *const ROWS_NEED_INDEX =
    "atom_scores, grad_coords and grad_features need an index: their rows are laid out in selection order (mvx_select_views)";

// What is wrong with the caller's selection of a views entry, or null: `rows` (the call has outputs laid out per row) needs one,
// and an index comes with its host offsets, whose extent lands in `e`.
const char *bad_selection(const int64_t *index, const int64_t *offsets_host, int32_t B, bool rows, Extent &e) {
    if (!index) return rows ? ROWS_NEED_INDEX : nullptr;
    return B > 0 ? bad_view_offsets(offsets_host, B, e) : nullptr;
}

// mvx_score_views (BWD_SCORE) and mvx_score_hessian_views (BWD_HESS) behind their argument lists: the rules that are checked
// before any device is touched, the selection (the caller's, or made here: one stream synchronisation) and the gather, then the
// walk of the batch entry on the compact batch, with the records as the caller gave them (device centres and poses). The two
// rules of the Hessian are judged here, behind the stride: backward_impl would find them only behind the gather.
int score_views_impl(mvx_handle *h, const Call &v, const int64_t *index, const int64_t *offsets_host, const GradOut &o) {
    const bool rows = o.score.atom_scores || o.grad_coords || o.grad_features || o.hess.atom_grad || o.hess.atom_hess;
    Extent e; // of the caller's selection
    const char *own = nullptr;
    if (o.grad_features && v.mode != MODE_FEATURES) own = "grad_features exists in features mode only";
    else if (o.score.mol_stride < 0) own = BAD_FIELD_VIEW_STRIDE;
    else if (v.B > 0 && !o.score.scores) own = "scores must not be null";
    else own = bad_selection(index, offsets_host, v.B, rows, e);
    if (!own && v.B > 0 && v.N > 0) {
        if (v.mode == MODE_FEATURES && !v.channels) own = "channels must not be null";
        else if (!o.grad_out && (!index || e.total > 0)) own = "field must not be null";
    }
    if (int rc = validate_views(h, v, own)) return rc;
    if (!stride_fits(h, v.C, o.score.mol_stride)) return fail(MVX_ERR_INVALID, BAD_FIELD_VIEW_STRIDE);
    if (o.kind == BWD_HESS)
        if (int rc = check_hessian(v, o, "views")) return rc;
    if (v.B == 0) return MVX_OK;
    ViewBatch batch(v); // (N == 0: B views without atoms, exact zeros, whatever the caller's selection says)
    if (int rc = compact_views(h, v, false, index, offsets_host, batch)) return rc;
    return backward_impl(h, batch, o);
}

} // namespace

int mvx_backward_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                       double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B,
                       int32_t C, const void *grad_out, double *grad_coords, void *grad_features, void *stream) {
    return backward_impl(h, batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream),
                         {BWD_PLAIN, grad_out, grad_coords, grad_features, nullptr, nullptr, nullptr, {}});
}

int mvx_backward_radii_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                             double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B,
                             int32_t C, const void *grad_out, double *grad_coords, void *grad_features, double *grad_radii,
                             void *stream) {
    return backward_impl(h, batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream),
                         {BWD_RADII, grad_out, grad_coords, grad_features, grad_radii, nullptr, nullptr, {}});
}

int mvx_backward_density_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                               double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B,
                               int32_t C, const void *grad_out, double *grad_coords, void *grad_features, double *grad_radii,
                               double *grad_sigma, double *grad_radius_scalar, void *stream) {
    return backward_impl(h, batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream),
                         {BWD_DENSITY, grad_out, grad_coords, grad_features, grad_radii, grad_sigma, grad_radius_scalar, {}});
}

int mvx_score_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                    double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B, int32_t C,
                    const void *field, int64_t field_mol_stride, double *scores, double *atom_scores, double *grad_coords,
                    void *grad_features, void *stream) {
    return backward_impl(h, batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream),
                         {BWD_SCORE, field, grad_coords, grad_features, nullptr, nullptr, nullptr, {field_mol_stride, scores, atom_scores}});
}

int mvx_score_hessian_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                            double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B,
                            int32_t C, const void *field, int64_t field_mol_stride, const double *pivots, double *scores,
                            double *atom_grad, double *atom_hess, double *twist_grad, double *twist_hess, void *stream) {
    GradOut o{BWD_HESS, field, nullptr, nullptr, nullptr, nullptr, nullptr, {field_mol_stride, scores, nullptr}};
    o.hess = {pivots, atom_grad, atom_hess, twist_grad, twist_hess};
    return backward_impl(h, batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream), o);
}

int mvx_score_hessian_flex_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                                 double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                                 int32_t B, int32_t C, const void *field, int64_t field_mol_stride, const double *pivots,
                                 double *scores, double *atom_grad, double *atom_hess, double *twist_grad, double *twist_hess,
                                 int32_t T, const int32_t *axes, const int32_t *moves, double *flex_grad, double *flex_hess,
                                 double *atom_pos, void *stream) {
    GradOut o{BWD_HESS, field, nullptr, nullptr, nullptr, nullptr, nullptr, {field_mol_stride, scores, nullptr}};
    o.hess = {pivots, atom_grad, atom_hess, twist_grad, twist_hess};
    o.flex = {true, T, axes, moves, flex_grad, flex_hess, atom_pos};
    return backward_impl(h, batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream), o);
}

int mvx_moments_backward_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                               double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                               int32_t B, int32_t C, const float *target, const double *grad_moments, double *grad_coords,
                               mvx_real *grad_features, void *stream) {
    const Call c = batch_call(mode, coords, channels, radii, radius_scalar, radii_type, offsets, xforms, B, C, stream);
    Extent e;
    // mvx_moments_batch's rules (it has no `moments` to miss here), then this entry's own; all before a device is touched
    if (int rc = check_summed(h, c, true, target, nullptr, nullptr, e)) return rc;
    if (B > 0 && !grad_moments) return fail(MVX_ERR_INVALID, "grad_moments must not be null");
    if (grad_features && mode != MODE_FEATURES) return fail(MVX_ERR_INVALID, "grad_features exists in features mode only");
    if (!grad_coords && !grad_features) return fail(MVX_ERR_INVALID, "grad_coords and grad_features are both null");
    if (B == 0 || e.total == 0) return MVX_OK; // (no atoms: no gradient rows, nothing is launched)
    // (one channel of a float32 grid stays below 4 GiB at every dimension mvx_create admits: the walk's 32-bit byte offsets hold)
    return moments_backward(h, c, e, target, 0, grad_moments, grad_coords, grad_features);
}

int mvx_pose_grad_batch(mvx_handle *h, const double *coords, const double *grad_coords, const int64_t *offsets,
                        const mvx_xform *xforms, int32_t B, double *grad_pose, void *stream) {
    // ---- what is checked before any device is touched ----
    if (B < 0) return fail(MVX_ERR_INVALID, "B must be >= 0");
    if (B > 0 && !grad_pose) return fail(MVX_ERR_INVALID, "grad_pose must not be null");
    if (B > 0 && !xforms) return fail(MVX_ERR_INVALID, "xforms must not be null");
    Extent e;
    if (const char *bad = check_offsets(offsets, B, e)) return fail(MVX_ERR_INVALID, bad);
    if (e.total > 0 && (!coords || !grad_coords)) return fail(MVX_ERR_INVALID, "coords / grad_coords must not be null");
    for (int b = 0; b < B; ++b)
        if (!(xforms[b].flags & MVX_XF_POSE_PTR)) return fail(MVX_ERR_INVALID, "every record must be a MVX_XF_POSE_PTR record");
    if (const char *bad = check_pose_records(xforms, B)) return fail(MVX_ERR_INVALID, bad);
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (B == 0) return MVX_OK;

    const Call c = batch_call(0, nullptr, nullptr, nullptr, 0.0, 0, offsets, xforms, B, 0, stream); // (what stage_meta reads)
    CallScope scope(h, c.stream);
    if (scope.rc) return scope.rc;
    // offsets and records through a pinned slot, as the backward entries stage them (the records stay as they are: the
    // kernel reads each pose through its pointer)
    DeviceInputs in;
    if (int rc = stage_meta(h, h->pose_meta, c, false, 0, in)) return rc;
    HIP_TRY(launch_pose_grad(coords, grad_coords, in.offsets, in.xforms, B, grad_pose, c.stream));
    return release_slot(in.slot, c.stream);
}

int mvx_score_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii,
                    double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                    const int64_t *index, const int64_t *offsets_host, const void *field, int64_t field_view_stride,
                    double *scores, double *atom_scores, double *grad_coords, void *grad_features, void *stream) {
    return score_views_impl(h, views_call(mode, coords, channels, radii, radius_scalar, radii_type, N, xforms, B, C, stream), index, offsets_host,
                            {BWD_SCORE, field, grad_coords, grad_features, nullptr, nullptr, nullptr, {field_view_stride, scores, atom_scores}});
}

// The Hessians of B views: mvx_score_views' rules, selection and gather, then mvx_score_hessian_batch's walk and reductions on the
// compact batch.
int mvx_score_hessian_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                            double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                            const int64_t *index, const int64_t *offsets_host, const void *field, int64_t field_view_stride,
                            const double *pivots, double *scores, double *atom_grad, double *atom_hess, double *twist_grad,
                            double *twist_hess, void *stream) {
    GradOut o{BWD_HESS, field, nullptr, nullptr, nullptr, nullptr, nullptr, {field_view_stride, scores, nullptr}};
    o.hess = {pivots, atom_grad, atom_hess, twist_grad, twist_hess};
    return score_views_impl(h, views_call(mode, coords, channels, radii, radius_scalar, radii_type, N, xforms, B, C, stream), index, offsets_host, o);
}

// The moments of B views: the selection (the caller's, or made here) and the gather of mvx_score_views, then mvx_moments_batch's
// walk on the compact batch, each view against its own target where the stride says so. What reads the handle (the stride against
// C * D^3, sum_config) is checked before a device is touched; run_summed checks the batch again, to no effect.
int mvx_moments_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const void *radii, double radius_scalar,
                      int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B, const int64_t *index,
                      const int64_t *offsets_host, const float *target, int64_t target_view_stride, double *moments, void *stream) {
    const Call v = views_call(mode, coords, channels, radii, radius_scalar, radii_type, N, xforms, B, C, stream);
    Extent e; // of the caller's selection
    const char *own = nullptr;
    if (B > 0 && !moments) own = "moments must not be null";
    else if (target_view_stride < 0) own = BAD_TARGET_STRIDE;
    else own = bad_selection(index, offsets_host, B, false, e);
    if (!own && B > 0 && N > 0 && mode == MODE_FEATURES && !channels) own = "channels must not be null";
    if (int rc = validate_views(h, v, own)) return rc;
    if (!stride_fits(h, C, target_view_stride)) return fail(MVX_ERR_INVALID, BAD_TARGET_STRIDE);
    if (B == 0) return MVX_OK;
    if (int rc = sum_config(h, v, true, target)) return rc;
    ViewBatch batch(v); // (N == 0: B views without atoms, exact zeros, whatever the caller's selection says)
    if (int rc = compact_views(h, v, true, index, offsets_host, batch)) return rc; // (no index: the selection itself, one stream synchronisation)
    // (a compact batch does not overlap its pre-pass, and a summed call never does: Forward::make_plan)
    return run_summed(h, {batch, moments, MVX_DEVICE, N > 0}, SumCall{nullptr, false, true, target, target ? target_view_stride : 0}, nullptr, nullptr);
}

// dL/dcoords and dL/dfeatures per (view, atom) row of a selection, through the moments of the views: the gather of
// mvx_moments_views with the caller's index, then mvx_moments_backward_batch's chunks on the compact batch.
int mvx_moments_backward_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                               double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                               const int64_t *index, const int64_t *offsets_host, const float *target, int64_t target_view_stride,
                               const double *grad_moments, double *grad_coords_rows, mvx_real *grad_features_rows, void *stream) {
    const Call v = views_call(mode, coords, channels, radii, radius_scalar, radii_type, N, xforms, B, C, stream);
    Extent e; // of the caller's selection
    // mvx_moments_backward_batch's own rules, then this entry's; validate_views puts them in front of the handle
    const char *own = nullptr;
    if (B > 0 && !grad_moments) own = "grad_moments must not be null";
    else if (grad_features_rows && mode != MODE_FEATURES) own = "grad_features exists in features mode only";
    else if (!grad_coords_rows && !grad_features_rows) own = "grad_coords and grad_features are both null";
    else if (target_view_stride < 0) own = BAD_TARGET_STRIDE;
    else own = bad_selection(index, offsets_host, B, true, e); // (every output is laid out per row)
    if (!own && B > 0 && N > 0 && mode == MODE_FEATURES && !channels) own = "channels must not be null";
    if (int rc = validate_views(h, v, own)) return rc;
    if (!stride_fits(h, C, target_view_stride)) return fail(MVX_ERR_INVALID, BAD_TARGET_STRIDE);
    if (B == 0) return MVX_OK;
    if (int rc = sum_config(h, v, true, target)) return rc;
    if (N == 0 || e.total == 0) return MVX_OK; // (no selected atom: no gradient rows, nothing is launched)
    ViewBatch batch(v);
    if (int rc = compact_views(h, v, true, index, offsets_host, batch)) return rc;
    // (one channel of a float32 grid stays below 4 GiB at every dimension mvx_create admits: the walk's 32-bit byte offsets hold)
    return moments_backward(h, batch, e, target, target ? target_view_stride : 0, grad_moments, grad_coords_rows, grad_features_rows);
}

int mvx_views_reduce(mvx_handle *h, const int64_t *index, const int64_t *offsets_host, int32_t B, int64_t N, const void *rows,
                     int32_t width, int32_t row_type, void *out, void *stream) {
    // ---- what is checked before any device is touched ----
    if (B < 0 || N < 0) return fail(MVX_ERR_INVALID, "B and N must be >= 0");
    if (width <= 0 || width > VIEW_REDUCE_MAX_WIDTH) return fail(MVX_ERR_INVALID, "width must be > 0 (and at most 65535 * 32)");
    if (row_type != MVX_ROW_FLOAT && row_type != MVX_ROW_DOUBLE) return fail(MVX_ERR_INVALID, "bad row_type");
    if (N >= (int64_t)1 << 31) return fail(MVX_ERR_INVALID, "too many atoms");
    Extent e;
    if (B > 0)
        if (const char *bad = bad_view_offsets(offsets_host, B, e)) return fail(MVX_ERR_INVALID, bad);
    if (e.total > 0 && (!index || !rows)) return fail(MVX_ERR_INVALID, "index / rows must not be null");
    if (N > 0 && !out) return fail(MVX_ERR_INVALID, "out must not be null");
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (N == 0) return MVX_OK;

    const Call c = batch_call(0, nullptr, nullptr, nullptr, 0.0, 0, offsets_host, nullptr, B, 0, stream); // (what stage_meta reads)
    CallScope scope(h, c.stream);
    if (scope.rc) return scope.rc;
    const bool f64 = row_type == MVX_ROW_DOUBLE;
    if (e.total == 0) { // no view holds an atom: exact zeros
        HIP_TRY(hipMemsetAsync(out, 0, (size_t)N * (size_t)width * (f64 ? sizeof(double) : sizeof(float)), c.stream));
        return MVX_OK;
    }
    // the offsets through a pinned slot, as the backward entries stage theirs
    DeviceInputs in;
    if (int rc = stage_meta(h, h->view_red_off, c, false, 0, in)) return rc;
    HIP_TRY(launch_view_reduce(index, in.offsets, B, N, rows, width, f64, out, c.stream));
    return release_slot(in.slot, c.stream);
}

namespace {

// The two step entries: the rules of a step record in their order, then its launch. `flex`: the whole record when `a` is the
// base of one, else null; `after_B` and `after_state`: what the flex entry found wrong with T, behind "B must be >= 0", and with
// its angles, behind the state pointers (null: nothing, as in check_batch).
int run_lm_step(mvx_handle *h, const LmArgs &a, const FlexLmArgs *flex, const char *after_B, const char *after_state, void *stream) {
    // ---- what is checked before any device is touched ----
    if (a.B < 0) return fail(MVX_ERR_INVALID, "B must be >= 0");
    if (after_B) return fail(MVX_ERR_INVALID, after_B);
    if (a.B > 0 && (!a.q || !a.t || !a.S || !a.G || !a.H || !a.lam || !a.taken || !a.dropped || !a.q2 || !a.t2))
        return fail(MVX_ERR_INVALID, "q, t, S, G, H, lam, taken, dropped, q2 and t2 must not be null");
    if (after_state) return fail(MVX_ERR_INVALID, after_state);
    if (a.B > 0 && a.have_trial && (!a.S2 || !a.G2 || !a.H2)) return fail(MVX_ERR_INVALID, "S2, G2 and H2 must not be null with have_trial");
    if (a.max_dropped < 1) return fail(MVX_ERR_INVALID, "max_dropped must be >= 1");
    if (!(a.lam_down > 0.0) || !(a.lam_up > 0.0) || !std::isfinite(a.lam_down) || !std::isfinite(a.lam_up))
        return fail(MVX_ERR_INVALID, "lam_down and lam_up must be finite and > 0");
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (a.B == 0) return MVX_OK;

    const hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    CallScope scope(h, s);
    if (scope.rc) return scope.rc;
    HIP_TRY(flex ? launch_flex_lm_step(*flex, s) : launch_lm_step(a, s));
    return MVX_OK;
}

} // namespace

int mvx_lm_step(mvx_handle *h, int32_t B, int32_t have_trial, double lam_down, double lam_up, int32_t max_dropped, double *q,
                double *t, double *S, double *G, double *H, double *lam, int32_t *taken, int32_t *dropped, double *q2, double *t2,
                const double *S2, const double *G2, const double *H2, double *xi, void *stream) {
    const LmArgs a{B, have_trial != 0, max_dropped, lam_down, lam_up, q, t, S, G, H, lam, taken, dropped, q2, t2, S2, G2, H2, xi};
    return run_lm_step(h, a, nullptr, nullptr, nullptr, stream);
}

int mvx_flex_lm_step(mvx_handle *h, int32_t B, int32_t T, int32_t have_trial, double lam_down, double lam_up, int32_t max_dropped,
                     double *q, double *t, double *theta, double *S, double *G, double *H, double *lam, int32_t *taken,
                     int32_t *dropped, double *q2, double *t2, double *theta2, const double *S2, const double *G2, const double *H2,
                     double *x, void *stream) {
    const FlexLmArgs a{{B, have_trial != 0, max_dropped, lam_down, lam_up, q, t, S, G, H, lam, taken, dropped, q2, t2, S2, G2, H2, x},
                       theta, theta2, T};
    return run_lm_step(h, a, &a, T < 0 || T > FLEX_MAX_T ? "T must be 0 ... 32" : nullptr,
                       B > 0 && T > 0 && (!theta || !theta2) ? "theta and theta2 must not be null with T > 0" : nullptr, stream);
}

int mvx_apply_torsions(mvx_handle *h, const double *coords, const int64_t *offsets, int32_t B, int32_t T, const int32_t *axes,
                       const int32_t *moves, const double *angles, double *out, void *stream) {
    // ---- what is checked before any device is touched ----
    if (B < 0) return fail(MVX_ERR_INVALID, "B must be >= 0");
    if (T < 0 || T > FLEX_MAX_T) return fail(MVX_ERR_INVALID, "T must be 0 ... 32");
    Extent e;
    if (const char *bad = check_offsets(offsets, B, e)) return fail(MVX_ERR_INVALID, bad);
    if (const char *bad = too_many_atoms(e.total)) return fail(MVX_ERR_INVALID, bad);
    if (e.total > 0 && (!coords || !out)) return fail(MVX_ERR_INVALID, "coords / out must not be null");
    if (e.total > 0 && T > 0 && (!axes || !moves || !angles)) return fail(MVX_ERR_INVALID, "axes, moves and angles must not be null with T > 0");
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (e.total == 0) return MVX_OK;

    const Call c = batch_call(0, nullptr, nullptr, nullptr, 0.0, 0, offsets, nullptr, B, 0, stream); // (what stage_meta reads)
    CallScope scope(h, c.stream);
    if (scope.rc) return scope.rc;
    DeviceInputs in; // the offsets through a pinned slot, as the backward entries stage theirs
    if (int rc = stage_meta(h, h->flex_off, c, false, 0, in)) return rc;
    HIP_TRY(launch_torsion_apply(coords, in.offsets, B, T, axes, moves, angles, out, c.stream));
    return release_slot(in.slot, c.stream);
}

int mvx_apply_torsions_backward(mvx_handle *h, const double *conformer, const int64_t *offsets, int32_t B, int32_t T,
                                const int32_t *axes, const int32_t *moves, const double *angles, const double *grad_out,
                                double *grad_coords, double *grad_angles, void *stream) {
    // ---- what is checked before any device is touched (mvx_apply_torsions' rules in its order) ----
    if (B < 0) return fail(MVX_ERR_INVALID, "B must be >= 0");
    if (T < 0 || T > FLEX_MAX_T) return fail(MVX_ERR_INVALID, "T must be 0 ... 32");
    Extent e;
    if (const char *bad = check_offsets(offsets, B, e)) return fail(MVX_ERR_INVALID, bad);
    if (const char *bad = too_many_atoms(e.total)) return fail(MVX_ERR_INVALID, bad);
    if (e.total > 0 && (!conformer || !grad_out || !grad_coords))
        return fail(MVX_ERR_INVALID, "conformer / grad_out / grad_coords must not be null");
    if (e.total > 0 && T > 0 && (!axes || !moves || !angles || !grad_angles))
        return fail(MVX_ERR_INVALID, "axes, moves, angles and grad_angles must not be null with T > 0");
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (e.total == 0) return MVX_OK;

    const Call c = batch_call(0, nullptr, nullptr, nullptr, 0.0, 0, offsets, nullptr, B, 0, stream); // (what stage_meta reads)
    CallScope scope(h, c.stream);
    if (scope.rc) return scope.rc;
    const size_t bytes = (size_t)e.total * 3 * sizeof(double);
    if (T == 0) { // no turn to pull the rows back through
        if (grad_coords != grad_out) HIP_TRY(hipMemcpyAsync(grad_coords, grad_out, bytes, hipMemcpyDeviceToDevice, c.stream));
        return MVX_OK;
    }
    if (int rc = ensure(h->torsion_pos, bytes)) return rc;
    DeviceInputs in; // the offsets through a pinned slot, as the backward entries stage theirs
    if (int rc = stage_meta(h, h->flex_off, c, false, 0, in)) return rc;
    HIP_TRY(launch_torsion_backward(conformer, in.offsets, B, T, axes, moves, angles, grad_out,
                                    reinterpret_cast<double *>(h->torsion_pos.p), grad_coords, grad_angles, c.stream));
    return release_slot(in.slot, c.stream);
}

int mvx_transform_coords(mvx_handle *h, const double *coords, int64_t N, const mvx_xform *xform, double *out,
                         int32_t in_kind, int32_t out_kind, void *stream) {
    if (!h || !xform || (N > 0 && (!coords || !out))) return fail(MVX_ERR_INVALID, "null argument");
    if (const char *bad = check_pose_records(xform, 1)) return fail(MVX_ERR_INVALID, bad);
    if (N <= 0) return MVX_OK;
    const Call c = batch_call(0, nullptr, nullptr, nullptr, 0.0, 0, nullptr, xform, 1, 0, stream, in_kind); // (what stage_meta reads: one record, no offsets)
    hipStream_t s = c.stream;
    CallScope scope(h, s);
    if (scope.rc) return scope.rc;
    const size_t co_bytes = (size_t)N * 3 * sizeof(double);
    const bool host_in = in_kind == MVX_HOST, host_out = out_kind == MVX_HOST;
    DeviceInputs in;
    int rc = stage_meta(h, h->xf_buf, c, true, host_in ? co_bytes : 0, in);
    if (rc) return rc;
    const double *d_in = coords;
    if (host_in && (rc = upload(h->in_coords, coords, co_bytes, in.rest, s, d_in))) return rc;
    double *d_out = out;
    if (host_out) {
        if ((rc = ensure(h->out_stage, co_bytes))) return rc;
        d_out = reinterpret_cast<double *>(h->out_stage.p);
    }
    HIP_TRY(launch_transform(d_in, N, in.xforms, d_out, s));
    if ((rc = release_slot(in.slot, s))) return rc;
    if (host_out) {
        HIP_TRY(hipMemcpyAsync(out, d_out, co_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return MVX_OK;
}

int mvx_set_profiling(mvx_handle *h, int32_t enable) {
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    DeviceGuard guard(h->device);
    if (enable && h->ev.empty()) {
        h->ev.reserve(2 * MVX_PROFILE_RING);
        for (int i = 0; i < 2 * MVX_PROFILE_RING; ++i) {
            hipEvent_t e;
            HIP_TRY(hipEventCreate(&e));
            h->ev.push_back(e);
        }
    }
    h->profiling = enable != 0;
    h->ev_count = 0;
    return MVX_OK;
}

int mvx_profile_read(mvx_handle *h, float *ms, int32_t capacity, int32_t *count) {
    if (!h || !count || (capacity > 0 && !ms)) return fail(MVX_ERR_INVALID, "null argument");
    DeviceGuard guard(h->device);
    const int n = std::min<int>(h->ev_count, capacity);
    if (h->ev_count > 0) HIP_TRY(hipEventSynchronize(h->ev[2 * h->ev_count - 1]));
    for (int i = 0; i < n; ++i) HIP_TRY(hipEventElapsedTime(&ms[i], h->ev[2 * i], h->ev[2 * i + 1]));
    *count = n;
    h->ev_count = 0;
    return MVX_OK;
}

int mvx_last_kernel_ms(mvx_handle *h, float *ms) {
    if (!h || !ms) return fail(MVX_ERR_INVALID, "null argument");
    if (h->ev_count <= 0) return fail(MVX_ERR_INVALID, "no timed launch (call mvx_set_profiling(h, 1) first)");
    DeviceGuard guard(h->device);
    const int i = h->ev_count - 1;
    HIP_TRY(hipEventSynchronize(h->ev[2 * i + 1]));
    HIP_TRY(hipEventElapsedTime(ms, h->ev[2 * i], h->ev[2 * i + 1]));
    return MVX_OK;
}

int mvx_debug_read_records(mvx_handle *h, void *host_dst, int64_t n, void *stream) {
    if (!h || !host_dst || n < 0) return fail(MVX_ERR_INVALID, "bad argument");
    const DevBuf &rec = h->ws[h->cur].rec;
    if ((size_t)n * sizeof(AtomRec) > rec.cap) return fail(MVX_ERR_INVALID, "more records requested than the workspace holds");
    if (n == 0) return MVX_OK;
    DeviceGuard guard(h->device);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(host_dst, rec.p, (size_t)n * sizeof(AtomRec), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return MVX_OK;
}

int mvx_debug_set_option(mvx_handle *h, const char *name, int32_t value) {
    if (!h || !name) return fail(MVX_ERR_INVALID, "null argument");
    const std::string n(name);
    PlanKnobs &k = h->knobs;
    if (n == "chunks") k.pipeline = std::max(1, std::min(16, (int)value));
    else if (n == "max_ct") k.max_ct = std::max(1, std::min(32, (int)value));
    else if (n == "direct") k.direct_mode = value < 0 ? -1 : (value ? 1 : 0);
    else if (n == "max_ct64") k.max_ct64 = value >= 32 ? 32 : 16;
    else if (n == "grad_order") h->grad_order = value ? 1 : 0;
    else if (n == "narrow_sub") h->narrow_sub = (value == 1 || value == 2 || value == 4) ? value : 0;
    else if (n == "dense_grid") (void)value; // (accepted and ignored: there is no second voxelize launch any more)
    else if (n == "nw") k.force_nw = (value >= 1 && value <= 16) ? value : 0; // waves (8-voxel z sub-tiles) per slab; 0 = the default plan
    else if (n == "mall_budget_kb") k.mall_budget = value > 0 ? 1024.0 * (double)value : MALL_BUDGET;
    else if (n == "mgrad_scratch_kb") h->mgrad_scratch = value > 0 ? 1024.0 * (double)value : MOMENTS_GRAD_SCRATCH;
#ifdef MVX_DIAG
    else if (n == "dbg") h->dbg = value;
    else if (n == "vk_stamps") { // value = workgroups to make room for (0: off); read back with mvx_debug_read_diag
        DeviceGuard guard(h->device);
        if (value > 0) {
            if (int rc = ensure(h->diag, (size_t)value * 128)) return rc;
            HIP_TRY(hipMemset(h->diag.p, 0, (size_t)value * 128));
        }
        HIP_TRY(set_diag_buffer(value > 0 ? h->diag.p : nullptr));
    }
    else if (n == "xb_stamps") { // the same for xbin_kernel: value = blocks, 64 B each
        DeviceGuard guard(h->device);
        if (value > 0) {
            if (int rc = ensure(h->diag, (size_t)value * 64)) return rc;
            HIP_TRY(hipMemset(h->diag.p, 0, (size_t)value * 64));
        }
        HIP_TRY(set_diag_buffer_xb(value > 0 ? h->diag.p : nullptr));
    }
#endif
    else return fail(MVX_ERR_INVALID, "unknown option: " + n);
    return MVX_OK;
}

int mvx_debug_last_plan(mvx_handle *h, mvx_plan *plan) {
    if (!h || !plan) return fail(MVX_ERR_INVALID, "null argument");
    if (!h->has_plan) return fail(MVX_ERR_INVALID, "no forward call on this handle yet");
    *plan = h->last_plan;
    return MVX_OK;
}

#ifdef MVX_DIAG
extern "C" int mvx_debug_read_diag(mvx_handle *h, void *host_dst, int64_t bytes) {
    if (!h || !host_dst || bytes < 0 || (size_t)bytes > h->diag.cap) return fail(MVX_ERR_INVALID, "bad argument");
    DeviceGuard guard(h->device);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host_dst, h->diag.p, (size_t)bytes, hipMemcpyDeviceToHost));
    return MVX_OK;
}
#endif

int mvx_alloc(mvx_handle *h, int64_t bytes, void **ptr) {
    if (!h || !ptr || bytes < 0) return fail(MVX_ERR_INVALID, "bad argument");
    DeviceGuard guard(h->device);
    *ptr = nullptr;
    hipError_t e = hipMalloc(ptr, (size_t)std::max<int64_t>(bytes, 16));
    if (e != hipSuccess) {
        g_err = std::string("hipMalloc: ") + hipGetErrorString(e);
        return MVX_ERR_ALLOC;
    }
    return MVX_OK;
}

int mvx_free(mvx_handle *h, void *ptr) {
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    if (!ptr) return MVX_OK;
    DeviceGuard guard(h->device);
    HIP_TRY(hipFree(ptr));
    return MVX_OK;
}

int mvx_memcpy(mvx_handle *h, void *dst, const void *src, int64_t bytes, int32_t dst_kind, int32_t src_kind,
               void *stream) {
    if (!h || bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(MVX_ERR_INVALID, "bad argument");
    if (bytes == 0) return MVX_OK;
    DeviceGuard guard(h->device);
    hipMemcpyKind kind;
    if (dst_kind == MVX_DEVICE && src_kind == MVX_HOST) kind = hipMemcpyHostToDevice;
    else if (dst_kind == MVX_HOST && src_kind == MVX_DEVICE) kind = hipMemcpyDeviceToHost;
    else if (dst_kind == MVX_DEVICE && src_kind == MVX_DEVICE) kind = hipMemcpyDeviceToDevice;
    else kind = hipMemcpyHostToHost;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMemcpyAsync(dst, src, (size_t)bytes, kind, s));
    HIP_TRY(hipStreamSynchronize(s)); // host memory may be pageable: return only when the copy is done
    return MVX_OK;
}

int mvx_memset_zero(mvx_handle *h, void *ptr, int64_t bytes, void *stream) {
    if (!h || bytes < 0 || (bytes > 0 && !ptr)) return fail(MVX_ERR_INVALID, "bad argument");
    if (bytes == 0) return MVX_OK;
    DeviceGuard guard(h->device);
    HIP_TRY(hipMemsetAsync(ptr, 0, (size_t)bytes, reinterpret_cast<hipStream_t>(stream)));
    return MVX_OK;
}

int mvx_stream_sync(mvx_handle *h, void *stream) {
    if (!h) return fail(MVX_ERR_INVALID, "null handle");
    DeviceGuard guard(h->device);
    HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    return MVX_OK;
}

} // extern "C"
