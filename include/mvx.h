/*
 * mvx.h — C ABI of the MI355X-native molecular voxelizer (libmvx_hip.so).
 *
 * This is the drop-in boundary for the hot path of SeonghwanSeo/molvoxel:
 * Voxelizer.forward_features / forward_types / forward_single (and the loop over a batch of
 * molecules the reference's timing harness runs, test/test_time_numpy.py:11-15).
 * The reference has no FFI layer of its own (it is pure Python); what it would bind is
 * exactly this header, from a new backend module molvoxel/voxelizer/hip/voxelizer.py via
 * ctypes (see INTEGRATION.md for the stub). Citations are file:line in the reference tree.
 *
 * Conventions
 *   - every function returns 0 (MVX_OK) or a negative mvx_status; mvx_last_error() returns a
 *     thread-local message for the last failure on the calling thread.
 *   - no ownership transfer: every buffer is caller-owned. Pointers are tagged host/device by
 *     the *_kind arguments (MVX_HOST / MVX_DEVICE). Device pointers must belong to the handle's
 *     device. A 16-byte aligned `out` with dimension % 4 == 0 gets 16-B stores; any other
 *     float-aligned `out` (e.g. slice i of a batch grid of odd dimension) is written run by run: aligned
 *     16-B stores inside each contiguous run of the grid, 4-B stores at its ends (float64 grids: 8-B stores).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream). With MVX_DEVICE
 *     outputs the call is asynchronous on that stream; with MVX_HOST outputs it returns after
 *     the copy back has completed.
 *   - a handle is not re-entrant: one host thread at a time. Calls may arrive on different streams:
 *     the handle's workspace is shared, so a call on another stream than the previous call's first
 *     makes its stream wait for the previous stream (hipStreamWaitEvent; no host synchronisation).
 *     A stream must stay alive until the next call on the handle (or mvx_destroy) has returned.
 *   - argument-shape errors are the Python layer's AssertionErrors (same messages as the
 *     reference, molvoxel/voxelizer/numpy/voxelizer.py:181-192, 327-342, 443-455) and are
 *     raised before the call; this library only validates what it needs to stay memory-safe.
 *
 * Numerical contract (verified against the imported reference by the goldens)
 *   An atom n at p (fp64, after centring / transform) with radius r contributes to voxel
 *   (i,j,k), g[i] = i*res - res*(D-1)/2, iff it passes
 *     1. the box cull            molvoxel/voxelizer/numpy/voxelizer.py:481-494  (strict, fp64)
 *     2. the cull of the reference block (blockdim) holding the voxel   :496-527 (strict, fp64)
 *     3. float32( float32(sqrt_f64((dx^2+dy^2)+dz^2)) / float32(r) ) <= 1          :544-555
 *   with value 1 (binary) or exp(-0.5*(dr/sigma)^2) in float32 (gaussian)            :557-560.
 *   Membership (1-3) is reproduced exactly; gaussian values agree to ~1e-6.
 *   A precision-64 handle keeps step 3 and the values in float64, as the reference does with
 *   precision=64 (:33-34): sqrt_f64(d2) / r <= 1, exp(-0.5*((dr/sigma)^2)) in float64; values agree to ~1e-15.
 */
#ifndef MVX_H
#define MVX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVX_VERSION 140 /* 0.1.4: mvx_forward_sum_batch (additive: one summed grid per batch); mvx_score_views and mvx_views_reduce (additive: scores of many views of one shared cloud and the reduction of their rows onto its atoms); MVX_XF_POSE_PTR, MVX_XF_TRANSLATE_ONCE and mvx_pose_grad_batch (additive: explicit rigid poses and their gradients); mvx_select_views and mvx_forward_views (additive: many views of one shared cloud); mvx_backward_density_batch (additive: sigma and scalar-radius gradients); mvx_config.grid_type (bfloat16 grids) and mvx_plan_call_grid (additive); mvx_plan_call (the decision table as a pure function), channel-wise radii grouped per chunk of 32 channels, narrow chunks in candidate pairs; 0.1.3: one voxelize launch per batched call, channel-wise radii grouped on the device; 0.1.2: mvx_xform.center_ptr, stream hand-over, unaligned out, mvx_debug_set_option */

typedef enum mvx_status {
    MVX_OK = 0,
    MVX_ERR_INVALID = -1, /* bad argument */
    MVX_ERR_HIP = -2,     /* a HIP runtime call failed (message has the hipError string) */
    MVX_ERR_NO_DEVICE = -3,
    MVX_ERR_ALLOC = -4
} mvx_status;

enum mvx_memkind { MVX_HOST = 0, MVX_DEVICE = 1 };
enum mvx_density { MVX_GAUSSIAN = 0, MVX_BINARY = 1 }; /* base/voxelizer.py:13  DENSITY_TYPE_LIST */
enum mvx_radii {                                         /* base/voxelizer.py:12  RADII_TYPE_LIST */
    MVX_RADII_SCALAR = 0,  /* one python float for every atom */
    MVX_RADII_ATOM = 1,    /* mvx_real (N,)  "atom-wise"    */
    MVX_RADII_CHANNEL = 2  /* mvx_real (C,)  "channel-wise" */
};
enum mvx_xform_flags {
    MVX_XF_CENTER = 1,    /* p = p - center first */
    MVX_XF_ROTATE = 2,    /* p = q * p * q^-1 */
    MVX_XF_TRANSLATE = 4, /* p = p + trans (twice when MVX_XF_ROTATE is also set, as the reference does) */
    MVX_XF_RECENTER = 8,  /* p = p + center after the rotation (do_transform with a center, numpy/transform.py:51-54) */
    MVX_XF_CENTER_PTR = 16, /* the centre is read from center_ptr (3 doubles in the memory `in_kind` names) instead of
                              center[]: a device-resident `center` tensor never has to visit the host */
    MVX_XF_POSE_PTR = 32,  /* an explicit rigid pose: center_ptr points at 10 doubles [c0 c1 c2 | q0 q1 q2 q3 | t0 t1 t2] in the
                              memory `in_kind` names, p = q (x - c) conj(q) + t: the centre subtracted, the sandwich product in
                              the operation order of MVX_XF_ROTATE with q as given (the linear part scales by |q|^2; normalise
                              q beforehand for a pure rotation), then t - rounded to float32 when it is read, as `trans` is -
                              added ONCE. Every other flag bit of such a record must be clear. Every entry that takes records
                              accepts it; a device-resident pose never visits the host (a small kernel rewrites the call's
                              device copy of the record as MVX_XF_CENTER | ROTATE | TRANSLATE | TRANSLATE_ONCE) */
    MVX_XF_TRANSLATE_ONCE = 64 /* with MVX_XF_ROTATE | MVX_XF_TRANSLATE: the translation is added once, not twice */
};

/*
 * Element type of the grid (mvx_config.grid_type). MVX_GRID_BF16 (precision 32 only): the arithmetic is the float32
 * handle's, bit for bit; every float32 value is rounded to bfloat16 (to nearest, ties to even; subnormals kept, a NaN stays
 * a NaN) as the kernels store it - the grid a float32 handle writes, converted by torch's .to(torch.bfloat16). `out` then
 * points to bfloat16 elements (2 bytes, 2-byte aligned; host outputs are staged with 2-byte elements); features and radii
 * stay float32. Rows of whole groups of four voxels (D % 4 == 0) on an 8-byte aligned grid get 8-byte stores, anything else
 * is written run by run (16-byte stores inside each run, 2-byte stores at its ends).
 */
enum mvx_grid_type { MVX_GRID_REAL = 0, MVX_GRID_BF16 = 1 };

/*
 * Memory layout of the grid (mvx_set_grid_layout). MVX_LAYOUT_NCDHW: (B, C, D, D, D) with z fastest, the default and the
 * reference's. MVX_LAYOUT_NDHWC (channels-last; precision 32 only, float32 or bfloat16 elements): element (b, c, x, y, z) lies
 * at index (((b D + x) D + y) D + z) C + c of `out` - torch.channels_last_3d of the same logical (B, C, D, D, D) tensor, what
 * the 3D convolutions want. Every value is bit for bit the one the NCDHW handle writes, every element is written once per
 * call, zeros included; only addresses differ. With C == 1 the two layouts coincide.
 */
enum mvx_grid_layout { MVX_LAYOUT_NCDHW = 0, MVX_LAYOUT_NDHWC = 1 };

/*
 * Geometry + density of one voxelizer. Replaces the constructor state of
 * BaseVoxelizer.__init__ (base/voxelizer.py:15-38) and numpy Voxelizer.__init__/_setup_block
 * (numpy/voxelizer.py:22-58).
 */
typedef struct mvx_config {
    double resolution; /* base/voxelizer.py:26 */
    double sigma;      /* base/voxelizer.py:37-38, default 0.5; ignored for binary */
    int32_t dimension; /* D = H = W */
    int32_t blockdim;  /* reference `blockdim` whose per-block cull is emulated (numpy/voxelizer.py:38,55);
                          <= 0 means the reference default 8; >= dimension means one block (no block cull) */
    int32_t density;   /* enum mvx_density */
    int32_t device;    /* HIP device ordinal */
    int32_t precision; /* 32 (or 0) | 64: the `precision` argument of Voxelizer.__init__ (numpy/voxelizer.py:28,33-34):
                          element type of features, radii and the grid, and the type distances, densities and sums
                          are evaluated in */
    int32_t grid_type; /* enum mvx_grid_type: element type of the grid (0 = the precision's real type) */
} mvx_config;

/* float for a precision-32 handle, double for a precision-64 handle (the reference's `self.fp`). */
typedef void mvx_real;

/*
 * Per-molecule rigid transform applied on the device before voxelization, in exactly the
 * reference's fp64 operation order: p = coords - center (numpy/voxelizer.py:120-121), then
 * do_transform(p, None, translation, quaternion) (numpy/transform.py:44-60, _quaternion.py:24-50),
 * including the reference's double application of the translation when a rotation is present.
 */
typedef struct mvx_xform {
    double center[3];
    double quat[4];   /* (q0, q1, q2, q3) as returned by random_quaternion, _quaternion.py:13-21 */
    float trans[3];   /* float32 like numpy/transform.py:76 */
    uint32_t flags;   /* enum mvx_xform_flags */
    const double *center_ptr; /* MVX_XF_CENTER_PTR: where the centre lives (same memory kind as coords);
                                 MVX_XF_POSE_PTR: where the 10 doubles of the pose live */
} mvx_xform;

typedef struct mvx_handle mvx_handle;

int mvx_version(void);
const char *mvx_last_error(void);
int mvx_device_count(int *count);

/* Replaces create_voxelizer(..., library=...) -> Voxelizer(...)  (molvoxel/__init__.py:25-40). */
int mvx_create(const mvx_config *cfg, mvx_handle **out);
int mvx_destroy(mvx_handle *h);
/* Replaces the density_type property setter (base/voxelizer.py:65-70). */
int mvx_set_density(mvx_handle *h, int32_t density, double sigma);
/*
 * Cross-call overlap for loops of large batched calls (no counterpart in the reference, which is synchronous).
 * A batched call is a pre-pass over the atoms (records, candidate lines: ~7 % of a 256-molecule cfg-2 step) followed
 * by the voxelize launches. With enable != 0 the handle keeps two workspace sets and runs the pre-pass of call k+1 on
 * an internal side stream while call k's voxelize launches still occupy the caller's stream; the voxelize launches
 * of call k+1 follow on the caller's stream as usual, so OUTPUTS keep plain stream-order semantics.
 * The INPUTS contract changes: the side stream does not wait for the caller's stream, so coords / features / types /
 * radii must be complete when the call is made (uploaded and synchronised earlier, or produced before a host-side
 * synchronisation), and must stay unchanged until the call's launches have run - not merely be ordered before the call
 * on the stream. Applies to MVX_DEVICE inputs and outputs on the batched three-launch path; other calls are unaffected.
 */
int mvx_set_overlap(mvx_handle *h, int32_t enable);
/*
 * Layout of the grids the forward entry points write from now on (enum mvx_grid_layout; a new handle writes MVX_LAYOUT_NCDHW).
 * MVX_ERR_INVALID, before any device is touched: an unknown layout value, a NULL handle, MVX_LAYOUT_NDHWC on a precision-64
 * handle. Host outputs (MVX_HOST) are supported: the staging buffer is written in the layout and copied as it is. The
 * backward entry points read `grad_out` as (B, C, D, D, D) contiguous whatever the handle's layout.
 */
int mvx_set_grid_layout(mvx_handle *h, int32_t layout);

/*
 * Batched entry points: B molecules stored back to back, molecule b owning atoms
 * [offsets[b], offsets[b+1]). `offsets` (B+1 int64) and `xforms` (B records, may be NULL =
 * identity) are host pointers. coords / features / types / radii share `in_kind`.
 * out is (B, C, D, D, D) mvx_real, fully overwritten (zeros included), `out_kind` tagged.
 *
 *   radii_type SCALAR : radius = radius_scalar for every atom (radii ignored, may be NULL)
 *              ATOM   : radii[sumN]
 *              CHANNEL: radii[C], shared by all molecules. forward_types gathers radii[types]
 *                       (numpy/voxelizer.py:284-285); forward_features tests each channel with its
 *                       own radius and culls with max(radii) (numpy/voxelizer.py:138,213-224).
 *
 * mvx_forward_features_batch replaces Voxelizer.forward_features (numpy/voxelizer.py:97-169)
 *   features: (sumN, C) mvx_real row-major.
 * mvx_forward_types_batch replaces Voxelizer.forward_types (numpy/voxelizer.py:240-315)
 *   types: (sumN,) int32 in [0, C); out has C channels (C may exceed max(types)+1, numpy/voxelizer.py:337).
 * mvx_forward_single_batch replaces Voxelizer.forward_single (numpy/voxelizer.py:370-436)
 *   out is (B, 1, D, D, D).
 */
int mvx_forward_features_batch(mvx_handle *h, const double *coords, const mvx_real *features, const mvx_real *radii,
                               double radius_scalar, int32_t radii_type, const int64_t *offsets,
                               const mvx_xform *xforms, int32_t B, int32_t C, mvx_real *out, int32_t in_kind,
                               int32_t out_kind, void *stream);
int mvx_forward_types_batch(mvx_handle *h, const double *coords, const int32_t *types, const mvx_real *radii,
                            double radius_scalar, int32_t radii_type, const int64_t *offsets,
                            const mvx_xform *xforms, int32_t B, int32_t C, mvx_real *out, int32_t in_kind,
                            int32_t out_kind, void *stream);
int mvx_forward_single_batch(mvx_handle *h, const double *coords, const mvx_real *radii, double radius_scalar,
                             int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms, int32_t B,
                             mvx_real *out, int32_t in_kind, int32_t out_kind, void *stream);

/* Single-molecule forms (B = 1, xform may be NULL): the reference's per-call signature. */
int mvx_forward_features(mvx_handle *h, const double *coords, const mvx_real *features, const mvx_real *radii,
                         double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xform,
                         mvx_real *out, int32_t in_kind, int32_t out_kind, void *stream);
int mvx_forward_types(mvx_handle *h, const double *coords, const int32_t *types, const mvx_real *radii,
                      double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xform,
                      mvx_real *out, int32_t in_kind, int32_t out_kind, void *stream);
int mvx_forward_single(mvx_handle *h, const double *coords, const mvx_real *radii, double radius_scalar,
                       int32_t radii_type, int64_t N, const mvx_xform *xform, mvx_real *out, int32_t in_kind,
                       int32_t out_kind, void *stream);

/*
 * Many views of ONE shared point cloud (no counterpart in the reference, which voxelizes one box per call): a large structure
 * voxelized into B boxes, each with its own transform (centre, optional rotation and translation) - binding-site scanning,
 * per-residue environments, sliding windows. Equivalent to the batched entry on the cloud repeated B times, bit for bit,
 * without the B copies: per view, the atoms that pass the forward's box cull (rule step 1) are selected on the device, their
 * rows are gathered into a compact batch, and that batch runs through the unchanged pipeline.
 *
 * The cloud is N atoms: coords (N, 3) double; channels as `mode` says (0 features: (N, C) mvx_real, 1 types: (N,) int32,
 * 2 single: NULL, C = 1); radii as in the batched entries for one molecule of N atoms. `xforms`: B records on the host, one
 * per view, never NULL with B > 0 (a view of the whole cloud is a record with flags = 0); a MVX_XF_CENTER_PTR centre lives in
 * the memory `in_kind` names. Host-resident inputs (MVX_HOST) are uploaded once - the cloud, not B copies of it.
 *
 * mvx_select_views: offsets_out_host (B + 1 int64, HOST memory) and index_out (int64, DEVICE memory, index_capacity
 *   elements): index_out[offsets[b] .. offsets[b + 1]) are the atoms of view b in ascending order - those whose transformed
 *   position passes the box cull with the radius the pre-pass culls with (the scalar radius; radii[n]; radii[types[n]], and
 *   types outside [0, C) never pass; max(radii) for channel-wise features). Every atom that reaches a voxel of view b is in
 *   the set. Deterministic: no atomics, two calls give the same bytes. `types` is read in types mode only and may be NULL
 *   otherwise. The offsets are copied to the host inside the call: ONE stream synchronisation per call, after which
 *   offsets_out_host is valid. If index_capacity < offsets[B] the call returns MVX_ERR_INVALID with offsets_out_host filled
 *   in and index_out untouched, so the caller can size the buffer and call again; index_out = NULL with index_capacity = 0 is
 *   that sizing call (MVX_OK when no view keeps an atom).
 * mvx_forward_views: out is (B, C, D, D, D) in the handle's grid type and layout, `out_kind` tagged, fully overwritten: the
 *   grids mvx_forward_*_batch writes for the cloud repeated B times with the same xforms. Selection (one stream
 *   synchronisation, as above), one gather launch into handle-owned buffers (per selected atom: 24 bytes of coordinates, its
 *   feature row or type, its radius when radii are atom-wise; 8 bytes of index; 12 bytes per (view, 1024 atoms) of counts),
 *   then the batched pipeline on the compact batch: bfloat16 and channels-last grids, precision 64, host outputs, molecule
 *   chunks and the debug options apply as they do there. mvx_set_overlap does not apply to this entry (its inputs are
 *   produced on the caller's stream by the call itself).
 * Both return MVX_ERR_INVALID before any device is touched for: a NULL handle; a bad mode, radii_type or memory kind; B < 0,
 * N < 0 or C <= 0 (single mode: C != 1); NULL xforms with B > 0; channel-wise radii in single mode; a missing array (coords
 * with N > 0, radii where the radii type needs them, types / channels where the mode needs them, out / offsets_out_host).
 * N == 0 or B == 0: zero offsets; zero grids (B > 0) or nothing.
 */
int mvx_select_views(mvx_handle *h, const double *coords, const int32_t *types_or_null, const mvx_real *radii,
                     double radius_scalar, int32_t radii_type, int32_t mode, int64_t N, int32_t C, const mvx_xform *xforms,
                     int32_t B, int64_t *index_out, int64_t index_capacity, int64_t *offsets_out_host, int32_t in_kind,
                     void *stream);
int mvx_forward_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                      double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                      mvx_real *out, int32_t in_kind, int32_t out_kind, void *stream);

/*
 * Backward pass of a batched call (no counterpart in the reference: its torch backend runs under torch.no_grad()).
 * Given G = dL/dgrid for the grid the forward call with the same arguments wrote, returns the gradients of L with respect
 * to the atom coordinates and (features mode) the feature rows. With p_n the position of atom n after centring / transform
 * and rho_{n,c}(v) = m_{n,c}(v) * exp2(k * float32(d2)) (gaussian; float64 grids: exp(c * d2)) or m_{n,c}(v) (binary),
 * m the forward's membership rule bit for bit (d2 <= T and the voxel inside the atom's admitted ranges; channel-wise radii
 * for features: per channel T_c, k_c), so that grid[c, v] = sum_n w[n,c] rho_{n,c}(v) (w: the feature row, onehot(type),
 * or 1):
 *   dL/dw[n,c]     = sum_v G[c,v] rho_{n,c}(v)                                                     (features mode only)
 *   dL/dp_n        = sum_v (sum_c G[c,v] w[n,c] rho_{n,c}(v) 2 ln2 k_{n,c}) (p_n - g_v)   (float64 grids: 2 c, not 2 ln2 k)
 *   dL/dcoords_n   = M^T dL/dp_n, M the linear part of the transform (identity without MVX_XF_ROTATE; with it M^T is the
 *                    same sandwich product with the conjugate quaternion, exact for |q| != 1 too)
 * The membership m is the forward's bit for bit; the float32 density value is too. Float64 Gaussian values are evaluated
 * with the library exp, while the forward's 32-channel float64 matrix-core walk uses its own exp (within ~1 ulp): there the
 * gradients are those of a density that may differ from the stored grid in the last ulp.
 * Derivative almost everywhere: the jump of rho at the truncation radius is ignored, so binary density gives zero coordinate
 * gradients. The gradient with respect to a centre is -sum of dL/dcoords over the molecule (no MVX_XF_RECENTER: the caller
 * reduces it). No gradients with respect to radii (mvx_backward_radii_batch gives them) or sigma
 * (mvx_backward_density_batch gives it, and the gradient of a scalar radius).
 * Outputs are fully overwritten (atoms that reach no voxel get exact zeros) and deterministic: no atomics, fixed-order
 * reductions; a molecule's gradients are bit for bit the same in any batch. Arguments as in the forward entries (same
 * offsets / xforms / radii: the pre-pass is recomputed from them, nothing is kept from the forward call).
 *   mode: 0 features, 1 types, 2 single (as mvx_plan_query.mode; single: C = 1). grad_out: (B, C, D, D, D) in the handle's
 *   grid type (float, double or bfloat16), every channel of one molecule below 4 GiB. grad_coords: (sumN, 3) double or
 *   NULL; grad_features: (sumN, C) mvx_real or NULL (features mode only); not both NULL.
 * Device pointers except offsets / xforms (host, as in the forward entries; a MVX_XF_CENTER_PTR centre is a device
 * pointer): this entry takes no host-resident arrays. Asynchronous on `stream`; not recorded by mvx_set_profiling. Keeps
 * buffers of its own, so it never writes a workspace set an overlapped forward pre-pass (mvx_set_overlap) may be using.
 * MVX_ERR_INVALID before any device is touched for a null handle, a bad mode, grad_features outside features mode,
 * C <= 0, both outputs NULL or non-monotone offsets.
 */
int mvx_backward_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                       double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                       int32_t B, int32_t C, const void *grad_out, double *grad_coords, mvx_real *grad_features,
                       void *stream);

/*
 * mvx_backward_batch plus the gradient with respect to the radii, in one walk: grad_coords / grad_features are the bits
 * mvx_backward_batch writes (either or both may be NULL here), and
 *   grad_radii: double, shaped like the radii array: (sumN,) for MVX_RADII_ATOM, (C,) for MVX_RADII_CHANNEL.
 * With kfac = 2 ln2 k (float32 arithmetic; float64 grids: 2 c) and k, c proportional to r^-2, d rho / d r = -(kfac / r) d2 rho:
 *   one radius per atom   dL/dr_n = -(1/r_n) sum_v (sum_c G[c,v] w[n,c] rho_{n,c}(v)) kfac_n d2_n(v)       (every mode)
 *   channel-wise, types   dL/dr_c = the same per-atom term summed over the atoms of type c (types >= C: none)
 *   channel-wise, feat.   dL/dr_c = -(kfac_c / r_c) sum_n w[n,c] sum_v G[c,v] rho_{n,c}(v) d2_n(v)
 * r is the value the forward used (the element of radii, widened to double). Channel-wise sums run over every atom of the
 * call, all molecules (one radius vector serves the batch), in a fixed order without atomics: deterministic. Binary density:
 * zeros. Not differentiated: the jump of m at the truncation threshold and the culls that depend on r (almost everywhere,
 * as for the coordinates). Channel-wise radii use handle-owned workspace of 8 bytes per atom (types) or per atom and
 * channel (features). MVX_ERR_INVALID before any device is touched for what mvx_backward_batch rejects (except that
 * grad_coords and grad_features may both be NULL), a NULL grad_radii, scalar radii and channel-wise radii in single mode.
 * No gradient with respect to sigma or to a scalar radius here: mvx_backward_density_batch gives both.
 */
int mvx_backward_radii_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                             double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                             int32_t B, int32_t C, const void *grad_out, double *grad_coords, mvx_real *grad_features,
                             double *grad_radii, void *stream);

/*
 * mvx_backward_radii_batch plus the gradients with respect to sigma and to a scalar radius, from the same walk: grad_coords /
 * grad_features / grad_radii, where requested, are the bits mvx_backward_batch / mvx_backward_radii_batch write (each may be
 * NULL here; grad_radii is invalid with MVX_RADII_SCALAR), and
 *   grad_sigma:          one double on the device, or NULL
 *   grad_radius_scalar:  one double on the device, or NULL; MVX_RADII_SCALAR only
 * At least one of grad_sigma, grad_radius_scalar and grad_radii must be non-NULL. k and c are proportional to (r sigma)^-2
 * and the membership m (d / r <= 1, the culls) does not depend on sigma, so with P_n = sum_v (sum_c G[c,v] w[n,c] rho_{n,c}(v))
 * kfac_n d2_n(v), the per-atom sum of mvx_backward_radii_batch:
 *   scalar radius         dL/dr     = -(1/r) sum_n P_n                                                      (every mode)
 *   one radius per atom, radii by type, scalar radius
 *                         dL/dsigma = -(1/sigma) sum_n P_n                                                   (every mode)
 *   channel-wise, feat.   dL/dsigma = -(1/sigma) sum_c kfac_c sum_n w[n,c] sum_v G[c,v] rho_{n,c}(v) d2_n(v)
 *                                   = sum_c (r_c / sigma) dL/dr_c
 * r and sigma are the values the forward used: float(radius_scalar) and float(sigma) widened to double for float32
 * arithmetic, the doubles for float64 grids. dL/dsigma is the exact derivative where the grid is smooth in sigma (m has no
 * jump in sigma); dL/dr is the derivative almost everywhere, as for the other radii. The sums run over every atom of the
 * call, all molecules (one sigma and one scalar radius serve the batch), in a fixed order without atomics: chunks of atoms,
 * a fixed butterfly per wave, the waves in order, the chunks in order. Two runs give the same bits, under either "grad_order".
 * One walk feeds grad_radii, grad_sigma and grad_radius_scalar (channel-wise features: the second walk of
 * mvx_backward_radii_batch). Outputs are fully overwritten; a call without atoms writes zeros; binary density: zeros.
 * Handle-owned workspace of 8 bytes per atom, or per atom and channel (channel-wise features), whether or not grad_radii is
 * asked for. MVX_ERR_INVALID before any device is touched for what mvx_backward_batch rejects (except that grad_coords and
 * grad_features may both be NULL), all three of grad_sigma / grad_radius_scalar / grad_radii NULL, grad_radius_scalar with
 * radii that are not scalar, grad_radii with scalar radii, and channel-wise radii in single mode.
 */
int mvx_backward_density_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                               double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                               int32_t B, int32_t C, const void *grad_out, double *grad_coords, mvx_real *grad_features,
                               double *grad_radii, double *grad_sigma, double *grad_radius_scalar, void *stream);

/*
 * Scores of a batch against a constant field grid F, without the grids (no counterpart in the reference): the score
 * S_b = sum_{c,v} F[c,v] grid_b[c,v] is linear in the grid, so with rho and w as for mvx_backward_batch it splits by atom,
 *   S_b = sum_{n in b} s_n,   s_n = sum_v sum_c F[c,v] w[n,c] rho_{n,c}(v),
 * and one walk of the atoms' admitted boxes over F - the walk of mvx_backward_batch - gives the scores, the per-atom
 * contributions s_n and the gradients of L = sum_b S_b. No grid is written or read and no copy of the field is made.
 *   field:            the handle's grid type (float, double or bfloat16), NCDHW contiguous whatever the handle's grid layout,
 *                     every channel below 4 GiB
 *   field_mol_stride: in elements: 0 = one (C, D, D, D) field shared by all molecules, C * D^3 = a (B, C, D, D, D) field per
 *                     molecule; anything else is MVX_ERR_INVALID
 *   scores:           (B,) double, never NULL with B > 0; a molecule without atoms scores exactly 0
 *   atom_scores:      (sumN,) double or NULL; an atom with no admitted voxel gets an exact zero
 *   grad_coords:      (sumN, 3) double or NULL; grad_features: (sumN, C) mvx_real or NULL (features mode only)
 * All three optional outputs may be NULL: scores only. grad_coords / grad_features are the bits mvx_backward_batch writes for
 * grad_out = the field laid out per molecule (each molecule's rows are dS_b/d(.)); binary density gives zero coordinate
 * gradients but non-zero scores and feature gradients. s_n is accumulated in float64 from the float32 products F w rho of the
 * coordinate path (float64 grids: double products), one fixed butterfly per atom; a molecule's score is the sum of its s_n in
 * a fixed order (one workgroup per molecule: each wave takes chunks of 64 atoms in order, a butterfly per wave, the waves in
 * order). No atomics: a molecule's score and rows are bit for bit the same in any batch, across runs and under either
 * "grad_order". Outputs are fully overwritten. Without atom_scores the per-atom scores live in handle-owned workspace of 8
 * bytes per atom. Device pointers except offsets / xforms (host; MVX_XF_CENTER_PTR and MVX_XF_POSE_PTR records included), as
 * in mvx_backward_batch, whose staging and buffers this entry shares: it never touches a forward workspace set. Asynchronous
 * on `stream`. MVX_ERR_INVALID before any device is touched for what mvx_backward_batch rejects (except that grad_coords and
 * grad_features may both be NULL), a NULL scores with B > 0, a NULL field with atoms present and a bad field_mol_stride.
 */
int mvx_score_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                    double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                    int32_t B, int32_t C, const void *field, int64_t field_mol_stride,
                    double *scores, double *atom_scores, double *grad_coords, mvx_real *grad_features, void *stream);

/*
 * Second-order information of the scores of mvx_score_batch (no counterpart in the reference): per atom the gradient and the
 * 3x3 Hessian of S_b with respect to the atom's position, and per molecule the gradient and the 6x6 Hessian of S_b under a rigid
 * twist - what a Newton or Levenberg-Marquardt step on a pose needs. Everything is in the GRID frame: p_n is the position the
 * pre-pass record holds for atom n, after centring and transform, relative to the box centre. The score splits by atom, so its
 * Hessian with respect to the positions is block diagonal. With d = p_n - voxel centre, rho the density, u(v) = sum_c F[c,v]
 * w[n,c] (types / single: F[type,v]), kfac with d rho / d p = kfac rho d, and e(v) = (double)(u rho) kfac - the product u rho in
 * the handle's real type, as the gradient walk forms it - over the admitted voxels v of atom n:
 *   s_n = sum_v (double)(u rho)                    mvx_score_batch's atom_scores, bit for bit
 *   g_n = dS/dp_n = sum_v e d                      mvx_score_batch's grad_coords before the rotation is transposed onto it:
 *                                                  the same bits on a call without rotation
 *   H_n = (sum_v e) I + kfac sum_v e d d^T         symmetric, stored as (xx, xy, xz, yy, yz, zz), accumulated in float64
 * The admitted set is held fixed: the truncation at the radius is not differentiated, as in every gradient of this library.
 * Binary density gives g = 0 and H = 0 but scores. An atom with no admitted voxel gets exact zero rows. A twist xi = (tau,
 * omega) about the pivot o_b moves the molecule's posed atoms to p' = R(omega) (p - o_b) + o_b + tau, R = exp([omega]x). With
 * r_n = p_n - o_b, at xi = 0:
 *   twist_grad[b] = (sum_n g_n, sum_n r_n x g_n)                                     (tau first, then omega)
 *   twist_hess[b] = sum_n J_n^T H_n J_n, J_n = [ I | -[r_n]x ], plus sum_n 0.5 (g_n r_n^T + r_n g_n^T) - (g_n . r_n) I
 *                   on the omega-omega block: symmetric to the bit, written in full, row-major
 *   field, field_mol_stride, scores: as for mvx_score_batch
 *   pivots:     (B, 3) double, device, grid frame, or NULL: the box centre (0, 0, 0) for every molecule. Under an explicit
 *               pose (MVX_XF_POSE_PTR) the image of the centre is the translation rounded to float32.
 *   atom_grad:  (sumN, 3) double or NULL; atom_hess: (sumN, 6) double or NULL
 *   twist_grad: (B, 6) double or NULL; twist_hess: (B, 36) double or NULL (needs twist_grad)
 * One walk of the atoms' boxes (one wave per atom record, eleven float64 lane partials, one fixed butterfly each), then one
 * workgroup per molecule sums its atoms in a fixed order (each wave takes chunks of 64 atoms in order, a butterfly per wave,
 * the waves in order): no atomics, a molecule's rows and values are bit for bit the same in any batch and across runs. In the
 * reduction an atom whose g and H rows are all zero is skipped: its position may be NaN or infinite. A molecule without atoms
 * gets zeros. Rows that are not handed out live in handle-owned workspace (80 bytes per atom). Outputs are fully overwritten.
 * Pointers, staging and buffers as for mvx_score_batch; asynchronous on `stream`. MVX_ERR_INVALID before any device is touched
 * for what mvx_score_batch rejects, in its order, then for channel-wise radii in features mode (not supported: the first-order
 * mvx_score_batch serves them) and for twist_hess without twist_grad.
 */
int mvx_score_hessian_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                            double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                            int32_t B, int32_t C, const void *field, int64_t field_mol_stride, const double *pivots,
                            double *scores, double *atom_grad, double *atom_hess, double *twist_grad, double *twist_hess,
                            void *stream);

/*
 * ONE grid for a whole batch (no counterpart in the reference): the sum, weighted or not, of the B grids the forward entries
 * would write for the same arguments, without those grids. With rho and w as for mvx_backward_batch and the atoms
 * n = 0 .. sumN-1 in the caller's order (molecule boundaries from offsets, a transform per molecule):
 *   out[c, v] = sum over n, in that order, of u[n,c] rho_{n,c}(v)
 *   u[n,c] = w[n,c], or float32(atom_weights[n] * w[n,c]) with atom_weights (one float per atom, any sign)
 * The sum is the float32 fma(u, rho, acc) chain the forward kernels run inside one molecule, continued across the molecule
 * boundaries, starting from 0 (accumulate == 0: out is fully overwritten; B == 0 or no atoms writes zeros) or from the value
 * already in out (accumulate == 1: out is read and updated; B == 0 or no atoms leaves it untouched). rho is the forward's
 * membership and density value bit for bit, so: an unweighted call whose molecules are only centred gives the bits of the
 * per-molecule forward on the one merged molecule concat_b(coords_b - c_b); a weighted features call the bits of the
 * unweighted call on the rows scaled in float32; a call split at a molecule boundary into two calls, the second accumulating,
 * the bits of the one call.
 *   out: (C, D, D, D) float32, NCDHW contiguous and 16-byte aligned, whatever the handle's grid_type / layout (a bfloat16
 *        partial sum could not be reloaded exactly). mode: 0 features, 1 types, 2 single (C = 1).
 * Deterministic: one workgroup per (output slab, chunk of 32 channels) walks the molecules' candidate lines of its slab one
 * after another with the accumulators in registers and writes once; no atomics, and no split of the molecules over
 * workgroups - the bits depend on the atom order alone, never on the launch shape or on how the batch is cut. Molecule
 * chunks: the pre-pass workspace is cut as the forward cuts it (Infinity Cache budget, "chunks" / "mall_budget_kb" options);
 * chunk k > 0 continues the sums chunk k - 1 wrote. Workspace: the forward's pre-pass buffers, with weight rows padded to whole
 * chunks of 32 channels (feature rows of such a width and without atom_weights are read in place).
 * Device pointers except offsets / xforms (host; MVX_XF_CENTER_PTR and MVX_XF_POSE_PTR records included), exactly as in
 * mvx_backward_batch. Asynchronous on `stream`.
 * MVX_ERR_INVALID before any device is touched for what mvx_backward_batch rejects for these arguments (a bad mode, C <= 0,
 * single mode with C != 1, B < 0, a bad radii_type, channel-wise radii in single mode, NULL or non-monotone offsets, a NULL
 * handle, a bad pose record, NULL arrays with atoms present), a NULL out, accumulate outside {0, 1}, an out that is not
 * 16-byte aligned, and for the four configurations the kernel does not serve, each named in the message: a precision-64
 * handle; channel-wise radii with features; a dimension that is no multiple of 4; a blockdim that needs per-lane ranges
 * (mvx_plan.lane_range = 1).
 */
int mvx_forward_sum_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                          double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                          int32_t B, int32_t C, const float *atom_weights /* (sumN,) or NULL */,
                          float *out /* (C, D, D, D) */, int32_t accumulate, void *stream);

/*
 * ONE summed grid for B views of ONE shared cloud (no counterpart in the reference): mvx_forward_sum_batch on the compact batch
 * mvx_forward_views voxelizes - the occupancy map of 1 024 docking poses of a ligand, or of 256 boxes of a pocket, without B
 * copies of the cloud and without the B grids. The cloud, `mode`, radii and the B host records are those of mvx_forward_views;
 * every array is a device array, as for mvx_forward_sum_batch and mvx_score_views (centre and pose pointers point into device
 * memory). view_weights: NULL or (B,) float32 on the device, one weight per view, expanded on the device to one per selected
 * atom from the selection's offsets (no host round trip): it behaves as a (B,) molecule weight does in a summed batch.
 * out: (C, D, D, D) float32 NCDHW, 16-byte aligned, whatever the handle's grid type and layout; accumulate as in
 * mvx_forward_sum_batch. ONE stream synchronisation (the selection, as mvx_forward_views), then asynchronous on `stream`.
 * The result is, bit for bit, mvx_forward_sum_batch on the cloud repeated B times with the same records - equivalently on
 * coords[index], the gathered channels and radii and the offsets of mvx_select_views: culled atoms add nothing and the atom
 * order is the same. B == 0: MVX_OK, nothing written. N == 0, or no view selects an atom: zeros, or with accumulate nothing
 * touched. mvx_set_sum_parts applies, with the views as the molecules.
 * MVX_ERR_INVALID, everything before any device is touched, in this order: a bad mode; a bad radii_type; B < 0, N < 0 or
 * C <= 0; NULL xforms with B > 0; channel-wise radii in single mode; single mode with C != 1; NULL coords with N > 0; a missing
 * radii array; NULL types in types mode with N > 0; N >= 2^31; accumulate outside {0, 1}; NULL out with B > 0; NULL channels in
 * features mode with B > 0 and N > 0; a NULL handle; a bad pose record; then (B > 0) the four configurations the summed kernel
 * does not serve, with the texts of mvx_forward_sum_batch - a precision-64 handle, channel-wise radii with features, a
 * dimension that is no multiple of 4, a blockdim that needs per-lane ranges - and an out that is not 16-byte aligned.
 */
int mvx_forward_views_sum(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                          double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                          const float *view_weights, float *out, int32_t accumulate, void *stream);

/*
 * Summed grids in parts (opt-in; a new handle has parts = 1, which is the path and the bits described above). A summed call
 * runs at most slabs x channel chunks workgroups, each walking all B molecules one after another: a batch of many small
 * molecules (1 024 poses of a ligand) leaves most of the card idle. With parts = K > 1 every summed call of the handle -
 * mvx_forward_sum_batch, mvx_forward_views_sum (the views are the molecules) - cuts the CALL's B molecules into parts:
 *   q = ceil(B / K); part g holds the molecules [g q, min(B, (g + 1) q)); G = ceil(B / q) parts exist
 *   S_g = the grid the parts = 1 call gives, from zero, for the molecules of part g alone
 *   out = the float32 chain r = (accumulate ? out : +0); r = r + S_0; r = r + S_1; ...; r = r + S_{G-1}
 * one rounding per add, in that order. No atomics: the bits are a function of the atom order, B and K alone, and never of how
 * the call is cut into molecule chunks - but they DIFFER from the bits of parts = 1 (other partial sums are rounded).
 * Workspace: G partial grids of C * D^3 floats, handle-owned, zeroed at the start of every such call.
 * MVX_ERR_INVALID for a NULL handle and for parts outside 1 ... 64.
 */
int mvx_set_sum_parts(mvx_handle *h, int32_t parts);

/*
 * Per-channel sums and norms of every molecule's grid, without the grids (no counterpart in the reference): what normalised
 * cross-correlation, shape Tanimoto, MSE against a target and the occupied volume need. For molecule b and channel c, with
 * g = g_b[c, v] the float32 value the forward entries store at voxel v for the same arguments (whatever the handle's grid_type
 * and layout: the moments are those of the float32 values):
 *   moments[b, c, 0] = sum_v (double)g
 *   moments[b, c, 1] = sum_v (double)g * (double)g
 *   moments[b, c, 2] = sum_v (double)g * (double)target[c, v]        (only with a target)
 *   target:  (C, D, D, D) float32 NCDHW on the device, 16-byte aligned, shared by all molecules, or NULL
 *   moments: (B, C, K) doubles on the device, K = target ? 3 : 2, fully overwritten. mode: 0 features, 1 types, 2 single (C = 1).
 * The plan is mvx_forward_sum_batch's (the binned route, chunks of 32 channels on zero-padded weight rows, radii[types] as
 * per-atom radii), run for one molecule per workgroup: the accumulators are bit for bit the values the forward writes. The
 * products are exact in float64 (a float32 times a float32 fits 53 bits), so the summation is the only rounding: each
 * moment lies within (n - 1) 2^-53 sum|term| of the exact sum of its n = D^3 terms, and sums of small integers (binary
 * density with types or one channel) are exact.
 * Deterministic, no atomics: per slab the two x planes of a register, a fixed butterfly over the 32 lanes of each half of a
 * wave, the waves in order; then a molecule's slabs in slab order (a second kernel). The slab decomposition depends on the
 * dimension alone, so a molecule's bits do not depend on its batch, on how the batch is cut into molecule chunks, or on the
 * presence of a target (moments 0 and 1). A molecule without atoms, or with none inside the box, gets exact zeros; B == 0:
 * MVX_OK, nothing written; a call without atoms writes zeros to all of `moments`.
 * Workspace: the forward's pre-pass buffers and, handle-owned, one partial per (molecule, slab, moment, channel) of the
 * largest molecule chunk (cut as the forward cuts it), not of the call.
 * Device pointers except offsets / xforms (host; MVX_XF_CENTER_PTR and MVX_XF_POSE_PTR records included), exactly as in
 * mvx_forward_sum_batch. Asynchronous on `stream`.
 * MVX_ERR_INVALID before any device is touched, in this order: a bad mode; C <= 0; single mode with C != 1; B < 0; NULL
 * moments with B > 0; a bad radii_type; channel-wise radii in single mode; NULL or non-monotone offsets; a NULL handle; a bad
 * pose record; too many atoms; NULL arrays with atoms present; then the four configurations the walk does not serve, each
 * named in a message that begins with "moments:": a precision-64 handle; channel-wise radii with features; a dimension that
 * is no multiple of 4; a blockdim that needs per-lane ranges (mvx_plan.lane_range = 1); and a target that is not 16-byte aligned.
 */
int mvx_moments_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                      double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                      int32_t B, int32_t C, const float *target /* (C, D, D, D) device, or NULL */,
                      double *moments /* (B, C, K) device, K = target ? 3 : 2 */, void *stream);

/*
 * Gradients through mvx_moments_batch (no counterpart in the reference): dL/dcoords and dL/dfeatures of a loss that reads the
 * grids through their moments only, without B grids of g and without any grid of dL/dgrid. With G0, G1, G2 =
 * grad_moments[b, c, 0..2] = dL/dm[b, c, 0..2] the upstream of the backward walk is
 *   dL/dgrid[b, c, v] = G0 + 2 G1 g[b, c, v] + G2 target[c, v]
 * and the walk forms it per voxel, in float32, from the three coefficients of its (molecule, channel):
 *   a0 = (float)G0, a1 = (float)(2.0 * G1), a2 = (float)G2
 *   u  = fmaf(a1, g, fmaf(a2, target[c, v], a0))          without a target: u = fmaf(a1, g, a0)
 * g is the float32 value mvx_forward_*_batch stores for the same arguments (whatever the handle's grid_type and layout: the
 * grids are written as float32 NCDHW into handle-owned scratch). Everything behind the upstream is mvx_backward_batch's walk:
 * grad_coords and grad_features are, bit for bit, what mvx_backward_batch gives for grad_out = u on a float32 NCDHW handle.
 * So grad_moments = (0, 0, 1) everywhere gives mvx_score_batch's gradients for field = target, (0, 0.5, 0) those of
 * mvx_backward_batch for grad_out = the grids themselves, (1, 0) without a target those for grad_out = 1.
 *   target:        (C, D, D, D) float32 NCDHW on the device, 16-byte aligned, shared by all molecules, or NULL
 *   grad_moments:  (B, C, K) doubles on the device, K = target ? 3 : 2
 *   grad_coords:   (sumN, 3) doubles or NULL; grad_features: (sumN, C) floats or NULL (features mode only); not both NULL. Fully
 *                  overwritten; binary density gives zero coordinate gradients; an atom of a type outside [0, C) gets zeros.
 * The call runs molecule chunk by molecule chunk, cut as the forward cuts a batch (Infinity Cache budget, gridDim.y limit, the
 * "chunks" and "mall_budget_kb" debug options) and then further, until the float32 grids of a chunk fit 1 GiB (one molecule
 * per chunk at least; the "mgrad_scratch_kb" option); mvx_debug_last_plan reports the cut. Per chunk the forward into the
 * scratch, then the backward's pre-pass and the walk over the chunk's atoms ("grad_order" applies per chunk). Deterministic,
 * no atomics; a molecule's rows do not depend on its batch or on the cut.
 * Workspace, handle-owned: the float32 grids of the largest chunk (nb * C * D^3 floats: at most 1 GiB, or one molecule's),
 * (B, C, 3) floats of coefficients, and the buffers of the forward and backward entries.
 * Device pointers except offsets / xforms (host), as in mvx_moments_batch. Asynchronous on `stream`.
 * MVX_ERR_INVALID before any device is touched: the rules of mvx_moments_batch in its order, up to and including the four
 * configurations named "moments:" and the target's alignment; then NULL grad_moments with B > 0; grad_features outside
 * features mode; grad_coords and grad_features both NULL. B == 0: MVX_OK; a call without atoms launches nothing.
 */
int mvx_moments_backward_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                               double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                               int32_t B, int32_t C, const float *target /* (C, D, D, D) device, or NULL */,
                               const double *grad_moments /* (B, C, K) device, K = target ? 3 : 2 */,
                               double *grad_coords, mvx_real *grad_features, void *stream);

/*
 * Gradients with respect to explicit rigid poses (MVX_XF_POSE_PTR records; no counterpart in the reference): the reduction of
 * the per-atom gradients a backward entry wrote for the same call (grad_coords = M^T dL/dp) to dL/dc, dL/dq and dL/dt of every
 * molecule, on the device. Per molecule with pose (c, q, t), M = M(q) the linear part of the sandwich product (it scales by
 * |q|^2), g_n = grad_coords[n], s = sum_n g_n, U = sum_n g_n (x_n - c)^T and n4 = |q|^4 (M M^T = |q|^4 I, so dL/dp_n = M g_n / n4):
 *   dL/dc   = -s
 *   dL/dt   = M s / n4                          (straight through the float32 rounding of t)
 *   dL/dq_k = < dM/dq_k , M U / n4 >            (k = 0 .. 3; q is used as given, nothing is normalised)
 * U is accumulated from x_n - c, never as sum g x^T - s c^T (centres lie tens of Angstrom from the origin).
 * grad_pose: (B, 10) doubles on the device, [dc0 dc1 dc2 | dq0 dq1 dq2 dq3 | dt0 dt1 dt2] per molecule, fully overwritten; a
 * molecule without atoms gets zeros; q = 0 gives a non-finite row. Deterministic: one workgroup per molecule, each wave takes
 * the molecule's atoms in chunks of 64 in order, a fixed butterfly per wave, the waves in order; no atomics; a molecule's row
 * is bit for bit the same in any batch and across runs. coords, grad_coords, grad_pose and the poses the records point at are
 * device pointers; offsets and xforms are host pointers as in the backward entries. Asynchronous on `stream`.
 * MVX_ERR_INVALID before any device is touched for: B < 0; NULL grad_pose, xforms or offsets with B > 0; non-monotone offsets;
 * NULL coords or grad_coords with atoms present; a record without MVX_XF_POSE_PTR (or with other flag bits, or a NULL
 * center_ptr); a NULL handle.
 */
int mvx_pose_grad_batch(mvx_handle *h, const double *coords, const double *grad_coords, const int64_t *offsets,
                        const mvx_xform *xforms, int32_t B, double *grad_pose, void *stream);

/*
 * Scores of B views of ONE shared cloud against a constant field, without the grids and without B copies of the cloud (no
 * counterpart in the reference): mvx_score_batch on the compact batch mvx_forward_views voxelizes. The cloud, `mode`, radii
 * and the B host records are those of mvx_forward_views; every array is a device array (centre and pose pointers point into
 * device memory). field, field_view_stride (0 = one (C, D, D, D) field for all views, C * D^3 = one per view) and the outputs
 * follow mvx_score_batch. The selected rows are gathered into handle-owned buffers (mvx_forward_views' gather) and walked once.
 *   index == NULL:  the entry selects the views' atoms itself (ONE stream synchronisation, as mvx_forward_views) and ignores
 *                   offsets_host. Only `scores` may be asked for: the caller cannot know the length of the per-row outputs,
 *                   so atom_scores, grad_coords and grad_features must be NULL.
 *   index != NULL:  index (device) and offsets_host (B + 1 entries, host) are a selection mvx_select_views returned for the same
 *                   cloud, radii and records; the entry does not synchronise. With total = offsets_host[B]: atom_scores (total,)
 *                   double, grad_coords (total, 3) double, grad_features (total, C) mvx_real (features mode), each or NULL, in
 *                   selection order: row k belongs to atom index[k] of its view. mvx_views_reduce sums such rows onto the atoms.
 * scores (B,) double: a view that keeps no atom scores exactly 0. B == 0 writes nothing; N == 0 writes zero scores.
 * Every value is the bit mvx_score_batch gives for coords[index], the gathered channels and radii, the offsets and the same
 * records; against the cloud repeated B times the per-atom values of kept atoms are the same bits, and a view's score is the
 * same bit when the view keeps the whole cloud (elsewhere the fixed-order sum of a view's atoms groups other atoms together: the
 * scores agree to float64 rounding). Deterministic, asynchronous on `stream` (apart from the selection).
 * MVX_ERR_INVALID before any device is touched for: what mvx_select_views rejects for the cloud and the records; features mode
 * without channels; grad_features outside features mode; a negative field_view_stride, or one that is neither 0 nor C * D^3; NULL
 * scores with B > 0; a NULL field with atoms to score; per-row outputs without an index; an index without offsets_host;
 * offsets_host[0] != 0, decreasing offsets or offsets_host[B] >= 2^31; a NULL handle.
 */
int mvx_score_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                    double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                    const int64_t *index, const int64_t *offsets_host, const void *field, int64_t field_view_stride,
                    double *scores, double *atom_scores, double *grad_coords, mvx_real *grad_features, void *stream);

/*
 * Second-order information of the scores of B views of ONE shared cloud (no counterpart in the reference): mvx_score_hessian_batch
 * on the compact batch mvx_score_views walks - what a Newton or Levenberg-Marquardt step on each of B poses of one ligand needs,
 * without B copies of the ligand. The cloud, `mode`, radii, the B host records, index, offsets_host, field and field_view_stride
 * are those of mvx_score_views; pivots and the outputs follow mvx_score_hessian_batch, per view instead of per molecule.
 *   index == NULL:  the entry selects the views' atoms itself (ONE stream synchronisation) and ignores offsets_host. Only the
 *                   per-view outputs may be asked for: atom_grad and atom_hess must be NULL.
 *   index != NULL:  a selection mvx_select_views returned for the same cloud, radii and records; the entry does not synchronise.
 *                   With total = offsets_host[B]: atom_grad (total, 3) double, atom_hess (total, 6) double, each or NULL, in
 *                   selection order: row k belongs to atom index[k] of its view. mvx_views_reduce sums such rows onto the atoms.
 *   pivots:         (B, 3) double, device, grid frame, one per view, or NULL: the box centre.
 *   scores (B,), twist_grad (B, 6) or NULL, twist_hess (B, 36) or NULL (needs twist_grad): double, device, fully overwritten.
 * Every value is the bit mvx_score_hessian_batch gives for coords[index], the gathered channels and radii, the selection's
 * offsets and the same records; against the cloud repeated B times the rows of kept atoms are the same bits, and a view's scores,
 * twist_grad and twist_hess are the same bits when the view keeps the whole cloud. A view that keeps no atom gets exact zeros;
 * N == 0 writes zeros; B == 0 writes nothing. Deterministic, asynchronous on `stream` (apart from the selection).
 * MVX_ERR_INVALID before any device is touched for what mvx_score_views rejects, in its order - atom_grad and atom_hess in the
 * place of its per-row outputs -, then for channel-wise radii in features mode and for twist_hess without twist_grad.
 */
int mvx_score_hessian_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                            double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                            const int64_t *index, const int64_t *offsets_host, const void *field, int64_t field_view_stride,
                            const double *pivots, double *scores, double *atom_grad, double *atom_hess, double *twist_grad,
                            double *twist_hess, void *stream);

/*
 * The moments of B views of ONE shared cloud, without the grids and without B copies of the cloud (no counterpart in the
 * reference): mvx_moments_batch on the compact batch mvx_forward_views voxelizes. The cloud, `mode`, radii and the B host records
 * are those of mvx_forward_views; every array is a device array (centre and pose pointers point into device memory).
 *   index == NULL:  the entry selects the views' atoms itself (ONE stream synchronisation) and ignores offsets_host.
 *   index != NULL:  index (device) and offsets_host (B + 1 entries, host) are a selection mvx_select_views returned for the same
 *                   cloud, radii and records; the entry does not synchronise.
 *   target:             float32 NCDHW on the device, 16-byte aligned, or NULL (K = 2).
 *   target_view_stride: elements between the targets of two views: 0 = one (C, D, D, D) target for all views, C * D^3 = one
 *                       per view, (B, C, D, D, D): view b is multiplied with target + b * target_view_stride. The target lives in
 *                       box coordinates, so views of different boxes want one each. Ignored without a target.
 *   moments:            (B, C, K) doubles on the device, K = target ? 3 : 2, fully overwritten.
 * Every value is the bit mvx_moments_batch gives for coords[index], the gathered channels and radii, the offsets and the same
 * records - with a target per view, the bit of the call that shares that view's target among all; the bits do not depend on how
 * the call is cut into chunks of views. B == 0: MVX_OK, nothing written; N == 0, or no atom selected: exact zeros.
 * MVX_ERR_INVALID before any device is touched, in this order: what mvx_select_views rejects for the cloud and the records up to
 * "too many atoms"; NULL moments with B > 0; a negative target_view_stride; an index without offsets_host, offsets_host[0] != 0,
 * decreasing offsets or offsets_host[B] >= 2^31; features mode without channels; a NULL handle; a bad pose record; a
 * target_view_stride that is neither 0 nor C * D^3; then, with B > 0, the configurations mvx_moments_batch names "moments:" and
 * the target's alignment.
 */
int mvx_moments_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                      double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                      const int64_t *index, const int64_t *offsets_host, const float *target, int64_t target_view_stride,
                      double *moments /* (B, C, K) device, K = target ? 3 : 2 */, void *stream);

/*
 * Gradients through mvx_moments_views: mvx_moments_backward_batch on the compact batch of a selection, each view against its own
 * target where target_view_stride says so (dL/dgrid[b, c, v] = G0 + 2 G1 g[b, c, v] + G2 target_b[c, v]). The rows come out per
 * (view, atom) in selection order, so the selection is required: index (device) and offsets_host (B + 1 entries, host) as
 * mvx_select_views returned them for the same cloud, radii and records. With total = offsets_host[B]:
 *   grad_moments:       (B, C, K) doubles on the device, K = target ? 3 : 2
 *   grad_coords_rows:   (total, 3) doubles or NULL; grad_features_rows: (total, C) floats or NULL (features mode only); not both
 *                       NULL. Row k belongs to atom index[k] of its view; mvx_views_reduce sums such rows onto the shared atoms,
 *                       mvx_pose_grad_batch reduces them to the views' poses. Fully overwritten.
 * Bit for bit mvx_moments_backward_batch's rows for coords[index], the gathered channels and radii, the offsets and the same
 * records; the call runs chunk by chunk of views exactly as that entry does (the same options, mvx_debug_last_plan reports the
 * cut), the target moving with the chunk, and the rows do not depend on the cut. Does not synchronise.
 * MVX_ERR_INVALID before any device is touched, in this order: what mvx_select_views rejects for the cloud and the records up to
 * "too many atoms"; NULL grad_moments with B > 0; grad_features_rows outside features mode; both row outputs NULL; a negative
 * target_view_stride; a NULL index (the text mvx_score_views has for per-row outputs without an index); what is wrong with
 * offsets_host; features mode without channels; a NULL handle; a bad pose record; a target_view_stride that is neither 0 nor
 * C * D^3; then, with B > 0, the configurations named "moments:" and the target's alignment. B == 0: MVX_OK; a selection
 * without atoms launches nothing.
 */
int mvx_moments_backward_views(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                               double radius_scalar, int32_t radii_type, int64_t N, int32_t C, const mvx_xform *xforms, int32_t B,
                               const int64_t *index, const int64_t *offsets_host, const float *target, int64_t target_view_stride,
                               const double *grad_moments /* (B, C, K) device */, double *grad_coords_rows,
                               mvx_real *grad_features_rows, void *stream);

/*
 * Rows of a selection summed back onto the shared atoms (the backward step of anything computed per (view, atom) row):
 *   out[n, j] = sum over the views b whose segment index[offsets[b] .. offsets[b + 1]) holds atom n of rows[slot(b, n), j]
 * index (device) and offsets_host (B + 1 entries, host) as mvx_select_views returns them: every segment ascending, entries in
 * [0, N). rows: (offsets_host[B], width) device array of `row_type` elements (enum mvx_row_type); out: (N, width) of the same
 * type, fully overwritten - an atom no view holds gets an exact-zero row. The sums are accumulated in double and rounded once
 * when the rows are float. No atomics: per atom and column, each lane of a wave adds its views in ascending order (wave w of
 * four takes the views 64 (w + 4 k) + lane), a fixed butterfly per wave, the four waves in a fixed order - the order of the
 * additions depends on (B, N, index, offsets) alone, never on the machine, the launch or the run. Workspace: the B + 1 offsets.
 * Asynchronous on `stream`. MVX_ERR_INVALID before any device is touched for: B < 0 or N < 0; width <= 0; a bad row_type; NULL
 * offsets_host with B > 0, offsets_host[0] != 0, decreasing offsets or offsets_host[B] >= 2^31; NULL index or rows with rows
 * present; NULL out with N > 0; a NULL handle.
 */
enum mvx_row_type { MVX_ROW_FLOAT = 0, MVX_ROW_DOUBLE = 1 };
int mvx_views_reduce(mvx_handle *h, const int64_t *index, const int64_t *offsets_host, int32_t B, int64_t N, const void *rows,
                     int32_t width, int32_t row_type, void *out, void *stream);

/*
 * One Levenberg-Marquardt bookkeeping step for B rigid poses in one launch (no counterpart in the reference): what lies between
 * two evaluations of mvx_score_hessian_batch / mvx_score_hessian_views in a damped Newton refinement that maximises the scores.
 * One thread per pose, float64, no atomics, no host read. Every array is a device array. The current state, read and written:
 *   q (B, 4), t (B, 3): the pose; S (B,), G (B, 6), H (B, 36): its score, twist gradient and twist Hessian; lam (B,): the damping;
 *   taken, dropped (B,) int32: the accepted steps, and the steps dropped in a row.
 * The trial: q2 (B, 4), t2 (B, 3): written, and read first when have_trial is set; S2 (B,), G2 (B, 6), H2 (B, 36): the evaluation
 * at (q2, t2), read when have_trial is set, NULL otherwise. xi: (B, 6) or NULL, the twist of the new trial. Per pose, in order:
 *   1. with have_trial and dropped < max_dropped: S2 > S (false for a NaN: a non-finite trial is dropped) makes the trial the
 *      state - q, t, S, G, H copied bit for bit, lam *= lam_down, taken += 1, dropped = 0; otherwise lam *= lam_up, dropped += 1.
 *   2. dropped >= max_dropped: the pose is finished: q2 = q, t2 = t, xi = 0; nothing else changes, on this or any later call.
 *   3. otherwise (-H + lam I) xi = G by Gaussian elimination with partial pivoting on the full 6x6, and (q2, t2) the pose moved by
 *      the twist xi = (tau, omega): q2 = u (x) q with u = (cos(|omega|/2), sin(|omega|/2) omega/|omega|), t2 = t + tau; omega = 0
 *      gives q2 = q exactly. A zero pivot, or a non-finite component of xi, q, t, lam, q2 or t2: xi = 0 and (q2, t2) = (q, t) - the
 *      next call sees S2 == S, drops the step and raises lam, so that a singular or NaN system damps itself out.
 * With the pivots at their default (the translation rounded to float32) the trial realises the twist exactly. A pose's values do
 * not depend on its batch; two runs give the same bits. Asynchronous on `stream`. MVX_ERR_INVALID before any device is touched
 * for: B < 0; a NULL q, t, S, G, H, lam, taken, dropped, q2 or t2 with B > 0; a NULL S2, G2 or H2 with have_trial and B > 0;
 * max_dropped < 1; lam_down or lam_up not finite or <= 0; a NULL handle. B == 0: MVX_OK.
 */
int mvx_lm_step(mvx_handle *h, int32_t B, int32_t have_trial, double lam_down, double lam_up, int32_t max_dropped, double *q,
                double *t, double *S, double *G, double *H, double *lam, int32_t *taken, int32_t *dropped, double *q2, double *t2,
                const double *S2, const double *G2, const double *H2, double *xi, void *stream);

/*
 * TORSION COORDINATES (no counterpart in the reference): rotatable bonds next to the rigid twist, for B molecules of T torsions
 * each, 0 <= T <= 32 (a molecule with fewer pads with axes of -1). Torsion k of a molecule has an axis from atom a_k to atom b_k
 * (indices local to the molecule) and a moving set M_k, bit k of the per-atom mask moves[n]. The sets form a tree: b_k in M_k,
 * a_k not in M_k; for k < l either M_l is a proper subset of M_k (then a_l, b_l in M_k) or the two are disjoint; parents come
 * before children - so "k is l or an ancestor of l" is bit k of moves[b_l]. The library does not check the tree (the Python
 * layer's check_torsions does). A torsion is INERT when a_k or b_k is outside [0, N_b), or the axis has zero or no finite
 * length: it turns nothing, its gradient entry and its Hessian row and column are exact zeros. No axis index is used unchecked.
 *
 * mvx_apply_torsions: the conformer C(theta): for k = 0 .. T-1 in order, the atoms of M_k are turned by angles[b, k] about the
 * CURRENT axis (a_k, b_k) through b_k (Rodrigues' formula, sin and cos in float64). One workgroup per molecule.
 *   coords, out: (sumN, 3) double, device; out may be coords. offsets: (B + 1,) int64, host. axes: (B, T, 2) int32, device.
 *   moves: (sumN,) int32, device, read as 32 bits. angles: (B, T) double, device.
 * An angle of exactly 0 and an inert torsion turn nothing; atoms in no turned set are copied bit for bit. Asynchronous on
 * `stream`. MVX_ERR_INVALID before any device is touched for, in order: B < 0; T outside 0 .. 32; NULL offsets with B > 0,
 * offsets[0] != 0 or decreasing offsets; offsets[B] >= 2^31; NULL coords or out with atoms; NULL axes, moves or angles with
 * atoms and T > 0; a NULL handle. No molecules or no atoms: MVX_OK.
 */
int mvx_apply_torsions(mvx_handle *h, const double *coords, const int64_t *offsets, int32_t B, int32_t T, const int32_t *axes,
                       const int32_t *moves, const double *angles, double *out, void *stream);

/*
 * mvx_apply_torsions_backward: the adjoint of mvx_apply_torsions: from the conformer C(theta) that call returned and grad_out =
 * dL/dC to grad_coords = dL/dcoords and grad_angles = dL/dangles. The turns are swept in reverse, k = T-1 .. 0, on working
 * positions in handle-owned workspace (sumN * 3 doubles; `conformer` is not written) and on the rows in grad_coords, which start
 * as grad_out. With c = cos angles[b, k], s = sin angles[b, k], R = c I + s [u]x + (1 - c) u u^T about the current axis, for
 * every atom n of M_k, w = y_n - p_b: the turn is undone, v = R^T w; grad_angles[b, k] += ybar_n . (u x w); the row becomes
 * R^T ybar_n; b_bar += ybar_n - R^T ybar_n; u_bar += s (v x ybar_n) + (1 - c) ((u . v) ybar_n + (u . ybar_n) v); then d_bar =
 * (u_bar - u (u . u_bar)) / |p_b - p_a| and the rows of b_k and a_k receive b_bar + d_bar and -d_bar. One workgroup per molecule;
 * the seven sums are float64 lane partials in a fixed order (thread i takes the atoms i, i + 256, ...), a butterfly per wave, the
 * four waves in a fixed order: no atomics, two runs give the same bits, a molecule's values do not depend on its batch.
 *   conformer, grad_out, grad_coords: (sumN, 3) double, device; grad_coords may be grad_out. grad_angles: (B, T) double, device.
 *   offsets, axes, moves, angles: as for mvx_apply_torsions, the arguments of the call that made `conformer`.
 * An angle of exactly 0 moves neither positions nor rows, and its grad_angles entry is the derivative all the same. An inert
 * torsion gets +0.0 and touches nothing else. An atom whose current row is all zero is left out of the sums and keeps its row:
 * its coordinates may be NaN or infinite. The tree rules are assumed, as undoing the turns needs them (a_k not in M_k): outside
 * them the call stays inside its arrays and its values are unspecified. T == 0 copies grad_out to grad_coords. Asynchronous on
 * `stream`. MVX_ERR_INVALID before any device is touched for, in order: B < 0; T outside 0 .. 32; NULL offsets with B > 0,
 * offsets[0] != 0 or decreasing offsets; offsets[B] >= 2^31; NULL conformer, grad_out or grad_coords with atoms; NULL axes, moves,
 * angles or grad_angles with atoms and T > 0; a NULL handle. No molecules or no atoms: MVX_OK.
 */
int mvx_apply_torsions_backward(mvx_handle *h, const double *conformer, const int64_t *offsets, int32_t B, int32_t T,
                                const int32_t *axes, const int32_t *moves, const double *angles, const double *grad_out,
                                double *grad_coords, double *grad_angles, void *stream);

/*
 * mvx_score_hessian_batch with torsions: the gradient and Hessian of the scores in the coordinates x = (tau, omega, theta_0 ..
 * theta_{T-1}), n = 6 + T, at x = 0, where p_n(x) = exp([omega]x) (C(theta)_n - o_b) + o_b + tau in the grid frame and the
 * caller's coords are the conformer the angles are counted from. The same walk and reductions as mvx_score_hessian_batch - its
 * arguments, rules and outputs, each bit for bit -, then per (molecule, torsion) one workgroup sums over the atoms of M_k, in
 * twist_hess's order and skipping atoms whose g and H rows are all zero, with r_n = p_n - o_b and J_n = [I | -[r_n]x]:
 *   F_k = sum g_n   N_k = sum r_n x g_n   X_k = sum J_n^T H_n J_n (6x6)   K_k = sum r_n g_n^T (3x3)
 * and with u_k the unit axis, s_k = (tau_k, u_k) = ((p_{b_k} - o_b) x u_k, u_k) and c_k = tau_k x F_k + (K_k - tr(K_k) I) u_k:
 *   flex_grad[b]: (n,)    [twist_grad | s_k . (F_k, N_k)]
 *   flex_hess[b]: (n, n)  [:6, :6] = twist_hess; [:6, 6 + k] = X_k s_k with c_k added to the omega rows; [6 + k, 6 + l] =
 *                         s_k^T X_l s_l + u_k . c_l where k is l or an ancestor of l, 0 for unrelated torsions; mirrored:
 *                         symmetric to the bit, written in full, row-major
 *   T, axes (B, T, 2) int32, moves (sumN,) int32: as for mvx_apply_torsions, device; NULL allowed with T == 0.
 *   flex_grad: (B, n) double; flex_hess: (B, n, n) double or NULL; atom_pos: (sumN, 3) double or NULL: the grid-frame positions
 *   p_n the records hold, copied out.
 * T == 0 gives the twist values. The subset sums live in handle-owned workspace (B * T * 36 doubles, and the twist values where
 * the caller passed NULL for them). No atomics; a molecule's values do not depend on its batch. MVX_ERR_INVALID before any device
 * is touched for what mvx_score_hessian_batch rejects, in its order, then for T outside 0 .. 32, for NULL axes with T > 0
 * and B > 0 or NULL moves with T > 0 and atoms, and for a NULL flex_grad with B > 0.
 */
int mvx_score_hessian_flex_batch(mvx_handle *h, int32_t mode, const double *coords, const void *channels, const mvx_real *radii,
                                 double radius_scalar, int32_t radii_type, const int64_t *offsets, const mvx_xform *xforms,
                                 int32_t B, int32_t C, const void *field, int64_t field_mol_stride, const double *pivots,
                                 double *scores, double *atom_grad, double *atom_hess, double *twist_grad, double *twist_hess,
                                 int32_t T, const int32_t *axes, const int32_t *moves, double *flex_grad, double *flex_hess,
                                 double *atom_pos, void *stream);

/*
 * mvx_lm_step in n = 6 + T coordinates: the same state machine per pose, statement for statement, with G, H, G2, H2 and x of
 * width n ((B, n), (B, n, n)) and the torsion angles theta, theta2 (B, T) next to the pose. One wave per pose, the n x (n + 1)
 * system in LDS; the same pivot rule (the first row at or below k with the largest |entry|), the same element operations and
 * back substitution in ascending column order: with T == 0 the results are mvx_lm_step's bits. An accepted trial also copies
 * theta2 -> theta; the next trial is theta2 = theta + x[6:]. A zero pivot or a non-finite component of x, q, t, theta, lam, q2,
 * t2 or theta2: x = 0 and the trial is the state. MVX_ERR_INVALID before any device is touched for: B < 0; T outside 0 .. 32; a
 * NULL q, t, S, G, H, lam, taken, dropped, q2 or t2 with B > 0, or a NULL theta or theta2 with B > 0 and T > 0; a NULL S2, G2 or
 * H2 with have_trial and B > 0; max_dropped < 1; lam_down or lam_up not finite or <= 0; a NULL handle. B == 0: MVX_OK.
 */
int mvx_flex_lm_step(mvx_handle *h, int32_t B, int32_t T, int32_t have_trial, double lam_down, double lam_up, int32_t max_dropped,
                     double *q, double *t, double *theta, double *S, double *G, double *H, double *lam, int32_t *taken,
                     int32_t *dropped, double *q2, double *t2, double *theta2, const double *S2, const double *G2, const double *H2,
                     double *x, void *stream);

/*
 * Replaces do_transform on an (N,3) fp64 point cloud (numpy/transform.py:44-60): out = transformed coords.
 * Exposed so that RandomTransform/T objects can run on device-resident coordinates.
 */
int mvx_transform_coords(mvx_handle *h, const double *coords, int64_t N, const mvx_xform *xform, double *out,
                         int32_t in_kind, int32_t out_kind, void *stream);

/* Kernel timing, measured with HIP events recorded on the launch stream immediately before and
 * after the dominant (voxelize) kernel of every call while profiling is enabled. Recording does not
 * synchronise; up to MVX_PROFILE_RING launches are kept. mvx_profile_read synchronises on the last
 * event, writes the per-launch durations (ms, oldest first) and resets the ring. bench.py uses it
 * for `roofline.achieved`; mvx_last_kernel_ms is the single-launch convenience form. */
#define MVX_PROFILE_RING 1024
int mvx_set_profiling(mvx_handle *h, int32_t enable);
int mvx_profile_read(mvx_handle *h, float *ms, int32_t capacity, int32_t *count);
int mvx_last_kernel_ms(mvx_handle *h, float *ms);

/* Device memory helpers for callers without a device allocator of their own (torch-less use;
 * numpy/voxelizer.py:60-70 get_empty_grid's role on the device). */
int mvx_alloc(mvx_handle *h, int64_t bytes, void **ptr);
int mvx_free(mvx_handle *h, void *ptr);
int mvx_memcpy(mvx_handle *h, void *dst, const void *src, int64_t bytes, int32_t dst_kind, int32_t src_kind,
               void *stream);
int mvx_memset_zero(mvx_handle *h, void *ptr, int64_t bytes, void *stream);
int mvx_stream_sync(mvx_handle *h, void *stream);

/* Testing aid: copy the first n 64-byte atom records of the last call (px, py, pz, T as 4 doubles;
 * k float; type int32; x/y/z admitted voxel ranges as lo | hi << 16; 12 B pad) to host memory.
 * Synchronises the stream. Lets the tests check the prep stage (transform, culls, thresholds) alone. */
int mvx_debug_read_records(mvx_handle *h, void *host_dst, int64_t n, void *stream);
/* Testing aid: explicit per-handle switches for code paths production sizes rarely reach. The library itself reads
 * no environment variable.
 *   "chunks" = k (1..16): cut batches of >= 4k molecules into k molecule chunks whose pre-pass runs on a side stream
 *              one chunk ahead (the loop that otherwise only runs beyond 65535 (molecule, channel chunk) pairs);
 *   "max_ct" = 1..32: upper bound on the channels one workgroup accumulates (more channel chunks);
 *   "direct" = 1 / 0 / -1: always / never / automatically take the single-launch per-molecule kernel (float32 grids);
 *   "mall_budget_kb" = k: cut batches into chunks of at most k KiB of pre-pass data (production: 288 MB, sized for
 *              the 256 MiB Infinity Cache), so that small test batches exercise the chunk-by-chunk launch order;
 *   "max_ct64" = 16 | 32: float64 grids: channels one workgroup accumulates (default 32: Gaussian grids of more than
 *              16 channels take 32 per workgroup on 4-wave slabs; 16 = the two-chunk form every other grid uses);
 *   "nw" = 1..16: waves (8-voxel z sub-tiles) per slab instead of the plan's (0 = the plan); measurement aid;
 *   "grad_order" = 0 / 1: mvx_backward_batch runs the atoms in the caller's order (0, the default) or in spatial order,
 *              each XCD one contiguous range of it (1); results are the same bits either way. Measurement aid;
 *   "mgrad_scratch_kb" = k: mvx_moments_backward_batch cuts its call until the float32 grids of a molecule chunk fit k KiB
 *              (production: 1 GiB; 0 restores it), so that small test batches exercise that cut;
 *   "dense_grid": accepted and ignored (round 2's second voxelize launch no longer exists). */
int mvx_debug_set_option(mvx_handle *h, const char *name, int32_t value);

/*
 * How a call of a given shape is executed: the library's whole decision table (route, slab decomposition, channel and
 * molecule chunks, pacing, write-out path) as a pure host function - no handle, no device, nothing is launched. The forward
 * entry points take exactly these decisions (with the handle's debug options applied on top). Exposed so that the table can
 * be pinned by tests and read by callers who size their batches (the reference has no counterpart: it has one code path).
 */
enum mvx_route {
    MVX_ROUTE_BINNED = 0,    /* prep -> xbin -> voxelize_kernel (slab lines; the batched float32 pipeline) */
    MVX_ROUTE_DIRECT = 1,    /* voxelize_pair_kernel: the whole call in one launch */
    MVX_ROUTE_F64_DENSE = 2, /* float64 grids, vector kernels */
    MVX_ROUTE_F64_MX = 3     /* float64 grids, 32-channel chunks on the matrix cores */
};
typedef struct mvx_plan_query {
    int32_t dimension;
    int32_t blockdim;      /* <= 0: the reference default 8 */
    int32_t precision;     /* 32 (or 0) | 64 */
    int32_t mode;          /* 0 features, 1 types, 2 single */
    int32_t radii_type;    /* enum mvx_radii */
    int32_t B, C;          /* molecules, channels */
    int32_t out_aligned16; /* 1: the grid pointer is 16-byte aligned */
    int64_t total_atoms;   /* over the batch */
    int64_t max_atoms;     /* of one molecule */
} mvx_plan_query;
typedef struct mvx_plan {
    int32_t route;            /* enum mvx_route */
    int32_t nsx, nsy, nzc;    /* slabs along x, along y, z chunks of a row */
    int32_t nw;               /* waves per slab: a slab is 2 x 4 x (8 nw) voxels */
    int32_t ct, ncc;          /* channels per workgroup, channel chunks */
    int32_t nfull, ct_rem;    /* chunks of the main launch; width of the remainder launch's kernel (0: none) */
    int32_t nchunk;           /* molecule chunks (gridDim.y limit, Infinity Cache budget, "chunks" option) */
    int32_t pace;             /* 0 none, 1 empty slabs hold their zero fill back, 2 light slabs pace their rounds too */
    int32_t grouped;          /* channel-wise radii for features: the grouped matrix-core launch */
    int32_t lane_range;       /* sub-tiles straddle reference blocks: per-lane index ranges */
    int32_t vec_store;        /* 16-byte stores (rows are whole 16-byte quads and the grid is aligned) */
    int32_t xcd_ranges;       /* run-wise write-out with one contiguous slab range per XCD */
    int32_t cpad;             /* channel weights per atom the voxelize kernels read */
    int32_t weights_in_place; /* 1: the caller's feature rows are read in place (no packed copy) */
    int32_t reserved;
} mvx_plan;
int mvx_plan_call(const mvx_plan_query *query, mvx_plan *plan);
/* The plan of a call on a grid of the given mvx_grid_type; mvx_plan_call is grid_type 0. MVX_GRID_BF16: `out_aligned16`
 * stands for the grid's 8-byte alignment (one store of four bfloat16 voxels), and the plan is the float32 plan of that query.
 * MVX_ERR_INVALID for an unknown grid_type, and for MVX_GRID_BF16 with precision 64. */
int mvx_plan_call_grid(const mvx_plan_query *q, int32_t grid_type, mvx_plan *p);
/* ... and of the given mvx_grid_layout; mvx_plan_call_grid is layout 0. MVX_LAYOUT_NDHWC: `out_aligned16` is the grid's 16-byte
 * alignment for either element type, vec_store = 1 exactly when every voxel's channel run starts on a 16-byte boundary
 * (C * element size a multiple of 16, aligned grid), rows are cut into slabs of at most 8 waves, no pacing, no XCD ranges;
 * C == 1 gives the contiguous plan. MVX_ERR_INVALID for an unknown layout, and for MVX_LAYOUT_NDHWC with precision 64. */
int mvx_plan_call_layout(const mvx_plan_query *q, int32_t grid_type, int32_t layout, mvx_plan *p);
/* Testing aid: the plan the last forward call on this handle took - mvx_plan_call_layout of that call's shape with the handle's
 * debug options ("chunks", "mall_budget_kb", "direct", "max_ct", "nw" ...) applied, which the pure functions above cannot see.
 * Lets a test assert that a call really was cut into `nchunk` molecule chunks where no launch count shows it (float64 grids
 * run every chunk's pre-pass and then one voxelize launch). MVX_ERR_INVALID before the first forward call. */
int mvx_debug_last_plan(mvx_handle *h, mvx_plan *plan);
#ifdef __cplusplus
}
#endif
#endif /* MVX_H */
