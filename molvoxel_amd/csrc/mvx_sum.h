// mvx_sum.h - launchers of the summed-grid kernels (mvx_sum.hip), used by mvx_forward_sum_batch and mvx_forward_views_sum (mvx_capi.hip).
#pragma once
#include "mvx_internal.h"

namespace mvx {

// One (C, D, D, D) float32 NCDHW grid = the sum of the grids of molecules [a.p.b0, a.p.b0 + nb), in molecule and atom order:
// a.out is that grid, a.p.C its channel count, a.p.ncc = ceil(C / 32) chunks of 32 channels whose weight rows (a.w, a.p.w_stride
// floats apart) are zero padded to whole chunks. accumulate: the sums start from the values in a.out instead of zero.
// Needs a.p.vec_store (D % 4 == 0, a 16-byte aligned grid) and candidate lists without per-lane ranges.
hipError_t launch_voxelize_sum(const VoxArgs &a, int32_t nb, bool gauss, bool accumulate, hipStream_t s);

// The opt-in split of a summed call into parts (mvx_set_sum_parts): at most SUM_PARTS_MAX parts of q = ceil(B / K) molecules each,
// B = a.p.B the molecules of the CALL. `parts`: G = ceil(B / q) partial grids of C * D^3 floats, zeroed at the start of the call.
// One launch per molecule chunk [a.p.b0, a.p.b0 + nb) covers the parts that meet the chunk: each sums its molecules of the chunk
// onto its partial grid. launch_sum_parts_reduce, once after the last chunk: out = (accumulate ? out : +0) + S_0 + ... + S_{G-1}
// in float32, one rounding per add, in that order (`voxels` = C * D^3, a multiple of 4; both pointers 16-byte aligned).
constexpr int SUM_PARTS_MAX = 64;
hipError_t launch_voxelize_sum_parts(const VoxArgs &a, int32_t nb, bool gauss, float *parts, int32_t q, hipStream_t s);
hipError_t launch_sum_parts_reduce(const float *parts, float *out, size_t voxels, int32_t G, bool accumulate, hipStream_t s);

// a[off[b] .. off[b + 1]) = view_weights[b] for the B views of a selection: `off` are its B + 1 DEVICE offsets, total = off[B]
hipError_t launch_view_weights(float *a, const float *view_weights, const int64_t *off, int32_t B, int64_t total, hipStream_t s);

// w[n, c] = fl32(weights[n] * w[n, c]) for the packed rows (cpad floats each) of atoms [first, total)
hipError_t launch_scale_rows(float *w, const float *weights, int64_t first, int64_t total, int32_t cpad, hipStream_t s);

} // namespace mvx
