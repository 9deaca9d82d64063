// mvx_sum.h - launchers of the summed-grid kernels (mvx_sum.hip), used by mvx_forward_sum_batch (mvx_capi.hip).
#pragma once
#include "mvx_internal.h"

namespace mvx {

// One (C, D, D, D) float32 NCDHW grid = the sum of the grids of molecules [a.p.b0, a.p.b0 + nb), in molecule and atom order:
// a.out is that grid, a.p.C its channel count, a.p.ncc = ceil(C / 32) chunks of 32 channels whose weight rows (a.w, a.p.w_stride
// floats apart) are zero padded to whole chunks. accumulate: the sums start from the values in a.out instead of zero.
// Needs a.p.vec_store (D % 4 == 0, a 16-byte aligned grid) and candidate lists without per-lane ranges.
hipError_t launch_voxelize_sum(const VoxArgs &a, int32_t nb, bool gauss, bool accumulate, hipStream_t s);

// w[n, c] = fl32(weights[n] * w[n, c]) for the packed rows (cpad floats each) of atoms [first, total)
hipError_t launch_scale_rows(float *w, const float *weights, int64_t first, int64_t total, int32_t cpad, hipStream_t s);

} // namespace mvx
