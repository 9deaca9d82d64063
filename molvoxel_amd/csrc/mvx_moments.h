// mvx_moments.h - launchers of the moments kernels (mvx_moments.hip), used by mvx_moments_batch (mvx_capi.hip).
#pragma once
#include "mvx_internal.h"

namespace mvx {

// Doubles of workspace one launch over nb molecules needs: one partial per (molecule, slab, moment, channel).
inline size_t moments_part_doubles(const VoxParams &p, int32_t nb, int32_t K) { return (size_t)nb * p.nslab * (size_t)K * (size_t)p.C; }

// The per-channel moments of molecules [a.p.b0, a.p.b0 + nb), K = target ? 3 : 2 per channel, from the plan of a summed call
// (a.p.ncc = ceil(C / 32) chunks on zero-padded weight rows, a.p.vec_store, no per-lane ranges; nb * a.p.ncc <= 65535):
// moments_kernel leaves one partial per (molecule, slab, moment, channel) in `part` (moments_part_doubles(a.p, nb, K) doubles),
// moments_finish_kernel sums every molecule's slabs in slab order into moments[(a.p.b0 + b), c, k]. target: (C, D, D, D)
// float32 NCDHW, or null. target_stride: elements between the targets of two molecules of the CALL - 0 (one target shared by all)
// or C * D^3 (molecule a.p.b0 + b reads target + (a.p.b0 + b) * target_stride). Nothing is written to a.out.
hipError_t launch_moments(const VoxArgs &a, int32_t nb, bool gauss, const float *target, int64_t target_stride, double *part, double *moments,
                          hipStream_t s);

} // namespace mvx
