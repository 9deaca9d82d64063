// mvx_sum.hip - one summed grid per batch (gfx950): G[c, v] = sum over the atoms of ALL molecules of a call, in the caller's
// order, of u[n, c] * rho_{n, c}(v) - the float32 fma chain the slab kernels run inside one molecule, carried across the
// molecule boundaries.
//
//   voxelize_sum_kernel  one workgroup per (output slab, chunk of 32 channels); the molecule is NOT a grid dimension. All
//                        molecules of a call share the box, and the pre-pass (prep + xbin) leaves one ordered candidate line
//                        per (molecule, slab): the workgroup walks the lines of its slab molecule after molecule with the
//                        rounds of mvx_slab_body.inc (stage, barrier, filter_walk, line extension, x-list), the accumulators
//                        in registers all the way, and writes the slab once. The sums start from zero or, with `accumulate`,
//                        from the values already in the grid (molecule chunks k > 0 of a cut call, and the caller's own
//                        accumulation). No atomics and no split of the molecules over workgroups: the bits depend on the atom
//                        order alone, never on the launch shape.
//                        Always the matrix-core walk (OpsMx32, bit for bit the fmaf chain of the narrow kernels): channel
//                        counts that are no multiple of 32 run zero-padded weight rows, and only real channels are written.
//                        Compiled for 128 registers (two 8-wave workgroups per compute unit): the accumulators are live across
//                        the staging loads of every molecule but the first, which the one-molecule kernels avoid by staging
//                        before the accumulators exist. One write per slab for the whole batch: no pacing.
//   scale_rows_kernel    per-atom weights: the packed weight rows scaled in float32, u[n, c] = fl32(a_n * w[n, c]).
//   voxelize_sum_parts_kernel  the same walk (mvx_sum_body.inc) with the call's molecules cut into G parts (mvx_set_sum_parts):
//                        one workgroup per (slab, chunk, part) sums its part into a partial grid of its own, so a batch of many
//                        small molecules fills the card with G times the workgroups. Still no atomics.
//   sum_parts_reduce_kernel  once per call: out = (out | +0) + S_0 + S_1 + ... in part order, 16 bytes per load and store.
//   view_weights_kernel  mvx_forward_views_sum: one weight per view expanded to one per selected atom from the device offsets.
#include "mvx_sum.h"

#include "mvx_device.h"
#include "mvx_ops32.h"

#include <algorithm>

namespace mvx {

// how both kernels end the walk of mvx_sum_body.inc: one ordinary write-out (it begins with a barrier); "molecule" 0: the grid is
// the only one behind `grid`
#define MVX_SUM_WRITE Ops::write(acc, 1, un, tid, lane, wave, NW, 0, L, x0, y0, z0, grid, P)

template <bool GAUSS, int MAXT>
__global__ void __launch_bounds__(MAXT, 4)
    voxelize_sum_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                        const uint2 *__restrict__ slist_ext, float *out, const int nb, const int accumulate, const VoxParams P) {
    float *const grid = out;
    const int mol0 = P.b0, nmol = nb, from_grid = accumulate;
#include "mvx_sum_body.inc"
    MVX_SUM_WRITE;
}

// The same walk for one PART of the call's molecules (mvx_set_sum_parts, K > 1): blockIdx.z + g0 is the part g, which owns the
// molecules [g q, min(B, (g + 1) q)) of the CALL (P.B of them) and the partial grid parts + g C D^3. The workgroup walks what of
// its part lies in this launch's molecule chunk [P.b0, P.b0 + nb), continuing from the partial grid unless the chunk holds the
// part's first molecule, and writes the partial grid back; a part that does not meet the chunk does nothing.
template <bool GAUSS, int MAXT>
__global__ void __launch_bounds__(MAXT, 4)
    voxelize_sum_parts_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                              const uint2 *__restrict__ slist_ext, float *parts, const int nb, const int q, const int g0, const VoxParams P) {
    const long long g = (long long)g0 + (long long)blockIdx.z; // (uniform)
    const long long first = g * q, lo = first > P.b0 ? first : (long long)P.b0;
    long long hi = first + q < (long long)P.B ? first + q : (long long)P.B;
    if (hi > (long long)P.b0 + nb) hi = (long long)P.b0 + nb;
    if (lo >= hi) return; // (the whole workgroup: before any barrier)
    float *const grid = parts + (size_t)g * ((size_t)P.C * P.D * P.D * P.D);
    const int mol0 = (int)lo, nmol = (int)(hi - lo), from_grid = lo > first ? 1 : 0;
#include "mvx_sum_body.inc"
    MVX_SUM_WRITE;
}

// out[v] = (accumulate ? out[v] : +0) + S_0[v] + S_1[v] + ... + S_{G-1}[v]: one float32 rounding per add, in part order; n4
// quads of four voxels, partial g at parts + g n4 quads.
__global__ void __launch_bounds__(256) sum_parts_reduce_kernel(const float4 *__restrict__ parts, float4 *__restrict__ out, size_t n4, int G,
                                                               int accumulate) {
    const size_t step = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += step) {
        float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
        if (accumulate) r = out[i];
        for (int g = 0; g < G; ++g) {
            const float4 p = parts[(size_t)g * n4 + i];
            r.x = r.x + p.x;
            r.y = r.y + p.y;
            r.z = r.z + p.z;
            r.w = r.w + p.w;
        }
        out[i] = r;
    }
}

__global__ void __launch_bounds__(256) scale_rows_kernel(float *__restrict__ w, const float *__restrict__ weights, int64_t first, int64_t count, int32_t cpad) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step) {
        const int64_t n = first + i / cpad;
        w[first * cpad + i] = weights[n] * w[first * cpad + i];
    }
}

// Per-view weights as per-atom weights of the gathered batch: a[off[b] .. off[b + 1]) = view_weights[b], the view of row n found
// by bisection of the B + 1 device offsets (views without atoms own no row).
__global__ void __launch_bounds__(256) view_weights_kernel(float *__restrict__ a, const float *__restrict__ view_weights,
                                                           const int64_t *__restrict__ off, int32_t B, int64_t total) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < total; n += step) {
        int lo = 0, hi = B; // the last b with off[b] <= n (off[0] = 0 <= n < total = off[B])
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (off[mid] <= n) lo = mid;
            else hi = mid;
        }
        a[n] = view_weights[lo];
    }
}

hipError_t launch_scale_rows(float *w, const float *weights, int64_t first, int64_t total, int32_t cpad, hipStream_t s) {
    const int64_t count = (total - first) * (int64_t)cpad;
    if (count <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<int64_t>((count + 255) / 256, 65536);
    hipLaunchKernelGGL(scale_rows_kernel, dim3(blocks), dim3(256), 0, s, w, weights, first, count, cpad);
    return hipGetLastError();
}

template <bool GAUSS, int MAXT>
static hipError_t launch_sum(const VoxArgs &a, int32_t nb, bool accumulate, hipStream_t s) {
    const VoxParams &p = a.p;
    return launch_kernel<voxelize_sum_kernel<GAUSS, MAXT>>(dim3(p.nslab, (unsigned)p.ncc), dim3(p.NW * 64), voxelize_mx_lds_bytes(p.NW), s, a.rec, a.w,
                                                           a.slist, a.slist_ext, static_cast<float *>(a.out), (int)nb, accumulate ? 1 : 0, p);
}

hipError_t launch_voxelize_sum(const VoxArgs &a, int32_t nb, bool gauss, bool accumulate, hipStream_t s) {
    if (!a.p.vec_store || a.p.xcd_ranges || a.p.ncc < 1 || a.p.ncc > 65535 || a.p.NW < 1 || a.p.NW > 16 || nb < 0) return hipErrorInvalidValue;
    if (a.p.NW <= 8) return gauss ? launch_sum<true, 512>(a, nb, accumulate, s) : launch_sum<false, 512>(a, nb, accumulate, s);
    return gauss ? launch_sum<true, 1024>(a, nb, accumulate, s) : launch_sum<false, 1024>(a, nb, accumulate, s);
}

hipError_t launch_view_weights(float *a, const float *view_weights, const int64_t *off, int32_t B, int64_t total, hipStream_t s) {
    if (total <= 0 || B <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<int64_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(view_weights_kernel, dim3(blocks), dim3(256), 0, s, a, view_weights, off, B, total);
    return hipGetLastError();
}

template <bool GAUSS, int MAXT>
static hipError_t launch_sum_parts(const VoxArgs &a, int32_t nb, float *parts, int32_t q, int32_t g0, int32_t ng, hipStream_t s) {
    const VoxParams &p = a.p;
    return launch_kernel<voxelize_sum_parts_kernel<GAUSS, MAXT>>(dim3(p.nslab, (unsigned)p.ncc, (unsigned)ng), dim3(p.NW * 64), voxelize_mx_lds_bytes(p.NW),
                                                                 s, a.rec, a.w, a.slist, a.slist_ext, parts, (int)nb, (int)q, (int)g0, p);
}

hipError_t launch_voxelize_sum_parts(const VoxArgs &a, int32_t nb, bool gauss, float *parts, int32_t q, hipStream_t s) {
    if (!a.p.vec_store || a.p.xcd_ranges || a.p.ncc < 1 || a.p.ncc > 65535 || a.p.NW < 1 || a.p.NW > 16 || nb < 0 || q < 1 || !parts)
        return hipErrorInvalidValue;
    if (nb == 0) return hipSuccess;
    // the parts that meet the chunk [b0, b0 + nb): at most MVX_SUM_PARTS_MAX of them, in gridDim.z
    const int32_t g0 = a.p.b0 / q, ng = (a.p.b0 + nb - 1) / q - g0 + 1;
    if (ng < 1 || ng > SUM_PARTS_MAX) return hipErrorInvalidValue;
    if (a.p.NW <= 8) return gauss ? launch_sum_parts<true, 512>(a, nb, parts, q, g0, ng, s) : launch_sum_parts<false, 512>(a, nb, parts, q, g0, ng, s);
    return gauss ? launch_sum_parts<true, 1024>(a, nb, parts, q, g0, ng, s) : launch_sum_parts<false, 1024>(a, nb, parts, q, g0, ng, s);
}

hipError_t launch_sum_parts_reduce(const float *parts, float *out, size_t voxels, int32_t G, bool accumulate, hipStream_t s) {
    if (voxels % 4 != 0 || G < 1 || ((reinterpret_cast<uintptr_t>(parts) | reinterpret_cast<uintptr_t>(out)) & 15u)) return hipErrorInvalidValue;
    const size_t n4 = voxels / 4;
    if (n4 == 0) return hipSuccess;
    const unsigned blocks = (unsigned)std::min<size_t>((n4 + 255) / 256, 8192);
    hipLaunchKernelGGL(sum_parts_reduce_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<const float4 *>(parts),
                       reinterpret_cast<float4 *>(out), n4, (int)G, accumulate ? 1 : 0);
    return hipGetLastError();
}

} // namespace mvx
