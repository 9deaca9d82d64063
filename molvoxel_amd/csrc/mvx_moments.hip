// mvx_moments.hip - per-channel sums and norms of every molecule's grid without the grid (gfx950). For molecule b and channel c,
// with g = the float32 value the forward kernels store at voxel v:
//   m[b, c, 0] = sum_v (double)g     m[b, c, 1] = sum_v (double)g * (double)g     m[b, c, 2] = sum_v (double)g * (double)target[c, v]
//
//   moments_kernel         the walk of the summed-grid kernels (mvx_sum_body.inc: OpsMx32, chunks of 32 channels on zero-padded
//                          weight rows) for ONE molecule per workgroup: grid = (slab, channel chunk, molecule of the launch). The
//                          accumulators are then bit for bit the values every forward route writes. Instead of a write-out the
//                          epilogue reduces them in float64: products of two float32 values are exact in float64, so the
//                          summation is the only rounding. Per register (one channel, the voxels (x0 | x0 + 1, iy, iz)) the two
//                          planes are added, voxels and channels that do not exist masked to +0; a fixed butterfly over the 32
//                          lanes of each half of the wave that halves the registers a lane carries at every step (16 values per
//                          lane -> 1 in four exchanges, a fifth completes the half); the waves' 32 channel sums through LDS (the
//                          row region, free after the walk), added in wave order; one partial per (molecule, slab, moment,
//                          channel) to the workspace. A slab whose line is empty writes zeros without the reduction. No atomics.
//                          The target is read as the grid is written - eight channels of the slab per round through the
//                          write-out's tile in LDS, 16 bytes per lane - and its moment comes last; the waves' sums then sit behind the tile.
//                          One target for all molecules, or one per molecule of the call (target_stride; mvx_moments_views).
//   moments_finish_kernel  one thread per (molecule, moment, channel): the partials of the molecule's slabs added in slab-id order.
#include "mvx_moments.h"

#include "mvx_device.h"
#include "mvx_ops32.h"

#include <algorithm>

namespace mvx {

// One step of the butterfly: lanes whose bit OFF is clear keep v[0 .. N) and hand over v[N .. 2N), the others the reverse; both
// add what they receive to what they keep, so v[0 .. N) of a lane is the sum over the lane pair of N of the 2N values.
template <int N, int OFF>
static __device__ __forceinline__ void fold_step(double (&v)[8], int lane) {
    const bool up = (lane & OFF) != 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const double keep = up ? v[i + N] : v[i];
        const double send = up ? v[i] : v[i + N];
        v[i] = keep + __shfl_xor(send, OFF);
    }
}

// The sums over the 32 lanes of this lane's half of the wave of the 16 values term(0) .. term(15) every lane brings: the lanes l
// and l ^ 1 both return the sum of term((l >> 1) & 15). The first step takes the terms as they are formed, two at a time, so a
// lane never holds more than eight of them.
template <typename Term>
static __device__ __forceinline__ double fold_half(Term term, int lane) {
    double v[8];
    const bool up = (lane & 16) != 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const double lo = term(i), hi = term(i + 8);
        v[i] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, 16);
    }
    fold_step<4, 8>(v, lane);
    fold_step<2, 4>(v, lane);
    fold_step<1, 2>(v, lane);
    return v[0] + __shfl_xor(v[0], 1);
}

// bytes of the tile a slab's target is read through: eight channels of RPC rows (OpsMx32::write's tile)
__host__ __device__ __forceinline__ size_t moments_tile_bytes(int NW) { return (size_t)MX_CR * RPC * row_stride_floats(NW) * sizeof(float); }

template <bool GAUSS, int MAXT, bool TARGET>
__global__ void __launch_bounds__(MAXT, 4)
    moments_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                   const uint2 *__restrict__ slist_ext, const float *__restrict__ target0, const int64_t target_stride,
                   double *__restrict__ part, const VoxParams P) {
    // blockIdx.z: the molecule of this launch's chunk [P.b0, P.b0 + gridDim.z); nothing is read from or written to a grid
    float *const grid = nullptr;
    const int mol0 = P.b0 + (int)blockIdx.z, nmol = 1, from_grid = 0;
#include "mvx_sum_body.inc"
    constexpr int K = TARGET ? 3 : 2;
    const int C = P.C;
    // this workgroup's partials: [moment][channel] of (molecule of the chunk, slab t)
    double *const slot = part + ((size_t)blockIdx.z * (size_t)TS + t) * (size_t)(K * C);
    if (!rows_live) { // (uniform) no candidate: the partial is zero
        for (int j = tid; j < 32 * K; j += NW * 64) {
            const int c = L.cbase + (j & 31);
            if (c < C) slot[(j >> 5) * C + c] = 0.0;
        }
        return;
    }
    // the register map of mvx_sum_body.inc's read-in: register r of this lane is channel cbase + 4 h + 8 (r / 4) + r % 4 at the
    // voxels (x0, iy, iz) in p0 and (x0 + 1, iy, iz) in p1; voxels beyond the grid and the channels of a padded chunk count as +0
    const int D = P.D, h = lane >> 5;
    const size_t D2 = (size_t)D * D, D3 = D2 * D;
    const bool yz = L.iy < D && L.iz < D;
    const bool ok0 = yz && x0 < D, ok1 = yz && x0 + 1 < D;
    const int c_lane = L.cbase + 4 * h;
    // [wave][moment][channel of the chunk]; with a target behind the tile the target is read through
    double *red = reinterpret_cast<double *>(smem + (TARGET ? moments_tile_bytes(NW) : 0));
    const int fr = (lane >> 1) & 15;                // the register whose sum fold_half leaves in this lane
    const int fc = 8 * (fr >> 2) + 4 * h + (fr & 3);
    // (every moment converts the accumulators again, behind an empty asm: the compiler would otherwise keep all 32 as doubles
    // across the three reductions - 64 registers, 45 of them spilled in the kernels with a target)
    auto val = [](float x) {
        asm volatile("" : "+v"(x));
        return (double)x;
    };
    auto okc = [&](int r) { return c_lane + 8 * (r / 4) + (r % 4) < C; };
    auto g0 = [&](int r) { return (ok0 && okc(r)) ? val(acc.p0[r]) : 0.0; };
    auto g1 = [&](int r) { return (ok1 && okc(r)) ? val(acc.p1[r]) : 0.0; };
    __syncthreads(); // every wave is done with the rows
    double s = fold_half([&](int r) { return g0(r) + g1(r); }, lane);
    if (!(lane & 1)) red[(wave * K + 0) * 32 + fc] = s;
    s = fold_half(
        [&](int r) {
            const double a0 = g0(r), a1 = g1(r);
            return a0 * a0 + a1 * a1;
        },
        lane);
    if (!(lane & 1)) red[(wave * K + 1) * 32 + fc] = s;
    if constexpr (TARGET) {
        // The target comes the way the grid goes out (OpsMx32::write, mirrored): round by round eight channels of the slab,
        // 16 bytes per lane and whole rows per load instruction, into the tile; every lane then takes the values of its own
        // voxels from the tile. (Read voxel by voxel with the read-in's address map - 32 bytes per row and instruction - the
        // call took 4.26 ms at cfg-2 x 256 instead of 3.27.) Tile entries of voxels or channels that do not
        // exist are never written and never used. Last of the moments: the accumulators die round by round as the
        // products take their registers.
        // The target of this molecule OF THE CALL (mol0 = P.b0 + blockIdx.z, not the launch's blockIdx.z alone), target_stride
        // elements apart: 0 is the one shared target. A workgroup-uniform base from kernel arguments and blockIdx alone, so it
        // is formed in scalar registers and costs the lanes nothing.
        const float *const target = target0 + (size_t)mol0 * (size_t)target_stride;
        float *tile = reinterpret_cast<float *>(un);
        const int RS = row_stride_floats(NW);
        const int F4 = (SUBZ / 4) * NW;
        const int rfirst = tid / F4, q4 = tid - rfirst * F4, zq = z0 + 4 * q4;
        const int sxx = (rfirst >> SUBY_SH) & (SUBX - 1), syy = rfirst & (SUBY - 1), cfirst = rfirst / RPC;
        const bool vox_ok = (x0 + sxx < D) && (y0 + syy < D) && (zq < D);
        const float *src0 = target + (size_t)(L.cbase + cfirst) * D3 + (size_t)(x0 + sxx) * D2 + (size_t)(y0 + syy) * D + zq;
        const float *mine = tile + (4 * h * RPC + (L.iy - y0)) * RS + (L.iz - z0); // + (c * RPC + x * SUBY) * RS
        double gt[16]; // g * target of this lane's registers, the two planes added
#pragma unroll
        for (int rd = 0; rd < 4; ++rd) {
            if (rd > 0) __syncthreads(); // the tile of the round before is consumed (first round: the barrier above)
            if (vox_ok) {
#pragma unroll
                for (int p = 0; p < 2; ++p) {
                    const int c = rd * MX_CR + cfirst + 4 * p;
                    if (L.cbase + c < C)
                        *reinterpret_cast<float4 *>(tile + (rfirst + 4 * RPC * p) * RS + 4 * q4) =
                            *reinterpret_cast<const float4 *>(src0 + (size_t)(rd * MX_CR + 4 * p) * D3);
                }
            }
            __syncthreads();
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int r = 4 * rd + c;
                double a0 = 0.0, a1 = 0.0;
                if (ok0 && okc(r)) a0 = val(acc.p0[r]) * (double)mine[(c * RPC) * RS];
                if (ok1 && okc(r)) a1 = val(acc.p1[r]) * (double)mine[(c * RPC + SUBY) * RS];
                gt[r] = a0 + a1;
            }
        }
        s = fold_half([&](int r) { return gt[r]; }, lane);
        if (!(lane & 1)) red[(wave * K + 2) * 32 + fc] = s;
    }
    __syncthreads();
    for (int j = tid; j < 32 * K; j += NW * 64) { // the waves in order
        const int k = j >> 5, cl = j & 31;
        if (L.cbase + cl < C) {
            double sum = red[k * 32 + cl];
            for (int wv = 1; wv < NW; ++wv) sum += red[(wv * K + k) * 32 + cl];
            slot[k * C + L.cbase + cl] = sum;
        }
    }
}

// moments[(b0 + b), c, k] = the partials [b][t][k][c] of molecule b added over t = 0 .. TS - 1 in that order
__global__ void __launch_bounds__(256) moments_finish_kernel(const double *__restrict__ part, double *__restrict__ moments, int nb, int b0, int TS,
                                                             int C, int K) {
    const int KC = K * C;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)nb * KC) return;
    const int b = (int)(i / KC), j = (int)(i - (size_t)b * KC);
    const int k = j / C, c = j - k * C;
    const double *p = part + (size_t)b * TS * KC + j;
    // (the adds are a chain, the loads are not: 32 in flight per thread - one at a time the kernel took 180 us at cfg-2 x 256)
    double s = 0.0;
    int t = 0;
    for (; t + 32 <= TS; t += 32) {
        double v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = p[(size_t)(t + i) * KC];
#pragma unroll
        for (int i = 0; i < 32; ++i) s += v[i];
    }
    for (; t < TS; ++t) s += p[(size_t)t * KC];
    moments[((size_t)(b0 + b) * C + c) * K + k] = s;
}

template <bool GAUSS, int MAXT>
static hipError_t launch_moments_walk(const VoxArgs &a, int32_t nb, const float *target, int64_t target_stride, double *part, hipStream_t s) {
    const VoxParams &p = a.p;
    const dim3 grid(p.nslab, (unsigned)p.ncc, (unsigned)nb), block(p.NW * 64);
    const size_t lds = voxelize_mx_lds_bytes(p.NW); // (the waves' partials, 16 * 2 * 32 doubles at most, fit the row region)
    if (target) // ... and sit behind the tile in the kernels that read a target
        return launch_kernel<moments_kernel<GAUSS, MAXT, true>>(grid, block, std::max(lds, moments_tile_bytes(p.NW) + (size_t)p.NW * 3 * 32 * sizeof(double)),
                                                                s, a.rec, a.w, a.slist, a.slist_ext, target, target_stride, part, p);
    return launch_kernel<moments_kernel<GAUSS, MAXT, false>>(grid, block, lds, s, a.rec, a.w, a.slist, a.slist_ext, target, (int64_t)0, part, p);
}

hipError_t launch_moments(const VoxArgs &a, int32_t nb, bool gauss, const float *target, int64_t target_stride, double *part, double *moments,
                          hipStream_t s) {
    const VoxParams &p = a.p;
    if (!p.vec_store || p.xcd_ranges || p.ncc < 1 || p.ncc > 65535 || p.NW < 1 || p.NW > 16 || nb < 0 || nb > 65535 || !part || !moments ||
        (reinterpret_cast<uintptr_t>(target) & 15u) || target_stride < 0 || (target_stride & 3))
        return hipErrorInvalidValue;
    if (nb == 0) return hipSuccess;
    static_assert(16 * 2 * 32 * sizeof(double) <= (size_t)2 * 64 * cand_stride_words(32) * 4, "the waves' partials must fit the row region");
    hipError_t e;
    if (p.NW <= 8) e = gauss ? launch_moments_walk<true, 512>(a, nb, target, target_stride, part, s) : launch_moments_walk<false, 512>(a, nb, target, target_stride, part, s);
    else e = gauss ? launch_moments_walk<true, 1024>(a, nb, target, target_stride, part, s) : launch_moments_walk<false, 1024>(a, nb, target, target_stride, part, s);
    if (e != hipSuccess) return e;
    const int K = target ? 3 : 2;
    const size_t n = (size_t)nb * K * p.C;
    hipLaunchKernelGGL(moments_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, part, moments, (int)nb, (int)p.b0, (int)p.nslab, (int)p.C, K);
    return hipGetLastError();
}

} // namespace mvx
