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
#include "mvx_sum.h"

#include "mvx_device.h"
#include "mvx_ops32.h"

#include <algorithm>

namespace mvx {

template <bool GAUSS, int MAXT>
__global__ void __launch_bounds__(MAXT, 4)
    voxelize_sum_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                        const uint2 *__restrict__ slist_ext, float *out, const int nb, const int accumulate, const VoxParams P) {
    typedef OpsMx32<GAUSS, false, false, false, float> Ops;
    constexpr bool BIG = MAXT > 512;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = P.NW;
    unsigned *un = reinterpret_cast<unsigned *>(smem);

    // grid = (T, ncc): t = slab id, blockIdx.y = channel chunk
    unsigned t = blockIdx.x;
    const unsigned TS = P.nslab;
    if (P.nzc > 1) { // consecutive blocks = consecutive x-slabs (mvx_slab_body.inc)
        const unsigned per_x = (unsigned)(P.nsy * P.nzc), nsx = (unsigned)P.nsx;
        const unsigned tq = __umulhi(t, P.nsx_inv);
        t = (t - tq * nsx) * per_x + tq;
    }
    const int cc = (int)blockIdx.y;
    int sx, sy, zc;
    decode_slab(t, P, sx, sy, zc);
    const int x0 = SUBX * sx, y0 = SUBY * sy, z0 = zc * SUBZ * NW;
    const LaneCtx L = Ops::ctx(lane, wave, x0, y0, z0, zc * NW, cc * 32, P);

    typename Ops::Acc acc;
    Ops::zero(acc);
    if (accumulate) {
        // read-in, the inverse of OpsMx32::write's map: register r of this lane is channel 8 (r / 4) + 4 (lane / 32) + r % 4 of
        // the chunk at voxel (x0 | x0 + 1, iy, iz). Channels and voxels that do not exist keep their zeros (never written).
        const int D = P.D, h = lane >> 5;
        const size_t D2 = (size_t)D * D, D3 = D2 * D;
        const bool yz = L.iy < D && L.iz < D;
        const bool ok0 = yz && x0 < D, ok1 = yz && x0 + 1 < D;
        const float *src = out + (size_t)(L.cbase + 4 * h) * D3 + (size_t)x0 * D2 + (size_t)L.iy * D + L.iz;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int c = 8 * (r / 4) + (r % 4);
            if (L.cbase + 4 * h + c < P.C) {
                if (ok0) acc.p0[r] = src[(size_t)c * D3];
                if (ok1) acc.p1[r] = src[(size_t)c * D3 + D2];
            }
        }
    }

    const RoundSrc<Ops> RS_ = round_src<Ops>(rec, w, lane, L, P);
    const int RW = 8 * NW < 64 ? 8 * NW : 64; // rows staged per round
    bool rows_live = false; // (uniform) the row region still holds the rows of the molecule before
    for (int i = 0; i < nb; ++i) {
        // the candidate line of (molecule b0 + i, this slab): {count, first atom}, then {atom index, packed ranges} per candidate
        const size_t li = (size_t)(P.b0 + i) * (size_t)TS + t;
        const uint2 *__restrict__ line = slist + li * SLOTS; // (uniform: scalar loads)
        const uint2 hdr = line[0];
        const unsigned n_hdr = __builtin_amdgcn_readfirstlane(hdr.x);
        if (n_hdr == 0) continue; // an empty line costs its header: no barrier
        const int64_t a0 = (int64_t)(unsigned)__builtin_amdgcn_readfirstlane(hdr.y);
        const bool xl = __builtin_expect(n_hdr > (unsigned)LINE_CAP, 0); // the slab walks its (molecule, x-slab) list
        const uint2 *__restrict__ ext = slist_ext + li * EXT_SLOTS;
        int n = (int)n_hdr;
        if (xl) { // (explicit scalar halves and the global address space keep every line entry on the scalar path: mvx_slab_body.inc)
            const uint2 where = line[1];
            const unsigned long long at = ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)where.y) << 32) |
                                          (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)where.x);
            typedef const uint2 __attribute__((address_space(1))) *global_u2;
            const global_u2 xlp = (global_u2)at;
            n = __builtin_amdgcn_readfirstlane((int)xlp[0].x);
            line = (const uint2 *)(xlp + (XL_HEADER - 1));
            ext = line + SLOTS;
        }
        if (rows_live) __syncthreads(); // every wave is done with the rows of the molecule before
        rows_live = true;
        stage_first_rounds<Ops, BIG>(line, ext, n, RW, un, RS_, a0, lane, wave);
        __syncthreads();
        filter_walk<Ops>(xl, acc, 0, n, RW, un, lane, wave, L, P, nullptr, nullptr);
        if (n >= RW) filter_walk<Ops>(xl, acc, RW, n, RW, un + RW * Ops::SW, lane, wave, L, P, nullptr, nullptr); // (staged with the first)
        for (int e0 = 2 * RW; e0 <= n; e0 += RW) {
            __syncthreads();
            stage_round<Ops, BIG>(line, ext, e0, n, un, RS_, a0, lane, wave, NW);
            __syncthreads();
            filter_walk<Ops>(xl, acc, e0, n, RW, un, lane, wave, L, P, nullptr, nullptr);
        }
    }
    // one ordinary write-out (it begins with a barrier); "molecule" 0: the grid is the call's only one
    Ops::write(acc, 1, un, tid, lane, wave, NW, 0, L, x0, y0, z0, out, P);
}

__global__ void __launch_bounds__(256) scale_rows_kernel(float *__restrict__ w, const float *__restrict__ weights, int64_t first, int64_t count, int32_t cpad) {
    const int64_t step = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += step) {
        const int64_t n = first + i / cpad;
        w[first * cpad + i] = weights[n] * w[first * cpad + i];
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
    // rows of two rounds (stage_first_rounds) or the write-out tile of eight channels, whichever is larger
    const size_t lds = std::max(voxelize_lds_bytes(32, p.NW, MX_CR), (size_t)2 * 64 * cand_stride_words(32) * 4);
    static LdsLimit raised;
    auto kern = &voxelize_sum_kernel<GAUSS, MAXT>;
    hipError_t e = raise_lds_limit(kern, lds, raised);
    if (e != hipSuccess) return e;
    launch_profiled(kern, dim3(p.nslab, (unsigned)p.ncc), dim3(p.NW * 64), lds, s, a.rec, a.w, a.slist, a.slist_ext,
                    static_cast<float *>(a.out), (int)nb, accumulate ? 1 : 0, p);
    return hipGetLastError();
}

hipError_t launch_voxelize_sum(const VoxArgs &a, int32_t nb, bool gauss, bool accumulate, hipStream_t s) {
    if (!a.p.vec_store || a.p.xcd_ranges || a.p.ncc < 1 || a.p.ncc > 65535 || a.p.NW < 1 || a.p.NW > 16 || nb < 0) return hipErrorInvalidValue;
    if (a.p.NW <= 8) return gauss ? launch_sum<true, 512>(a, nb, accumulate, s) : launch_sum<false, 512>(a, nb, accumulate, s);
    return gauss ? launch_sum<true, 1024>(a, nb, accumulate, s) : launch_sum<false, 1024>(a, nb, accumulate, s);
}

} // namespace mvx
