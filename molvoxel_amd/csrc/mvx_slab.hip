// mvx_slab.hip - the batched float32 voxelize kernels (gfx950): one workgroup per output slab.
//
//   voxelize_kernel  one workgroup per output slab of 2 x 4 x (8*NW) voxels (NW waves, one 2x4x8 sub-tile per
//                    wave, one voxel per lane, CT channel accumulators per lane in registers): load the slab's
//                    candidate line, stage the candidates' rows in LDS, every wave walks the candidates that
//                    touch its sub-tile (fp64 d2, compare with T, exp2, channel update), then the accumulators are
//                    transposed through LDS and written with non-temporal 16-B/lane stores in whole-row runs.
//                    Every output byte is written exactly once, zeros included (the reference's overwrite
//                    semantics, numpy/voxelizer.py:133-135,158-160); no atomics, no memset, no (V, DHW)
//                    intermediate; HBM-write bound. The channel update of 32-channel chunks - the one dense
//                    contraction in the walk, the reference's own matmul - runs on the matrix cores in exact
//                    float32 (OpsMx32: v_mfma_f32_32x32x2_f32, bit-identical to the fmaf chain), narrower chunks on
//                    the vector ALU (OpsF32, packed FMAs).
//   voxelize_runs_kernel  the same walk for grids whose rows are not whole 16-byte quads (run-wise write-out).
#include "mvx_device.h"
#include "mvx_ops32.h"

#include <algorithm>

namespace mvx {

#ifdef MVX_DIAG
hipError_t set_diag_buffer(void *p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_diag), &p, sizeof(p)); }
#endif

size_t voxelize_lds_bytes(int32_t ct, int32_t NW, int32_t crmax) {
    const int cr = ct < crmax ? ct : crmax;
    const size_t tile = (size_t)cr * RPC * row_stride_floats(NW) * 4;
    const size_t cand = (size_t)64 * cand_stride_words(ct) * 4;
    return tile > cand ? tile : cand;
}

// (the matrix-core kernels keep the rows of TWO rounds: stage_first_rounds)
size_t voxelize_mx_lds_bytes(int32_t NW) { return std::max(voxelize_lds_bytes(32, NW, MX_CR), (size_t)2 * 64 * cand_stride_words(32) * 4); }

// voxelize_kernel's arithmetic: 32-channel chunks go to the matrix cores (OpsMx32), narrower chunks to the vector ALU in
// candidate pairs (OpsPair); the per-lane-range variants keep one voxel per lane and candidate (OpsF32)
template <int CT, bool GAUSS, bool LANE_RANGE, bool GROUPED, typename OT = float>
struct SlabOps {
    typedef OpsF32<CT, GAUSS, LANE_RANGE, OT> type;
};
template <int CT, bool GAUSS, typename OT>
struct SlabOps<CT, GAUSS, false, false, OT> {
    typedef OpsPair<CT, GAUSS, false, OT> type;
};
// (not the per-lane-range variants - blockdim 4, 5, 12, ...: their six extra index comparisons per voxel do not fit the
// 64 registers of the two-voxel layout without scratch: 0.527 against 0.479 ms per 64 cfg-2 molecules at blockdim 5)
template <bool GAUSS, typename OT>
struct SlabOps<32, GAUSS, false, false, OT> {
    typedef OpsMx32<GAUSS, false, false, false, OT> type;
};
template <bool GAUSS, typename OT>
struct SlabOps<32, GAUSS, false, true, OT> {
    typedef OpsMx32<GAUSS, false, true, false, OT> type;
};
// (grouped launches - channel-wise features by radius - exist on the matrix-core path only, per-lane ranges or not)
template <bool GAUSS, typename OT>
struct SlabOps<32, GAUSS, true, true, OT> {
    typedef OpsMx32<GAUSS, true, true, true, OT> type;
};

// OT: the grid type - float, __bf16 (bfloat16 grids, mvx_config.grid_type = MVX_GRID_BF16: only the store of the write-out differs)
// or a channels-last tag (Ndhwc<float>, Ndhwc<__bf16>, mvx_set_grid_layout: every lane stores its voxel's channel run from
// registers; slabs of at most 8 waves only - plan_call cuts longer rows: a cut costs that layout nothing, a voxel's channels are
// whole 16-byte groups). One instantiation per grid type over the same slab body; grid_elem<OT> is the element type of `out`.
template <int CT, bool GAUSS, bool LANE_RANGE, int MAXT, bool GROUPED = false, typename OT = float>
__global__ void __launch_bounds__(MAXT, (MAXT <= 512 ? 8 : BIG_WAVES_PER_SIMD))
    voxelize_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                    const uint2 *__restrict__ slist_ext, const double *__restrict__ Tc, const float *__restrict__ kc,
                    typename grid_elem<OT>::type *__restrict__ out, const VoxParams P) {
    typedef typename SlabOps<CT, GAUSS, LANE_RANGE, GROUPED, OT>::type Ops;
#include "mvx_slab_body.inc"
}

// ---- voxelize_narrow_kernel: narrow chunks with NSUB (2 or 4) sub-tiles per wave -------------------------------------------
// What is left of a narrow launch after OpsPair is per-wave fixed cost: at cfg-3 density a wave walks two or three candidate
// pairs (~85 vector instructions) around ~110 of prologue, staging, row filter and write-out, and as many scalar ones. Here a
// slab of NW sub-tiles is served by NW / NSUB waves: wave w owns sub-tiles NSUB w ... NSUB w + NSUB - 1 - one prologue, one
// share of the staging (stage_round_v: eight slots per trip), then filter + pair walk once per sub-tile (filter_walk:
// OpsPair::walk with that sub-tile's z coordinate) into NSUB accumulator sets, and one write-out (write_slab /
// write_ndhwc_sets over the sets). The slab body itself: its Ops is OpsPair with NSUB sets, nothing else differs. Same candidates,
// same order, same arithmetic per voxel as voxelize_kernel<CT < 32>: bit-identical grids. At most 8 waves per workgroup
// whatever the row length (16 sub-tiles: 128 voxels), so there is no 1024-thread variant. Same box, one -> two sub-tiles
// per wave, kernel: forward_single 0.118 -> 0.109 ms, 8 types 0.173 -> 0.162, cfg-3 x 256 0.219 -> 0.164 (profiles/r04_narrow.txt).
// Waves per SIMD the kernel is compiled for: its natural register need with two sub-tiles is 66 / 72 / 80 for 1 / 4 / 8
// channels (accumulator sets, eight row loads in flight); at the 64 of voxelize_kernel it spilled 1 ... 17 registers.
// (16 channels: 96 registers and no gain over one sub-tile per wave, 0.228 ms both - they keep voxelize_kernel.)
template <int CT, bool GAUSS, int NSUB, typename OT = float>
__global__ void __launch_bounds__(512, 8)
    voxelize_narrow_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                           const uint2 *__restrict__ slist_ext, typename grid_elem<OT>::type *__restrict__ out, const VoxParams P) {
    typedef OpsPair<CT, GAUSS, false, OT, NSUB> Ops;
    constexpr bool GROUPED = false;
    constexpr int MAXT = 512;
    const double *const Tc = nullptr; // (the per-channel tables of the float64 kernels)
    const float *const kc = nullptr;
#include "mvx_slab_body.inc"
}

// 32-channel chunks of float32 grids whose rows are not whole 16-byte quads (odd dimensions, unaligned grid slices): the
// matrix-core walk with the run-wise write-out (store_runs). A kernel of its own: compiled into voxelize_kernel<32, ...>
// the extra write-out path costs the aligned-grid kernels six more spilled registers and 0.5 % of the headline rate.
template <bool GAUSS, int MAXT, typename OT = float>
__global__ void __launch_bounds__(MAXT, (MAXT <= 512 ? 8 : BIG_WAVES_PER_SIMD))
    voxelize_runs_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                         const uint2 *__restrict__ slist_ext, const double *__restrict__ Tc, const float *__restrict__ kc,
                         typename grid_elem<OT>::type *__restrict__ out, const VoxParams P) {
    typedef OpsMx32<GAUSS, false, false, true, OT> Ops;
    constexpr int CT = 32;
    constexpr bool GROUPED = false;
#include "mvx_slab_body.inc"
}

// Narrow chunks (1 ... 16 channels) of such grids: the candidate-pair walk (OpsPair) with the run-wise write-out. Until late in
// round 4 these launches went to the per-lane-range kernels (OpsF32: one candidate and one voxel per lane step, six index
// comparisons per voxel), the only narrow ones that carried store_runs: D = 49 / 50 / 63 ran at half the rate of D = 48 / 64
// (C = 4, kernel ms: 0.238 / 0.228 / 0.200 against 0.120 / 0.099 - profiles/r04_slab_plans.txt).
template <int CT, bool GAUSS, int MAXT, typename OT = float>
__global__ void __launch_bounds__(MAXT, (MAXT <= 512 ? 8 : BIG_WAVES_PER_SIMD))
    voxelize_pair_runs_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                              const uint2 *__restrict__ slist_ext, const double *__restrict__ Tc, const float *__restrict__ kc,
                              typename grid_elem<OT>::type *__restrict__ out, const VoxParams P) {
    typedef OpsPair<CT, GAUSS, true, OT> Ops;
    constexpr bool GROUPED = false;
#include "mvx_slab_body.inc"
}

// (Measured and removed, round 3: channel counts of 32 k + r with the remainder chunk's workgroups - CTR vector-ALU
// accumulators - in the SAME launch as the full chunks' (a kernel that branches on the chunk index into two inclusions of
// the slab body). Bit-identical, and slower than the second launch it replaced: C = 33 0.618 against 0.580 ms per 64
// molecules, C = 40 0.647 / 0.605, C = 48 0.708 / 0.652, C = 65 0.967 / 0.912 - the remainder's workgroups take slots from
// the store-streaming ones for longer than their own launch lasts.)


// ------------------------------------------------------------------------------------------------
// dispatch
// ------------------------------------------------------------------------------------------------
struct KernelKey {
    int ct;
    bool gauss, lane_range;
    int maxt;
};

// Calls fn.template operator()<CT, GAUSS, LANE_RANGE, MAXT>() for the instantiation `k` names.
template <typename Fn>
static hipError_t for_kernel(const KernelKey &k, Fn &&fn) {
#define MVX_CASE(CT_, G_, LR_, MT_) \
    if (k.ct == CT_ && k.gauss == G_ && k.lane_range == LR_ && k.maxt == MT_) return fn.template operator()<CT_, G_, LR_, MT_>();
#define MVX_CASES_CT(CT_, MT_)      \
    MVX_CASE(CT_, true, false, MT_)  \
    MVX_CASE(CT_, false, false, MT_) \
    MVX_CASE(CT_, true, true, MT_)   \
    MVX_CASE(CT_, false, true, MT_)
#define MVX_CASES_MT(MT_) \
    MVX_CASES_CT(1, MT_)  \
    MVX_CASES_CT(4, MT_)  \
    MVX_CASES_CT(8, MT_)  \
    MVX_CASES_CT(16, MT_) \
    MVX_CASES_CT(32, MT_)
    MVX_CASES_MT(512)
    MVX_CASES_MT(1024)
#undef MVX_CASES_MT
#undef MVX_CASES_CT
#undef MVX_CASE
    return hipErrorInvalidValue;
}

template <int CT, bool GAUSS, bool LANE_RANGE>
constexpr bool mx_kernel() {
    return std::is_same<typename SlabOps<CT, GAUSS, LANE_RANGE, false>::type, OpsMx32<GAUSS, LANE_RANGE, false>>::value;
}

template <typename OT>
struct GroupedFn {
    const VoxArgs &a;
    int32_t nb;
    hipStream_t s;
    template <int CT, bool GAUSS, bool LANE_RANGE, int MAXT>
    hipError_t operator()() const {
        if constexpr (CT != 32 || (grid_elem<OT>::NDHWC && MAXT > 512)) { // (channels-last: slabs of at most 8 waves)
            return hipErrorInvalidValue;
        } else {
            VoxParams p = a.p;
            if (nb <= 0) return hipSuccess;
            if ((long long)nb * p.ncc > 65535) return hipErrorInvalidConfiguration;
            const size_t main_lds = voxelize_mx_lds_bytes(p.NW);
            p.dcap = (int32_t)main_lds; // where the slots' {T, k} table sits in LDS
            return launch_kernel<voxelize_kernel<CT, GAUSS, LANE_RANGE, MAXT, true, OT>>(
                dim3(slab_grid_x(p), (unsigned)(nb * p.ncc)), dim3(p.NW * 64), main_lds + 16 * CHAN_GROUP_SLOTS, s, a.rec, a.w, a.slist,
                a.slist_ext, a.Tc, a.kc, static_cast<typename grid_elem<OT>::type *>(a.out), p);
        }
    }
};

template <typename OT>
struct LaunchFn {
    const VoxArgs &a;
    int32_t nb;
    hipStream_t s;
    template <int CT, bool GAUSS, bool LANE_RANGE, int MAXT>
    hipError_t operator()() const {
        constexpr bool NDHWC = grid_elem<OT>::NDHWC;
        if constexpr (NDHWC && MAXT > 512) return hipErrorInvalidValue; // (channels-last: slabs of at most 8 waves, plan_call)
        else {
        const VoxParams &p = a.p;
        if (nb <= 0) return hipSuccess;
        if ((long long)nb * p.ncc > 65535) return hipErrorInvalidConfiguration;
        constexpr bool mx = mx_kernel<CT, GAUSS, LANE_RANGE>();
        size_t lds = mx ? voxelize_mx_lds_bytes(p.NW) : voxelize_lds_bytes(CT, p.NW, CR_F32);
        if (CT < 32 && !LANE_RANGE) lds = std::max(lds, (size_t)65 * cand_stride_words(CT) * 4); // (the vector staging's dump row: stage_round_v)
        const dim3 grid(slab_grid_x(p), (unsigned)(nb * p.ncc));
        typename grid_elem<OT>::type *const out = static_cast<typename grid_elem<OT>::type *>(a.out);
        if constexpr (CT < 16 && !LANE_RANGE) { // narrow chunks: several sub-tiles per wave (voxelize_narrow_kernel)
            // four where the accumulator sets fit (1 or 4 channels) and the row is a multiple of four sub-tiles, else two
            // (channels-last: four sub-tiles for one channel only - four sets of four accumulators and their channel runs need
            // 66 registers, 2 spilled at the 64 of this kernel)
            constexpr int CT4 = NDHWC ? 1 : 4; // widest chunk served with four sub-tiles per wave
            const int nsub = a.narrow_sub > 0 ? a.narrow_sub : ((CT <= CT4 && p.NW % 4 == 0) ? 4 : 2);
            if (nsub > 1 && p.NW % nsub == 0 && (p.vec_store || NDHWC)) { // (the channels-last write-out has both store forms)
                // (lds: 64 rows + the staging's dump row)
                if constexpr (CT <= CT4) {
                    if (nsub == 4)
                        return launch_kernel<voxelize_narrow_kernel<CT, GAUSS, 4, OT>>(grid, dim3(p.NW / 4 * 64), lds, s, a.rec, a.w, a.slist,
                                                                                        a.slist_ext, out, a.p);
                }
                if (nsub == 2)
                    return launch_kernel<voxelize_narrow_kernel<CT, GAUSS, 2, OT>>(grid, dim3(p.NW / 2 * 64), lds, s, a.rec, a.w, a.slist,
                                                                                    a.slist_ext, out, a.p);
            }
        }
        const dim3 block(p.NW * 64);
        if constexpr (!NDHWC) if (!p.vec_store) { // rows that are not whole 16-byte quads: the kernels with the run-wise write-out
            if constexpr (mx)
                return launch_kernel<voxelize_runs_kernel<GAUSS, MAXT, OT>>(grid, block, lds, s, a.rec, a.w, a.slist, a.slist_ext, a.Tc, a.kc, out, a.p);
            else if constexpr (!LANE_RANGE) // narrow chunks: the pair walk with store_runs
                return launch_kernel<voxelize_pair_runs_kernel<CT, GAUSS, MAXT, OT>>(grid, block, lds, s, a.rec, a.w, a.slist, a.slist_ext, a.Tc, a.kc,
                                                                                      out, a.p);
        }
        return launch_kernel<voxelize_kernel<CT, GAUSS, LANE_RANGE, MAXT, false, OT>>(grid, block, lds, s, a.rec, a.w, a.slist, a.slist_ext, a.Tc,
                                                                                       a.kc, out, a.p);
        }
    }
};

hipError_t launch_voxelize(const VoxArgs &a, int32_t nb, int32_t ct, bool gauss, bool lane_range, hipStream_t s) {
    KernelKey k{ct, gauss, lane_range, a.p.NW <= 8 ? 512 : 1024};
    return for_grid_type(a.bf16, a.ndhwc, [&](auto g) { return for_kernel(k, LaunchFn<typename decltype(g)::type>{a, nb, s}); });
}

hipError_t launch_voxelize_grouped(const VoxArgs &a, int32_t nb, bool gauss, bool lane_range, hipStream_t s) {
    KernelKey k{32, gauss, lane_range, a.p.NW <= 8 ? 512 : 1024};
    return for_grid_type(a.bf16, a.ndhwc, [&](auto g) { return for_kernel(k, GroupedFn<typename decltype(g)::type>{a, nb, s}); });
}

} // namespace mvx
