// mvx_pair.hip - voxelize_pair_kernel: a whole per-molecule forward() call in ONE launch, two slabs per workgroup (gfx950).
//
// The reference's unit of work is one molecule per forward() call (test/test_time_numpy.py:11-15; Voxelizer.forward_features /
// forward_types / forward_single, numpy/voxelizer.py:97-169, 240-315, 370-436). Such a call is a chain of latencies, not
// work: launch -> coordinates -> which atoms reach this slab -> their records and weights -> walk -> stores, in front of
// ~5.5 us of HBM drain for a cfg-2 grid. This kernel replaced the round-2 voxelize_direct_kernel (one slab per
// workgroup, every wave scanning for itself) on that path: cfg-2 call 20.5 -> 14.9 us, the reference's timing loop 17.9 -> 12.9
// (profiles/r04_single_calls.txt). What the old kernel's phase timeline showed (tools/direct_timeline.py, cfg-2: scan 12.0 of
// a workgroup's 25.6 kcycles, 21 of 27 on the reference's own timing loop) and the rules this one is built on:
//   * Sixteen waves run the front side by side on one compute unit, so every instruction of it costs ~16 cycles of the call:
//     the front is bound by its INSTRUCTION COUNT per compute unit, not by memory latency (stashing data to save a second
//     trip to memory, prefetching rows during the scan: both measured slower until the instruction count came down).
//   * A workgroup owns TWO slabs side by side along x (4 x 4 x 8 NW voxels, 2 NW waves = up to 1024 threads, one workgroup
//     per compute unit): one scan, one staged set of rows for both - half the scan work of a workgroup per slab.
//   * Scan: every load of a wave's share is issued before anything else (16-byte loads, 32-bit offsets from one scalar
//     base, 3 per 128 atoms), the box constants are computed under them, the test is ~30 instructions per 64 atoms. What
//     the scan held about a survivor (float64 position, atom-wise radius, type) stays in LDS: no second trip to memory.
//   * Stage: the survivors of all waves are gathered into rows in candidate (= atom) order - prefix over the waves by DPP -
//     and the FIRST one to four waves prepare them, one lane per row, all 64 lanes busy: the exact float64 preparation is
//     issued once or twice per workgroup instead of sixteen times with ~4 active lanes. The other waves set up their walk
//     (voxel centres, accumulators, filter constants) meanwhile.
//   * Walk and write-out are the batched kernels' (OpsMx32 on the matrix cores for 32-channel chunks, OpsPair below that),
//     so the sums are the same float32 chains in atom order: bit-identical to every other route.
//   * No scratch: the rare rounds / segments that run with the accumulators alive use lighter variants of scan and stage
//     (one block in flight, no per-lane row prefetch). A per-wave private segment of a few hundred bytes throttles the waves
//     a launch may have in flight (an in-kernel loop over channel chunks that needed 452 B: cfg-2 kernel 13.8 -> 18.0 us).
// Exactness is unchanged: the float32 scan only decides which atoms are LOOKED AT (a superset, error-bounded); box cull,
// block culls, threshold and coefficient are decided in float64 with the reference's comparisons (stage), membership per
// voxel by d2 <= T (walk).
// LDS map (dynamic): u16 list[2 NW][segw] | PairStash stash[2 NW][48] | int wcnt[32] | float rtab[256] |
//                    union { float64 strips 2 NW x 3 KB ; rows 256 x SW words ; 2 tiles }.
#include "mvx_device.h"
#include "mvx_ops32.h"

#include <algorithm>

namespace mvx {

constexpr int PAIR_BLOCK = 128;                           // atoms per transposition block (3 x 1 KB of coordinates)
constexpr int PAIR_MAX_BLOCKS = 4;                        // blocks a wave fetches at once (all loads in flight: 48 registers)
constexpr int PAIR_SEGW_MIN = PAIR_BLOCK * PAIR_MAX_BLOCKS; // atoms per wave and segment: 512 (molecules of up to 8 192 atoms on
constexpr int PAIR_SEGW_MAX = 2048;                         // 16 waves) ... 2 048 (32 768 atoms), chosen at launch (VoxParams::dcap)
constexpr int PAIR_ROWS = 256;                            // candidate rows staged per round (both slabs share them), 64 per staging wave:
                                                          // a pair of slabs at cfg-2's density holds ~62 candidates at radius 1 A, ~140 at 2 A;
                                                          // more than a round's rows means further, slower rounds (with 128 rows per round a
                                                          // molecule of 12 000 atoms took 27.9 us, with 256 23.0)
constexpr int PAIR_STASH = 48;                            // survivors per wave and segment whose float64 position, radius and type stay in LDS
constexpr int PAIR_RTAB = 256;                            // per-type radii kept in LDS (forward_types with channel-wise radii)
struct __attribute__((aligned(16))) PairStash {           // what the scan already held about a survivor: no second trip to memory
    double x, y, z;
    float r;      // atom-wise radius
    int32_t type; // forward_types channel
};
static_assert(sizeof(PairStash) == 32, "two 16-byte LDS writes per survivor");

// (the write-outs carry the run-wise path - store_runs - beside the 16-byte one: grids whose rows are not whole quads, odd
// dimensions and unaligned slices of a batch grid, take this kernel too)
// LR: blockdims whose reference blocks cut through sub-tiles (4, 5, 12, ...) - every lane checks its voxel's index against the
// atom's admitted ranges (prep_atom's block_interval), one voxel per lane and candidate (OpsF32 / OpsMx32 with per-lane ranges)
template <int CT, bool GAUSS, bool LR, typename OT = float>
struct PairOps {
    typedef OpsPair<CT, GAUSS, true, OT> type;
};
template <bool GAUSS, typename OT>
struct PairOps<32, GAUSS, false, OT> {
    typedef OpsMx32<GAUSS, false, false, true, OT> type;
};
template <int CT, bool GAUSS, typename OT>
struct PairOps<CT, GAUSS, true, OT> {
    typedef OpsF32<CT, GAUSS, true, OT> type;
};
template <bool GAUSS, typename OT>
struct PairOps<32, GAUSS, true, OT> {
    typedef OpsMx32<GAUSS, true, false, true, OT> type;
};

__host__ __device__ inline int pair_tile_words(int ct, int NW) { // one slab's write-out tile (Ops::write)
    const int cr = ct == 32 ? MX_CR : (ct < CR_F32 ? ct : CR_F32);
    return cr * RPC * row_stride_floats(NW);
}
// atoms per wave and segment for molecules of up to max_atoms atoms: one segment whenever the list can hold it (a second
// segment repeats scan, barriers, stage and walk with the accumulators alive: 12 000 atoms took 37.8 us in two segments of
// 8 192 against 30.6 us binned)
static int32_t pair_segw(int64_t max_atoms, int32_t NW) {
    int64_t per_wave = (max_atoms + 2 * NW - 1) / (2 * NW);
    per_wave = (per_wave + PAIR_BLOCK - 1) / PAIR_BLOCK * PAIR_BLOCK;
    return (int32_t)std::min<int64_t>(std::max<int64_t>(per_wave, PAIR_SEGW_MIN), PAIR_SEGW_MAX);
}
__host__ __device__ inline int pair_rows(int NW) { return PAIR_ROWS < 128 * NW ? PAIR_ROWS : 128 * NW; } // (64 per wave of the workgroup at most)
static size_t pair_lds_bytes(int32_t ct, int32_t NW, int32_t segw) {
    const size_t strips = (size_t)2 * NW * PAIR_BLOCK * 24;
    const size_t rows = (size_t)pair_rows(NW) * cand_stride_words(ct) * 4;
    const size_t tiles = (size_t)2 * pair_tile_words(ct, NW) * 4;
    const size_t un = std::max(strips, std::max(rows, tiles));
    return (size_t)2 * NW * ((size_t)segw * 2 + PAIR_STASH * sizeof(PairStash)) + 128 + PAIR_RTAB * 4 + un;
}

typedef unsigned u4a8 __attribute__((ext_vector_type(4), aligned(8)));
typedef float f4a16 __attribute__((ext_vector_type(4)));

// inclusive prefix over the 16 lanes of a row (row_shr: lanes shifted in from outside the row read 0)
__device__ __forceinline__ int row_prefix16(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    return v;
}

// OT: the grid type (float, __bf16, or a channels-last tag Ndhwc<...>): the same body with that type's write-out (Ops<..., OT>)
template <int CT, bool GAUSS, bool XF, bool LR = false, typename OT = float>
__global__ void __launch_bounds__(1024)
    voxelize_pair_kernel(const DirectArgs A, typename grid_elem<OT>::type *__restrict__ out, const VoxParams P) {
    typedef typename PairOps<CT, GAUSS, LR, OT>::type Ops;
#include "mvx_pair_body.inc"
}

// ------------------------------------------------------------------------------------------------
// dispatch
// ------------------------------------------------------------------------------------------------
template <int CT, bool GAUSS, bool XF, bool LR, typename OT>
static hipError_t launch_pair_t(const DirectArgs &d, const VoxParams &p, int64_t max_atoms, void *out, hipStream_t s) {
    VoxParams q = p;
    q.dcap = pair_segw(max_atoms, p.NW);
    return launch_kernel<voxelize_pair_kernel<CT, GAUSS, XF, LR, OT>>(dim3((unsigned)(p.nsy * ((p.nsx + 1) / 2)), (unsigned)(p.B * p.ncc)),
                                                                      dim3(p.NW * 128), pair_lds_bytes(CT, p.NW, q.dcap), s, d,
                                                                      static_cast<typename grid_elem<OT>::type *>(out), q);
}

// The whole call in one launch: float32 grids with whole rows per slab (NW <= 8); rows of whole 16-byte quads or not (run-wise
// write-out), an even number of x-slabs or not (the last pair's second slab then lies outside the grid). lane_range: sub-tiles
// cut by reference blocks (blockdim 4, 5, 12, ...) - built with the transform-capable instantiation only (an identity
// transform costs that rare case little and keeps the number of kernels down).
template <typename OT>
static hipError_t launch_direct_t(const DirectArgs &d, const VoxParams &p, int64_t max_atoms, void *out, int32_t ct, bool gauss,
                                  bool lane_range, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (p.NW > 8 || p.nzc != 1 || (long long)p.B * p.ncc > 65535) return hipErrorInvalidConfiguration;
    if (max_atoms > (int64_t)100000000) return hipErrorInvalidConfiguration; // (24-byte rows addressed with 32-bit offsets; plan_call stops at 131 072 atoms)
    const bool xf = d.pa.xforms != nullptr || d.pa.xf_one.flags != 0;
#define MVX_CASE(CT_)                                                                                                                   \
    if (ct == CT_) {                                                                                                                    \
        if (lane_range)                                                                                                                 \
            return gauss ? launch_pair_t<CT_, true, true, true, OT>(d, p, max_atoms, out, s) : launch_pair_t<CT_, false, true, true, OT>(d, p, max_atoms, out, s); \
        if (gauss)                                                                                                                      \
            return xf ? launch_pair_t<CT_, true, true, false, OT>(d, p, max_atoms, out, s) : launch_pair_t<CT_, true, false, false, OT>(d, p, max_atoms, out, s); \
        return xf ? launch_pair_t<CT_, false, true, false, OT>(d, p, max_atoms, out, s) : launch_pair_t<CT_, false, false, false, OT>(d, p, max_atoms, out, s);   \
    }
    MVX_CASE(1)
    MVX_CASE(4)
    MVX_CASE(8)
    MVX_CASE(16)
    MVX_CASE(32)
#undef MVX_CASE
    return hipErrorInvalidValue;
}
hipError_t launch_voxelize_direct(const DirectArgs &d, const VoxParams &p, int64_t max_atoms, void *out, bool bf16, bool ndhwc, int32_t ct,
                                  bool gauss, bool lane_range, hipStream_t s) {
    return for_grid_type(bf16, ndhwc, [&](auto g) { return launch_direct_t<typename decltype(g)::type>(d, p, max_atoms, out, ct, gauss, lane_range, s); });
}

void scalar_radius_constants(double radius_scalar, float sigma32, bool gauss, double *T, float *k) {
    const float r32 = (float)radius_scalar;
    *T = d2_threshold(r32);
    *k = gauss && *T >= 0.0 ? gauss_coeff(r32, sigma32) : 0.0f;
}

} // namespace mvx
