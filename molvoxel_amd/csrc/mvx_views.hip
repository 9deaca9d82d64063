// mvx_views.hip - many views of one shared point cloud (gfx950): per view, the atoms that pass the forward's box cull, in atom
// order, and the gather of their rows into a compact batch for the unchanged pipeline (mvx_select_views / mvx_forward_views).
//
//   view_rmax_kernel    channel-wise radii for features: max(radii), the radius the culls use
//   view_count_kernel   one workgroup per (view, tile of 1 024 atoms): how many atoms of the tile the view keeps
//   view_scan_kernel    exclusive scan of the counts in (view, tile) order: every tile's base and offsets[B + 1]
//   view_fill_kernel    the same test again; the kept atoms' indices to their places (ballot / prefix, no atomics)
//   view_gather_kernel  rows of coordinates, channels and radii by index, widest aligned accesses
//
// The test is the pre-pass's own: apply_xform of mvx_device.h and the box cull of mvx_box_cull.inc, so a view keeps exactly the atoms whose records
// prep_kernel would not drop at the box cull. Order inside a view is atom order, because the voxelize kernels sum a voxel's
// candidates in list order: the compact batch then gives the bits of the repeated cloud.
#include "mvx_views.h"
#include "mvx_device.h"

#include <algorithm>

namespace mvx {

namespace {
constexpr int VIEW_THREADS = 256;
constexpr int VIEW_WAVES = VIEW_THREADS / 64;
constexpr int VIEW_CH = VIEW_TILE / VIEW_THREADS; // chunks of 64 consecutive atoms per wave
static_assert(VIEW_CH * VIEW_THREADS == VIEW_TILE, "a tile is whole chunks");

// prep_atom's box cull for atom a at p (mvx_box_cull.inc: the same text, so the same decisions)
__device__ __forceinline__ bool view_keeps(const PrepArgs &A, int64_t a, const double (&p)[3], float rmax32, double rmax64) {
    const bool f64 = (A.precision == 64);
    const Geom g = A.g;
    const double ub = g.half, lb = -1 * g.half;
    float r32;
    double rc, rwin, r64 = 0.0;
#include "mvx_box_cull.inc"
    (void)r32, (void)rwin, (void)r64, (void)type;
    return keep;
}

// Wave w of the workgroup owns atoms [256 w, 256 (w + 1)) of the tile as VIEW_CH chunks of 64 consecutive atoms (one per lane:
// consecutive lanes read consecutive coordinate rows). m[u]: the atom of chunk u passes; n0: the lane's atom of chunk 0.
__device__ __forceinline__ void view_test(const ViewArgs &V, int view, int tile, int wave, int lane, bool (&m)[VIEW_CH], int64_t &n0) {
    const PrepArgs &A = V.pa;
    const mvx_xform xf = A.xforms[view]; // (workgroup-uniform: scalar loads)
    float rmax32 = 0.0f;
    double rmax64 = 0.0;
    if (A.radii_src == RAD_CHANNEL_FEATURES) {
        if (A.precision == 64) rmax64 = static_cast<const double *>(A.chan_aux)[0];
        else rmax32 = static_cast<const float *>(A.chan_aux)[0];
    }
    n0 = (int64_t)tile * VIEW_TILE + wave * (VIEW_CH * 64) + lane;
    double p[VIEW_CH][3];
#pragma unroll
    for (int u = 0; u < VIEW_CH; ++u) { // every load first (clamped: the mask below drops what lies beyond the cloud)
        const int64_t n = n0 + 64 * u, nl = n < A.total ? n : A.total - 1;
        p[u][0] = A.coords[3 * nl];
        p[u][1] = A.coords[3 * nl + 1];
        p[u][2] = A.coords[3 * nl + 2];
    }
#pragma unroll
    for (int u = 0; u < VIEW_CH; ++u) {
        const int64_t n = n0 + 64 * u, nl = n < A.total ? n : A.total - 1;
        if (xf.flags) apply_xform(xf, p[u][0], p[u][1], p[u][2]);
        m[u] = view_keeps(A, nl, p[u], rmax32, rmax64) && n < A.total;
    }
}

__device__ __forceinline__ void view_block(const ViewArgs &V, int &view, int &tile) {
    view = V.views_in_x ? (int)blockIdx.x : (int)blockIdx.y;
    tile = V.views_in_x ? (int)blockIdx.y : (int)blockIdx.x;
}
} // namespace

__global__ void view_rmax_kernel(const void *radii, int C, int precision, void *rmax) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (precision == 64) {
        const double *r = static_cast<const double *>(radii);
        double m = r[0];
        for (int c = 1; c < C; ++c) m = r[c] > m ? r[c] : m;
        static_cast<double *>(rmax)[0] = m;
    } else {
        const float *r = static_cast<const float *>(radii);
        float m = r[0];
        for (int c = 1; c < C; ++c) m = r[c] > m ? r[c] : m;
        static_cast<float *>(rmax)[0] = m;
    }
}

__global__ void __launch_bounds__(VIEW_THREADS) view_count_kernel(ViewArgs V, int32_t *__restrict__ counts) {
    __shared__ int wcnt[VIEW_WAVES];
    int view, tile;
    view_block(V, view, tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool m[VIEW_CH];
    int64_t n0;
    view_test(V, view, tile, wave, lane, m, n0);
    int own = 0;
#pragma unroll
    for (int u = 0; u < VIEW_CH; ++u) own += __popcll(__ballot(m[u]));
    if (lane == 0) wcnt[wave] = own;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < VIEW_WAVES; ++w) sum += wcnt[w];
        counts[(size_t)view * V.ntiles + tile] = sum;
    }
}

// One workgroup: thread t sums a contiguous piece of the counts, the 1 024 piece sums are scanned through LDS, and the thread
// walks its piece again writing the bases. M = B * ntiles counts (a few thousand for a protein and a few thousand views).
constexpr int SCAN_THREADS = 1024;
__global__ void __launch_bounds__(SCAN_THREADS) view_scan_kernel(const int32_t *__restrict__ counts, int B, int ntiles,
                                                                int64_t *__restrict__ tile_base, int64_t *__restrict__ offsets) {
    __shared__ long long part[SCAN_THREADS];
    const int64_t M = (int64_t)B * ntiles;
    const int64_t per = (M + SCAN_THREADS - 1) / SCAN_THREADS;
    const int64_t i0 = (int64_t)threadIdx.x * per, i1 = (i0 + per < M) ? i0 + per : M;
    long long sum = 0;
    for (int64_t i = i0; i < i1; ++i) sum += counts[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    // Hillis-Steele inclusive scan of the piece sums
    for (int d = 1; d < SCAN_THREADS; d <<= 1) {
        const long long add = ((int)threadIdx.x >= d) ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    long long base = part[threadIdx.x] - sum; // exclusive
    if (i0 < i1) {
        int64_t v = i0 / ntiles;
        int t = (int)(i0 - v * ntiles);
        for (int64_t i = i0; i < i1; ++i) {
            tile_base[i] = base;
            if (t == 0) offsets[v] = base;
            base += counts[i];
            if (++t == ntiles) {
                t = 0;
                ++v;
            }
        }
    }
    if (threadIdx.x == SCAN_THREADS - 1) offsets[B] = part[SCAN_THREADS - 1];
}

__global__ void __launch_bounds__(VIEW_THREADS) view_fill_kernel(ViewArgs V, const int64_t *__restrict__ tile_base,
                                                                 int64_t *__restrict__ index) {
    __shared__ int wcnt[VIEW_WAVES];
    int view, tile;
    view_block(V, view, tile);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    bool m[VIEW_CH];
    int64_t n0;
    view_test(V, view, tile, wave, lane, m, n0);
    unsigned long long mk[VIEW_CH];
    int own = 0;
#pragma unroll
    for (int u = 0; u < VIEW_CH; ++u) {
        mk[u] = __ballot(m[u]);
        own += __popcll(mk[u]);
    }
    if (lane == 0) wcnt[wave] = own;
    __syncthreads();
    int64_t at = tile_base[(size_t)view * V.ntiles + tile];
#pragma unroll
    for (int w = 0; w < VIEW_WAVES; ++w) at += (w < wave) ? wcnt[w] : 0; // the waves before this one, in wave order
#pragma unroll
    for (int u = 0; u < VIEW_CH; ++u) {
        const int before = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk[u] >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk[u], 0u));
        if (m[u]) index[at + before] = n0 + 64 * u;
        at += __popcll(mk[u]);
    }
}

// Thread -> (row, piece of W bytes): a row is one contiguous run of row_bytes / W pieces in both arrays.
template <typename T>
__device__ __forceinline__ void gather_piece(const GatherArgs &G, int arr, int64_t u) {
    const int ppr = G.row_bytes[arr] / (int)sizeof(T); // pieces per row
    const int64_t row = u / ppr;
    if (row >= G.total) return;
    const int k = (int)(u - row * ppr);
    const T *src = reinterpret_cast<const T *>(G.src[arr] + (size_t)G.index[row] * G.row_bytes[arr]);
    T *dst = reinterpret_cast<T *>(G.dst[arr] + (size_t)row * G.row_bytes[arr]);
    dst[k] = src[k];
}

__global__ void __launch_bounds__(256) view_gather_kernel(GatherArgs G) {
    const int arr = blockIdx.y; // (< G.narr: the launch's gridDim.y)
    const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int W = G.width[arr];
    if (W == 16) gather_piece<uint4>(G, arr, u);
    else if (W == 8) gather_piece<uint2>(G, arr, u);
    else gather_piece<uint32_t>(G, arr, u);
}

hipError_t launch_view_rmax(const void *radii, int32_t C, int32_t precision, void *rmax, hipStream_t s) {
    hipLaunchKernelGGL(view_rmax_kernel, dim3(1), dim3(64), 0, s, radii, C, precision, rmax);
    return hipGetLastError();
}

static dim3 view_grid(const ViewArgs &a) {
    return a.views_in_x ? dim3((unsigned)a.pa.B, (unsigned)a.ntiles) : dim3((unsigned)a.ntiles, (unsigned)a.pa.B);
}

hipError_t launch_view_count(const ViewArgs &a, int32_t *counts, hipStream_t s) {
    if (a.pa.B <= 0 || a.ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(view_count_kernel, view_grid(a), dim3(VIEW_THREADS), 0, s, a, counts);
    return hipGetLastError();
}

hipError_t launch_view_scan(const int32_t *counts, int32_t B, int32_t ntiles, int64_t *tile_base, int64_t *offsets, hipStream_t s) {
    if (B <= 0 || ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(view_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, counts, B, ntiles, tile_base, offsets);
    return hipGetLastError();
}

hipError_t launch_view_fill(const ViewArgs &a, const int64_t *tile_base, int64_t *index, hipStream_t s) {
    if (a.pa.B <= 0 || a.ntiles <= 0) return hipSuccess;
    hipLaunchKernelGGL(view_fill_kernel, view_grid(a), dim3(VIEW_THREADS), 0, s, a, tile_base, index);
    return hipGetLastError();
}

hipError_t launch_view_gather(const GatherArgs &g, hipStream_t s) {
    if (g.total <= 0 || g.narr <= 0) return hipSuccess;
    int64_t units = 0;
    for (int i = 0; i < g.narr; ++i) units = std::max<int64_t>(units, g.total * (g.row_bytes[i] / g.width[i]));
    hipLaunchKernelGGL(view_gather_kernel, dim3((unsigned)((units + 255) / 256), (unsigned)g.narr), dim3(256), 0, s, g);
    return hipGetLastError();
}

} // namespace mvx
