// mvx_views_reduce.hip - per-(view, atom) rows of a selection summed back onto the shared atoms (gfx950; mvx_views_reduce):
//   out[n, j] = sum over the views b that hold atom n of rows[slot(b, n), j]
// the backward step of every quantity computed on the compact batch of mvx_select_views.
//
//   view_reduce_kernel  one workgroup (4 waves) per (atom n, chunk of NC columns). Wave w takes the chunks w, w + 4, ... of 64
//                       views in order, lane l of a chunk one view. A view's segment index[off[b] .. off[b + 1]) is ascending:
//                       the slot of n is found by binary search - or is off[b] + n when the segment has N entries (the view
//                       kept the whole cloud: no search). Each lane keeps NC double partials; a fixed butterfly per wave, the
//                       four waves in a fixed order through LDS; one rounding to the rows' type at the store.
//
// No atomics: the order of the additions is a function of (B, N, index, offsets) alone. Nothing an index entry says is used as
// an address: entries are only compared with n, and a slot lies inside [off[b], off[b + 1]) by construction.
#include "mvx_grad_device.h"
#include "mvx_views.h"

namespace mvx {

namespace {
constexpr int RED_WAVES = 4;

// where atom n sits in the ascending segment index[o0 .. o1), or -1
__device__ __forceinline__ int64_t view_slot(const int64_t *__restrict__ index, int64_t o0, int64_t o1, int64_t n, int64_t N) {
    if (o1 - o0 == N) return o0 + n; // the whole cloud, in atom order
    int64_t lo = o0, hi = o1;        // lower bound of n
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (index[mid] < n) lo = mid + 1;
        else hi = mid;
    }
    return (lo < o1 && index[lo] == n) ? lo : -1;
}
} // namespace

template <typename T, int NC>
__global__ void __launch_bounds__(64 * RED_WAVES) view_reduce_kernel(const int64_t *__restrict__ index,
                                                                     const int64_t *__restrict__ offsets, int32_t B, int64_t N,
                                                                     const T *__restrict__ rows, int32_t width, T *__restrict__ out) {
    __shared__ double part[RED_WAVES][NC];
    const int64_t n = blockIdx.x;
    const int c0 = (int)blockIdx.y * NC;
    const int nc = width - c0 < NC ? width - c0 : NC; // columns of this chunk (> 0: the launch's gridDim.y)
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    double acc[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) acc[j] = 0.0;
    for (int64_t b = 64 * wave + lane; b < B; b += 64 * RED_WAVES) {
        const int64_t slot = view_slot(index, offsets[b], offsets[b + 1], n, N);
        if (slot < 0) continue;
        const T *row = rows + (size_t)slot * (size_t)width + c0;
        if (nc == NC) {
#pragma unroll
            for (int j = 0; j < NC; ++j) acc[j] += (double)row[j];
        } else {
#pragma unroll
            for (int j = 0; j < NC; ++j)
                if (j < nc) acc[j] += (double)row[j];
        }
    }
    if constexpr (NC == 32) {
        const double v = wave_sum32_regs(acc, lane); // lane l: the wave's sum of column l / 2
        if ((lane & 1) == 0) part[wave][lane >> 1] = v;
    } else {
#pragma unroll
        for (int j = 0; j < NC; ++j) {
            const double v = wave_sum(acc[j]);
            if (lane == 0) part[wave][j] = v;
        }
    }
    __syncthreads();
    const int j = (int)threadIdx.x;
    if (j < nc) out[(size_t)n * (size_t)width + c0 + j] = (T)sum4(part[0][j], part[1][j], part[2][j], part[3][j]);
}

template <typename T>
static hipError_t launch_reduce_t(const int64_t *index, const int64_t *offsets, int32_t B, int64_t N, const void *rows,
                                  int32_t width, void *out, hipStream_t s) {
    const T *r = static_cast<const T *>(rows);
    T *o = static_cast<T *>(out);
    const dim3 block(64 * RED_WAVES);
    if (width == 1)
        hipLaunchKernelGGL((view_reduce_kernel<T, 1>), dim3((unsigned)N, 1), block, 0, s, index, offsets, B, N, r, width, o);
    else if (width <= 4)
        hipLaunchKernelGGL((view_reduce_kernel<T, 4>), dim3((unsigned)N, 1), block, 0, s, index, offsets, B, N, r, width, o);
    else
        hipLaunchKernelGGL((view_reduce_kernel<T, 32>), dim3((unsigned)N, (unsigned)((width + 31) / 32)), block, 0, s, index,
                           offsets, B, N, r, width, o);
    return hipGetLastError();
}

hipError_t launch_view_reduce(const int64_t *index, const int64_t *offsets, int32_t B, int64_t N, const void *rows, int32_t width,
                              bool rows_f64, void *out, hipStream_t s) {
    if (B <= 0 || N <= 0 || width <= 0) return hipSuccess;
    return for_real(rows_f64, [&](auto t) { return launch_reduce_t<typename decltype(t)::type>(index, offsets, B, N, rows, width, out, s); });
}

} // namespace mvx
