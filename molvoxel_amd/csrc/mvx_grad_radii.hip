// mvx_grad_radii.hip - gradients with respect to the radii (mvx_backward_radii_batch): the gradient walk of mvx_grad.hip with
// the radius partials, and the fixed-order reduction of channel-wise radii over the atoms of a call.
//
//   grad_radii_kernel   grad_kernel's walk (mvx_grad_body.inc with RADII = true): the coordinate and feature gradients are
//                       grad_kernel's bits; besides them one float64 partial sum_v e(v) d2(v) per atom (one radius per atom,
//                       or radii by type), or per chunk of 32 channels a second walk for sum_v G w rho d2 per (atom, channel)
//   grad_radii_reduce   channel-wise radii: block (chunk of RCHUNK atoms, channel) sums the chunk's partials in a fixed order,
//   grad_radii_finish   then one thread per channel sums the chunks in order and applies -(1/r_c) or -(kfac_c / r_c)
//
// Derivative of the density in the radius (DESIGN.md "Backward pass"): float32 k = f32(-0.5 log2(e) / (f32(r) f32(sigma))^2),
// float64 c64 = -0.5 / (r sigma)^2, both proportional to r^-2, so d rho / d r = -(kfac / r) d2 rho with the walk's kfac
// (2 ln2 k or 2 c64). The jump of the membership at the truncation threshold and the culls that depend on r are not
// differentiated (almost everywhere, as for the coordinates).
#include "mvx_grad_device.h"

namespace mvx {

template <typename GT, int MODE, bool GAUSS, bool CHANWISE>
__global__ void __launch_bounds__(256) grad_radii_kernel(GradArgs A, RadiiArgs RA) {
    constexpr bool RADII = true;
    constexpr bool SCORE = false;
    constexpr ScoreArgs SA{}; // (no scores: never read)
#include "mvx_grad_body.inc"
}

constexpr int RCHUNK = 4096; // atoms per block of the first reduction stage

// stage[c * nchunk + chunk] = sum of the chunk's partials of channel c: thread t adds atoms t, t + 256, ... in order, then a
// butterfly per wave and the four waves in a fixed order
__global__ void __launch_bounds__(256) grad_radii_reduce_kernel(const double *__restrict__ part, const int32_t *__restrict__ types,
                                                                int64_t total, int32_t C, int32_t nchunk, double *__restrict__ stage) {
    __shared__ double wsum[4];
    const int64_t lo = (int64_t)blockIdx.x * RCHUNK;
    const int64_t hi = lo + RCHUNK < total ? lo + RCHUNK : total;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        const double *p = types ? part : part + (size_t)c * total;
        double s = 0.0;
        for (int64_t a = lo + threadIdx.x; a < hi; a += 256)
            if (!types || types[a] == c) s += p[a]; // (types mode: atoms of type >= C belong to no channel)
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) stage[(size_t)c * nchunk + blockIdx.x] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
        __syncthreads();
    }
}

template <typename real>
__global__ void __launch_bounds__(256) grad_radii_finish_kernel(const double *__restrict__ stage, int32_t nchunk, int32_t C,
                                                                const real *__restrict__ radii, const real *__restrict__ kc,
                                                                double *__restrict__ grad_radii) {
    for (int c = blockIdx.x * 256 + threadIdx.x; c < C; c += gridDim.x * 256) {
        double s = 0.0;
        for (int j = 0; j < nchunk; ++j) s += stage[(size_t)c * nchunk + j];
        const double r = (double)radii[c]; // (the radius the forward used)
        double g;
        if (kc) { // features: the partials hold sum G w rho d2, the channel's kfac is common to all of them
            const double kfac = std::is_same<real, double>::value ? 2.0 * (double)kc[c] : 2.0 * LN2 * (double)kc[c];
            g = -(kfac / r) * s;
        } else { // types: the partials are sum e d2 of the atoms of this type
            g = -s / r;
        }
        grad_radii[c] = s != 0.0 ? g : 0.0;
    }
}

size_t grad_radii_stage_doubles(int64_t total, int32_t C) {
    return (size_t)((total + RCHUNK - 1) / RCHUNK) * (size_t)C;
}

hipError_t launch_grad_radii_reduce(const double *part, const int32_t *types, const void *radii, const void *kc, bool f64, int64_t total,
                                    int32_t C, double *stage, double *grad_radii, hipStream_t s) {
    const int32_t nchunk = (int32_t)((total + RCHUNK - 1) / RCHUNK);
    hipLaunchKernelGGL(grad_radii_reduce_kernel, dim3((unsigned)nchunk, (unsigned)(C < 65535 ? C : 65535)), dim3(256), 0, s, part,
                       types, total, C, nchunk, stage);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const dim3 fg((unsigned)((C + 255) / 256));
    if (f64)
        hipLaunchKernelGGL(grad_radii_finish_kernel<double>, fg, dim3(256), 0, s, stage, nchunk, C, static_cast<const double *>(radii),
                           static_cast<const double *>(kc), grad_radii);
    else
        hipLaunchKernelGGL(grad_radii_finish_kernel<float>, fg, dim3(256), 0, s, stage, nchunk, C, static_cast<const float *>(radii),
                           static_cast<const float *>(kc), grad_radii);
    return hipGetLastError();
}

template <typename GT>
static hipError_t launch_grad_radii_grid(const GradArgs &a, const RadiiArgs &r, int32_t mode, bool chanwise, hipStream_t s) {
    const unsigned nblk = (unsigned)((a.total + 3) / 4);
    const dim3 grid(a.xcd_span ? 8u * (unsigned)a.xcd_span : nblk), block(256);
    if (mode == MODE_FEATURES) {
        if (chanwise) hipLaunchKernelGGL((grad_radii_kernel<GT, MODE_FEATURES, true, true>), grid, block, 0, s, a, r);
        else hipLaunchKernelGGL((grad_radii_kernel<GT, MODE_FEATURES, true, false>), grid, block, 0, s, a, r);
    } else { // (single mode: type 0 in every record)
        hipLaunchKernelGGL((grad_radii_kernel<GT, MODE_TYPES, true, false>), grid, block, 0, s, a, r);
    }
    return hipGetLastError();
}

hipError_t launch_grad_radii(const GradArgs &a, const RadiiArgs &r, int32_t mode, int32_t grid_kind, bool chanwise, hipStream_t s) {
    if (a.total <= 0) return hipSuccess;
    if (grid_kind == 2) return launch_grad_radii_grid<double>(a, r, mode, chanwise, s);
    if (grid_kind == 1) return launch_grad_radii_grid<__bf16>(a, r, mode, chanwise, s);
    return launch_grad_radii_grid<float>(a, r, mode, chanwise, s);
}

} // namespace mvx
