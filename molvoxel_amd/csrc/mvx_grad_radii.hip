// mvx_grad_radii.hip - gradients with respect to the radii (mvx_backward_radii_batch): the gradient walk of mvx_grad.hip with
// the radius partials, and the fixed-order reduction of channel-wise radii over the atoms of a call.
//
//   grad_radii_kernel   grad_kernel's walk (mvx_grad_body.inc with RADII = true): the coordinate and feature gradients are
//                       grad_kernel's bits; besides them one float64 partial sum_v e(v) d2(v) per atom (one radius per atom,
//                       or radii by type), or per chunk of 32 channels a second walk for sum_v G w rho d2 per (atom, channel)
//   grad_radii_reduce   channel-wise radii: block (chunk of GRAD_CHUNK atoms, channel) sums the chunk's partials in a fixed order,
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
    constexpr bool MOMENTS = false, TARGET = false;
    constexpr MomentsArgs MA{}; // (the upstream is read, not formed: never read)
#include "mvx_grad_body.inc"
}

// stage[c * nchunk + chunk] = sum of the chunk's partials of channel c: thread t adds atoms t, t + 256, ... in order, then
// block_sum4's steps spelled out: through the helper this kernel compiles to another body, one instruction less in the
// hand-over's address; switch when a changed body may be measured
__global__ void __launch_bounds__(256) grad_radii_reduce_kernel(const double *__restrict__ part, const int32_t *__restrict__ types,
                                                                int64_t total, int32_t C, int32_t nchunk, double *__restrict__ stage) {
    __shared__ double wsum[4];
    const int64_t lo = (int64_t)blockIdx.x * GRAD_CHUNK;
    const int64_t hi = lo + GRAD_CHUNK < total ? lo + GRAD_CHUNK : total;
    for (int c = blockIdx.y; c < C; c += gridDim.y) {
        const double *p = types ? part : part + (size_t)c * total;
        double s = 0.0;
        for (int64_t a = lo + threadIdx.x; a < hi; a += 256)
            if (!types || types[a] == c) s += p[a]; // (types mode: atoms of type >= C belong to no channel)
        s = wave_sum(s);
        if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) stage[(size_t)c * nchunk + blockIdx.x] = sum4(wsum[0], wsum[1], wsum[2], wsum[3]);
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

hipError_t launch_grad_radii_reduce(const double *part, const int32_t *types, const void *radii, const void *kc, bool f64, int64_t total,
                                    int32_t C, double *stage, double *grad_radii, hipStream_t s) {
    const int32_t nchunk = grad_nchunk(total);
    hipLaunchKernelGGL(grad_radii_reduce_kernel, dim3((unsigned)nchunk, (unsigned)(C < 65535 ? C : 65535)), dim3(256), 0, s, part,
                       types, total, C, nchunk, stage);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return for_real(f64, [&](auto t) {
        typedef typename decltype(t)::type real;
        hipLaunchKernelGGL(grad_radii_finish_kernel<real>, dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, stage, nchunk, C,
                           static_cast<const real *>(radii), static_cast<const real *>(kc), grad_radii);
        return hipGetLastError();
    });
}

hipError_t launch_grad_radii(const GradArgs &a, const RadiiArgs &r, const WalkKey &key, hipStream_t s) {
    return for_walk(key, [&](auto gt, auto mode, auto gauss, auto chanwise) {
        if constexpr (gauss) return launch_walk(grad_radii_kernel<typename decltype(gt)::type, mode, true, chanwise>, a, s, r);
        else return hipErrorInvalidValue; // (no binary instantiation: its radius gradients are zeros)
    });
}

} // namespace mvx
