// mvx_grad_density.hip - gradients with respect to sigma and to a scalar radius (mvx_backward_density_batch): the fixed-order
// reduction of the walk's radius partials over every atom of a call to one double.
//
// The walk is grad_radii_kernel's (mvx_grad_radii.hip, mvx_grad_body.inc with RADII = true), launched with RadiiArgs::part set:
// it leaves P_n = sum_v e_n(v) d2_n(v) per atom (one radius per atom, radii by type, or a scalar radius: the record carries T and
// k whatever the radii type), or S[c, n] = sum_v G w rho d2 per (channel, atom) (channel-wise features). k and c64 are
// proportional to (r sigma)^-2 and the membership does not depend on sigma, so (DESIGN.md "Sigma and scalar-radius gradients")
//   dL/dr_n   = -(1/r_n) P_n                  density_sum_kernel writes it beside its sums (the walk's own expression and bits)
//   dL/dr     = -(1/r) sum_n P_n              scalar radius
//   dL/dsigma = -(1/sigma) sum_n P_n          one radius per atom, radii by type, scalar radius
//   dL/dsigma = -(1/sigma) sum_c kfac_c S_c   channel-wise features, S_c = sum_n S[c, n]: grad_radii_reduce's stage sums
//
//   density_sum_kernel          block = chunk of GRAD_CHUNK atoms: thread t adds atoms t, t + 256, ... in order, then
//                               block_sum4 (a butterfly per wave, the four waves in a fixed order) -> stage[chunk]
//   density_finish_kernel       one thread adds the chunks in order and writes -(1/sigma) s and -(1/r) s
//   density_chan_finish_kernel  channel-wise features: thread t adds kfac_c S_c (S_c: the chunks in order) of channels t,
//                               t + 256, ... in order, a butterfly per wave, the waves in order, then -(1/sigma)
// No atomics: two runs give the same bits, in any processing order of the walk (the partials are per atom).
#include "mvx_grad_device.h"

namespace mvx {

template <typename real>
__global__ void __launch_bounds__(256) density_sum_kernel(const double *__restrict__ part, int64_t total,
                                                          const real *__restrict__ radii, double *__restrict__ grad_radii,
                                                          double *__restrict__ stage) {
    const int64_t lo = (int64_t)blockIdx.x * GRAD_CHUNK;
    const int64_t hi = lo + GRAD_CHUNK < total ? lo + GRAD_CHUNK : total;
    double s = 0.0;
    for (int64_t a = lo + threadIdx.x; a < hi; a += 256) {
        const double S = part[a];
        s += S;
        if (grad_radii) { // one radius per atom: what grad_radii_kernel writes without RadiiArgs::part
            const double r = (double)radii[a];
            grad_radii[a] = S != 0.0 ? -S / r : 0.0;
        }
    }
    block_sum4(s, [&](double sum) { stage[blockIdx.x] = sum; });
}

// r, sigma: the values the forward used (float32 handles: the float widened)
__global__ void __launch_bounds__(64) density_finish_kernel(const double *__restrict__ stage, int32_t nchunk, double r, double sigma,
                                                            double *__restrict__ grad_sigma, double *__restrict__ grad_radius) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int j = 0; j < nchunk; ++j) s += stage[j];
    if (grad_sigma) grad_sigma[0] = s != 0.0 ? -s / sigma : 0.0;
    if (grad_radius) grad_radius[0] = s != 0.0 ? -s / r : 0.0;
}

// stage: grad_radii_reduce_kernel's (C, nchunk) sums of the per-(channel, atom) partials; kc: launch_grad_chan's coefficients
template <typename real>
__global__ void __launch_bounds__(256) density_chan_finish_kernel(const double *__restrict__ stage, int32_t nchunk, int32_t C,
                                                                  const real *__restrict__ kc, double sigma,
                                                                  double *__restrict__ grad_sigma) {
    double acc = 0.0;
    for (int c = threadIdx.x; c < C; c += 256) {
        double s = 0.0;
        for (int j = 0; j < nchunk; ++j) s += stage[(size_t)c * nchunk + j];
        const double kfac = std::is_same<real, double>::value ? 2.0 * (double)kc[c] : 2.0 * LN2 * (double)kc[c];
        acc += kfac * s;
    }
    block_sum4(acc, [&](double s) { grad_sigma[0] = s != 0.0 ? -s / sigma : 0.0; });
}

hipError_t launch_grad_density_sum(const double *part, int64_t total, const void *radii, bool f64, double *grad_radii, double r,
                                   double sigma, double *stage, double *grad_sigma, double *grad_radius, hipStream_t s) {
    const int32_t nchunk = grad_nchunk(total);
    const hipError_t e = for_real(f64, [&](auto t) {
        typedef typename decltype(t)::type real;
        hipLaunchKernelGGL(density_sum_kernel<real>, dim3((unsigned)nchunk), dim3(256), 0, s, part, total,
                           static_cast<const real *>(radii), grad_radii, stage);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(density_finish_kernel, dim3(1), dim3(64), 0, s, stage, nchunk, r, sigma, grad_sigma, grad_radius);
    return hipGetLastError();
}

hipError_t launch_grad_density_chan(const double *stage, int64_t total, int32_t C, const void *kc, bool f64, double sigma,
                                    double *grad_sigma, hipStream_t s) {
    return for_real(f64, [&](auto t) {
        typedef typename decltype(t)::type real;
        hipLaunchKernelGGL(density_chan_finish_kernel<real>, dim3(1), dim3(256), 0, s, stage, grad_nchunk(total), C,
                           static_cast<const real *>(kc), sigma, grad_sigma);
        return hipGetLastError();
    });
}

} // namespace mvx
