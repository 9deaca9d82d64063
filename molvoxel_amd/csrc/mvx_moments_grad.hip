// mvx_moments_grad.hip - gradients of the moments (mvx_moments_backward_batch): dL/dcoords and dL/dfeatures for a loss that reads
// the grids only through m[b,c,0] = sum g, m[b,c,1] = sum g^2 and m[b,c,2] = sum g t.
//
// With G0, G1, G2 = dL/dm[b, c, 0..2] the upstream of the backward walk is dL/dgrid[b,c,v] = G0 + 2 G1 g[b,c,v] + G2 t[c,v]: the
// existing walk with an upstream that is never stored. The host layer (mvx_capi.hip) writes the float32 grids g of one molecule
// chunk into scratch and launches this walk over the chunk's atoms.
//
//   moments_coef_kernel   dL/dm (n, K) doubles -> the walk's coefficients (n, 3) floats: a0 = (float)G0, a1 = (float)(2.0 * G1),
//                         a2 = (float)G2 (0 without a target)
//   moments_grad_kernel   grad_kernel's walk (mvx_grad_body.inc with MOMENTS = true): where grad_kernel loads G[c,v] this one
//                         loads g[c,v] (and t[c,v]) and forms u = fmaf(a1, g, fmaf(a2, t, a0)) in float32 - without a target
//                         fmaf(a1, g, a0); everything behind the upstream is the body's, so the gradients are grad_kernel's
//                         bits for G = u. The coefficients are wave-uniform (one molecule per wave, the channels of a chunk).
//                         Float32 grids, no channel-wise radii for features: what mvx_moments_batch serves.
#include "mvx_grad_device.h"

namespace mvx {

template <int MODE, bool GAUSS, bool TARGET>
__global__ void __launch_bounds__(256) moments_grad_kernel(GradArgs A, MomentsArgs MA) {
    typedef float GT; // the scratch grids: float32 NCDHW whatever the handle's grid type and layout
    constexpr bool CHANWISE = false;
    constexpr bool RADII = false;
    constexpr RadiiArgs RA{}; // (no radius partials: never read)
    constexpr bool SCORE = false;
    constexpr ScoreArgs SA{}; // (no scores: never read)
    constexpr bool MOMENTS = true;
#include "mvx_grad_body.inc"
}

__global__ void __launch_bounds__(256) moments_coef_kernel(const double *__restrict__ gm, int64_t n, int K, float *__restrict__ coef) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    coef[3 * i] = (float)gm[i * K];
    coef[3 * i + 1] = (float)(2.0 * gm[i * K + 1]);
    coef[3 * i + 2] = K == 3 ? (float)gm[i * K + 2] : 0.0f;
}

hipError_t launch_moments_coef(const double *grad_moments, int64_t n, int32_t K, float *coef, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(moments_coef_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, grad_moments, n, K, coef);
    return hipGetLastError();
}

hipError_t launch_moments_grad(const GradArgs &a, const MomentsArgs &ma, const WalkKey &key, hipStream_t s) {
    return for_moments_walk(key, ma.target != nullptr, [&](auto mode, auto gauss, auto target) {
        return launch_walk(moments_grad_kernel<mode, gauss, target>, a, s, ma); // (the tags convert as constants)
    });
}

} // namespace mvx
