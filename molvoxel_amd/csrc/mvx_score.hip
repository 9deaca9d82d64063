// mvx_score.hip - scores of poses against a constant field grid (mvx_score_batch): S_b = <F, grid_b> without the grids.
//
// The score is linear in the grid, so it splits by atom: S_b = sum_{n in b} s_n with s_n = sum_v sum_c F[c,v] w[n,c] rho_{n,c}(v),
// and sum_c F w rho is what the gradient walk forms per voxel anyway (its `e` without kfac). One walk of the atoms' boxes
// over the one field therefore gives the per-atom scores, dS/dcoords and dS/dfeatures; no grid is written or read.
//
//   score_kernel         grad_kernel's walk (mvx_grad_body.inc with SCORE = true): one wave per atom record, the coordinate and
//                        feature gradients are grad_kernel's bits for G = F laid out per molecule; besides them one float64
//                        lane partial of the float32 products F w rho, one fixed butterfly, lane 0 writes s_n. Binary density
//                        walks the box in types / single mode too: it scores although its coordinate gradients are zero.
//   score_reduce_kernel  one workgroup (4 waves) per molecule, in the shape of pose_grad_kernel: wave w takes the chunks w, w + 4,
//                        ... of 64 atoms in order, a fixed butterfly per wave, the four waves in a fixed order through LDS, lane 0
//                        writes scores[b]. No atomics: a molecule's score depends on nothing but its own atoms' s_n in their
//                        own order - the same bits in any batch and in every run.
#include "mvx_grad_device.h"

namespace mvx {

template <typename GT, int MODE, bool GAUSS, bool CHANWISE>
__global__ void __launch_bounds__(256) score_kernel(GradArgs A, ScoreArgs SA) {
    constexpr bool RADII = false;
    constexpr RadiiArgs RA{}; // (no radius partials: never read)
    constexpr bool SCORE = true;
    constexpr bool MOMENTS = false, TARGET = false;
    constexpr MomentsArgs MA{}; // (the upstream is the field, read as it is: never read)
#include "mvx_grad_body.inc"
}

constexpr int SCORE_WAVES = 4;

__global__ void __launch_bounds__(64 * SCORE_WAVES) score_reduce_kernel(const double *__restrict__ atom_scores,
                                                                        const int64_t *__restrict__ offsets,
                                                                        double *__restrict__ scores) {
    __shared__ double part[SCORE_WAVES];
    const int b = (int)blockIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t a0 = offsets[b], a1 = offsets[b + 1];
    double s = 0.0;
    for (int64_t a = a0 + 64 * wave + lane; a < a1; a += 64 * SCORE_WAVES) s += atom_scores[a];
    // (block_sum4's steps spelled out: through the helper this kernel compiles to another body, one instruction less in the
    // hand-over's address; switch when a changed body may be measured - DESIGN.md section 13)
    s = wave_sum(s);
    if (lane == 0) part[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) scores[b] = sum4(part[0], part[1], part[2], part[3]); // (no atoms: an exact zero)
}

hipError_t launch_score(const GradArgs &a, const ScoreArgs &sa, const WalkKey &key, hipStream_t s) {
    return for_walk(key, [&](auto gt, auto mode, auto gauss, auto chanwise) {
        return launch_walk(score_kernel<typename decltype(gt)::type, mode, gauss, chanwise>, a, s, sa);
    });
}

hipError_t launch_score_reduce(const double *atom_scores, const int64_t *offsets, int32_t B, double *scores, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(score_reduce_kernel, dim3((unsigned)B), dim3(64 * SCORE_WAVES), 0, s, atom_scores, offsets, scores);
    return hipGetLastError();
}

} // namespace mvx
