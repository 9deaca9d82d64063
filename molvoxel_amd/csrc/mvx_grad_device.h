// mvx_grad_device.h - device helpers and the walk launch of the backward family, included by its eight kernel files:
// mvx_grad.hip, mvx_grad_radii.hip, mvx_score.hip and mvx_moments_grad.hip (the walks of mvx_grad_body.inc, launch_walk), mvx_hess.hip
// (a walk of its own through launch_walk, wave sums, sum4), mvx_grad_radii.hip and mvx_grad_density.hip (the reductions over a call:
// block_sum4, sum4), mvx_pose.hip and mvx_views_reduce.hip (wave sums, sum4); and by mvx_newton_device.h (wave sums), through
// which mvx_flex.hip and mvx_lm.hip get it.
#pragma once
#include "mvx_device.h"
#include "mvx_grad.h"

namespace mvx {

constexpr double LN2 = 0.69314718055994531; // d exp2(k d2) / d d2 = ln2 k exp2(k d2)

// element type of the grid -> the arithmetic of the handle (float32 for float and bfloat16 grids)
template <typename GT> struct GradReal { typedef float type; };
template <> struct GradReal<double> { typedef double type; };

__device__ __forceinline__ float load_grad(const float *p) { return *p; }
__device__ __forceinline__ float load_grad(const __bf16 *p) { return (float)*p; } // (exact widening)
__device__ __forceinline__ double load_grad(const double *p) { return *p; }

// dL/dcoords = M^T dL/dp: apply_xform's rotation with the conjugate quaternion, in the same operation order. Exact for
// |q| != 1 too: M = q (.) conj(q) and M^T = conj(q) (.) q. Centring and translations are constants.
__device__ __forceinline__ void apply_xform_transpose(const mvx_xform &xf, double &x, double &y, double &z) {
    if (!(xf.flags & MVX_XF_ROTATE)) return;
    const double q0 = xf.quat[0], q1 = -xf.quat[1], q2 = -xf.quat[2], q3 = -xf.quat[3];
    const double zero = 0.0;
    const double a0 = ((q0 * zero - q1 * x) - q2 * y) - q3 * z;
    const double a1 = ((q0 * x + q1 * zero) + q2 * z) - q3 * y;
    const double a2 = ((q0 * y - q1 * z) + q2 * zero) + q3 * x;
    const double a3 = ((q0 * z + q1 * y) - q2 * x) + q3 * zero;
    const double i0 = q0, i1 = q1 * -1, i2 = q2 * -1, i3 = q3 * -1;
    x = ((a0 * i1 + a1 * i0) + a2 * i3) - a3 * i2;
    y = ((a0 * i2 - a1 * i3) + a2 * i0) + a3 * i1;
    z = ((a0 * i3 + a1 * i2) - a2 * i1) + a3 * i0;
}

// sum over the 64 lanes, the same butterfly in every lane: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// The fixed order in which four waves' sums are added - part of the contract "no atomics: the same bits in any batch and in
// every run" of every reduction here
__device__ __forceinline__ double sum4(double w0, double w1, double w2, double w3) { return (w0 + w1) + (w2 + w3); }

// Sum of v over a workgroup of four waves: a butterfly per wave, lane 0 of each wave hands its sum over in LDS, a barrier,
// then thread 0 alone gets sum4 of the four: thread0(sum). Every thread of the workgroup must call it (the barrier). The two
// density reductions call it; grad_radii_reduce_kernel and score_reduce_kernel spell the same steps out (see there).
template <typename Fn>
__device__ __forceinline__ void block_sum4(double v, Fn &&thread0) {
    __shared__ double wsum[4];
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) thread0(sum4(wsum[0], wsum[1], wsum[2], wsum[3]));
}

// 32 per-lane channel partials -> lane l holds the wave's sum of channel l / 2 (31 exchanges instead of 32 x 6): each step
// halves the channels a lane keeps - the lane with the mask bit set keeps the upper half - and adds its partner's copy of
// them. a + b and b + a are the same bits, so both lanes of a pair agree and the order is fixed.
template <typename T>
__device__ __forceinline__ T wave_sum32(T (&v)[32], int lane) {
#pragma unroll
    for (int h = 16, m = 32; h >= 1; h >>= 1, m >>= 1) {
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const T send = up ? v[j] : v[j + h];
            const T keep = up ? v[j + h] : v[j];
            v[j] = keep + __shfl_xor(send, m, 64);
        }
    }
    return v[0] + __shfl_xor(v[0], 1, 64);
}

// wave_sum32 with the selects made on values rather than on addresses: the same exchanges, sums and bits, but a double[32]
// stays in registers (wave_sum32's address selects leave it in scratch). grad_kernel keeps wave_sum32, so its code stays put.
template <typename T>
__device__ __forceinline__ T wave_sum32_regs(T (&v)[32], int lane) {
#pragma unroll
    for (int h = 16, m = 32; h >= 1; h >>= 1, m >>= 1) {
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const T lo = v[j], hi = v[j + h];
            const T send = up ? lo : hi;
            const T keep = up ? hi : lo;
            v[j] = keep + __shfl_xor(send, m, 64);
        }
    }
    return v[0] + __shfl_xor(v[0], 1, 64);
}

// The launch of a walk kernel (one of for_walk's or for_moments_walk's instantiations; extra: its RadiiArgs, ScoreArgs or MomentsArgs): four atoms per block of
// 256 in atom order, or 8 a.xcd_span blocks under the spatial order; nothing without atoms. Not launch_kernel<Kern>
// (mvx_device.h): that one consumes timed_launch's pending profiling events, which the backward entries must not.
template <typename Kern, typename... Extra>
static hipError_t launch_walk(Kern kern, const GradArgs &a, hipStream_t s, const Extra &...extra) {
    if (a.total <= 0) return hipSuccess;
    const unsigned nblk = (unsigned)((a.total + 3) / 4);
    hipLaunchKernelGGL(kern, dim3(a.xcd_span ? 8u * (unsigned)a.xcd_span : nblk), dim3(256), 0, s, a, extra...);
    return hipGetLastError();
}

} // namespace mvx
