// mvx_grad_device.h - device helpers of the backward pass, shared by mvx_grad.hip (grad_kernel) and mvx_grad_radii.hip
// (grad_radii_kernel and the radius reductions).
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

} // namespace mvx
