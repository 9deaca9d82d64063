// mvx_pose.hip - explicit rigid poses (MVX_XF_POSE_PTR): the kernel that turns device-resident poses into plain records, and
// the reduction of per-atom gradients to pose gradients (mvx_pose_grad_batch).
//
// A pose (c, q, t) maps x to p = M(q) (x - c) + t, M the matrix of the sandwich product q (.) conj(q) (make_xform_f32 writes
// it out; it scales by |q|^2, so M M^T = |q|^4 I). The backward entries return g_n = M^T dL/dp_n per atom, hence
// dL/dp_n = M g_n / n4 with n4 = |q|^4, and with s = sum_n g_n, U = sum_n g_n (x_n - c)^T  (DESIGN.md section 16):
//   dL/dc   = -s
//   dL/dt   = sum_n dL/dp_n = M s / n4
//   dL/dq_k = sum_n dL/dp_n . (dM/dq_k (x_n - c)) = < dM/dq_k , M U / n4 >
//
//   pose_resolve_kernel  thread b reads the 10 doubles of record b's pose and rewrites the record as CENTER | ROTATE |
//                        TRANSLATE | TRANSLATE_ONCE with trans = (float)t: the hot kernels never see a pose pointer
//   pose_grad_kernel     one workgroup (4 waves) per molecule: wave w takes the chunks w, w + 4, ... of 64 atoms in order, each
//                        lane keeps 12 double partials (s, U); a fixed butterfly per wave, the four waves in a fixed order through
//                        LDS; lane 0 finishes (M, n4, the contractions) in double. No atomics: a molecule's row depends on
//                        nothing but its own atoms - the same bits in any batch and in every run.
#include "mvx_grad_device.h"
#include "mvx_pose.h"

namespace mvx {

__global__ void __launch_bounds__(64) pose_resolve_kernel(mvx_xform *__restrict__ xf, int32_t B) {
    const int b = (int)(blockIdx.x * 64 + threadIdx.x);
    if (b >= B) return;
    if (!(xf[b].flags & MVX_XF_POSE_PTR)) return;
    const double *src = xf[b].center_ptr;
    double pose[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) pose[i] = src[i];
    mvx_xform out;
    pose_to_record(pose, out);
    xf[b] = out;
}

constexpr int POSE_WAVES = 4;

__global__ void __launch_bounds__(64 * POSE_WAVES) pose_grad_kernel(const double *__restrict__ coords,
                                                                    const double *__restrict__ grad_coords,
                                                                    const int64_t *__restrict__ offsets,
                                                                    const mvx_xform *__restrict__ xf, double *__restrict__ grad_pose) {
    __shared__ double part[POSE_WAVES][12];
    const int b = (int)blockIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t a0 = offsets[b], a1 = offsets[b + 1];
    const double *pose = xf[b].center_ptr;
    const double c0 = pose[0], c1 = pose[1], c2 = pose[2];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    double u00 = 0.0, u01 = 0.0, u02 = 0.0, u10 = 0.0, u11 = 0.0, u12 = 0.0, u20 = 0.0, u21 = 0.0, u22 = 0.0;
    for (int64_t a = a0 + 64 * wave + lane; a < a1; a += 64 * POSE_WAVES) {
        const double g0 = grad_coords[3 * a], g1 = grad_coords[3 * a + 1], g2 = grad_coords[3 * a + 2];
        // an atom that reaches no voxel has a zero row, and its x may be NaN or infinite: 0 * x would poison U. For finite x the
        // skipped terms are +-0 added to sums that start at +0: no bit changes.
        if (g0 == 0.0 && g1 == 0.0 && g2 == 0.0) continue;
        const double x0 = coords[3 * a] - c0, x1 = coords[3 * a + 1] - c1, x2 = coords[3 * a + 2] - c2;
        s0 += g0;
        s1 += g1;
        s2 += g2;
        u00 += g0 * x0;
        u01 += g0 * x1;
        u02 += g0 * x2;
        u10 += g1 * x0;
        u11 += g1 * x1;
        u12 += g1 * x2;
        u20 += g2 * x0;
        u21 += g2 * x1;
        u22 += g2 * x2;
    }
    const double v[12] = {wave_sum(s0),  wave_sum(s1),  wave_sum(s2),  wave_sum(u00), wave_sum(u01), wave_sum(u02),
                          wave_sum(u10), wave_sum(u11), wave_sum(u12), wave_sum(u20), wave_sum(u21), wave_sum(u22)};
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < 12; ++i) part[wave][i] = v[i];
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double *out = grad_pose + 10 * (size_t)b;
    if (a1 <= a0) { // a molecule without atoms: zeros, whatever its pose
#pragma unroll
        for (int i = 0; i < 10; ++i) out[i] = 0.0;
        return;
    }
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = sum4(part[0][i], part[1][i], part[2][i], part[3][i]);
    const double q0 = pose[3], q1 = pose[4], q2 = pose[5], q3 = pose[6];
    const double n2 = ((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3;
    const double n4 = n2 * n2; // (q = 0: 0 / 0 below, a non-finite row)
    const double m[3][3] = {{q0 * q0 + q1 * q1 - q2 * q2 - q3 * q3, 2.0 * (q1 * q2 - q0 * q3), 2.0 * (q1 * q3 + q0 * q2)},
                            {2.0 * (q1 * q2 + q0 * q3), q0 * q0 - q1 * q1 + q2 * q2 - q3 * q3, 2.0 * (q2 * q3 - q0 * q1)},
                            {2.0 * (q1 * q3 - q0 * q2), 2.0 * (q2 * q3 + q0 * q1), q0 * q0 - q1 * q1 - q2 * q2 + q3 * q3}};
    out[0] = -t[0];
    out[1] = -t[1];
    out[2] = -t[2];
    double w[3][3]; // M U / n4 = sum_n dL/dp_n (x_n - c)^T
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        out[7 + i] = ((m[i][0] * t[0] + m[i][1] * t[1]) + m[i][2] * t[2]) / n4;
#pragma unroll
        for (int j = 0; j < 3; ++j) w[i][j] = ((m[i][0] * t[3 + j] + m[i][1] * t[6 + j]) + m[i][2] * t[9 + j]) / n4;
    }
    // dM/dq_k / 2, row by row
    const double d[4][3][3] = {{{q0, -q3, q2}, {q3, q0, -q1}, {-q2, q1, q0}},
                               {{q1, q2, q3}, {q2, -q1, -q0}, {q3, q0, -q1}},
                               {{-q2, q1, q0}, {q1, q2, q3}, {-q0, q3, -q2}},
                               {{-q3, -q0, q1}, {q0, -q3, q2}, {q1, q2, q3}}};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc += d[k][i][j] * w[i][j];
        out[3 + k] = 2.0 * acc;
    }
}

hipError_t launch_pose_resolve(mvx_xform *xf_dev, int32_t B, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(pose_resolve_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, xf_dev, B);
    return hipGetLastError();
}

hipError_t launch_pose_grad(const double *coords, const double *grad_coords, const int64_t *offsets, const mvx_xform *xf_dev,
                            int32_t B, double *grad_pose, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(pose_grad_kernel, dim3((unsigned)B), dim3(64 * POSE_WAVES), 0, s, coords, grad_coords, offsets, xf_dev, grad_pose);
    return hipGetLastError();
}

} // namespace mvx
