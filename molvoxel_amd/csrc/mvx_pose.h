// mvx_pose.h - what the C-ABI TU (mvx_capi.hip) needs of the explicit rigid poses (mvx_pose.hip).
#pragma once
#include "mvx_internal.h"

namespace mvx {

constexpr uint32_t POSE_PLAIN_FLAGS = MVX_XF_CENTER | MVX_XF_ROTATE | MVX_XF_TRANSLATE | MVX_XF_TRANSLATE_ONCE;

// The plain record of a pose [c | q | t]: what every kernel sees of a MVX_XF_POSE_PTR record (host poses are folded with it on
// the host, device poses by pose_resolve_kernel with the same expression).
__host__ __device__ inline void pose_to_record(const double *pose, mvx_xform &xf) {
    for (int i = 0; i < 3; ++i) xf.center[i] = pose[i];
    for (int i = 0; i < 4; ++i) xf.quat[i] = pose[3 + i];
    for (int i = 0; i < 3; ++i) xf.trans[i] = (float)pose[7 + i];
    xf.flags = POSE_PLAIN_FLAGS;
    xf.center_ptr = nullptr;
}

// Rewrites every MVX_XF_POSE_PTR record of the B device records as a plain one (the poses are device memory).
hipError_t launch_pose_resolve(mvx_xform *xf_dev, int32_t B, hipStream_t s);
// grad_pose (B, 10) from grad_coords = M^T dL/dp: one workgroup per molecule, fixed-order sums, no atomics. xf_dev: the B
// records as the caller gave them (MVX_XF_POSE_PTR, not resolved).
hipError_t launch_pose_grad(const double *coords, const double *grad_coords, const int64_t *offsets, const mvx_xform *xf_dev,
                            int32_t B, double *grad_pose, hipStream_t s);

} // namespace mvx
