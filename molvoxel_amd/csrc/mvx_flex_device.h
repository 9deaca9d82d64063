// mvx_flex_device.h - what the torsion kernels share on the device, included by mvx_flex.hip (torsion_apply_kernel,
// flex_subset_kernel, flex_assemble_kernel) and mvx_torsion_grad.hip (torsion_backward_kernel): the axis of a torsion. Functions
// only, no kernels. The build forbids contraction and fast math, so an expression here gives the same bits in every kernel that
// calls it: the backward sweep forms the axis the forward turned about, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace mvx {

// The unit axis u from pa to pb, or false: no length, or none that is finite (then pa and pb are not both finite).
__device__ __forceinline__ bool unit_axis(const double (&pa)[3], const double (&pb)[3], double (&u)[3]) {
    const double d0 = pb[0] - pa[0], d1 = pb[1] - pa[1], d2 = pb[2] - pa[2];
    const double len2 = (d0 * d0 + d1 * d1) + d2 * d2;
    if (!(len2 > 0.0) || !isfinite(len2)) return false;
    const double len = sqrt(len2);
    u[0] = d0 / len;
    u[1] = d1 / len;
    u[2] = d2 / len;
    return true;
}

} // namespace mvx
