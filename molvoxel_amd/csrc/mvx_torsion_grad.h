// mvx_torsion_grad.h - what the C-ABI TU (mvx_capi.hip) needs of the adjoint of the conformer kernel (mvx_torsion_grad.hip;
// mvx_apply_torsions_backward): the launcher of its one kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvx {

// dL/dcoords and dL/dangles of C(theta) = launch_torsion_apply's output: conformer (total, 3) is that output, grad_out (total, 3)
// is dL/dC; grad_coords (total, 3) may be grad_out; grad_angles (B, T), every entry written (+0.0 for an inert torsion); pos
// (total, 3): workspace for the positions the sweep turns back - conformer is not written. offsets, axes, moves, angles as
// launch_torsion_apply takes them. One workgroup per molecule. The tree rules (include/mvx.h) are assumed: outside them the
// kernel stays inside its arrays and its values are unspecified.
hipError_t launch_torsion_backward(const double *conformer, const int64_t *offsets, int32_t B, int32_t T, const int32_t *axes,
                                   const int32_t *moves, const double *angles, const double *grad_out, double *pos, double *grad_coords,
                                   double *grad_angles, hipStream_t s);

} // namespace mvx
