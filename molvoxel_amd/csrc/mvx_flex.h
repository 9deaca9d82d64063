// mvx_flex.h - what the C-ABI TU (mvx_capi.hip) needs of the torsion coordinates (mvx_flex.hip; mvx_apply_torsions,
// mvx_score_hessian_flex_batch, mvx_flex_lm_step): the argument records and launchers of its four kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mvx_internal.h"
#include "mvx_lm.h"

namespace mvx {

constexpr int FLEX_MAX_T = 32;      // torsions per molecule: one bit each of an atom's 32-bit mask
constexpr int FLEX_SUBSET = 36;     // per (molecule, torsion): F (3), N (3), the upper triangle of X (21), K (9)
constexpr int FLEX_MAX_N = 6 + FLEX_MAX_T;

// C(theta): every molecule's torsions applied in order to coords -> out ((total, 3); out may be coords). axes (B, T, 2): atoms
// local to the molecule; moves (total,): bit k set = the atom turns with torsion k; angles (B, T). One workgroup per molecule.
hipError_t launch_torsion_apply(const double *coords, const int64_t *offsets, int32_t B, int32_t T, const int32_t *axes,
                                const int32_t *moves, const double *angles, double *out, hipStream_t s);

// The torsion part of a Hessian call, behind the walk and launch_twist_reduce: the subset sums of every (molecule, torsion) into
// `subset` (B, T, 36), then G (B, n) and H (B, n, n), n = 6 + T, whose first six rows and columns are twist_grad and twist_hess
// copied. flex_hess may be null. atom_pos (total, 3), unless null: the records' positions copied out.
struct FlexArgs {
    const AtomRec *rec;
    const double *atom_grad, *atom_hess; // (total, 3), (total, 6): the walk's rows
    const int64_t *offsets;              // (B + 1,) device
    const double *pivots;                // (B, 3) or null: the origin
    const int32_t *axes, *moves;         // (B, T, 2), (total,); unread with T == 0
    const double *twist_grad, *twist_hess; // (B, 6), (B, 36): launch_twist_reduce's
    double *subset;                      // (B, T, 36) workspace
    double *flex_grad, *flex_hess;       // (B, n), (B, n, n) or null
    double *atom_pos;                    // (total, 3) or null
    int64_t total;
    int32_t B, T;
};
hipError_t launch_flex(const FlexArgs &a, hipStream_t s);

// mvx_flex_lm_step: LmArgs (mvx_lm.h) for n = 6 + T coordinates - G, G2 and xi (B, n), H and H2 (B, n, n) - with the torsion angles next
// to the pose
struct FlexLmArgs : LmArgs {
    double *theta, *theta2; // (B, T): the state's angles, and the trial's, read on an accepted trial, then written
    int32_t T;              // (behind the pointers: in front of them flex_lm_step_kernel needs one more scalar load)
};
// One wave per pose: the decision on the trial, then the damped Newton step in n dimensions and the trial it leads to.
hipError_t launch_flex_lm_step(const FlexLmArgs &a, hipStream_t s);

} // namespace mvx
