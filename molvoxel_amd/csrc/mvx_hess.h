// mvx_hess.h - what the C-ABI TU (mvx_capi.hip) needs of the second-order score walk (mvx_hess.hip, mvx_score_hessian_batch):
// the argument record of score_hess_kernel and the launchers of the walk and of the per-molecule twist reduction.
#pragma once
#include "mvx_grad.h"

namespace mvx {

// score_hess_kernel reads a walk's GradArgs (rec, w, g = the field, offsets, order, xcd_span, total, B, C, D, res, half; xforms,
// Tc, kc, grad_coords and grad_w are not read: every row is in the grid frame) and writes the rows named here, all of them
struct HessArgs {
    double *atom_scores; // (total,)   s_n
    double *atom_grad;   // (total, 3) g_n = dS/dp_n, grid frame
    double *atom_hess;   // (total, 6) H_n as (xx, xy, xz, yy, yz, zz), grid frame
    int64_t mol_stride;  // elements between the fields of two molecules: 0 (one field shared by all) or C * D^3
};

// One wave per atom record over the constant field (launch_walk's grid, order and xcd_span): s_n, g_n and H_n per atom.
// hipErrorInvalidValue for a key with channel-wise radii for features (no such instantiation).
hipError_t launch_score_hess(const GradArgs &a, const HessArgs &ha, const WalkKey &key, hipStream_t s);
// twist_grad[b] (6) and - unless null - twist_hess[b] (36, symmetric, row-major) of every molecule about pivots[b] (null: the
// origin) from the rows of the walk and the records' positions, in a fixed order (one workgroup per molecule, no atomics)
hipError_t launch_twist_reduce(const AtomRec *rec, const double *atom_grad, const double *atom_hess, const int64_t *offsets,
                               const double *pivots, int32_t B, double *twist_grad, double *twist_hess, hipStream_t s);

} // namespace mvx
