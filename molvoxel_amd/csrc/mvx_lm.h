// mvx_lm.h - what the C-ABI TU (mvx_capi.hip) needs of the Levenberg-Marquardt bookkeeping step (mvx_lm.hip, mvx_lm_step): the
// argument record of lm_step_kernel and its launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mvx {

// every array on the device; the current state is read and written, the trial's S2, G2 and H2 are read with have_trial only.
// The shapes are the rigid step's, n = 6; FlexLmArgs (mvx_flex.h) extends the record for n = 6 + T.
struct LmArgs {
    int32_t B, have_trial, max_dropped;
    double lam_down, lam_up;
    double *q, *t, *S, *G, *H, *lam; // (B, 4) (B, 3) (B,) (B, 6) (B, 36) (B,)
    int32_t *taken, *dropped;        // (B,) (B,)
    double *q2, *t2;                 // (B, 4) (B, 3): the trial pose, read on an accepted trial, then written
    const double *S2, *G2, *H2;      // (B,) (B, 6) (B, 36)
    double *xi;                      // (B, 6) or null: the step
};

// One thread per pose, blocks of 64: the decision on the trial, then the damped Newton step and the pose it leads to.
hipError_t launch_lm_step(const LmArgs &a, hipStream_t s);

} // namespace mvx
