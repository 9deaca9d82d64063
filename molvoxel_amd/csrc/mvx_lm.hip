// mvx_lm.hip - one Levenberg-Marquardt bookkeeping step for B rigid poses in one launch (gfx950; mvx_lm_step, DESIGN.md
// section 26): what lies between two evaluations of mvx_score_hessian_batch / mvx_score_hessian_views in a damped Newton
// refinement - the accept / drop decision on the last trial, the damping update, the 6x6 solve and the twist onto the pose.
//
//   lm_step_kernel  one thread per pose, blocks of 64, float64 throughout. Per pose:
//                   1. with a trial and dropped < max_dropped: the decision (lm_decide, mvx_newton_device.h); an accepted trial
//                      becomes the state - q, t, S, G, H copied bit for bit, taken += 1
//                   2. dropped >= max_dropped: the pose is finished; q2 = q, t2 = t, xi = 0 and nothing else is written
//                   3. otherwise (-H + lam I) xi = G by Gaussian elimination with partial pivoting (the matrix may be indefinite
//                      while lam is small), and (q2, t2) = apply_twist(q, t, xi) (mvx_newton_device.h). A zero pivot, a
//                      non-finite xi, q, t, lam, q2 or t2: xi = 0 and (q2, t2) = (q, t) - the next call sees S2 == S, drops the
//                      step and raises lam.
// The decision rule and the twist are shared with the step in torsion coordinates (mvx_flex.hip); the solve is this kernel's own.
//
// The 6x7 system lives in registers: every loop over it is unrolled with compile-time indices, the pivot row is exchanged by
// selects and never used as an index, so nothing goes to scratch (tests/test_lm_host.py pins scratch 0 and no spills). No
// atomics, no LDS, no host read; a pose's values do not depend on its batch.
#include "mvx_lm.h"
#include "mvx_newton_device.h"

#include <math.h>

namespace mvx {

namespace {
constexpr int LM_BLOCK = 64;
}

__global__ void __launch_bounds__(LM_BLOCK) lm_step_kernel(const LmArgs a) {
    const int b = (int)(blockIdx.x * LM_BLOCK + threadIdx.x);
    if (b >= a.B) return;
    const size_t i = (size_t)b;
    double S = a.S[i], lam = a.lam[i];
    int32_t dropped = a.dropped[i];
    // ---- 1. the decision on the trial ----
    bool accept = false;
    if (lm_has_trial(a, dropped)) {
        accept = lm_decide(a, a.S2[i], S, lam, dropped, [&] {
            a.S[i] = S;
            a.taken[i] += 1;
        });
        a.lam[i] = lam;
        a.dropped[i] = dropped;
    }
    // the state the step starts from: the accepted trial, copied, or the state as it is
    const double *qs = accept ? a.q2 + 4 * i : a.q + 4 * i;
    const double *ts = accept ? a.t2 + 3 * i : a.t + 3 * i;
    const double *Gs = accept ? a.G2 + 6 * i : a.G + 6 * i;
    const double *Hs = accept ? a.H2 + 36 * i : a.H + 36 * i;
    double q[4], t[3], m[6][7];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = qs[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = ts[k];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 6; ++c) m[r][c] = Hs[6 * r + c];
        m[r][6] = Gs[r];
    }
    if (accept) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.q[4 * i + k] = q[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.t[3 * i + k] = t[k];
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 6; ++c) a.H[36 * i + 6 * r + c] = m[r][c];
            a.G[6 * i + r] = m[r][6];
        }
    }
    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double q2[4] = {q[0], q[1], q[2], q[3]}, t2[3] = {t[0], t[1], t[2]};
    // ---- 2. a finished pose stays where it is; 3. the step ----
    if (dropped < a.max_dropped) {
#pragma unroll
        for (int r = 0; r < 6; ++r) {
#pragma unroll
            for (int c = 0; c < 6; ++c) m[r][c] = (r == c ? lam : 0.0) - m[r][c];
        }
        bool ok = true;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            // the pivot: the first row at or below k with the largest |entry| of column k
            double best = fabs(m[k][k]);
            int p = k;
#pragma unroll
            for (int r = k + 1; r < 6; ++r) {
                const double v = fabs(m[r][k]);
                if (v > best) {
                    best = v;
                    p = r;
                }
            }
#pragma unroll
            for (int r = k + 1; r < 6; ++r) {
                const bool sw = p == r;
#pragma unroll
                for (int c = k; c < 7; ++c) {
                    const double top = m[k][c], low = m[r][c];
                    m[k][c] = sw ? low : top;
                    m[r][c] = sw ? top : low;
                }
            }
            const double piv = m[k][k];
            ok = ok && piv != 0.0;
#pragma unroll
            for (int r = k + 1; r < 6; ++r) {
                const double f = m[r][k] / piv;
#pragma unroll
                for (int c = k + 1; c < 7; ++c) m[r][c] -= f * m[k][c];
            }
        }
#pragma unroll
        for (int k = 5; k >= 0; --k) {
            double s = m[k][6];
#pragma unroll
            for (int c = k + 1; c < 6; ++c) s -= m[k][c] * x[c];
            x[k] = s / m[k][k];
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) ok = ok && isfinite(x[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k) ok = ok && isfinite(q[k]); // (spelled out: see mvx_newton_device.h)
#pragma unroll
        for (int k = 0; k < 3; ++k) ok = ok && isfinite(t[k]);
        ok = ok && isfinite(lam);
        if (ok) {
            apply_twist(q, t, x, q2, t2);
#pragma unroll
            for (int k = 0; k < 4; ++k) ok = ok && isfinite(q2[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) ok = ok && isfinite(t2[k]);
        }
        if (!ok) {
#pragma unroll
            for (int k = 0; k < 6; ++k) x[k] = 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) q2[k] = q[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t2[k] = t[k];
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) a.q2[4 * i + k] = q2[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) a.t2[3 * i + k] = t2[k];
    if (a.xi) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.xi[6 * i + k] = x[k];
    }
}

hipError_t launch_lm_step(const LmArgs &a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(lm_step_kernel, dim3((unsigned)((a.B + LM_BLOCK - 1) / LM_BLOCK)), dim3(LM_BLOCK), 0, s, a);
    return hipGetLastError();
}

} // namespace mvx
