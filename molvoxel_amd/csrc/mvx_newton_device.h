// mvx_newton_device.h - what the rigid and the torsion form of the damped Newton refinement share on the device, included by
// mvx_hess.hip (twist_reduce_kernel), mvx_lm.hip (lm_step_kernel) and mvx_flex.hip (flex_subset_kernel, flex_assemble_kernel,
// flex_lm_step_kernel): the twist sum of the walk's rows - its slots, the rule for an atom without rows, one atom's terms and
// the hand-over of the lane partials -, and the step rule - the decision on the trial and the twist onto the pose. Functions only, no kernels: who loads, who writes and when stays with each kernel. The build forbids contraction
// and fast math, so an expression here gives the same bits in every kernel that calls it.
#pragma once
#include "mvx_grad_device.h"
#include "mvx_lm.h"

#include <math.h>

namespace mvx {

constexpr int TWIST_WAVES = 4;       // waves of a workgroup that forms a twist sum
constexpr int TWIST_VALUES = 6 + 21; // G = J^T g, then the upper triangle of X = J^T H J row by row
constexpr int TWIST_K_SLOT = 27;     // the split form keeps K = sum r g^T behind them, row by row (FLEX_SUBSET values in all)
// where entry (i, j), i <= j, of the 6x6 sits among them
__host__ __device__ constexpr int twist_slot(int i, int j) { return 6 + 6 * i - i * (i - 1) / 2 + (j - i); }

// An atom that reaches no voxel has zero rows g (3) and h (6: xx xy xz yy yz zz), and its position may be NaN or infinite: 0 * r
// would poison the sums, so the twist sums skip it. For a finite position the skipped terms are +-0 added to sums that start
// at +0: no bit changes.
__device__ __forceinline__ bool twist_rows_zero(const double (&g)[3], const double (&h)[6]) {
    return g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0 && h[0] == 0.0 && h[1] == 0.0 && h[2] == 0.0 && h[3] == 0.0 && h[4] == 0.0 && h[5] == 0.0;
}

// One atom's terms of a twist sum, from its rows g, h and r = p - o: with J = [ I | A ], A = -[r]x, acc[0..5] += J^T g =
// (g, r x g) and acc[twist_slot(i, j)] += (J^T H J)[i][j]: rows 0..2 hold [H | H A], rows 3..5 hold [. | A^T H A]. The second
// derivative of the rotation adds K - tr(K) I, K = sym(r g^T), to the angular block:
//   SPLIT_K false  w + kk goes into the block's slot (the rigid twist Hessian, complete)
//   SPLIT_K true   w alone goes there and r_i g_j into acc[TWIST_K_SLOT + 3 i + j]: a torsion contracts K with its own axis
template <bool SPLIT_K, int NV>
__device__ __forceinline__ void twist_accumulate(const double (&g)[3], const double (&h)[6], const double (&r)[3], double (&acc)[NV]) {
    static_assert(NV >= (SPLIT_K ? TWIST_K_SLOT + 9 : TWIST_VALUES), "acc holds every slot");
    const double H[3][3] = {{h[0], h[1], h[2]}, {h[1], h[3], h[4]}, {h[2], h[4], h[5]}};
    const double A[3][3] = {{0.0, r[2], -r[1]}, {-r[2], 0.0, r[0]}, {r[1], -r[0], 0.0}}; // A[i][j]: row i, column j
#pragma unroll
    for (int i = 0; i < 3; ++i) acc[i] += g[i];
    acc[3] += r[1] * g[2] - r[2] * g[1];
    acc[4] += r[2] * g[0] - r[0] * g[2];
    acc[5] += r[0] * g[1] - r[1] * g[0];
    // HAm = H A (3x3), w = A^T H A (symmetric)
    double HAm[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) HAm[i][j] = (H[i][0] * A[0][j] + H[i][1] * A[1][j]) + H[i][2] * A[2][j];
    const double gr = (g[0] * r[0] + g[1] * r[1]) + g[2] * r[2]; // (SPLIT_K: unused)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i; j < 3; ++j) acc[twist_slot(i, j)] += H[i][j];
#pragma unroll
        for (int j = 0; j < 3; ++j) acc[twist_slot(i, 3 + j)] += HAm[i][j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double w = (A[0][i] * HAm[0][j] + A[1][i] * HAm[1][j]) + A[2][i] * HAm[2][j];
            if constexpr (SPLIT_K) acc[twist_slot(3 + i, 3 + j)] += w;
            else acc[twist_slot(3 + i, 3 + j)] += w + (0.5 * (g[i] * r[j] + r[i] * g[j]) - (i == j ? gr : 0.0)); // w + kk
        }
    }
    if constexpr (SPLIT_K) {
#pragma unroll
        for (int e = 0; e < 9; ++e) acc[TWIST_K_SLOT + e] += r[e / 3] * g[e % 3]; // K[i][j] at 3 i + j
    }
}

// The tail of a twist sum: a fixed butterfly per value, lane 0 of each wave hands the wave's sums over in LDS, a barrier;
// behind it part[0..3][i] go through sum4. Every thread of the workgroup must call it.
template <int NV>
__device__ __forceinline__ void twist_wave_partials(const double (&acc)[NV], double (&part)[TWIST_WAVES][NV], int lane, int wave) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) part[wave][i] = v;
    }
    __syncthreads();
}

// The decision on a trial. There is one to decide on when the call brings a trial and the pose is not finished: a pose that
// has dropped max_dropped trials in a row stays as it is. S2 > S - false for a NaN, so a non-finite trial is dropped - makes
// the trial the state: S = S2, lam *= lam_down, dropped = 0; any other trial is dropped: lam *= lam_up, dropped += 1. Returns
// whether the trial was accepted. `accepted()`: what the kernel writes on an accepted trial, inside the accepting branch -
// behind the call the compiler turns the branches into selects, which is one instruction more in lm_step_kernel.
__device__ __forceinline__ bool lm_has_trial(const LmArgs &a, int32_t dropped) { return a.have_trial && dropped < a.max_dropped; }
template <typename Accepted>
__device__ __forceinline__ bool lm_decide(const LmArgs &a, double S2, double &S, double &lam, int32_t &dropped, Accepted &&accepted) {
    const bool accept = S2 > S;
    if (accept) {
        S = S2;
        lam *= a.lam_down;
        dropped = 0;
        accepted();
    } else {
        lam *= a.lam_up;
        dropped += 1;
    }
    return accept;
}

// (The finiteness gates on q, t, lam and on q2, t2 are spelled out in both step kernels as `ok = ok && isfinite(..)` chains:
// through a helper the compiler tests six values by a compare with infinity, not a class test: one instruction more.)
// (q2, t2) = the twist x = (tau, w) onto the pose (q, t): u = (cos(|w|/2), sin(|w|/2) w/|w|), q2 = u (x) q, t2 = t + tau.
// w = 0: u = (1, 0, 0, 0), q2 keeps the quaternion itself, bit for bit.
__device__ __forceinline__ void apply_twist(const double (&q)[4], const double (&t)[3], const double *x, double (&q2)[4], double (&t2)[3]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) q2[k] = q[k];
    const double wx = x[3], wy = x[4], wz = x[5];
    const double half = 0.5 * sqrt(wx * wx + wy * wy + wz * wz);
    if (half != 0.0) {
        const double u0 = cos(half), f = 0.5 * (sin(half) / half);
        const double u1 = f * wx, u2 = f * wy, u3 = f * wz;
        q2[0] = u0 * q[0] - u1 * q[1] - u2 * q[2] - u3 * q[3];
        q2[1] = u0 * q[1] + u1 * q[0] + u2 * q[3] - u3 * q[2];
        q2[2] = u0 * q[2] - u1 * q[3] + u2 * q[0] + u3 * q[1];
        q2[3] = u0 * q[3] + u1 * q[2] - u2 * q[1] + u3 * q[0];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) t2[k] = t[k] + x[k];
}

} // namespace mvx
