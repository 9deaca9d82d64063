// mvx_flex.hip - torsion angles as coordinates next to the rigid twist (gfx950, float64 throughout; mvx_apply_torsions,
// mvx_score_hessian_flex_batch, mvx_flex_lm_step). A molecule has T <= 32 torsions: torsion k turns the atoms
// whose mask has bit k set about the axis from atom a_k to atom b_k, through b_k. The sets form a tree, parents before children,
// so "k is l or an ancestor of l" is bit k of moves[b_l]. With x = (tau, omega, theta_0 .. theta_{T-1}), n = 6 + T and
// p_n(x) = exp([omega]x) (C(theta)_n - o) + o + tau, the gradient and Hessian of S = sum_n s_n(p_n) at x = 0 are fixed-order sums
// of the walk's rows g_n, H_n (mvx_hess.hip): with r_n = p_n - o, J_n = [I | -[r_n]x], u_k the unit axis and
// s_k = ((p_{b_k} - o) x u_k, u_k) the twist of torsion k,
//   F_k = sum g_n   N_k = sum r_n x g_n   X_k = sum J_n^T H_n J_n   K_k = sum r_n g_n^T      over the atoms n of set k
//   c_k = tau_k x F_k + (K_k - tr(K_k) I) u_k
//   G[6 + k] = s_k . (F_k, N_k)      H[:6, 6 + k] = X_k s_k + (0, c_k)      H[6 + k, 6 + l] = s_k^T X_l s_l + u_k . c_l  (k <= l related)
// and 0 for unrelated pairs. G[:6] and H[:6, :6] are the rigid twist sums (launch_twist_reduce), copied. One atom's terms of
// F, N, X and K, the rule for an atom without rows, the decision on a trial and the twist onto the pose are mvx_newton_device.h's;
// the unit axis of a torsion is mvx_flex_device.h's, shared with the adjoint of torsion_apply_kernel (mvx_torsion_grad.hip).
//
//   torsion_apply_kernel  one workgroup per molecule; the positions are worked on in the output array. Per torsion in order: every
//                         thread reads the current axis atoms, a barrier, the atoms of the set are turned (Rodrigues), a barrier.
//                         An angle of exactly 0 and an inert torsion turn nothing: those atoms keep their bits.
//   flex_subset_kernel    grid (B, T), one workgroup (4 waves) per (torsion, molecule): wave w takes the chunks w, w + 4, ... of 64
//                         atoms in order and keeps the atoms of the set, 36 float64 lane partials (the twist sum with K kept
//                         apart), a fixed butterfly per wave, the four waves through sum4, one thread per value writes.
//   flex_assemble_kernel  one workgroup per molecule: thread l forms s_l, X_l s_l, c_l and G[6 + l]; then every entry of G and H
//                         is written once, entry (i, j) and (j, i) from the same expression: H is symmetric to the bit.
//   flex_lm_step_kernel   the damped Newton step for n = 6 + T, one wave per pose: every lane decides on the trial alike and lane
//                         0 writes; (-H + lam I) x = G by Gaussian elimination with partial pivoting on the n x (n + 1) system
//                         in LDS, one row per lane; the twist x[:6] onto the pose, theta2 = theta + x[6:], lane j holding angle j.
//
// A torsion is inert when an axis index is outside [0, N_b) (padding: -1), or the axis has no or no finite length: zero gradient
// entry, zero Hessian row and column; no axis index is used before it is checked. No atomics, no scratch
// (tests/test_flex_host.py pins it), no host read; a molecule's values do not depend on its batch.
#include "mvx_flex.h"
#include "mvx_flex_device.h"
#include "mvx_newton_device.h"

#include <math.h>

namespace mvx {

namespace {

static_assert(FLEX_SUBSET == TWIST_K_SLOT + 9, "F, N, the upper triangle of X, K");

// Torsion `ax` = (a, b) of a molecule with atoms [a0, a0 + N) in the records: false when it is inert, else p_b and the axis.
__device__ __forceinline__ bool record_axis(const AtomRec *rec, int64_t a0, int64_t N, const int32_t *ax, double (&pb)[3], double (&u)[3]) {
    const int64_t ia = ax[0], ib = ax[1];
    if (ia < 0 || ia >= N || ib < 0 || ib >= N) return false;
    const AtomRec &A = rec[a0 + ia], &Bq = rec[a0 + ib];
    const double pa[3] = {A.px, A.py, A.pz};
    pb[0] = Bq.px;
    pb[1] = Bq.py;
    pb[2] = Bq.pz;
    return unit_axis(pa, pb, u);
}

} // namespace

__global__ void __launch_bounds__(256) torsion_apply_kernel(const double *coords, const int64_t *__restrict__ offsets, int32_t T,
                                                            const int32_t *__restrict__ axes, const int32_t *__restrict__ moves,
                                                            const double *__restrict__ angles, double *out) {
    const int b = (int)blockIdx.x;
    const int64_t a0 = offsets[b], N = offsets[b + 1] - a0;
    for (int64_t n = threadIdx.x; n < N; n += 256) { // (bit for bit; out == coords: every element onto itself)
        const int64_t a = a0 + n;
        const double x = coords[3 * a], y = coords[3 * a + 1], z = coords[3 * a + 2];
        out[3 * a] = x;
        out[3 * a + 1] = y;
        out[3 * a + 2] = z;
    }
    __syncthreads();
    for (int k = 0; k < T; ++k) {
        // (every thread reads the same values: the branches below are uniform over the workgroup)
        const int32_t *ax = axes + ((size_t)b * T + k) * 2;
        const int64_t ia = ax[0], ib = ax[1];
        const double th = angles[(size_t)b * T + k];
        bool turn = th != 0.0 && ia >= 0 && ia < N && ib >= 0 && ib < N;
        double pb[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0};
        if (turn) {
            const double *A = out + 3 * (a0 + ia), *Bq = out + 3 * (a0 + ib);
            const double pa[3] = {A[0], A[1], A[2]};
            pb[0] = Bq[0];
            pb[1] = Bq[1];
            pb[2] = Bq[2];
            turn = unit_axis(pa, pb, u);
        }
        __syncthreads(); // the axis is read before any atom of the set moves (b_k is one of them)
        if (turn) {
            const double c = cos(th), s = sin(th), c1 = 1.0 - c;
            for (int64_t n = threadIdx.x; n < N; n += 256) {
                const int64_t a = a0 + n;
                if (!(((uint32_t)moves[a] >> k) & 1u)) continue;
                const double v0 = out[3 * a] - pb[0], v1 = out[3 * a + 1] - pb[1], v2 = out[3 * a + 2] - pb[2];
                const double w0 = u[1] * v2 - u[2] * v1, w1 = u[2] * v0 - u[0] * v2, w2 = u[0] * v1 - u[1] * v0; // u x v
                const double ud = ((u[0] * v0 + u[1] * v1) + u[2] * v2) * c1;
                out[3 * a] = pb[0] + ((v0 * c + w0 * s) + u[0] * ud);
                out[3 * a + 1] = pb[1] + ((v1 * c + w1 * s) + u[1] * ud);
                out[3 * a + 2] = pb[2] + ((v2 * c + w2 * s) + u[2] * ud);
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(64 * TWIST_WAVES) flex_subset_kernel(const FlexArgs a) {
    __shared__ double part[TWIST_WAVES][FLEX_SUBSET];
    const int b = (int)blockIdx.x, k = (int)blockIdx.y;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t a0 = a.offsets[b], a1 = a.offsets[b + 1];
    double *out = a.subset + ((size_t)b * a.T + k) * FLEX_SUBSET;
    double pb[3], u[3];
    if (!record_axis(a.rec, a0, a1 - a0, a.axes + ((size_t)b * a.T + k) * 2, pb, u)) { // (uniform over the workgroup)
        if (threadIdx.x < FLEX_SUBSET) out[threadIdx.x] = 0.0;
        return;
    }
    const double o0 = a.pivots ? a.pivots[3 * b] : 0.0, o1 = a.pivots ? a.pivots[3 * b + 1] : 0.0, o2 = a.pivots ? a.pivots[3 * b + 2] : 0.0;
    double acc[FLEX_SUBSET];
#pragma unroll
    for (int i = 0; i < FLEX_SUBSET; ++i) acc[i] = 0.0;
    for (int64_t n = a0 + 64 * wave + lane; n < a1; n += 64 * TWIST_WAVES) {
        if (!(((uint32_t)a.moves[n] >> k) & 1u)) continue;
        const double g[3] = {a.atom_grad[3 * n], a.atom_grad[3 * n + 1], a.atom_grad[3 * n + 2]};
        const double h[6] = {a.atom_hess[6 * n],     a.atom_hess[6 * n + 1], a.atom_hess[6 * n + 2],
                             a.atom_hess[6 * n + 3], a.atom_hess[6 * n + 4], a.atom_hess[6 * n + 5]};
        if (twist_rows_zero(g, h)) continue;
        const double r[3] = {a.rec[n].px - o0, a.rec[n].py - o1, a.rec[n].pz - o2};
        twist_accumulate<true>(g, h, r, acc);
    }
    twist_wave_partials(acc, part, lane, wave);
    if (threadIdx.x < FLEX_SUBSET) {
        const int i = (int)threadIdx.x;
        out[i] = sum4(part[0][i], part[1][i], part[2][i], part[3][i]);
    }
}

__global__ void __launch_bounds__(256) flex_assemble_kernel(const FlexArgs a) {
    __shared__ double sh_s[FLEX_MAX_T][6], sh_z[FLEX_MAX_T][6], sh_y[FLEX_MAX_T][6], sh_c[FLEX_MAX_T][3], sh_g[FLEX_MAX_T];
    __shared__ uint32_t sh_m[FLEX_MAX_T]; // moves[b_l], 0 for an inert torsion
    __shared__ int sh_ok[FLEX_MAX_T];
    const int b = (int)blockIdx.x, T = a.T, n = 6 + T;
    const int64_t a0 = a.offsets[b], a1 = a.offsets[b + 1];
    if (a.atom_pos) {
        for (int64_t i = a0 + threadIdx.x; i < a1; i += 256) {
            a.atom_pos[3 * i] = a.rec[i].px;
            a.atom_pos[3 * i + 1] = a.rec[i].py;
            a.atom_pos[3 * i + 2] = a.rec[i].pz;
        }
    }
    if ((int)threadIdx.x < T) {
        const int l = (int)threadIdx.x;
        const int32_t *ax = a.axes + ((size_t)b * T + l) * 2;
        double pb[3], u[3];
        const bool ok = record_axis(a.rec, a0, a1 - a0, ax, pb, u);
        sh_ok[l] = ok ? 1 : 0;
        sh_m[l] = ok ? (uint32_t)a.moves[a0 + ax[1]] : 0u;
        if (ok) {
            const double *v = a.subset + ((size_t)b * T + l) * FLEX_SUBSET;
            const double o0 = a.pivots ? a.pivots[3 * b] : 0.0, o1 = a.pivots ? a.pivots[3 * b + 1] : 0.0, o2 = a.pivots ? a.pivots[3 * b + 2] : 0.0;
            const double rb[3] = {pb[0] - o0, pb[1] - o1, pb[2] - o2};
            // s_l = (tau_l, u_l), tau_l = (p_b - o) x u
            const double s[6] = {rb[1] * u[2] - rb[2] * u[1], rb[2] * u[0] - rb[0] * u[2], rb[0] * u[1] - rb[1] * u[0], u[0], u[1], u[2]};
            const double F[3] = {v[0], v[1], v[2]}, N[3] = {v[3], v[4], v[5]};
            double X[6][6];
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int j = i; j < 6; ++j) X[i][j] = X[j][i] = v[twist_slot(i, j)];
            double K[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) K[i][j] = v[TWIST_K_SLOT + 3 * i + j];
            const double trK = (K[0][0] + K[1][1]) + K[2][2];
            // c_l = tau_l x F_l + (K_l - tr(K_l) I) u_l
            const double tF[3] = {s[1] * F[2] - s[2] * F[1], s[2] * F[0] - s[0] * F[2], s[0] * F[1] - s[1] * F[0]};
            double c[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) c[i] = tF[i] + (((K[i][0] * u[0] + K[i][1] * u[1]) + K[i][2] * u[2]) - trK * u[i]);
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                double y = X[i][0] * s[0];
#pragma unroll
                for (int j = 1; j < 6; ++j) y += X[i][j] * s[j];
                sh_s[l][i] = s[i];
                sh_y[l][i] = y;
                sh_z[l][i] = i < 3 ? y : y + c[i - 3]; // H[:6, 6 + l]
            }
#pragma unroll
            for (int i = 0; i < 3; ++i) sh_c[l][i] = c[i];
            sh_g[l] = ((s[0] * F[0] + s[1] * F[1]) + s[2] * F[2]) + ((s[3] * N[0] + s[4] * N[1]) + s[5] * N[2]);
        }
    }
    __syncthreads();
    double *G = a.flex_grad + (size_t)b * n;
    for (int i = (int)threadIdx.x; i < n; i += 256) {
        if (i < 6) G[i] = a.twist_grad[6 * (size_t)b + i];
        else G[i] = sh_ok[i - 6] ? sh_g[i - 6] : 0.0;
    }
    if (!a.flex_hess) return;
    double *H = a.flex_hess + (size_t)b * n * n;
    for (int e = (int)threadIdx.x; e < n * n; e += 256) {
        const int i = e / n, j = e - i * n;
        const int lo = i < j ? i : j, hi = i < j ? j : i; // entry (lo, hi) of the upper triangle, stored at both places
        double v = 0.0;
        if (hi < 6) {
            v = a.twist_hess[36 * (size_t)b + 6 * i + j]; // (symmetric to the bit already)
        } else {
            const int l = hi - 6;
            if (sh_ok[l]) {
                if (lo < 6) {
                    v = sh_z[l][lo];
                } else {
                    const int k = lo - 6;
                    if (sh_ok[k] && ((sh_m[l] >> k) & 1u)) {
                        const double sy = ((sh_s[k][0] * sh_y[l][0] + sh_s[k][1] * sh_y[l][1]) + sh_s[k][2] * sh_y[l][2]) +
                                          ((sh_s[k][3] * sh_y[l][3] + sh_s[k][4] * sh_y[l][4]) + sh_s[k][5] * sh_y[l][5]);
                        const double uc = (sh_s[k][3] * sh_c[l][0] + sh_s[k][4] * sh_c[l][1]) + sh_s[k][5] * sh_c[l][2];
                        v = sy + uc;
                    }
                }
            }
        }
        H[e] = v;
    }
}

__global__ void __launch_bounds__(64) flex_lm_step_kernel(const FlexLmArgs a) {
    // row r at m[r * ld], the right-hand side in column n; ld = n + 1 made odd, so that the lanes of the elimination, one row each,
    // do not meet on a bank (ld <= 39)
    __shared__ double m[FLEX_MAX_N * (FLEX_MAX_N + 1)];
    __shared__ double xs[FLEX_MAX_N];
    const int lane = (int)threadIdx.x;
    const int T = a.T, n = 6 + T, ld = (n + 1) | 1;
    const size_t i = (size_t)blockIdx.x;
    double S = a.S[i], lam = a.lam[i];
    int32_t dropped = a.dropped[i];
    // ---- 1. the decision on the trial (every lane decides alike, lane 0 writes) ----
    bool accept = false;
    if (lm_has_trial(a, dropped)) {
        accept = lm_decide(a, a.S2[i], S, lam, dropped, [] {}); // (nothing is written in the accepting branch: lane 0, below)
        const int32_t taken = a.taken[i] + 1; // (read by every lane, written on an accepted trial)
        __syncthreads(); // every lane has read the state before lane 0 changes it
        if (lane == 0) {
            if (accept) {
                a.S[i] = S;
                a.taken[i] = taken;
            }
            a.lam[i] = lam;
            a.dropped[i] = dropped;
        }
    }
    // the state the step starts from: the accepted trial, copied, or the state as it is
    const double *qs = accept ? a.q2 + 4 * i : a.q + 4 * i;
    const double *ts = accept ? a.t2 + 3 * i : a.t + 3 * i;
    const double *Gs = accept ? a.G2 + (size_t)n * i : a.G + (size_t)n * i;
    const double *Hs = accept ? a.H2 + (size_t)n * n * i : a.H + (size_t)n * n * i;
    double q[4], t[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = qs[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = ts[k];
    // lane j < T holds torsion angle j
    const double th = lane < T ? (accept ? a.theta2[(size_t)T * i + lane] : a.theta[(size_t)T * i + lane]) : 0.0;
    for (int e = lane; e < n * n; e += 64) {
        const int r = e / n, c = e - r * n;
        m[r * ld + c] = Hs[e];
    }
    for (int r = lane; r < n; r += 64) m[r * ld + n] = Gs[r];
    __syncthreads();
    if (accept) {
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k) a.q[4 * i + k] = q[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) a.t[3 * i + k] = t[k];
        }
        if (lane < T) a.theta[(size_t)T * i + lane] = th;
        for (int e = lane; e < n * n; e += 64) {
            const int r = e / n, c = e - r * n;
            a.H[(size_t)n * n * i + e] = m[r * ld + c];
        }
        for (int r = lane; r < n; r += 64) a.G[(size_t)n * i + r] = m[r * ld + n];
    }
    double q2[4] = {q[0], q[1], q[2], q[3]}, t2[3] = {t[0], t[1], t[2]};
    double th2 = th;
    bool step = false; // the solve succeeded: xs holds x
    // ---- 2. a finished pose stays where it is; 3. the step ----
    if (dropped < a.max_dropped) { // (uniform over the wave)
        for (int e = lane; e < n * n; e += 64) {
            const int r = e / n, c = e - r * n;
            m[r * ld + c] = (r == c ? lam : 0.0) - m[r * ld + c];
        }
        __syncthreads();
        bool ok = true;
        for (int k = 0; k < n; ++k) {
            // the pivot: the first row at or below k with the largest |entry| of column k
            double best = fabs(m[k * ld + k]);
            int p = k;
            for (int r = k + 1; r < n; ++r) {
                const double v = fabs(m[r * ld + k]);
                if (v > best) {
                    best = v;
                    p = r;
                }
            }
            __syncthreads(); // column k is read before the exchange writes it
            if (p != k) {
                for (int c = k + lane; c <= n; c += 64) {
                    const double top = m[k * ld + c], low = m[p * ld + c];
                    m[k * ld + c] = low;
                    m[p * ld + c] = top;
                }
            }
            __syncthreads();
            const double piv = m[k * ld + k];
            ok = ok && piv != 0.0;
            for (int r = k + 1 + lane; r < n; r += 64) { // one row per lane
                const double f = m[r * ld + k] / piv;
                for (int c = k + 1; c <= n; ++c) m[r * ld + c] -= f * m[k * ld + c];
            }
            __syncthreads();
        }
        for (int k = n - 1; k >= 0; --k) { // every lane forms the same sum; lane 0 keeps it
            double s = m[k * ld + n];
            for (int c = k + 1; c < n; ++c) s -= m[k * ld + c] * xs[c];
            s = s / m[k * ld + k];
            if (lane == 0) xs[k] = s;
            __syncthreads();
            ok = ok && isfinite(s);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) ok = ok && isfinite(q[k]); // (spelled out: see mvx_newton_device.h)
#pragma unroll
        for (int k = 0; k < 3; ++k) ok = ok && isfinite(t[k]);
        ok = ok && isfinite(lam);
        ok = ok && __all(isfinite(th) ? 1 : 0);
        if (ok) {
            apply_twist(q, t, xs, q2, t2);
            if (lane < T) th2 = th + xs[6 + lane];
#pragma unroll
            for (int k = 0; k < 4; ++k) ok = ok && isfinite(q2[k]);
#pragma unroll
            for (int k = 0; k < 3; ++k) ok = ok && isfinite(t2[k]);
            ok = ok && __all(isfinite(th2) ? 1 : 0);
        }
        if (!ok) {
#pragma unroll
            for (int k = 0; k < 4; ++k) q2[k] = q[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) t2[k] = t[k];
            th2 = th;
        }
        step = ok;
    }
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) a.q2[4 * i + k] = q2[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) a.t2[3 * i + k] = t2[k];
    }
    if (lane < T) a.theta2[(size_t)T * i + lane] = th2;
    if (a.xi) {
        for (int r = lane; r < n; r += 64) a.xi[(size_t)n * i + r] = step ? xs[r] : 0.0;
    }
}

hipError_t launch_torsion_apply(const double *coords, const int64_t *offsets, int32_t B, int32_t T, const int32_t *axes,
                                const int32_t *moves, const double *angles, double *out, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(torsion_apply_kernel, dim3((unsigned)B), dim3(256), 0, s, coords, offsets, T, axes, moves, angles, out);
    return hipGetLastError();
}

hipError_t launch_flex(const FlexArgs &a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.T > 0) {
        hipLaunchKernelGGL(flex_subset_kernel, dim3((unsigned)a.B, (unsigned)a.T), dim3(64 * TWIST_WAVES), 0, s, a);
        if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(flex_assemble_kernel, dim3((unsigned)a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_flex_lm_step(const FlexLmArgs &a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(flex_lm_step_kernel, dim3((unsigned)a.B), dim3(64), 0, s, a);
    return hipGetLastError();
}

} // namespace mvx
