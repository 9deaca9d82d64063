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
// and 0 for unrelated pairs. G[:6] and H[:6, :6] are twist_reduce_kernel's values, copied.
//
//   torsion_apply_kernel  one workgroup per molecule; the positions are worked on in the output array. Per torsion in order: every
//                         thread reads the current axis atoms, a barrier, the atoms of the set are turned (Rodrigues), a barrier.
//                         An angle of exactly 0 and an inert torsion turn nothing: those atoms keep their bits.
//   flex_subset_kernel    grid (B, T), one workgroup (4 waves) per (torsion, molecule) in the shape of twist_reduce_kernel: wave w
//                         takes the chunks w, w + 4, ... of 64 atoms in order, 36 float64 lane partials, a fixed butterfly per
//                         wave, the four waves through sum4. An atom whose g and H rows are all zero is skipped.
//   flex_assemble_kernel  one workgroup per molecule: thread l forms s_l, X_l s_l, c_l and G[6 + l]; then every entry of G and H
//                         is written once, entry (i, j) and (j, i) from the same expression: H is symmetric to the bit.
//   flex_lm_step_kernel   lm_step_kernel's state machine for n = 6 + T, one wave per pose, the n x (n + 1) system in LDS.
//
// A torsion is inert when an axis index is outside [0, N_b) (padding: -1), or the axis has no or no finite length: zero gradient
// entry, zero Hessian row and column; no axis index is used before it is checked. No atomics, no scratch
// (tests/test_flex_host.py pins it), no host read; a molecule's values do not depend on its batch.
#include "mvx_flex.h"
#include "mvx_grad_device.h"

#include <math.h>

namespace mvx {

namespace {

constexpr int FLEX_WAVES = 4;
// where entry (i, j), i <= j, of the 6x6 X sits among the 36 (twist_reduce_kernel's order, behind F and N)
__host__ __device__ constexpr int x_slot(int i, int j) { return 6 + 6 * i - i * (i - 1) / 2 + (j - i); }
constexpr int K_SLOT = 27;

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

__global__ void __launch_bounds__(64 * FLEX_WAVES) flex_subset_kernel(const FlexArgs a) {
    __shared__ double part[FLEX_WAVES][FLEX_SUBSET];
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
    for (int64_t n = a0 + 64 * wave + lane; n < a1; n += 64 * FLEX_WAVES) {
        if (!(((uint32_t)a.moves[n] >> k) & 1u)) continue;
        const double g[3] = {a.atom_grad[3 * n], a.atom_grad[3 * n + 1], a.atom_grad[3 * n + 2]};
        const double hxx = a.atom_hess[6 * n], hxy = a.atom_hess[6 * n + 1], hxz = a.atom_hess[6 * n + 2];
        const double hyy = a.atom_hess[6 * n + 3], hyz = a.atom_hess[6 * n + 4], hzz = a.atom_hess[6 * n + 5];
        // (as twist_reduce_kernel: an atom that reaches no voxel has zero rows, and its position may be NaN)
        if (g[0] == 0.0 && g[1] == 0.0 && g[2] == 0.0 && hxx == 0.0 && hxy == 0.0 && hxz == 0.0 && hyy == 0.0 && hyz == 0.0 && hzz == 0.0)
            continue;
        const double r[3] = {a.rec[n].px - o0, a.rec[n].py - o1, a.rec[n].pz - o2};
        const double H[3][3] = {{hxx, hxy, hxz}, {hxy, hyy, hyz}, {hxz, hyz, hzz}};
        const double A[3][3] = {{0.0, r[2], -r[1]}, {-r[2], 0.0, r[0]}, {r[1], -r[0], 0.0}}; // -[r]x: J = [I | A]
        acc[0] += g[0];
        acc[1] += g[1];
        acc[2] += g[2];
        acc[3] += r[1] * g[2] - r[2] * g[1];
        acc[4] += r[2] * g[0] - r[0] * g[2];
        acc[5] += r[0] * g[1] - r[1] * g[0];
        double HAm[3][3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) HAm[i][j] = (H[i][0] * A[0][j] + H[i][1] * A[1][j]) + H[i][2] * A[2][j];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i; j < 3; ++j) acc[x_slot(i, j)] += H[i][j];
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[x_slot(i, 3 + j)] += HAm[i][j];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int j = i; j < 3; ++j)
                acc[x_slot(3 + i, 3 + j)] += (A[0][i] * HAm[0][j] + A[1][i] * HAm[1][j]) + A[2][i] * HAm[2][j];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[K_SLOT + 3 * i + j] += r[i] * g[j];
    }
#pragma unroll
    for (int i = 0; i < FLEX_SUBSET; ++i) {
        const double v = wave_sum(acc[i]);
        if (lane == 0) part[wave][i] = v;
    }
    __syncthreads();
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
                for (int j = i; j < 6; ++j) X[i][j] = X[j][i] = v[x_slot(i, j)];
            double K[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) K[i][j] = v[K_SLOT + 3 * i + j];
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
    if (a.have_trial && dropped < a.max_dropped) {
        const double S2 = a.S2[i];
        accept = S2 > S; // (a NaN compares false: a non-finite trial is dropped)
        int32_t taken = a.taken[i];
        if (accept) {
            S = S2;
            lam *= a.lam_down;
            dropped = 0;
            taken += 1;
        } else {
            lam *= a.lam_up;
            dropped += 1;
        }
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
        for (int k = 0; k < 4; ++k) ok = ok && isfinite(q[k]);
#pragma unroll
        for (int k = 0; k < 3; ++k) ok = ok && isfinite(t[k]);
        ok = ok && isfinite(lam);
        ok = ok && __all(isfinite(th) ? 1 : 0);
        if (ok) {
            const double wx = xs[3], wy = xs[4], wz = xs[5];
            const double half = 0.5 * sqrt(wx * wx + wy * wy + wz * wz);
            if (half != 0.0) { // (w = 0: u = (1, 0, 0, 0), the quaternion itself)
                const double u0 = cos(half), f = 0.5 * (sin(half) / half);
                const double u1 = f * wx, u2 = f * wy, u3 = f * wz;
                q2[0] = u0 * q[0] - u1 * q[1] - u2 * q[2] - u3 * q[3];
                q2[1] = u0 * q[1] + u1 * q[0] + u2 * q[3] - u3 * q[2];
                q2[2] = u0 * q[2] - u1 * q[3] + u2 * q[0] + u3 * q[1];
                q2[3] = u0 * q[3] + u1 * q[2] - u2 * q[1] + u3 * q[0];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) t2[k] = t[k] + xs[k];
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
    if (a.x) {
        for (int r = lane; r < n; r += 64) a.x[(size_t)n * i + r] = step ? xs[r] : 0.0;
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
        hipLaunchKernelGGL(flex_subset_kernel, dim3((unsigned)a.B, (unsigned)a.T), dim3(64 * FLEX_WAVES), 0, s, a);
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
