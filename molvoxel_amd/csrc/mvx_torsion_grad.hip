// mvx_torsion_grad.hip - the adjoint of torsion_apply_kernel (gfx950, float64 throughout; mvx_apply_torsions_backward; DESIGN.md
// section 29): from the conformer C(theta) the forward returned and ybar = dL/dC to dL/dcoords and dL/dtheta. The forward is a
// program of T dependent turns; the backward runs it in reverse, k = T-1 .. 0, undoing turn k on working positions while it
// pulls the gradient rows back through it. With c = cos theta_k, s = sin theta_k, R = c I + s [u]x + (1 - c) u u^T about the unit
// axis u from p_a to p_b, for every atom n of the set M_k, w = y_n - p_b:
//   v = R^T w                                  (the turn undone: the working position becomes p_b + v)
//   theta_bar_k += ybar_n . (u x w)
//   xbar_n       = R^T ybar_n                  (replaces the row)
//   b_bar       += ybar_n - R^T ybar_n
//   u_bar       += s (v x ybar_n) + (1 - c) ((u . v) ybar_n + (u . ybar_n) v)
// and behind the sums d_bar = (u_bar - u (u . u_bar)) / |p_b - p_a|, xbar_b += b_bar + d_bar, xbar_a -= d_bar.
//
//   torsion_backward_kernel  one workgroup (4 waves) per molecule. The positions are worked on in `pos` (workspace), the rows in
//                            grad_coords; neither the caller's conformer nor - unless it is grad_coords - grad_out is written.
//                            Per torsion, last first: every thread reads the current axis atoms, a barrier, thread i takes the
//                            atoms i, i + 256, ... of the set, seven float64 lane partials (theta_bar, b_bar, u_bar), a fixed
//                            butterfly per wave, the four waves through sum4, thread 0 writes grad_angles[b, k] and the two axis
//                            rows, a barrier.
//
// Under the tree rules (include/mvx.h) a_k is in no set that turns at or after k and b_k is a fixed point of turn k, so the axis
// read here is the axis the forward turned about, bit for bit. Outside the rules the kernel stays inside its arrays and its values
// are unspecified. An angle of exactly 0 moves neither positions nor rows - R = I, b_bar and u_bar are exact zeros, nothing is added
// to the axis rows - and theta_bar_k is the derivative all the same. An inert torsion (an axis index outside [0, N_b), an axis with
// no or no finite length) gets grad_angles[b, k] = +0.0 and touches nothing else; no axis index is used before it is checked. An
// atom whose current row is all zero is left out of the sums and keeps its row (its position may be NaN or infinite: the rule of
// twist_rows_zero); for a finite position the terms left out are +-0 added to sums that start at +0: no bit changes. Its working
// position is still turned back. No atomics, no scratch, no host read; a molecule's values do not depend on its batch.
#include "mvx_torsion_grad.h"
#include "mvx_flex_device.h"
#include "mvx_newton_device.h"

#include <math.h>

namespace mvx {

namespace {

constexpr int TORSION_SUMS = 7; // theta_bar, b_bar (3), u_bar (3)

} // namespace

__global__ void __launch_bounds__(64 * TWIST_WAVES) torsion_backward_kernel(const double *__restrict__ conformer,
                                                                            const int64_t *__restrict__ offsets, int32_t T,
                                                                            const int32_t *__restrict__ axes,
                                                                            const int32_t *__restrict__ moves,
                                                                            const double *__restrict__ angles, const double *grad_out,
                                                                            double *__restrict__ pos, double *grad_coords,
                                                                            double *__restrict__ grad_angles) {
    __shared__ double part[TWIST_WAVES][TORSION_SUMS];
    const int b = (int)blockIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t a0 = offsets[b], N = offsets[b + 1] - a0;
    for (int64_t n = threadIdx.x; n < N; n += 256) { // (bit for bit; grad_out == grad_coords: every element onto itself)
        const int64_t a = a0 + n;
        const double x = conformer[3 * a], y = conformer[3 * a + 1], z = conformer[3 * a + 2];
        const double g0 = grad_out[3 * a], g1 = grad_out[3 * a + 1], g2 = grad_out[3 * a + 2];
        pos[3 * a] = x;
        pos[3 * a + 1] = y;
        pos[3 * a + 2] = z;
        grad_coords[3 * a] = g0;
        grad_coords[3 * a + 1] = g1;
        grad_coords[3 * a + 2] = g2;
    }
    __syncthreads();
    for (int k = T - 1; k >= 0; --k) {
        // (every thread reads the same values: the branches below are uniform over the workgroup)
        const int32_t *ax = axes + ((size_t)b * T + k) * 2;
        const int64_t ia = ax[0], ib = ax[1];
        const double th = angles[(size_t)b * T + k];
        bool live = ia >= 0 && ia < N && ib >= 0 && ib < N;
        double pb[3] = {0.0, 0.0, 0.0}, u[3] = {0.0, 0.0, 0.0}, len = 1.0;
        if (live) {
            const double *A = pos + 3 * (a0 + ia), *Bq = pos + 3 * (a0 + ib);
            const double pa[3] = {A[0], A[1], A[2]};
            pb[0] = Bq[0];
            pb[1] = Bq[1];
            pb[2] = Bq[2];
            live = unit_axis(pa, pb, u);
            const double d0 = pb[0] - pa[0], d1 = pb[1] - pa[1], d2 = pb[2] - pa[2];
            len = sqrt((d0 * d0 + d1 * d1) + d2 * d2); // (unit_axis's own length)
        }
        __syncthreads(); // the axis is read before any atom of the set is turned back (b_k is one of them)
        if (!live) {
            if (threadIdx.x == 0) grad_angles[(size_t)b * T + k] = 0.0;
            continue;
        }
        const bool turn = th != 0.0;
        const double c = cos(th), s = sin(th), c1 = 1.0 - c;
        double acc[TORSION_SUMS];
#pragma unroll
        for (int i = 0; i < TORSION_SUMS; ++i) acc[i] = 0.0;
        for (int64_t n = threadIdx.x; n < N; n += 256) {
            const int64_t a = a0 + n;
            if (!(((uint32_t)moves[a] >> k) & 1u)) continue;
            const double w[3] = {pos[3 * a] - pb[0], pos[3 * a + 1] - pb[1], pos[3 * a + 2] - pb[2]};
            const double uw[3] = {u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]}; // u x w
            double v[3] = {w[0], w[1], w[2]};
            if (turn) { // v = R^T w
                const double ud = ((u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]) * c1;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    v[i] = (w[i] * c - uw[i] * s) + u[i] * ud;
                    pos[3 * a + i] = pb[i] + v[i];
                }
            }
            const double y[3] = {grad_coords[3 * a], grad_coords[3 * a + 1], grad_coords[3 * a + 2]};
            if (y[0] == 0.0 && y[1] == 0.0 && y[2] == 0.0) continue; // (no row: twist_rows_zero's rule)
            acc[0] += (y[0] * uw[0] + y[1] * uw[1]) + y[2] * uw[2];
            if (turn) {
                const double uy[3] = {u[1] * y[2] - u[2] * y[1], u[2] * y[0] - u[0] * y[2], u[0] * y[1] - u[1] * y[0]}; // u x ybar
                const double udy = (u[0] * y[0] + u[1] * y[1]) + u[2] * y[2], udv = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
                const double yd = udy * c1;
                const double vy[3] = {v[1] * y[2] - v[2] * y[1], v[2] * y[0] - v[0] * y[2], v[0] * y[1] - v[1] * y[0]}; // v x ybar
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double x = (y[i] * c - uy[i] * s) + u[i] * yd; // R^T ybar
                    grad_coords[3 * a + i] = x;
                    acc[1 + i] += y[i] - x;
                    acc[4 + i] += vy[i] * s + (udv * y[i] + udy * v[i]) * c1;
                }
            }
        }
        twist_wave_partials(acc, part, lane, wave); // (its barrier: the rows of the set are written before thread 0 adds to two)
        if (threadIdx.x == 0) {
            double sum[TORSION_SUMS];
#pragma unroll
            for (int i = 0; i < TORSION_SUMS; ++i) sum[i] = sum4(part[0][i], part[1][i], part[2][i], part[3][i]);
            grad_angles[(size_t)b * T + k] = sum[0];
            if (turn) {
                const double uu = (u[0] * sum[4] + u[1] * sum[5]) + u[2] * sum[6];
                double *ga = grad_coords + 3 * (a0 + ia), *gb = grad_coords + 3 * (a0 + ib);
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const double d = (sum[4 + i] - u[i] * uu) / len; // d_bar
                    gb[i] += sum[1 + i] + d;
                    ga[i] -= d;
                }
            }
        }
        __syncthreads(); // the axis rows and `part` are settled before the next torsion
    }
}

hipError_t launch_torsion_backward(const double *conformer, const int64_t *offsets, int32_t B, int32_t T, const int32_t *axes,
                                   const int32_t *moves, const double *angles, const double *grad_out, double *pos, double *grad_coords,
                                   double *grad_angles, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(torsion_backward_kernel, dim3((unsigned)B), dim3(64 * TWIST_WAVES), 0, s, conformer, offsets, T, axes, moves,
                       angles, grad_out, pos, grad_coords, grad_angles);
    return hipGetLastError();
}

} // namespace mvx
