// mvx_hess.hip - second-order information of the scores against a constant field (mvx_score_hessian_batch): per atom the
// gradient and the 3x3 Hessian of S_b with respect to the atom's position, per molecule the gradient and the 6x6 Hessian under a
// rigid twist. Everything in the grid frame (the records' positions): no rotation is transposed onto any row.
//
// S_b = sum_{n in b} s_n(p_n), so the Hessian with respect to the positions is block diagonal, one symmetric 3x3 block per atom
// over the voxels the gradient walk visits. With d = p_n - voxel centre, u = sum_c F[c,v] w[n,c], rho the density (d rho / d p =
// kfac rho d) and e = (double)(u rho) kfac, the admitted set held fixed:
//   s_n = sum_v (double)(u rho)      g_n = sum_v e d      H_n = (sum_v e) I + kfac sum_v e d d^T
//
//   score_hess_kernel    one wave per atom record, launch_walk's grid, order and xcd_span. A body of its own beside
//                        mvx_grad_body.inc (no acc[32], no grad_w, no channel-wise radii): eleven float64 lane partials - sp,
//                        cp0..2 in the operation order of that body, so s_n and g_n are score_kernel's bits; E = sum e and the
//                        six Q = sum e d_i d_j -, one fixed butterfly each, lane 0 writes the rows. Features: chunks of 32
//                        channels with all 32 loads in flight before the first use. No atomics, no LDS, no scratch.
//   twist_reduce_kernel  one workgroup (4 waves) per molecule, in the shape of pose_grad_kernel: wave w takes the chunks w, w + 4,
//                        ... of 64 atoms in order, each lane keeps 6 + 21 double partials (G and the upper triangle of Hxi); a
//                        fixed butterfly per wave, the four waves in a fixed order through LDS; thread 0 writes G and the full
//                        symmetric Hxi. One atom's terms, the rule for an atom without rows and the hand-over of the partials
//                        are mvx_newton_device.h's, with the K term folded into the angular block.
#include "mvx_grad_device.h"
#include "mvx_hess.h"
#include "mvx_newton_device.h"

namespace mvx {

template <typename GT, int MODE, bool GAUSS>
__global__ void __launch_bounds__(256) score_hess_kernel(GradArgs A, HessArgs HA) {
    typedef typename GradReal<GT>::type real;
    constexpr bool F64 = std::is_same<real, double>::value;
    constexpr bool FEAT = MODE == MODE_FEATURES;
    const int lane = threadIdx.x & 63;
    // (launch_walk's grid: with `xcd_span` each XCD walks one contiguous range of the order, as in mvx_grad_body.inc)
    const unsigned blk = A.xcd_span ? (blockIdx.x & 7u) * (unsigned)A.xcd_span + (blockIdx.x >> 3) : blockIdx.x;
    const int64_t i = (int64_t)blk * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (wave-uniform)
    if (i >= A.total) return;
    const int64_t a = A.order ? (int64_t)A.order[i] : i;
    const AtomRec &R = A.rec[a];
    const double px = R.px, py = R.py, pz = R.pz, T = R.T;
    const uint32_t xr = R.xr, yr = R.yr, zr = R.zr;
    const int xlo = (int)(xr & 0xffff), ylo = (int)(yr & 0xffff), zlo = (int)(zr & 0xffff);
    const int nx = (int)(xr >> 16) - xlo + 1, ny = (int)(yr >> 16) - ylo + 1, nz = (int)(zr >> 16) - zlo + 1;
    const int nbox = (nx > 0 && ny > 0 && nz > 0) ? nx * ny * nz : 0; // (EMPTY_RANGE: nothing admitted)
    double kfac; // d rho / d d2 = kfac / 2 * rho
    float k32 = 0.0f;
    double c64 = 0.0;
    if constexpr (F64) {
        __builtin_memcpy(&c64, &R.pad[1], 8);
        kfac = 2.0 * c64;
    } else {
        k32 = R.k;
        kfac = 2.0 * LN2 * (double)k32;
    }
    const int bm = A.B > 1 ? find_molecule(A.offsets, A.B, a) : 0; // this atom's molecule
    const int D = A.D;
    const size_t D3 = (size_t)D * D * D;
    const GT *gm = static_cast<const GT *>(A.g) + (size_t)bm * (size_t)HA.mol_stride; // (stride 0: the one field)

    auto voxel = [&](int v, double &dx, double &dy, double &dz, size_t &off) {
        const int iz = v % nz, t = v / nz, iy = t % ny, ix = t / ny;
        const int gi = xlo + ix, gj = ylo + iy, gk = zlo + iz;
        dx = px - ((double)gi * A.res - A.half); // the forward's voxel centre and cdist operands
        dy = py - ((double)gj * A.res - A.half);
        dz = pz - ((double)gk * A.res - A.half);
        off = ((size_t)gi * D + gj) * D + gk;
    };
    auto density = [&](double d2, bool in) -> real {
        if (!(in && d2 <= T)) return (real)0;
        if constexpr (!GAUSS) return (real)1;
        if constexpr (F64) return exp(c64 * d2);
        else return __builtin_amdgcn_exp2f(k32 * (float)d2);
    };

    double sp = 0.0;                        // this lane's share of s_n
    double cp0 = 0.0, cp1 = 0.0, cp2 = 0.0; // ... of g_n
    double E = 0.0;                         // ... of sum_v e
    double q00 = 0.0, q01 = 0.0, q02 = 0.0, q11 = 0.0, q12 = 0.0, q22 = 0.0; // ... of sum_v e d d^T
    // one admitted voxel's terms from the product u rho; cp* as mvx_grad_body.inc forms them
    auto add = [&](real ur, double dx, double dy, double dz) {
        if constexpr (GAUSS) {
            const double e = (double)ur * kfac;
            const double ex = e * dx, ey = e * dy, ez = e * dz;
            cp0 += ex;
            cp1 += ey;
            cp2 += ez;
            E += e;
            q00 += ex * dx;
            q01 += ex * dy;
            q02 += ex * dz;
            q11 += ey * dy;
            q12 += ey * dz;
            q22 += ez * dz;
        }
        sp += (double)ur;
    };
    if constexpr (!FEAT) {
        const int ch = MODE == MODE_TYPES ? R.type : 0; // (an atom of type >= C has no admitted box)
        const GT *gc = gm + (size_t)(ch < A.C ? ch : 0) * D3;
        for (int v0 = 0; v0 < nbox; v0 += 64) { // (binary density has no derivatives, but it scores)
            const int v = v0 + lane;
            double dx, dy, dz;
            size_t off;
            voxel(v < nbox ? v : 0, dx, dy, dz, off);
            const double d2 = (dx * dx + dy * dy) + dz * dz; // cdist order, no fma
            const real rho = density(d2, v < nbox);
            if (rho != (real)0) add(load_grad(gc + off) * rho, dx, dy, dz);
        }
    } else {
        const real *wrow = static_cast<const real *>(A.w) + (size_t)a * A.C;
        for (int c0 = 0; c0 < A.C; c0 += 32) { // chunks of 32 channels: the box is walked once per chunk
            const int nc = A.C - c0 < 32 ? A.C - c0 : 32;
            for (int v0 = 0; v0 < nbox; v0 += 64) {
                const int v = v0 + lane;
                double dx, dy, dz;
                size_t off;
                voxel(v < nbox ? v : 0, dx, dy, dz, off);
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                // (per channel a uniform base and one 32-bit byte offset for all channels: the entry checks D^3 fits)
                const uint32_t boff = (uint32_t)off * (uint32_t)sizeof(GT);
                const real rho = density(d2, v < nbox);
                if (rho != (real)0) {
                    // all 32 loads in flight before the first use: the walk is bound by the latency of these round trips
                    real gv[32];
#pragma unroll
                    for (int c = 0; c < 32; ++c)
                        gv[c] = c < nc ? load_grad(reinterpret_cast<const GT *>(reinterpret_cast<const char *>(gm + (size_t)(c0 + c) * D3) + boff))
                                       : (real)0;
                    real s = (real)0; // sum_c F w
#pragma unroll
                    for (int c = 0; c < 32; ++c)
                        if (c < nc) s = fma(gv[c], wrow[c0 + c], s);
                    add(s * rho, dx, dy, dz);
                }
            }
        }
    }
    const double S = wave_sum(sp);
    const double g0 = wave_sum(cp0), g1 = wave_sum(cp1), g2 = wave_sum(cp2);
    const double e = wave_sum(E);
    const double Q[6] = {wave_sum(q00), wave_sum(q01), wave_sum(q02), wave_sum(q11), wave_sum(q12), wave_sum(q22)};
    if (lane != 0) return;
    // an atom without admitted voxels gets exact zeros whatever its radius (kfac of a radius 0 is not finite: 0 * kfac)
    auto kq = [&](double q) { return q != 0.0 ? kfac * q : 0.0; };
    HA.atom_scores[a] = S;
    double *g = HA.atom_grad + 3 * a, *H = HA.atom_hess + 6 * a;
    g[0] = g0;
    g[1] = g1;
    g[2] = g2;
    H[0] = e + kq(Q[0]);
    H[1] = kq(Q[1]);
    H[2] = kq(Q[2]);
    H[3] = e + kq(Q[3]);
    H[4] = kq(Q[4]);
    H[5] = e + kq(Q[5]);
}

__global__ void __launch_bounds__(64 * TWIST_WAVES) twist_reduce_kernel(const AtomRec *__restrict__ rec, const double *__restrict__ atom_grad,
                                                                        const double *__restrict__ atom_hess,
                                                                        const int64_t *__restrict__ offsets,
                                                                        const double *__restrict__ pivots, double *__restrict__ twist_grad,
                                                                        double *__restrict__ twist_hess) {
    __shared__ double part[TWIST_WAVES][TWIST_VALUES];
    const int b = (int)blockIdx.x;
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t a0 = offsets[b], a1 = offsets[b + 1];
    const double o0 = pivots ? pivots[3 * b] : 0.0, o1 = pivots ? pivots[3 * b + 1] : 0.0, o2 = pivots ? pivots[3 * b + 2] : 0.0;
    double acc[TWIST_VALUES];
#pragma unroll
    for (int i = 0; i < TWIST_VALUES; ++i) acc[i] = 0.0;
    for (int64_t a = a0 + 64 * wave + lane; a < a1; a += 64 * TWIST_WAVES) {
        const double g[3] = {atom_grad[3 * a], atom_grad[3 * a + 1], atom_grad[3 * a + 2]};
        const double h[6] = {atom_hess[6 * a],     atom_hess[6 * a + 1], atom_hess[6 * a + 2],
                             atom_hess[6 * a + 3], atom_hess[6 * a + 4], atom_hess[6 * a + 5]};
        if (twist_rows_zero(g, h)) continue;
        const double r[3] = {rec[a].px - o0, rec[a].py - o1, rec[a].pz - o2};
        twist_accumulate<false>(g, h, r, acc);
    }
    twist_wave_partials(acc, part, lane, wave);
    if (threadIdx.x != 0) return;
    double t[TWIST_VALUES]; // (no atoms: exact zeros)
#pragma unroll
    for (int i = 0; i < TWIST_VALUES; ++i) t[i] = sum4(part[0][i], part[1][i], part[2][i], part[3][i]);
    double *G = twist_grad + 6 * (size_t)b;
#pragma unroll
    for (int i = 0; i < 6; ++i) G[i] = t[i];
    if (!twist_hess) return;
    double *X = twist_hess + 36 * (size_t)b;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) X[6 * i + j] = X[6 * j + i] = t[twist_slot(i, j)];
    }
}

hipError_t launch_score_hess(const GradArgs &a, const HessArgs &ha, const WalkKey &key, hipStream_t s) {
    return for_walk(key, [&](auto gt, auto mode, auto gauss, auto chanwise) {
        if constexpr (chanwise) return hipErrorInvalidValue;
        else return launch_walk(score_hess_kernel<typename decltype(gt)::type, mode, gauss>, a, s, ha);
    });
}

hipError_t launch_twist_reduce(const AtomRec *rec, const double *atom_grad, const double *atom_hess, const int64_t *offsets,
                               const double *pivots, int32_t B, double *twist_grad, double *twist_hess, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    hipLaunchKernelGGL(twist_reduce_kernel, dim3((unsigned)B), dim3(64 * TWIST_WAVES), 0, s, rec, atom_grad, atom_hess, offsets, pivots,
                       twist_grad, twist_hess);
    return hipGetLastError();
}

} // namespace mvx
