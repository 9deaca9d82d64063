// mvx_grad_body.inc - the body of the gradient walk, included by grad_kernel (mvx_grad.hip, RADII = false), by its twin
// grad_radii_kernel (mvx_grad_radii.hip, RADII = true), by score_kernel (mvx_score.hip, SCORE = true) and by moments_grad_kernel
// (mvx_moments_grad.hip, MOMENTS = true): one text, four kernels whose names stay apart and whose coordinate and feature
// gradients are the same bits for the same upstream; for_walk and for_moments_walk (mvx_grad.h) name their instantiations and
// launch_walk (mvx_grad_device.h) launches each of them. Expects the kernel parameters A (GradArgs), RA (RadiiArgs),
// SA (ScoreArgs) and MA (MomentsArgs), the template parameters GT, MODE, GAUSS, CHANWISE and the constexpr bools RADII, SCORE,
// MOMENTS and TARGET. With MOMENTS, A.g holds the float32 grids g of the call's molecules and the upstream of voxel v in
// channel c is formed here, in float32: u = fmaf(a1, g[c,v], fmaf(a2, t[c,v], a0)) - without TARGET fmaf(a1, g[c,v], a0) -
// from the three coefficients MA.coef keeps per (molecule, channel) and the target MA.target (one per molecule, or one for all:
// MA.mol_stride). With SCORE, A.g is a constant field F (one per molecule, or one for all: SA.mol_stride) and the walk also
// forms the atom's score s_n = sum_v sum_c F[c,v] w[n,c] rho_{n,c}(v) - e without kfac - in float64 from the float32 products
// of the coordinate path, for binary density too. With RADII the walk also forms the radius partials
// (kfac: dk/dr = -2k/r, so d rho / d r = -(kfac / r) d2 rho):
//   one radius per atom       rp = sum_v e(v) d2(v), e as for the coordinates; dL/dr_n = -rp / r_n, or rp alone into RA.part
//                             (types mode, radii by type: grad_radii_reduce sums it per type and scales by -1/r_c)
//   channel-wise (features)   per chunk of 32 channels a second walk of the box: sum_v G[c,v] w[n,c] rho_{n,c}(v) d2(v) into
//                             RA.part[c * total + n] (grad_radii_reduce: sum over n, times -(kfac_c / r_c))
    typedef typename GradReal<GT>::type real;
    constexpr bool F64 = std::is_same<real, double>::value;
    constexpr bool FEAT = MODE == MODE_FEATURES;
    const int lane = threadIdx.x & 63;
    // Workgroups reach the XCDs round robin (workgroup i on XCD i % 8): with `xcd_span` each XCD walks one contiguous
    // range of the order, so atoms that are neighbours in it share that XCD's L2
    const unsigned blk = A.xcd_span ? (blockIdx.x & 7u) * (unsigned)A.xcd_span + (blockIdx.x >> 3) : blockIdx.x;
    const int64_t i = (int64_t)blk * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6); // (wave-uniform)
    if (i >= A.total) return;
    const int64_t a = A.order ? (int64_t)A.order[i] : i; // (the order changes which wave runs an atom, not its result)
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
    const GT *gm = static_cast<const GT *>(A.g) + (size_t)bm * A.C * D3; // this molecule's G
    if constexpr (SCORE) gm = static_cast<const GT *>(A.g) + (size_t)bm * (size_t)SA.mol_stride; // (stride 0: the one field)

    auto voxel = [&](int v, double &dx, double &dy, double &dz, size_t &off) {
        const int iz = v % nz, t = v / nz, iy = t % ny, ix = t / ny;
        const int gi = xlo + ix, gj = ylo + iy, gk = zlo + iz;
        dx = px - ((double)gi * A.res - A.half); // the forward's voxel centre (make_lane_ctx) and cdist operands
        dy = py - ((double)gj * A.res - A.half);
        dz = pz - ((double)gk * A.res - A.half);
        off = ((size_t)gi * D + gj) * D + gk;
    };
    auto density = [&](double d2, double Tv, float kv32, double kv64, bool in) -> real {
        if (!(in && d2 <= Tv)) return (real)0;
        if constexpr (!GAUSS) return (real)1;
        if constexpr (F64) return exp(kv64 * d2);
        else return __builtin_amdgcn_exp2f(kv32 * (float)d2);
    };

    double cp0 = 0.0, cp1 = 0.0, cp2 = 0.0; // this lane's coordinate partials
    double rp = 0.0;                        // RADII, one radius per atom: this lane's sum of e d2
    double sp = 0.0;                        // SCORE: this lane's share of s_n
    if constexpr (!FEAT) {
        const int ch = MODE == MODE_TYPES ? R.type : 0; // (an atom of type >= C has no admitted box)
        const GT *gc = gm + (size_t)(ch < A.C ? ch : 0) * D3;
        // the upstream at a voxel of this atom's channel; MOMENTS: formed from g, the target and the channel's coefficients
        const float *mc = nullptr, *tc = nullptr;
        if constexpr (MOMENTS) {
            mc = MA.coef + ((size_t)bm * A.C + (size_t)(ch < A.C ? ch : 0)) * 3;
            if constexpr (TARGET) tc = MA.target + (size_t)bm * (size_t)MA.mol_stride + (size_t)(ch < A.C ? ch : 0) * D3;
        }
        auto upstream = [&](size_t off) -> real {
            if constexpr (MOMENTS) {
                if constexpr (TARGET) return __builtin_fmaf(mc[1], load_grad(gc + off), __builtin_fmaf(mc[2], tc[off], mc[0]));
                else return __builtin_fmaf(mc[1], load_grad(gc + off), mc[0]);
            } else {
                return load_grad(gc + off);
            }
        };
        if (GAUSS || SCORE) { // (binary density has no coordinate gradient, but it scores)
            for (int v0 = 0; v0 < nbox; v0 += 64) {
                const int v = v0 + lane;
                double dx, dy, dz;
                size_t off;
                voxel(v < nbox ? v : 0, dx, dy, dz, off);
                const double d2 = (dx * dx + dy * dy) + dz * dz; // cdist order, no fma
                const real rho = density(d2, T, k32, c64, v < nbox);
                if (rho != (real)0) { // (binary density: no coordinate gradient, nothing to read)
                    if constexpr (GAUSS) {
                        const double e = (double)(upstream(off) * rho) * kfac;
                        cp0 += e * dx;
                        cp1 += e * dy;
                        cp2 += e * dz;
                        if constexpr (RADII) rp += e * d2;
                    }
                    if constexpr (SCORE) sp += (double)(upstream(off) * rho);
                }
            }
        }
    } else {
        const real *wrow = static_cast<const real *>(A.w) + (size_t)a * A.C;
        real *gw = static_cast<real *>(A.grad_w);
        for (int c0 = 0; c0 < A.C; c0 += 32) { // chunks of 32 channels: the box is walked once per chunk
            real acc[32];
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = (real)0;
            const int nc = A.C - c0 < 32 ? A.C - c0 : 32;
            for (int v0 = 0; v0 < nbox; v0 += 64) {
                const int v = v0 + lane;
                double dx, dy, dz;
                size_t off;
                voxel(v < nbox ? v : 0, dx, dy, dz, off);
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                // (per channel a uniform base and one 32-bit byte offset for all channels: launch_grad checks D^3 fits)
                const uint32_t boff = (uint32_t)off * (uint32_t)sizeof(GT);
                auto gload = [&](int c) {
                    return load_grad(reinterpret_cast<const GT *>(reinterpret_cast<const char *>(gm + (size_t)(c0 + c) * D3) + boff));
                };
                if constexpr (!CHANWISE) {
                    const real rho = density(d2, T, k32, c64, v < nbox);
                    if (rho != (real)0) {
                        real s = (real)0; // sum_c G w
                        // all 32 loads in flight before the first use: the kernel is bound by the latency of these
                        // round trips (groups of eight, one after the other, cost the same registers and 4x the waits)
                        real gv[32];
                        if constexpr (MOMENTS) {
                            // the grids' values and, with a target, its values: up to 64 loads in flight, then u in their place
                            real tv[TARGET ? 32 : 1];
#pragma unroll
                            for (int c = 0; c < 32; ++c) gv[c] = c < nc ? gload(c) : (real)0;
                            if constexpr (TARGET) {
                                // (this molecule's target: a wave-uniform base, as gm is - stride 0: the one shared target)
                                const float *tm = MA.target + (size_t)bm * (size_t)MA.mol_stride;
#pragma unroll
                                for (int c = 0; c < 32; ++c)
                                    tv[c] = c < nc ? *reinterpret_cast<const float *>(reinterpret_cast<const char *>(tm + (size_t)(c0 + c) * D3) + boff) : 0.0f;
                            }
                            const float *mc = MA.coef + ((size_t)bm * A.C + (size_t)c0) * 3;
#pragma unroll
                            for (int c = 0; c < 32; ++c) {
                                if (c < nc) {
                                    if constexpr (TARGET) gv[c] = __builtin_fmaf(mc[3 * c + 1], gv[c], __builtin_fmaf(mc[3 * c + 2], tv[c], mc[3 * c]));
                                    else gv[c] = __builtin_fmaf(mc[3 * c + 1], gv[c], mc[3 * c]);
                                }
                            }
                        } else {
#pragma unroll
                            for (int c = 0; c < 32; ++c) gv[c] = c < nc ? gload(c) : (real)0;
                        }
#pragma unroll
                        for (int c = 0; c < 32; ++c) {
                            if (c < nc) {
                                acc[c] = fma(gv[c], rho, acc[c]);
                                s = fma(gv[c], wrow[c0 + c], s);
                            }
                        }
                        if constexpr (GAUSS) {
                            const double e = (double)(s * rho) * kfac;
                            cp0 += e * dx;
                            cp1 += e * dy;
                            cp2 += e * dz;
                            if constexpr (RADII) rp += e * d2;
                        }
                        if constexpr (SCORE) sp += (double)(s * rho);
                    }
                } else { // per channel: its own threshold and coefficient, the box of the largest radius
                    const real *kcr = static_cast<const real *>(A.kc);
                    if (v < nbox && d2 <= T) { // (T: the record's threshold of the largest radius: a superset)
                        double e = 0.0;
#pragma unroll
                        for (int c = 0; c < 32; ++c) {
                            if (c < nc) {
                                const int ch = c0 + c;
                                const real kv = kcr[ch];
                                const real rho = density(d2, A.Tc[ch], (float)kv, (double)kv, true);
                                if (rho != (real)0) {
                                    const real gv = gload(c);
                                    acc[c] = fma(gv, rho, acc[c]);
                                    if constexpr (GAUSS) e += (double)(gv * wrow[ch] * rho) * (F64 ? 2.0 : 2.0 * LN2) * (double)kv;
                                    if constexpr (SCORE) sp += (double)(gv * wrow[ch] * rho);
                                }
                            }
                        }
                        cp0 += e * dx;
                        cp1 += e * dy;
                        cp2 += e * dz;
                    }
                }
            }
            const real sum = wave_sum32(acc, lane);
            const int ch = c0 + (lane >> 1);
            if (gw && !(lane & 1) && ch < A.C) gw[(size_t)a * A.C + ch] = sum;
            if constexpr (RADII && CHANWISE && GAUSS) {
                // the per-channel radius partials sum_v G[c,v] w[n,c] rho_{n,c}(v) d2 of this chunk: a second walk of the box
                // (32 more accumulators beside acc would spill), the same voxels, thresholds and densities as the first
                const real *kcr = static_cast<const real *>(A.kc);
                double racc[32];
#pragma unroll
                for (int c = 0; c < 32; ++c) racc[c] = 0.0;
                for (int v0 = 0; v0 < nbox; v0 += 64) {
                    const int v = v0 + lane;
                    double dx, dy, dz;
                    size_t off;
                    voxel(v < nbox ? v : 0, dx, dy, dz, off);
                    const double d2 = (dx * dx + dy * dy) + dz * dz;
                    const uint32_t boff = (uint32_t)off * (uint32_t)sizeof(GT);
                    if (v < nbox && d2 <= T) {
#pragma unroll
                        for (int c = 0; c < 32; ++c) {
                            if (c < nc) {
                                const int cc = c0 + c;
                                const real kv = kcr[cc];
                                const real rho = density(d2, A.Tc[cc], (float)kv, (double)kv, true);
                                if (rho != (real)0) {
                                    const real gv = load_grad(
                                        reinterpret_cast<const GT *>(reinterpret_cast<const char *>(gm + (size_t)cc * D3) + boff));
                                    racc[c] += (double)(gv * wrow[cc] * rho) * d2;
                                }
                            }
                        }
                    }
                }
                const double rsum = wave_sum32_regs(racc, lane);
                if (!(lane & 1) && ch < A.C) RA.part[(size_t)ch * A.total + a] = rsum; // (channel-major: the reduction reads rows)
            }
        }
    }
    if (A.grad_coords) {
        double g0 = wave_sum(cp0), g1 = wave_sum(cp1), g2 = wave_sum(cp2);
        if (A.xforms) apply_xform_transpose(A.xforms[bm], g0, g1, g2);
        // an atom without admitted voxels has a zero row whatever its molecule's pose: M^T 0 is NaN under a non-finite quaternion.
        // Under a finite one it is +-0, which passes the compares: no bit changes.
        if (nbox == 0 && !(g0 == g0 && g1 == g1 && g2 == g2)) g0 = g1 = g2 = 0.0;
        if (lane == 0) {
            A.grad_coords[3 * a] = g0;
            A.grad_coords[3 * a + 1] = g1;
            A.grad_coords[3 * a + 2] = g2;
        }
    }
    if constexpr (RADII && !CHANWISE) {
        // one radius per atom (radii[a]), or the atom's share of its type's radius (RA.part: reduced by grad_radii_reduce)
        const double S = wave_sum(rp);
        if (lane == 0) {
            if (RA.part) {
                RA.part[a] = S;
            } else {
                const double r = (double)static_cast<const real *>(RA.radii)[a]; // (the radius the forward used)
                RA.grad_radii[a] = S != 0.0 ? -S / r : 0.0;                      // dL/dr = -(1/r) sum_v e d2
            }
        }
    }
    if constexpr (SCORE) { // s_n: one fixed butterfly, an atom without admitted voxels gets an exact zero
        const double S = wave_sum(sp);
        if (lane == 0) SA.atom_scores[a] = S;
    }
