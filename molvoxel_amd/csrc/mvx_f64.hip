// mvx_f64.hip - float64 grids (precision = 64; gfx950): the reference then keeps distances, ratios, densities and sums in
// float64 (numpy/voxelizer.py:33-34, 544-560).
//
//   voxelize64_kernel      chunks of 32 channels, scalar / atom-wise radii: the slab body (mvx_slab_body.inc) with OpsMx64 -
//                          v_mfma_f64_16x16x4_f64, four candidates per instruction, bit for bit the fma chain in candidate order.
//   voxelize64_vec_kernel  chunks of 1 / 4 / 8 / 16 channels, or channel-wise radii: the same slab body with OpsF64 - one voxel
//                          per lane on the vector ALU, the library's exp, the fma chain in candidate order.
#include "mvx_device.h"

namespace mvx {

__host__ __device__ __forceinline__ int row_stride_doubles(int NW) { return SUBZ * NW + 8; }
// LDS of either float64 kernel: the 64 rows of a round (sw words each) or the write-out tile (min(ct, CR64) channels),
// whichever is larger
static size_t voxelize64_lds_bytes(int32_t sw, int32_t ct, int32_t NW) {
    const size_t rows = (size_t)64 * sw * 4;
    const size_t tile = (size_t)(ct < CR64 ? ct : CR64) * RPC * row_stride_doubles(NW) * 8;
    return rows > tile ? rows : tile;
}

// float64 write-out: the same transposition through an LDS tile, 8 channels per round, rows of SUBZ*NW doubles read
// back as 16-B pairs: 32 lanes per 512-B row instead of eight 64-B runs per store instruction straight from registers
// (2.5 -> TB/s on cfg-2). Begins with a barrier (the region may still hold candidate rows) and ends without one.
template <int CT>
__device__ __forceinline__ void write_slab64(const double (&acc)[CT], double *tile, int tid, int lane, int wave, int NW, int b,
                                             int cbase, int x0, int y0, int z0, double *out, const VoxParams &P) {
    constexpr int CR = CT < CR64 ? CT : CR64;
    constexpr int NROUND = (CT + CR - 1) / CR;
    const int D = P.D;
    const int RS = row_stride_doubles(NW);
    const size_t D2 = (size_t)D * D, D3 = D2 * D;
    const int F2 = (SUBZ / 2) * NW;   // 16-B slots per row
    const int nthr = NW * 64;
    const int rows_per_pass = nthr / F2; // 16 for any NW
    const int q = tid % F2, rfirst = tid / F2;
    const int zq = z0 + 2 * q;
    const int lz = lane & (SUBZ - 1), ly = (lane >> SUBZ_SH) & (SUBY - 1), lx = lane >> (SUBZ_SH + SUBY_SH);
    const int col = SUBZ * wave + lz;
    const int rxy = lx * SUBY + ly;
    const bool vec = P.vec_store != 0; // D even and a 16-B aligned grid
#pragma unroll
    for (int rd = 0; rd < NROUND; ++rd) {
        __syncthreads(); // candidate rows (round 0) / previous tile (later rounds) fully consumed
#pragma unroll
        for (int c = 0; c < CR; ++c)
            if (rd * CR + c < CT) tile[(c * RPC + rxy) * RS + col] = acc[rd * CR + c];
        __syncthreads();
        for (int row = rfirst; row < CR * RPC; row += rows_per_pass) {
            const int c = row / RPC, r = row - c * RPC;
            const int sxx = (r >> SUBY_SH) & (SUBX - 1), syy = r & (SUBY - 1);
            const int ch = cbase + rd * CR + c;
            if (rd * CR + c < CT && ch < P.C && x0 + sxx < D && y0 + syy < D && zq < D) {
                const double2 v = *reinterpret_cast<const double2 *>(tile + row * RS + 2 * q);
                double *dst = out + ((size_t)b * P.C + ch) * D3 + (size_t)(x0 + sxx) * D2 + (size_t)(y0 + syy) * D + zq;
                if (vec) {
                    typedef double d2v __attribute__((ext_vector_type(2)));
                    __builtin_nontemporal_store((d2v){v.x, v.y}, reinterpret_cast<d2v *>(dst));
                } else {
                    dst[0] = v.x;
                    if (zq + 1 < D) dst[1] = v.y;
                }
            }
        }
    }
}

// float64 grids (precision = 64): the reference then keeps distances, ratios, densities and sums in float64
// (numpy/voxelizer.py:33-34, 544-560). Membership sqrt_f64(d2) / r <= 1 is decided exactly by d2 <= T (d2_threshold64,
// T in the record's T slot; per channel for channel-wise radii), so misses cost no sqrt / division; the gaussian value
// is exp(c * d2) (gauss_coeff64, c in the record's last two words), evaluated only when some lane of the wave hits.
template <int CT, bool GAUSS, bool CHANWISE, bool LANE_RANGE>
__device__ __forceinline__ void accumulate_row64(double (&acc)[CT], const unsigned *r, const LaneCtx &L, int C,
                                                 const double *__restrict__ Tc, const double *__restrict__ kc) {
    const double2 Pxy = *reinterpret_cast<const double2 *>(r);     // px, py
    const double2 PzT = *reinterpret_cast<const double2 *>(r + 4); // pz, T
    const double dx = Pxy.x - L.gx, dy = Pxy.y - L.gy, dz = PzT.x - L.gz;
    const double d2 = (dx * dx + dy * dy) + dz * dz; // cdist order, no fma
    bool in_range = true;
    if (LANE_RANGE) {
        const uint4 q = *reinterpret_cast<const uint4 *>(r + 8);
        const unsigned zr = r[12];
        in_range = (L.ix >= (int)(q.z & 0xffff)) && (L.ix <= (int)(q.z >> 16)) && (L.iy >= (int)(q.w & 0xffff)) &&
                   (L.iy <= (int)(q.w >> 16)) && (L.iz >= (int)(zr & 0xffff)) && (L.iz <= (int)(zr >> 16));
    }
    const double *f = reinterpret_cast<const double *>(r + 16);
    if constexpr (CHANWISE) {
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int ch = (L.cbase + c < C) ? L.cbase + c : C - 1;
            const bool hit = in_range && d2 <= Tc[ch];
            double val = 0.0;
            if (hit) val = GAUSS ? exp(kc[ch] * d2) : 1.0;
            acc[c] = fma(val, f[c], acc[c]);
        }
    } else {
        const bool hit = in_range && d2 <= PzT.y;
        double val = 0.0;
        if (hit) val = GAUSS ? exp(*reinterpret_cast<const double *>(r + 14) * d2) : 1.0;
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = fma(val, f[c], acc[c]);
    }
}

// ---- float64 grids, 32 channels, on the matrix cores ---------------------------------------------------------------------
// The same idea as OpsMx32 with v_mfma_f64_16x16x4_f64: D(16 x 16) += A(16 x 4) B(4 x 16), float64, the four k steps
// accumulated in sequence with one rounding each (tools/micro/mfma64_layout.hip) - bit for bit the chain of fma in
// candidate order of accumulate_row64. Operands one double per lane: A[i = lane % 16][k = lane / 16], B[k][j = lane % 16];
// D[i = 4 r + lane / 16][j = lane % 16] in register r = 0..3. Per FOUR candidates (k = lane / 16 picks the lane's
// candidate): lane l evaluates its candidate for four voxels - (x0 | x0 + 1, y0 + ly | y0 + 2 + ly, z) with (ly, lz) =
// ((l % 16) / 8, l % 8): dx^2 and dy^2 each shared by two of them, dz^2 by all four - and the 64 voxels x 32 channels take
// eight MFMAs (4 voxel blocks x 2 channel blocks, A = 16 channel weights of the candidate, B = the block's values).
// The vector path spent 32 float64 FMAs (128 issue cycles) and sixteen 16-byte LDS reads per candidate and wave on this.
typedef double d4v __attribute__((ext_vector_type(4)));
// exp(x) for x <= 0 in float64, for the matrix-core float64 walk: the library's exp is ~45 float64 instructions and, four
// per lane and candidate group, was what that walk spent most of its vector issue (and 27 spilled registers) on.
// x = (64 m + j) ln2 / 64 + r, |r| <= ln2 / 128: exp(x) = 2^m * 2^(j/64) * (1 + expm1(r)), the 64 table values correctly
// rounded (generated with 60-digit decimals), ln2 / 64 split so that k * LN2_64_HI is exact for |k| < 2^20, expm1 by its
// series to r^6 (the next term is below 3e-20 relative): ~1 ulp, like the library's (the reference's own chain of sqrt, two
// divisions and a square puts its argument ~4 ulp away already; the float64 goldens hold values to 1e-12).
__constant__ double EXP2_64TH[64] = {
    0x1.0000000000000p+0, 0x1.02c9a3e778061p+0, 0x1.059b0d3158574p+0, 0x1.0874518759bc8p+0,
    0x1.0b5586cf9890fp+0, 0x1.0e3ec32d3d1a2p+0, 0x1.11301d0125b51p+0, 0x1.1429aaea92de0p+0,
    0x1.172b83c7d517bp+0, 0x1.1a35beb6fcb75p+0, 0x1.1d4873168b9aap+0, 0x1.2063b88628cd6p+0,
    0x1.2387a6e756238p+0, 0x1.26b4565e27cddp+0, 0x1.29e9df51fdee1p+0, 0x1.2d285a6e4030bp+0,
    0x1.306fe0a31b715p+0, 0x1.33c08b26416ffp+0, 0x1.371a7373aa9cbp+0, 0x1.3a7db34e59ff7p+0,
    0x1.3dea64c123422p+0, 0x1.4160a21f72e2ap+0, 0x1.44e086061892dp+0, 0x1.486a2b5c13cd0p+0,
    0x1.4bfdad5362a27p+0, 0x1.4f9b2769d2ca7p+0, 0x1.5342b569d4f82p+0, 0x1.56f4736b527dap+0,
    0x1.5ab07dd485429p+0, 0x1.5e76f15ad2148p+0, 0x1.6247eb03a5585p+0, 0x1.6623882552225p+0,
    0x1.6a09e667f3bcdp+0, 0x1.6dfb23c651a2fp+0, 0x1.71f75e8ec5f74p+0, 0x1.75feb564267c9p+0,
    0x1.7a11473eb0187p+0, 0x1.7e2f336cf4e62p+0, 0x1.82589994cce13p+0, 0x1.868d99b4492edp+0,
    0x1.8ace5422aa0dbp+0, 0x1.8f1ae99157736p+0, 0x1.93737b0cdc5e5p+0, 0x1.97d829fde4e50p+0,
    0x1.9c49182a3f090p+0, 0x1.a0c667b5de565p+0, 0x1.a5503b23e255dp+0, 0x1.a9e6b5579fdbfp+0,
    0x1.ae89f995ad3adp+0, 0x1.b33a2b84f15fbp+0, 0x1.b7f76f2fb5e47p+0, 0x1.bcc1e904bc1d2p+0,
    0x1.c199bdd85529cp+0, 0x1.c67f12e57d14bp+0, 0x1.cb720dcef9069p+0, 0x1.d072d4a07897cp+0,
    0x1.d5818dcfba487p+0, 0x1.da9e603db3285p+0, 0x1.dfc97337b9b5fp+0, 0x1.e502ee78b3ff6p+0,
    0x1.ea4afa2a490dap+0, 0x1.efa1bee615a27p+0, 0x1.f50765b6e4540p+0, 0x1.fa7c1819e90d8p+0};
__device__ __forceinline__ double exp_nonpos64(double x, const double *__restrict__ tab /* LDS copy of EXP2_64TH */) {
    const double kd = __builtin_rint(x * 0x1.71547652b82fep+6); // 64 / ln2
    double r = fma(-kd, 0x1.62e42fee00000p-7, x);                // ln2 / 64, upper 32 bits
    r = fma(-kd, 0x1.a39ef35793c76p-39, r);                       // ... and the rest
    const int ki = (int)kd;
    const double t = tab[ki & 63];
    double q = fma(0x1.6c16c16c16c17p-10, r, 0x1.1111111111111p-7); // 1/720, 1/120
    q = fma(q, r, 0x1.5555555555555p-5);                             // 1/24
    q = fma(q, r, 0x1.5555555555555p-3);                             // 1/6
    q = fma(q, r, 0.5);
    const double p = fma(q * r, r, r); // expm1(r)
    return ldexp(fma(t, p, t), ki >> 6);
}
constexpr int MX64_SW = 84; // 16 + 64 words, padded to an odd number of 16-B quads (one row per lane in the row filter)

template <bool GAUSS, bool LANE_RANGE>
struct OpsMx64 {
    static constexpr bool RUNS = false;
    static constexpr int CT = 32;
    static constexpr int NSUB = 1;
    static constexpr bool GROUPED = false;
    static constexpr bool VSTAGE = false;
    static constexpr bool CULL = true;
    static constexpr bool PRESTAGE = false;
    struct Acc {
        d4v a[2][4]; // [channel block of 16][voxel block m = 2 x + yh]: channels 16 cb + 4 r + lane / 16, r = 0..3
    };
    static constexpr int WORDS = 2;
    static constexpr int WW = 64;
    static constexpr int SW = MX64_SW;
    static __device__ __forceinline__ void zero(Acc &acc) {
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int m = 0; m < 4; ++m) acc.a[cb][m] = (d4v){0.0, 0.0, 0.0, 0.0};
    }
    static __device__ __forceinline__ LaneCtx ctx(int lane, int wave, int x0, int y0, int z0, int zt_lo, int cbase, const VoxParams &P) {
        const int lz = lane & (SUBZ - 1), ly = (lane >> SUBZ_SH) & 1;
        LaneCtx L;
        L.ix = x0;
        L.iy = y0 + ly;
        L.iz = z0 + SUBZ * wave + lz;
        L.gx = (double)L.ix * P.res - P.half;
        L.gx1 = (double)(L.ix + 1) * P.res - P.half;
        L.gy = (double)L.iy * P.res - P.half;
        L.gy1 = (double)(L.iy + 2) * P.res - P.half;
        L.gz = (double)L.iz * P.res - P.half;
        L.zt_w = zt_lo + wave;
        L.cbase = cbase;
        return L;
    }
    // the 2^(j/64) table of exp_nonpos64, behind the rows / tile region (P.dcap bytes)
    static __device__ __forceinline__ void tables(LaneCtx &L, char *smem, const VoxParams &P, int tid) {
        double *tab = reinterpret_cast<double *>(smem + P.dcap);
        if (tid < 64) tab[tid] = EXP2_64TH[tid];
        L.gtab = tab;
    }
    static __device__ __forceinline__ void walk(Acc &acc, unsigned long long mask, const unsigned *un, int lane, const LaneCtx &L,
                                                const VoxParams &P, const double *__restrict__, const float *__restrict__) {
        const int q = lane >> 4; // which candidate of the four this lane evaluates
        const int j = lane & 15; // ... and which of its 16-channel blocks' weights it feeds
        while (mask) {
            // up to four rows, in order (uniform)
            int s[4];
            int have = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                s[k] = 0;
                if (mask) {
                    s[k] = __builtin_ctzll(mask);
                    mask &= mask - 1;
                    have = k + 1;
                }
            }
            const bool valid = q < have; // a short last group: the missing candidates add fma(0, 0, acc) = acc
            const int sq = q == 0 ? s[0] : (q == 1 ? s[1] : (q == 2 ? s[2] : s[3]));
            const unsigned *r = un + sq * SW;
            const double2 Pxy = *reinterpret_cast<const double2 *>(r);     // px, py
            const double2 PzT = *reinterpret_cast<const double2 *>(r + 4); // pz, T
            const double dx0 = Pxy.x - L.gx, dx1 = Pxy.x - L.gx1, dy0 = Pxy.y - L.gy, dy1 = Pxy.y - L.gy1, dz = PzT.x - L.gz;
            const double sx0 = dx0 * dx0, sx1 = dx1 * dx1, sy0 = dy0 * dy0, sy1 = dy1 * dy1, sz = dz * dz;
            double d2[4]; // m = 2 x + yh; cdist order (dx^2 + dy^2) + dz^2, no fma
            d2[0] = (sx0 + sy0) + sz;
            d2[1] = (sx0 + sy1) + sz;
            d2[2] = (sx1 + sy0) + sz;
            d2[3] = (sx1 + sy1) + sz;
            bool hit[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) hit[m] = valid && d2[m] <= PzT.y;
            if (LANE_RANGE) {
                const uint4 rg = *reinterpret_cast<const uint4 *>(r + 8); // k, type, xr, yr
                const unsigned zr = r[12];
                const bool zok = (L.iz >= (int)(zr & 0xffff)) && (L.iz <= (int)(zr >> 16));
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int ix = L.ix + (m >> 1), iy = L.iy + 2 * (m & 1);
                    hit[m] = hit[m] && zok && (ix >= (int)(rg.z & 0xffff)) && (ix <= (int)(rg.z >> 16)) && (iy >= (int)(rg.w & 0xffff)) &&
                             (iy <= (int)(rg.w >> 16));
                }
            }
            const double w0 = valid ? *reinterpret_cast<const double *>(r + 16 + 2 * j) : 0.0;        // channel j of the row
            const double w1 = valid ? *reinterpret_cast<const double *>(r + 16 + 2 * (16 + j)) : 0.0; // channel 16 + j
            const double c64 = GAUSS ? *reinterpret_cast<const double *>(r + 14) : 0.0;
#pragma unroll
            for (int m = 0; m < 4; ++m) { // (one voxel block at a time: its value lives only until its two MFMAs are issued)
                double val = hit[m] ? 1.0 : 0.0;
                if (GAUSS && __ballot(hit[m]) != 0ull) { // (wave-uniform)
                    const double e = exp_nonpos64(c64 * d2[m], L.gtab);
                    val = hit[m] ? e : 0.0;
                }
                acc.a[0][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(w0, val, acc.a[0][m], 0, 0, 0);
                acc.a[1][m] = __builtin_amdgcn_mfma_f64_16x16x4f64(w1, val, acc.a[1][m], 0, 0, 0);
            }
        }
    }
    // Write-out through the float64 tile of write_slab64 ([channel][x, y row][z], CR64 = 8 channels per round). Round t
    // holds channels 8 t .. 8 t + 7 = channel block t / 2, i = 8 (t % 2) + 4 rr + lane / 16 with rr = 0, 1, i.e. registers
    // r = 2 (t % 2) + rr of every lane: each lane writes 2 channels x 4 voxels per round.
    static __device__ __forceinline__ void write(const Acc &acc, int any, unsigned *un, int tid, int lane, int wave, int NW, int b,
                                                 const LaneCtx &L, int x0, int y0, int z0, void *out_, const VoxParams &P) {
        double *out = static_cast<double *>(out_);
        double *tile = reinterpret_cast<double *>(un);
        constexpr int CR = CR64, NROUND = 32 / CR;
        const int D = P.D;
        const int RS = row_stride_doubles(NW);
        const size_t D2 = (size_t)D * D, D3 = D2 * D;
        const int F2 = (SUBZ / 2) * NW; // 16-B slots per row
        const int nthr = NW * 64;
        const int rows_per_pass = nthr / F2; // 16 for any NW
        const int qq = tid % F2, rfirst = tid / F2;
        const int zq = z0 + 2 * qq;
        const int lz = lane & (SUBZ - 1), ly = (lane >> SUBZ_SH) & 1, q = lane >> 4;
        const bool vec = P.vec_store != 0; // D even and a 16-B aligned grid
        double *mine = tile + (q * RPC + ly) * RS + SUBZ * wave + lz; // + (4 rr * RPC + x * SUBY + 2 yh) * RS
#pragma unroll
        for (int t = 0; t < NROUND; ++t) {
            __syncthreads(); // candidate rows (round 0) / previous tile (later rounds) fully consumed
#pragma unroll
            for (int rr = 0; rr < 2; ++rr)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    mine[(4 * rr * RPC + (m >> 1) * SUBY + 2 * (m & 1)) * RS] = acc.a[t / 2][m][2 * (t % 2) + rr];
            __syncthreads();
            for (int row = rfirst; row < CR * RPC; row += rows_per_pass) {
                const int c = row / RPC, rw = row - c * RPC;
                const int sxx = (rw >> SUBY_SH) & (SUBX - 1), syy = rw & (SUBY - 1);
                const int ch = L.cbase + t * CR + c;
                if (ch < P.C && x0 + sxx < D && y0 + syy < D && zq < D) {
                    const double2 v = *reinterpret_cast<const double2 *>(tile + row * RS + 2 * qq);
                    double *dst = out + ((size_t)b * P.C + ch) * D3 + (size_t)(x0 + sxx) * D2 + (size_t)(y0 + syy) * D + zq;
                    if (vec) {
                        typedef double d2v __attribute__((ext_vector_type(2)));
                        __builtin_nontemporal_store((d2v){v.x, v.y}, reinterpret_cast<d2v *>(dst));
                    } else {
                        dst[0] = v.x;
                        if (zq + 1 < D) dst[1] = v.y;
                    }
                }
            }
            // (round pacing as in OpsMx32::write, measured here: -7 % at 1280 cycles per round, -11 % at 2560 - two
            // workgroups per unit with a float64 walk between their write-outs do not queue loads behind stores)
            (void)any;
        }
    }
};

template <int CT_, bool GAUSS, bool CHANWISE, bool LANE_RANGE>
struct OpsF64 {
    static constexpr bool RUNS = false;
    static constexpr int CT = CT_;
    static constexpr int NSUB = 1;
    static constexpr bool GROUPED = false;
    static constexpr bool VSTAGE = false;
    static constexpr bool CULL = false; // (every wave walks the rows whose z range meets its sub-tile, hit or not)
    static constexpr bool PRESTAGE = false;
    typedef double Acc[CT];
    static constexpr int WORDS = 2;
    static constexpr int WW = 2 * CT;
    static constexpr int SW = 16 + 2 * CT;
    static_assert(16 + WW <= 64, "a row is staged by one wave-wide load");
    static __device__ __forceinline__ void zero(Acc &acc) {
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = 0.0;
    }
    static __device__ __forceinline__ LaneCtx ctx(int lane, int wave, int x0, int y0, int z0, int zt_lo, int cbase, const VoxParams &P) {
        return make_lane_ctx(lane, wave, x0, y0, z0, zt_lo, cbase, P);
    }
    static __device__ __forceinline__ void tables(LaneCtx &, char *, const VoxParams &, int) {}
    static __device__ __forceinline__ void accumulate(Acc &acc, const unsigned *r, const LaneCtx &L, const VoxParams &P,
                                                      const double *__restrict__ Tc, const float *__restrict__ kc) {
        // (float64 handles keep float64 per-channel coefficients behind the `kc` pointer)
        accumulate_row64<CT, GAUSS, CHANWISE, LANE_RANGE>(acc, r, L, P.C, Tc, reinterpret_cast<const double *>(kc));
    }
    // the rows of `mask` (one bit per staged row, atom order) into the accumulators
    static __device__ __forceinline__ void walk(Acc &acc, unsigned long long mask, const unsigned *un, int lane, const LaneCtx &L,
                                                const VoxParams &P, const double *__restrict__ Tc, const float *__restrict__ kc) {
        while (mask) {
            const int sl = __builtin_ctzll(mask);
            mask &= mask - 1;
            accumulate(acc, un + sl * SW, L, P, Tc, kc);
        }
    }
    static __device__ __forceinline__ void write(const Acc &acc, bool, unsigned *un, int tid, int lane, int wave, int NW, int b,
                                                 const LaneCtx &L, int x0, int y0, int z0, void *out, const VoxParams &P) {
        write_slab64<CT>(acc, reinterpret_cast<double *>(un), tid, lane, wave, NW, b, L.cbase, x0, y0, z0,
                         static_cast<double *>(out), P);
    }
};

// float64 grids, chunks of 32 channels, scalar / atom-wise radii: the slab body with OpsMx64 (128 registers)
template <bool GAUSS, bool LANE_RANGE, int MAXT>
__global__ void __launch_bounds__(MAXT, (MAXT <= 512 ? 4 : 2))
    voxelize64_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                      const uint2 *__restrict__ slist_ext, double *__restrict__ out, const VoxParams P) {
    typedef OpsMx64<GAUSS, LANE_RANGE> Ops;
    constexpr int CT = 32;
    constexpr bool GROUPED = false;
    const double *const Tc = nullptr;
    const float *const kc = nullptr;
#include "mvx_slab_body.inc"
}

// float64 grids, chunks of 1 / 4 / 8 / 16 channels, any radii: the slab body with OpsF64. One instantiation per key, compiled
// for workgroups of up to 16 waves (the plan's slabs have at most 8; debug_option("nw") asks for more): no key needs more
// registers for that.
template <int CT_, bool GAUSS, bool CHANWISE, bool LANE_RANGE>
__global__ void __launch_bounds__(1024, 1)
    voxelize64_vec_kernel(const unsigned *__restrict__ rec, const unsigned *__restrict__ w, const uint2 *__restrict__ slist,
                          const uint2 *__restrict__ slist_ext, const double *__restrict__ Tc, const float *__restrict__ kc,
                          double *__restrict__ out, const VoxParams P) {
    typedef OpsF64<CT_, GAUSS, CHANWISE, LANE_RANGE> Ops;
    constexpr int CT = CT_;
    constexpr bool GROUPED = false;
    constexpr int MAXT = 1024;
#include "mvx_slab_body.inc"
}

// ------------------------------------------------------------------------------------------------
// dispatch
// ------------------------------------------------------------------------------------------------
struct KernelKey64 {
    int ct;
    bool gauss, chanwise, lane_range;
};

// fn(ct constant, gauss constant, chanwise constant, lane_range constant) for the key's instantiation of the vector family, and
// the one place that knows which exist: CT 1 / 4 / 8 / 16 x Gaussian / binary x {wave-uniform block cull, per-lane ranges,
// channel-wise radii (always with per-lane ranges)} - 24 in all.
template <typename Fn>
static hipError_t for_kernel64(const KernelKey64 &k, Fn &&fn) {
    auto width = [&](auto ct) {
        auto density = [&](auto chanwise, auto lane_range) {
            return k.gauss ? fn(ct, std::true_type{}, chanwise, lane_range) : fn(ct, std::false_type{}, chanwise, lane_range);
        };
        if (k.chanwise) return density(std::true_type{}, std::true_type{});
        return k.lane_range ? density(std::false_type{}, std::true_type{}) : density(std::false_type{}, std::false_type{});
    };
    if (k.ct == 1) return width(std::integral_constant<int, 1>{});
    if (k.ct == 4) return width(std::integral_constant<int, 4>{});
    if (k.ct == 8) return width(std::integral_constant<int, 8>{});
    if (k.ct == 16) return width(std::integral_constant<int, 16>{});
    return hipErrorInvalidValue;
}

// The one launch sequence of both float64 kernels: one workgroup per (slab, molecule, channel chunk), 65535 / ncc molecules per
// launch (gridDim.y limit); the profiling bracket rides on the first launch. extra: the kernel's arguments between the lines
// and the grid.
template <auto Kern, typename... A>
static hipError_t launch_slabs64(const VoxArgs &a, VoxParams p, size_t lds, hipStream_t s, A... extra) {
    if (p.NW > 16) return hipErrorInvalidConfiguration;
    const int per = 65535 / p.ncc;
    for (int m0 = 0; m0 < p.B; m0 += per) {
        p.b0 = m0;
        const int nb = p.B - m0 < per ? p.B - m0 : per;
        const hipError_t e = launch_kernel<Kern>(dim3(slab_grid_x(p), (unsigned)(nb * p.ncc)), dim3(p.NW * 64), lds, s, a.rec, a.w, a.slist,
                                                 a.slist_ext, extra..., static_cast<double *>(a.out), p);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <bool GAUSS, bool LANE_RANGE>
static hipError_t launch_mx64(const VoxArgs &a, hipStream_t s) {
    VoxParams p = a.p;
    const size_t main_lds = voxelize64_lds_bytes(MX64_SW, 32, p.NW);
    p.dcap = (int32_t)main_lds; // where the kernel keeps its copy of the 2^(j/64) table
    return launch_slabs64<voxelize64_kernel<GAUSS, LANE_RANGE, 512>>(a, p, main_lds + 512, s);
}

hipError_t launch_voxelize64(const VoxArgs &a, int32_t ct, bool gauss, bool chanwise, bool lane_range, hipStream_t s) {
    if (ct == 32) { // chunks of 32 channels with scalar / atom-wise radii on slabs of at most 8 waves: the matrix-core kernel
        if (chanwise || a.p.NW > 8) return hipErrorInvalidValue;
        if (gauss) return lane_range ? launch_mx64<true, true>(a, s) : launch_mx64<true, false>(a, s);
        return lane_range ? launch_mx64<false, true>(a, s) : launch_mx64<false, false>(a, s);
    }
    const KernelKey64 k{ct, gauss, chanwise, chanwise ? true : lane_range};
    return for_kernel64(k, [&](auto ct_, auto gauss_, auto chanwise_, auto lane_range_) {
        constexpr int CT = decltype(ct_)::value;
        constexpr bool GAUSS = decltype(gauss_)::value, CHANWISE = decltype(chanwise_)::value, LANE_RANGE = decltype(lane_range_)::value;
        return launch_slabs64<voxelize64_vec_kernel<CT, GAUSS, CHANWISE, LANE_RANGE>>(
            a, a.p, voxelize64_lds_bytes(OpsF64<CT, GAUSS, CHANWISE, LANE_RANGE>::SW, CT, a.p.NW), s, a.Tc, a.kc);
    });
}

} // namespace mvx
