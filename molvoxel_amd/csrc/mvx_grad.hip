// mvx_grad.hip - the backward pass (mvx_backward_batch): gradients of a loss L with respect to the atom coordinates and the
// channel weights, given G = dL/dgrid.
//
//   grad_chan_kernel  channel-wise radii for features: max radius (the pre-pass culls with it) and the per-channel threshold
//                     and coefficient, from the forward's own d2_threshold / gauss_coeff (float64: d2_threshold64 /
//                     gauss_coeff64)
//   grad_kernel       one wave per atom record (written by the forward's prep_kernel): the lanes walk the atom's admitted
//                     box, test every voxel exactly as the forward does (fp64 d2 in cdist order, d2 <= T), read G there and
//                     accumulate the channel partials and the three coordinate partials; fixed-order wave reductions, one
//                     write of the atom's gradient row. No atomics: an atom's gradients depend on its record, its weights and
//                     G over its own box only, so they are bit for bit the same in any batch and in any run.
//
// The contract (include/mvx.h, DESIGN.md "Backward pass"): with rho_{n,c}(v) = m_{n,c}(v) exp2(k f32(d2)) (float32; float64
// grids: exp(c64 d2)) and m the forward's membership,
//   dL/dw[n,c] = sum_v G[c,v] rho_{n,c}(v)
//   dL/dp_n    = sum_v (sum_c G[c,v] w[n,c] rho_{n,c}(v) 2 ln2 k_{n,c}) (p_n - g_v)     (float64 grids: 2 c64 instead of 2 ln2 k)
//   dL/dcoords = M^T dL/dp_n, M the linear part of apply_xform (M^T: the same sandwich product with the conjugate quaternion)
// Binary density: dL/dp = 0 (the a.e. derivative; the jump at the truncation radius is ignored, as it is for Gaussians).
#include "mvx_device.h"
#include "mvx_grad.h"

#include <hipcub/hipcub.hpp>

namespace mvx {

constexpr double LN2 = 0.69314718055994531; // d exp2(k d2) / d d2 = ln2 k exp2(k d2)

// element type of the grid -> the arithmetic of the handle (float32 for float and bfloat16 grids)
template <typename GT> struct GradReal { typedef float type; };
template <> struct GradReal<double> { typedef double type; };

__device__ __forceinline__ float load_grad(const float *p) { return *p; }
__device__ __forceinline__ float load_grad(const __bf16 *p) { return (float)*p; } // (exact widening)
__device__ __forceinline__ double load_grad(const double *p) { return *p; }

// dL/dcoords = M^T dL/dp: apply_xform's rotation with the conjugate quaternion, in the same operation order. Exact for
// |q| != 1 too: M = q (.) conj(q) and M^T = conj(q) (.) q. Centring and translations are constants.
__device__ __forceinline__ void apply_xform_transpose(const mvx_xform &xf, double &x, double &y, double &z) {
    if (!(xf.flags & MVX_XF_ROTATE)) return;
    const double q0 = xf.quat[0], q1 = -xf.quat[1], q2 = -xf.quat[2], q3 = -xf.quat[3];
    const double zero = 0.0;
    const double a0 = ((q0 * zero - q1 * x) - q2 * y) - q3 * z;
    const double a1 = ((q0 * x + q1 * zero) + q2 * z) - q3 * y;
    const double a2 = ((q0 * y - q1 * z) + q2 * zero) + q3 * x;
    const double a3 = ((q0 * z + q1 * y) - q2 * x) + q3 * zero;
    const double i0 = q0, i1 = q1 * -1, i2 = q2 * -1, i3 = q3 * -1;
    x = ((a0 * i1 + a1 * i0) + a2 * i3) - a3 * i2;
    y = ((a0 * i2 - a1 * i3) + a2 * i0) + a3 * i1;
    z = ((a0 * i3 + a1 * i2) - a2 * i1) + a3 * i0;
}

// sum over the 64 lanes, the same butterfly in every lane: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// 32 per-lane channel partials -> lane l holds the wave's sum of channel l / 2 (31 exchanges instead of 32 x 6): each step
// halves the channels a lane keeps - the lane with the mask bit set keeps the upper half - and adds its partner's copy of
// them. a + b and b + a are the same bits, so both lanes of a pair agree and the order is fixed.
template <typename T>
__device__ __forceinline__ T wave_sum32(T (&v)[32], int lane) {
#pragma unroll
    for (int h = 16, m = 32; h >= 1; h >>= 1, m >>= 1) {
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int j = 0; j < h; ++j) {
            const T send = up ? v[j] : v[j + h];
            const T keep = up ? v[j + h] : v[j];
            v[j] = keep + __shfl_xor(send, m, 64);
        }
    }
    return v[0] + __shfl_xor(v[0], 1, 64);
}

// MODE: MODE_FEATURES (weights = the feature row), or MODE_TYPES / MODE_SINGLE (weight 1 on channel `type` / 0)
template <typename GT, int MODE, bool GAUSS, bool CHANWISE>
__global__ void __launch_bounds__(256) grad_kernel(GradArgs A) {
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
    if constexpr (!FEAT) {
        const int ch = MODE == MODE_TYPES ? R.type : 0; // (an atom of type >= C has no admitted box)
        const GT *gc = gm + (size_t)(ch < A.C ? ch : 0) * D3;
        if (GAUSS) {
            for (int v0 = 0; v0 < nbox; v0 += 64) {
                const int v = v0 + lane;
                double dx, dy, dz;
                size_t off;
                voxel(v < nbox ? v : 0, dx, dy, dz, off);
                const double d2 = (dx * dx + dy * dy) + dz * dz; // cdist order, no fma
                const real rho = density(d2, T, k32, c64, v < nbox);
                if (rho != (real)0) { // (binary density: no coordinate gradient, nothing to read)
                    const double e = (double)(load_grad(gc + off) * rho) * kfac;
                    cp0 += e * dx;
                    cp1 += e * dy;
                    cp2 += e * dz;
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
#pragma unroll
                        for (int c = 0; c < 32; ++c) gv[c] = c < nc ? gload(c) : (real)0;
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
                        }
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
        }
    }
    if (A.grad_coords) {
        double g0 = wave_sum(cp0), g1 = wave_sum(cp1), g2 = wave_sum(cp2);
        if (A.xforms) apply_xform_transpose(A.xforms[bm], g0, g1, g2);
        if (lane == 0) {
            A.grad_coords[3 * a] = g0;
            A.grad_coords[3 * a + 1] = g1;
            A.grad_coords[3 * a + 2] = g2;
        }
    }
}

template <typename real>
__global__ void grad_chan_kernel(const real *radii, int C, int gauss, float sigma32, double sigma64, real *rmax, double *Tc,
                                 real *kc) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
        if constexpr (std::is_same<real, double>::value) { // as chan_aux64_kernel
            Tc[c] = d2_threshold64(radii[c]);
            kc[c] = (gauss && Tc[c] >= 0.0) ? gauss_coeff64(radii[c], sigma64) : 0.0;
        } else { // as chan_aux_kernel's slots
            const float r = radii[c];
            Tc[c] = d2_threshold(r);
            kc[c] = gauss ? gauss_coeff(r, sigma32) : 0.0f;
        }
    }
    if (threadIdx.x == 0) { // the culls' radius: max(radii) as numpy evaluates it (numpy/voxelizer.py:138)
        real m = radii[0];
        for (int c = 1; c < C; ++c) m = radii[c] > m ? radii[c] : m;
        rmax[0] = m;
    }
}

hipError_t launch_grad_chan(const void *radii, int32_t C, bool f64, bool gauss, float sigma32, double sigma64, void *rmax, double *Tc,
                            void *kc, hipStream_t s) {
    if (f64)
        hipLaunchKernelGGL(grad_chan_kernel<double>, dim3(1), dim3(256), 0, s, static_cast<const double *>(radii), C, gauss ? 1 : 0,
                           sigma32, sigma64, static_cast<double *>(rmax), Tc, static_cast<double *>(kc));
    else
        hipLaunchKernelGGL(grad_chan_kernel<float>, dim3(1), dim3(256), 0, s, static_cast<const float *>(radii), C, gauss ? 1 : 0,
                           sigma32, sigma64, static_cast<float *>(rmax), Tc, static_cast<float *>(kc));
    return hipGetLastError();
}

// Spatial order of the atoms: key = (molecule, 4^3-voxel cell of the admitted box's low corner), cells x-major, sorted
// by a stable radix sort. Consecutive atoms then read overlapping rows of G.
__global__ void __launch_bounds__(256) grad_key_kernel(const AtomRec *__restrict__ rec, const int64_t *__restrict__ offsets, int B,
                                                       int64_t total, int nc, uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= total) return;
    const AtomRec &R = rec[a];
    auto cell = [&](uint32_t r) { const int lo = (int)(r & 0xffff) >> 2; return lo < nc ? lo : 0; }; // (empty range: 0)
    const uint64_t b = B > 1 ? (uint64_t)find_molecule(offsets, B, a) : 0;
    keys[a] = (b * (uint64_t)nc + (uint64_t)cell(R.xr)) * (uint64_t)(nc * nc) + (uint64_t)(cell(R.yr) * nc + cell(R.zr));
    idx[a] = (uint32_t)a;
}

static int key_bits(int B, int D) {
    const int nc = (D + 3) / 4;
    const unsigned long long span = (unsigned long long)B * nc * nc * nc;
    int bits = 1;
    while (bits < 64 && (span >> bits) != 0) ++bits;
    return bits;
}

size_t grad_order_bytes(int64_t total, int B, int D) {
    size_t temp = 0;
    (void)hipcub::DeviceRadixSort::SortPairs(nullptr, temp, (const uint64_t *)nullptr, (uint64_t *)nullptr, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, (int)total, 0, key_bits(B, D));
    return 256 + 2 * (size_t)total * (sizeof(uint64_t) + sizeof(uint32_t)) + temp;
}

hipError_t launch_grad_order(const AtomRec *rec, const int64_t *offsets, int B, int64_t total, int D, void *ws, size_t ws_bytes,
                             const uint32_t **order, hipStream_t s) {
    const int nc = (D + 3) / 4;
    char *p = static_cast<char *>(ws);
    uint64_t *keys = reinterpret_cast<uint64_t *>(p), *keys_out = keys + total;
    uint32_t *idx = reinterpret_cast<uint32_t *>(keys_out + total), *idx_out = idx + total;
    char *temp = reinterpret_cast<char *>(idx_out + total);
    temp += (256 - reinterpret_cast<uintptr_t>(temp) % 256) % 256;
    size_t temp_bytes = ws_bytes - (size_t)(temp - p);
    hipLaunchKernelGGL(grad_key_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, rec, offsets, B, total, nc, keys, idx);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipcub::DeviceRadixSort::SortPairs(temp, temp_bytes, keys, keys_out, idx, idx_out, (int)total, 0, key_bits(B, D), s);
    *order = idx_out;
    return e;
}

template <typename GT, int MODE>
static hipError_t launch_grad_mode(const GradArgs &a, bool gauss, bool chanwise, hipStream_t s) {
    const unsigned nblk = (unsigned)((a.total + 3) / 4);
    const dim3 grid(a.xcd_span ? 8u * (unsigned)a.xcd_span : nblk), block(256);
    if constexpr (MODE == MODE_FEATURES) {
        if (chanwise) {
            if (gauss) hipLaunchKernelGGL((grad_kernel<GT, MODE, true, true>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((grad_kernel<GT, MODE, false, true>), grid, block, 0, s, a);
            return hipGetLastError();
        }
    }
    if (gauss) hipLaunchKernelGGL((grad_kernel<GT, MODE, true, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((grad_kernel<GT, MODE, false, false>), grid, block, 0, s, a);
    return hipGetLastError();
}

template <typename GT>
static hipError_t launch_grad_grid(const GradArgs &a, int32_t mode, bool gauss, bool chanwise, hipStream_t s) {
    if (mode == MODE_FEATURES) return launch_grad_mode<GT, MODE_FEATURES>(a, gauss, chanwise, s);
    return launch_grad_mode<GT, MODE_TYPES>(a, gauss, false, s); // (single mode: type 0 in every record)
}

hipError_t launch_grad(const GradArgs &a, int32_t mode, int32_t grid_kind, bool gauss, bool chanwise, hipStream_t s) {
    if (a.total <= 0) return hipSuccess;
    if (grid_kind == 2) return launch_grad_grid<double>(a, mode, gauss, chanwise, s);
    if (grid_kind == 1) return launch_grad_grid<__bf16>(a, mode, gauss, chanwise, s);
    return launch_grad_grid<float>(a, mode, gauss, chanwise, s);
}

} // namespace mvx
