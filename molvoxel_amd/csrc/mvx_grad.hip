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
// The walk itself is mvx_grad_body.inc, shared with grad_radii_kernel (mvx_grad_radii.hip: the same walk plus dL/dradii).
#include "mvx_grad_device.h"

#include <hipcub/hipcub.hpp>

namespace mvx {

// MODE: MODE_FEATURES (weights = the feature row), or MODE_TYPES / MODE_SINGLE (weight 1 on channel `type` / 0)
template <typename GT, int MODE, bool GAUSS, bool CHANWISE>
__global__ void __launch_bounds__(256) grad_kernel(GradArgs A) {
    constexpr bool RADII = false;
    constexpr RadiiArgs RA{}; // (no radius partials: never read)
    constexpr bool SCORE = false;
    constexpr ScoreArgs SA{}; // (no scores: never read)
    constexpr bool MOMENTS = false, TARGET = false;
    constexpr MomentsArgs MA{}; // (the upstream is read, not formed: never read)
#include "mvx_grad_body.inc"
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
    return for_real(f64, [&](auto t) {
        typedef typename decltype(t)::type real;
        hipLaunchKernelGGL(grad_chan_kernel<real>, dim3(1), dim3(256), 0, s, static_cast<const real *>(radii), C, gauss ? 1 : 0,
                           sigma32, sigma64, static_cast<real *>(rmax), Tc, static_cast<real *>(kc));
        return hipGetLastError();
    });
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

hipError_t launch_grad(const GradArgs &a, const WalkKey &key, hipStream_t s) {
    return for_walk(key, [&](auto gt, auto mode, auto gauss, auto chanwise) {
        return launch_walk(grad_kernel<typename decltype(gt)::type, mode, gauss, chanwise>, a, s); // (the tags convert as constants)
    });
}

} // namespace mvx
