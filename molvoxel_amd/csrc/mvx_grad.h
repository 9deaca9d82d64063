// mvx_grad.h - what the C-ABI TU (mvx_capi.hip) needs of the backward family: the argument records and launchers of the
// four walks (mvx_grad.hip, mvx_grad_radii.hip, mvx_score.hip, mvx_moments_grad.hip) and of the reductions (mvx_grad_radii.hip,
// mvx_grad_density.hip), and the host-side dispatch (WalkKey / for_walk, for_moments_walk, for_real) those files launch through.
// Included by mvx_capi.hip and, through mvx_grad_device.h, by the eight kernel files of the family (those six, mvx_pose.hip,
// mvx_views_reduce.hip and mvx_hess.hip, whose own records and launchers are in mvx_hess.h). WalkKey, for_walk and for_real are plain host C++: tests/test_walk_dispatch_host.py compiles them alone.
#pragma once
#include <type_traits>

#include "mvx_internal.h"

namespace mvx {

// Which instantiation of a walk kernel (grad_kernel, grad_radii_kernel, score_kernel <GT, MODE, GAUSS, CHANWISE>) a call takes.
struct WalkKey {
    int32_t grid_kind, mode; // grid_kind: 0 float, 1 bfloat16, 2 double. mode: Mode
    bool gauss, chanwise;    // Gaussian density; channel-wise radii (features only)
};

template <typename T>
struct TypeTag {
    typedef T type;
};
template <typename GT>
using GridTag = TypeTag<GT>;
template <int MODE>
using ModeTag = std::integral_constant<int, MODE>;

// fn(GridTag<GT>, ModeTag<MODE>, gauss constant, chanwise constant) for the key's instantiation, and the one place that knows
// which exist: per grid type, features x one radius / channel-wise x Gaussian / binary, and MODE_TYPES x Gaussian / binary
// for types and single mode alike (single: the records carry type 0) - 18 in all. CHANWISE occurs with MODE_FEATURES only.
template <typename Fn>
static hipError_t for_walk(const WalkKey &k, Fn &&fn) {
    auto grid = [&](auto gt) {
        auto density = [&](auto mode, auto chanwise) {
            return k.gauss ? fn(gt, mode, std::true_type{}, chanwise) : fn(gt, mode, std::false_type{}, chanwise);
        };
        if (k.mode == MODE_FEATURES)
            return k.chanwise ? density(ModeTag<MODE_FEATURES>{}, std::true_type{}) : density(ModeTag<MODE_FEATURES>{}, std::false_type{});
        return density(ModeTag<MODE_TYPES>{}, std::false_type{});
    };
    if (k.grid_kind == 2) return grid(GridTag<double>{});
    if (k.grid_kind == 1) return grid(GridTag<__bf16>{});
    return grid(GridTag<float>{});
}

// fn(ModeTag<MODE>, gauss constant, target constant) for the moments walk (moments_grad_kernel<MODE, GAUSS, TARGET>): what
// mvx_moments_batch serves - float32 grids, features and MODE_TYPES (types and single) x Gaussian / binary x with / without a
// target, 8 in all. hipErrorInvalidValue for a key of another grid type or with channel-wise radii for features.
template <typename Fn>
static hipError_t for_moments_walk(const WalkKey &k, bool target, Fn &&fn) {
    if (k.grid_kind != 0 || k.chanwise) return hipErrorInvalidValue;
    auto mode = [&](auto m) {
        auto density = [&](auto gauss) { return target ? fn(m, gauss, std::true_type{}) : fn(m, gauss, std::false_type{}); };
        return k.gauss ? density(std::true_type{}) : density(std::false_type{});
    };
    return k.mode == MODE_FEATURES ? mode(ModeTag<MODE_FEATURES>{}) : mode(ModeTag<MODE_TYPES>{});
}

// fn(TypeTag<real>): the handle's real type (float, or double at precision 64) of the arrays a launcher takes as void *
template <typename Fn>
static hipError_t for_real(bool f64, Fn &&fn) {
    return f64 ? fn(TypeTag<double>{}) : fn(TypeTag<float>{});
}

struct GradArgs {
    const AtomRec *rec;      // prep_kernel's records of the call
    const void *w;           // features (total, C) in the handle's real type (features mode)
    const void *g;           // G = dL/dgrid: (B, C, D, D, D) in the handle's grid type
    const int64_t *offsets;  // device, B + 1
    const mvx_xform *xforms; // device, B records, or null
    const double *Tc;        // channel-wise radii for features: per-channel thresholds ...
    const void *kc;          // ... and coefficients (float, or double for float64 grids)
    double *grad_coords;     // (total, 3) or null
    void *grad_w;            // (total, C) real or null
    const uint32_t *order;   // the atoms in processing order (launch_grad_order), or null: atom order
    int64_t total;
    int32_t B, C, D;
    int32_t xcd_span;        // > 0: XCD x takes workgroups [x * xcd_span, (x + 1) * xcd_span) of the order (8 xcd_span launched)
    double res, half;
};

// radius gradients (mvx_backward_radii_batch, grad_radii_kernel): where the walk puts its radius partials
struct RadiiArgs {
    const void *radii;  // the call's radii array (real): atom-wise radii, read by the per-atom write
    double *grad_radii; // one radius per atom: (total,) dL/dr, written by the walk itself
    double *part;       // or the partials grad_radii_reduce sums: (total,) per atom (types mode, radii by type) or
                        // (C, total) channel-major per (channel, atom) (features, channel-wise radii)
};

// scores against a constant field (mvx_score_batch, score_kernel): GradArgs::g is the field F instead of dL/dgrid
struct ScoreArgs {
    double *atom_scores; // (total,) s_n, written by the walk: the caller's array or handle-owned workspace
    int64_t mol_stride;  // elements between the fields of two molecules: 0 (one field shared by all) or C * D^3
};

// gradients of the moments (mvx_moments_backward_batch, moments_grad_kernel): GradArgs::g holds the float32 NCDHW grids g of the
// launch's molecules, and the walk forms the upstream itself: u[b,c,v] = fmaf(a1, g[b,c,v], fmaf(a2, t[c,v], a0)) in float32
struct MomentsArgs {
    const float *coef;   // (B, C, 3): a0 = (float)G0, a1 = (float)(2 G1), a2 = (float)G2 of the launch's molecules (launch_moments_coef)
    const float *target; // t: (C, D, D, D) float32 NCDHW of the launch's first molecule, or null (then u = fmaf(a1, g, a0))
    int64_t mol_stride;  // elements between the targets of two molecules: 0 (one target shared by all) or C * D^3
};

// channel-wise radii for features: rmax[0] = max(radii) (what prep_kernel culls with), per-channel thresholds Tc and
// coefficients kc (float, or double for f64), from the forward's d2_threshold / gauss_coeff (float64: their *64 forms)
hipError_t launch_grad_chan(const void *radii, int32_t C, bool f64, bool gauss, float sigma32, double sigma64, void *rmax, double *Tc,
                            void *kc, hipStream_t s);
// Spatial processing order of the atoms ("grad_order" option: key kernel + radix sort) in `ws` (grad_order_bytes); *order points into ws.
size_t grad_order_bytes(int64_t total, int B, int D);
hipError_t launch_grad_order(const AtomRec *rec, const int64_t *offsets, int B, int64_t total, int D, void *ws, size_t ws_bytes,
                             const uint32_t **order, hipStream_t s);
// One wave per atom record; nothing is launched without atoms.
hipError_t launch_grad(const GradArgs &a, const WalkKey &key, hipStream_t s);
// The same walk with the radius partials, in one pass with the coordinate and feature gradients, which are grad_kernel's
// bits. Gaussian density only (a binary density has zero radius gradients): hipErrorInvalidValue for a key without gauss.
hipError_t launch_grad_radii(const GradArgs &a, const RadiiArgs &r, const WalkKey &key, hipStream_t s);
// The same walk over a constant field F (mvx_score.hip): s_n = sum_v sum_c F[c,v] w[n,c] rho_{n,c}(v) per atom into
// ScoreArgs::atom_scores, in one pass with the coordinate and feature gradients, which are grad_kernel's bits for G = F laid
// out per molecule. Binary density walks the box too (it scores, though its coordinate gradients are zero).
hipError_t launch_score(const GradArgs &a, const ScoreArgs &sa, const WalkKey &key, hipStream_t s);
// scores[b] = sum of atom_scores over molecule b in a fixed order (one workgroup per molecule, no atomics); 0 without atoms
hipError_t launch_score_reduce(const double *atom_scores, const int64_t *offsets, int32_t B, double *scores, hipStream_t s);
// The coefficients of the moments walk from dL/dm: grad_moments (n, K) doubles, K = 3 | 2 (no target: a2 = 0) -> coef (n, 3)
// floats, n = B * C: a0 = (float)G0, a1 = (float)(2.0 * G1), a2 = (float)G2.
hipError_t launch_moments_coef(const double *grad_moments, int64_t n, int32_t K, float *coef, hipStream_t s);
// The same walk over the float32 grids g in GradArgs::g with the upstream formed from them (mvx_moments_grad.hip): the
// coordinate and feature gradients are grad_kernel's bits for G = u. `key`: grid_kind 0 and no channel-wise radii for features.
hipError_t launch_moments_grad(const GradArgs &a, const MomentsArgs &ma, const WalkKey &key, hipStream_t s);
// Both reductions over the atoms of a call sum chunks of GRAD_CHUNK atoms first (one block per chunk), then the chunks in order.
constexpr int GRAD_CHUNK = 4096;
inline int32_t grad_nchunk(int64_t total) { return (int32_t)((total + GRAD_CHUNK - 1) / GRAD_CHUNK); }
// Channel-wise radii: dL/dr_c from RadiiArgs::part in a fixed order (no atomics). types: the atoms' (total,) partials of type c,
// scaled by -1/r_c; else the (C, total) partials, scaled by -(kfac_c / r_c) with kc from launch_grad_chan. `stage` holds
// grad_radii_stage_doubles(total, C) doubles.
inline size_t grad_radii_stage_doubles(int64_t total, int32_t C) { return (size_t)grad_nchunk(total) * (size_t)C; }
hipError_t launch_grad_radii_reduce(const double *part, const int32_t *types, const void *radii, const void *kc, bool f64, int64_t total,
                                    int32_t C, double *stage, double *grad_radii, hipStream_t s);
// Sigma and scalar-radius gradients (mvx_backward_density_batch, mvx_grad_density.hip): the (total,) per-atom partials of
// RadiiArgs::part summed over the call in a fixed order (no atomics), then grad_sigma[0] = -sum / sigma and grad_radius[0] =
// -sum / r (each or NULL). With `grad_radii` (one radius per atom, `radii` the call's array) also dL/dr_n = -part[n] / radii[n],
// the bits the walk writes itself without RadiiArgs::part. `stage` holds grad_density_stage_doubles(total) doubles.
inline size_t grad_density_stage_doubles(int64_t total) { return (size_t)grad_nchunk(total); }
hipError_t launch_grad_density_sum(const double *part, int64_t total, const void *radii, bool f64, double *grad_radii, double r,
                                   double sigma, double *stage, double *grad_sigma, double *grad_radius, hipStream_t s);
// Channel-wise radii for features: grad_sigma[0] = -(1/sigma) sum_c kfac_c S_c from launch_grad_radii_reduce's `stage` sums
// (S_c: the chunks of channel c in order) and launch_grad_chan's kc, the channels in a fixed order.
hipError_t launch_grad_density_chan(const double *stage, int64_t total, int32_t C, const void *kc, bool f64, double sigma,
                                    double *grad_sigma, hipStream_t s);

} // namespace mvx
