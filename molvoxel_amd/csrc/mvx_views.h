// mvx_views.h - many views of one shared point cloud (mvx_select_views / mvx_forward_views / mvx_score_views /
// mvx_views_reduce): what mvx_views.hip and mvx_views_reduce.hip launch for the C-ABI TU (mvx_capi.hip).
#pragma once
#include "mvx_internal.h"

namespace mvx {

constexpr int VIEW_TILE = 1024; // atoms per (view, tile) workgroup

// The selection's arguments: the cloud as the pre-pass would see ONE molecule of pa.total atoms (pa.coords, pa.types, pa.radii,
// pa.chan_aux, pa.radii_src, pa.radius_scalar, pa.precision, pa.C, pa.g), the views' transforms on the device (pa.xforms, pa.B
// records) and the launch shape: the grid is (tiles) x (views), the larger extent in gridDim.x.
struct ViewArgs {
    PrepArgs pa;
    int32_t ntiles;     // ceil(pa.total / VIEW_TILE)
    int32_t views_in_x; // 1: blockIdx.x = view, blockIdx.y = tile; 0: the other way round
};

// up to three arrays gathered by one launch (blockIdx.y = array): coordinates, feature rows or types, atom-wise radii
struct GatherArgs {
    const char *src[3];
    char *dst[3];
    int32_t row_bytes[3];
    int32_t width[3]; // bytes per access: 16, 8 or 4 - the widest that divides the row length with both arrays aligned to it
    int32_t narr;
    const int64_t *index; // rows to take, `total` of them
    int64_t total;
};

// max(radii) as numpy evaluates it (numpy/voxelizer.py:138): rmax[0], float or double by precision
hipError_t launch_view_rmax(const void *radii, int32_t C, int32_t precision, void *rmax, hipStream_t s);
// counts[view * ntiles + tile] = atoms of the tile that pass the view's box cull
hipError_t launch_view_count(const ViewArgs &a, int32_t *counts, hipStream_t s);
// tile_base = exclusive scan of counts in (view, tile) order; offsets[b] = tile_base[b * ntiles], offsets[B] = the total
hipError_t launch_view_scan(const int32_t *counts, int32_t B, int32_t ntiles, int64_t *tile_base, int64_t *offsets, hipStream_t s);
// index[offsets[b] ..] = the passing atoms of view b in ascending order
hipError_t launch_view_fill(const ViewArgs &a, const int64_t *tile_base, int64_t *index, hipStream_t s);
hipError_t launch_view_gather(const GatherArgs &g, hipStream_t s);

// mvx_views_reduce.hip: out[n, :] = the sum of rows[slot, :] over the views whose segment of `index` holds atom n (rows and out
// float, or double with rows_f64; `width` columns, at most VIEW_REDUCE_MAX_WIDTH); every row of out is written
constexpr int32_t VIEW_REDUCE_MAX_WIDTH = 65535 * 32;
hipError_t launch_view_reduce(const int64_t *index, const int64_t *offsets, int32_t B, int64_t N, const void *rows, int32_t width,
                              bool rows_f64, void *out, hipStream_t s);

} // namespace mvx
