// sar_basin.hpp — what the two halves of the basins of attraction share (include/sar.h: sar_basin_*, sar_runtime_basin,
// sar_runtime_basin_colorize): the expressions of a pixel's start point and of a point's node, bit for bit the same on the host and on
// the device, the argument block of the kernels of sar_basin.hip and their launch wrappers, called from sar_basin.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_corr.hpp"
#include "sar_internal.hpp"
#include "sar_search.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kMaxBasinGrid = 128;            // parent[] and the cells' roots are 4 B per cell each: 8 MiB apiece at 128^3
constexpr uint32_t kMaxBasinPixels = 1u << 24;     // per call
constexpr uint32_t kDefaultBasinChunk = 1u << 20;  // pixels per launch (whole tiles): keeps one dispatch short
constexpr uint32_t kMaxBasinChunk = 1u << 30;
constexpr uint32_t kBasinEmpty = 0xFFFFFFFFu;      // parent[] of a cell no tail has visited; root / label of a DIVERGED pixel

// The plane's parameter of index i of n along one axis: i / (n - 1) (0 when n == 1). A division: evaluated once per column and once
// per row into two small tables (sar_basin.cpp), not once per pixel, so that k_basin_screen holds no division and the fused-op audit
// can pin it at 0.
__host__ __device__ inline double basin_param(uint32_t i, uint32_t n) { return n > 1u ? (double)i / (double)(n - 1u) : 0.; }

// Coordinate k of the start point whose parameters are (tu, tv): two multiplies and two adds in this order
__host__ __device__ inline double basin_start(double origin, double du, double dv, double tu, double tv) {
    return (origin + du * tu) + dv * tv;
}

// The cell of coordinate p along one axis of the box: a subtract, a multiply and three compares
__host__ __device__ inline uint32_t basin_cell(double p, double lo, double scale, uint32_t grid) {
    const double u = (p - lo) * scale;
    // u < 0 ? 0 : u >= grid ? grid - 1 : (uint32_t)u, written so that a NaN (inf * 0 with an absurd box) is cell 0, not undefined
    return !(u >= 0.) ? 0u : (u >= (double)grid ? grid - 1u : (uint32_t)u);  // (0 <= u < grid <= 128: the conversion is in range)
}

struct BasinArgs {
    SearchCoeffs map;             // canonicalised; wave-uniform: every lane of every kernel steps the same one
    double origin[3], du[3], dv[3];
    double box_lo[3], scale[3];   // scale = grid / (box_hi - box_lo)
    double bound;
    const double* tu;             // [width]: basin_param(x, width)
    const double* tv;             // [height]: basin_param(height - 1 - y, height) — row 0 is the high end
    sar_basin_pixel* pixels;      // [height][width]: k_basin_screen writes status / escape_step, k_basin_finish root; label is the host's
    uint32_t* counter;            // [1] survivors of this launch's pixels (zero before k_basin_screen)
    uint32_t* surv_pix;           // [pixels of a launch] pixel index of every survivor, by survivor slot
    double* surv_xyz;             // [3][pixels of a launch] SoA: the point after the transient, by survivor slot
    uint32_t* parent;             // [grid^3] the union-find (kBasinEmpty before the first launch)
    uint32_t* last_node;          // [height][width]: the node of a survivor's last tail point
    uint32_t* node_root;          // [grid^3] k_basin_finish: the root of every visited cell, kBasinEmpty elsewhere
    unsigned long long* extent;   // [6] sortable images of xmin, xmax, ymin, ymax, zmin, zmax (~0 / 0 before the first launch)
    uint32_t width, height, tiles_x;
    uint32_t first_tile, n_tiles; // this launch's 8 x 8 tiles, row-major over the plane
    uint32_t slots;               // n_tiles * 64: the stride of surv_xyz
    uint32_t transient, steps;    // each <= 2^31, the sum below 2^32
    uint32_t grid, nodes;         // nodes = grid^3
};

// launch wrappers (sar_basin.hip)
void launch_basin_screen(const BasinArgs& a, hipStream_t s);
void launch_basin_mark(const BasinArgs& a, hipStream_t s);
void launch_basin_finish(const BasinArgs& a, hipStream_t s);
void launch_basin_colorize(const sar_basin_pixel* pixels, const uint32_t* labels, uint32_t npix, const PaletteParams& pal,
                           uint32_t attractors, double fade, void* rgba16_out, hipStream_t s);

}  // namespace sar
