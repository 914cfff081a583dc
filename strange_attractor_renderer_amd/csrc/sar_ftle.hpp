// sar_ftle.hpp — what the two halves of the FTLE maps share (include/sar.h: sar_ftle_*, sar_runtime_ftle, sar_runtime_ftle_colorize):
// the argument block of the kernels of sar_ftle.hip and their launch wrappers, called from sar_ftle.cpp. The start point of a pixel
// is the basins' (basin_param, basin_start: sar_basin.hpp), one expression for both families.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_basin.hpp"
#include "sar_internal.hpp"
#include "sar_search.hpp"

namespace sar {

constexpr uint32_t kDefaultFtleChunk = 1u << 20;  // pixels per launch of k_ftle_flow (whole tiles): keeps one dispatch short
constexpr uint32_t kMaxFtleChunk = 1u << 30;

struct FtleArgs {
    SearchCoeffs map;             // canonicalised; wave-uniform: every lane steps the same one
    double origin[3], du[3], dv[3];
    double bound;
    const double* tu;             // [width]: basin_param(x, width)
    const double* tv;             // [height]: basin_param(height - 1 - y, height) — row 0 is the high end
    sar_ftle_pixel* pixels;       // [height][width]: k_ftle_flow writes status / escape_step / end, k_ftle_gram flags and g11, g12, g22
    uint32_t width, height, tiles_x;
    uint32_t first_tile, n_tiles; // this launch's 8 x 8 tiles, row-major over the plane (k_ftle_flow)
    uint32_t steps;               // 1 .. 2^31
};

// launch wrappers (sar_ftle.hip)
void launch_ftle_flow(const FtleArgs& a, hipStream_t s);
void launch_ftle_gram(const FtleArgs& a, hipStream_t s);  // the whole picture, behind every band of launch_ftle_flow
void launch_ftle_colorize(const sar_ftle_pixel* pixels, const double* stretch2, uint32_t npix, const PaletteParams& pal, double two_n,
                          double lo, double span, double fade, void* rgba16_out, hipStream_t s);

}  // namespace sar
