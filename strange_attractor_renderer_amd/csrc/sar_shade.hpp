// sar_shade.hpp — what the two halves of shaded rendering share (include/sar.h: sar_shade, sar_shade_device): the tile, the host
// constants of the contract, the argument block of k_shade (sar_shade.hip) and its launch wrapper, called from sar_shade.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

namespace sar {

constexpr uint32_t kShadeTileW = 32;     // pixels per tile row: one half-wave reads one LDS row
constexpr uint32_t kShadeTileH = 16;     // a lane owns two pixels of one column, 8 rows apart
constexpr uint32_t kShadeThreads = 256;
constexpr uint32_t kShadeMaxRadius = 8, kShadeMaxShininessLog2 = 10;

struct ShadeArgs {
    const unsigned long long* key;  // hi word: sortable(zbuf)
    const uint32_t* count;
    const double* steps;
    ushort4* out;                   // [height][width] RGBA16
    sar_shade_stats* stats;         // zeroed before the launch
    uint32_t width, height, tiles_x;
    uint32_t R, Rz;                 // the occlusion radius; the halo of z~, max(R, 1): the normal reads the four neighbours
    uint32_t min_count, shininess_log2, taps;  // taps: N
    int32_t smooth, spec_on, window;
    uint16_t background[4];         // [3]: the alpha of a background pixel
    double k;                       // (double)width * scale
    double L[3], H[3];              // H is read when spec_on
    double ambient, diffuse, specular, ao_strength, ao_range, smooth_range;
    double w_lo, w_span, w_pos_lo, w_dpos;  // read when window
    double inv_d[kShadeMaxRadius * kShadeMaxRadius + 1];  // [d2], 1 <= d2 <= R * R
    PaletteParams pal;
};

// raw depths (floats) of tile plus an (Rz + 1)-wide halo behind z~ (doubles) of tile plus an Rz-wide halo: 19 088 bytes at R = 8
inline size_t shade_lds_bytes(uint32_t Rz) {
    const size_t zt = static_cast<size_t>(kShadeTileW + 2u * Rz) * (kShadeTileH + 2u * Rz);
    const size_t raw = static_cast<size_t>(kShadeTileW + 2u * Rz + 2u) * (kShadeTileH + 2u * Rz + 2u);
    return zt * 8u + raw * 4u;
}

// launch wrapper (sar_shade.hip)
void launch_shade(const ShadeArgs& a, uint32_t tiles, hipStream_t s);

}  // namespace sar
