// sar_gallery.hpp — what the two halves of the gallery share (include/sar.h: sar_runtime_gallery): the argument blocks of k_gallery
// (sar_gallery.hip) and its launch wrapper, called from sar_gallery.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

namespace sar {

constexpr uint32_t kMaxGalleryTilePixels = 16384;  // a tile's depth keys (8 B per pixel) fill 128 KiB of a CU's 160 KiB of LDS
constexpr uint32_t kGalleryBlock = 1024;           // lanes of a tile's workgroup: four waves per SIMD, 128 VGPRs per lane
constexpr uint32_t kDefaultGalleryChunk = 512;     // tiles per launch: two rounds of one tile per CU; 128 MiB of raw scratch at 128 x 128
constexpr uint32_t kMaxGalleryChunk = 1u << 16;

// What differs from tile to tile, one block per tile in device memory: the workgroup reads its own through the constant address
// space (load_frame_args) — scalar loads into SGPRs, what the by-value arguments of the render kernels are.
struct GalleryTile {
    MapParams p;              // cfg_i's hoisted constants (fill_map_params)
    ColorTransformParams ct;  // (fill_ct_params)
};
static_assert(sizeof(GalleryTile) % 8 == 0, "read as 8-byte words");

struct GalleryArgs {
    const GalleryTile* tiles;  // [n]: every tile of the call
    const double* starts;      // [jobs][3]: the start points, the same for every tile
    double* warm;              // [chunk][3][jobs]: the points after the warm-up (NaN x: the job died in it)
    uint32_t* count;           // [chunk][npix] raw tiles of this launch, tile-major
    float* zbuf;               // [chunk][npix]
    double* steps;             // [chunk][npix]
    void* atlas;               // RGBA16, atlas_width pixels per row: the whole call's
    sar_gallery_stats* stats;  // [n]
    const double* lut;         // colorize's ln table (ln_u32)
    uint32_t lut_len;
    uint32_t first_tile;       // the launch's first tile; workgroup b renders tile first_tile + b into raw slot b
    uint32_t tile_width, tile_height, npix;
    uint32_t cols, atlas_width;
    uint32_t jobs;
    uint32_t iters;            // counted iterations per job; jobs * iters < 2^32
    int32_t render_kind, transparent;
    uint32_t _pad;
    double b_offset, b_factor;
    PaletteParams pal;
};

int launch_gallery(const GalleryArgs& a, uint32_t n_tiles, hipStream_t s);  // 0, or the hipError_t of setting the LDS attribute

}  // namespace sar
