// sar_density.hpp — what the two halves of density estimation share (include/sar.h: sar_density_*, sar_runtime_density): the weight
// plan's layout, the argument block of k_density (sar_density.hip) and its launch wrapper, called from sar_density.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "sar_internal.hpp"

namespace sar {

constexpr uint32_t kDensityMinSamples = 2, kDensityMaxSamples = 256, kDensityDefaultSamples = 64;
constexpr uint32_t kDensityTileW = 32;          // pixels per tile row: one half-wave reads one LDS row
constexpr uint32_t kDensityDefaultTileH = 16;   // "density_tile" option: 8, 16 or 32 rows
constexpr uint32_t kDensityPlanMaxWords = 2048;  // the plan at S = 256 (1968 words) fits (sar_density.cpp checks)
constexpr uint32_t kDensityThreads = 256;       // 8 rows of 32 lanes; a lane owns tile_h / 8 pixels of one column

// R = floor(sqrt(S - 1)) in integers
constexpr uint32_t density_radius(uint32_t S) {
    uint32_t r = 0;
    while ((r + 1u) * (r + 1u) < S) ++r;
    return r;
}

// The plan as the kernel holds it in LDS, packed by d2 so that a tap's row is wave-uniform:
//   words [0, S)        off[d2]: where row d2 starts
//   row 0               W_c[0] for c = 1 .. S-1            (index c - 1)
//   row d2 >= 1         W_c[d2] for c = 1 .. (S-1) / d2     (the classes the tap is live for: d2 * c < S)
// 1968 words (7.7 KiB) at S = 256, 400 at the default.
std::vector<uint32_t> density_plan(uint32_t S);
// class c's table W_c[0 .. S): the contract's arithmetic (include/sar.h), host only
void density_row(uint32_t S, uint32_t c, uint32_t* out);

// what one call reduces into (zeroed before the launch): the public statistics and the launch's own two counters
struct DensityDeviceStats {
    sar_density_stats s;
    uint32_t tiles, tiles_copied;
};

struct DensityArgs {
    const double* snap_steps;     // the snapshot the taps read: [height][width]
    const uint32_t* snap_count;
    double* steps;                // the live buffers the results go to
    uint32_t* count;
    uint32_t* scalars;            // SC_MAX (zeroed before the launch) takes the maximum of count'
    DensityDeviceStats* stats;
    const uint32_t* plan;         // density_plan(S), plan_words words
    uint32_t width, height;
    uint32_t S, R;
    uint32_t tile_h, tiles_x;
    uint32_t plan_words;
};

inline size_t density_lds_bytes(uint32_t R, uint32_t tile_h, uint32_t plan_words) {
    const size_t n = static_cast<size_t>(kDensityTileW + 2u * R) * (tile_h + 2u * R);
    return n * 12u + static_cast<size_t>(plan_words) * 4u;
}

// launch wrapper (sar_density.hip)
void launch_density(const DensityArgs& a, uint32_t tiles, hipStream_t s);

}  // namespace sar
