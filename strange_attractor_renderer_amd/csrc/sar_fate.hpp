// sar_fate.hpp — what the two halves of the basin probes share (include/sar.h: sar_runtime_basin_fates,
// sar_runtime_basin_uncertainty): the expression of a ladder's probe point, bit for bit the same on the host and on the device, the
// argument block of the kernels of sar_fate.hip and their launch wrappers, called from sar_fate.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_basin.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kMaxFatePoints = 1u << 24;          // per call
constexpr uint32_t kFateChunk = 1u << 20;              // points per launch of k_basin_fate: keeps one dispatch short, bounds the staging
constexpr uint32_t kMaxLadderBases = 1u << 20;         // per call
constexpr uint32_t kDefaultLadderChunk = 1u << 16;     // base points per launch of k_basin_ladder: at K = 24 a wave each, 2^16 waves
constexpr uint32_t kMaxLadderLevels = SAR_BASIN_MAX_LEVELS;
constexpr uint32_t kFateUnknown = SAR_BASIN_UNKNOWN;   // label of a BOUNDED probe none of whose tail points lies in a labelled cell

// Coordinate c of a ladder's probe: member 0 of a group is the base point itself, members 1..K are base + dir * e_k, members
// K + 1..2K base - dir * e_k: one multiply, then one add or subtract
__host__ __device__ inline double ladder_probe(double base, double dir, double e, bool minus) {
    const double d = dir * e;
    return minus ? base - d : base + d;
}

struct FateArgs {
    SearchCoeffs map;             // the held picture's, canonicalised; wave-uniform
    double box_lo[3], scale[3];   // the held box: scale = grid / (box_hi - box_lo)
    double bound;
    double dir[3];                // the ladder's direction
    double eps[kMaxLadderLevels]; // the ladder's e_k = ldexp(eps0, -(k - 1)), entry k - 1
    const uint32_t* label;        // [grid^3] the held table: a cell's attractor label, kBasinEmpty where no tail went
    const double* points;         // [n][3] this launch's points (k_basin_fate) or base points (k_basin_ladder)
    sar_basin_fate* fates;        // [n] the points' fates / the base points' own fates
    sar_basin_ladder_mask* masks; // [n] k_basin_ladder: the base points' level bits
    unsigned long long* counts;   // [levels][2] k_basin_ladder: uncertain, unknown per level (zero before the first launch)
    uint32_t n;                   // points / base points of this launch
    uint32_t transient, steps;    // each <= 2^31, the sum below 2^32
    uint32_t grid;
    uint32_t levels;              // K
    uint32_t _pad;
};

// lanes per base point, and base points per wave: g = 1 + 2K <= 63, so at least one
inline uint32_t ladder_group(uint32_t levels) { return 1u + 2u * levels; }
inline uint32_t ladder_groups_per_wave(uint32_t levels) { return 64u / ladder_group(levels); }

// launch wrappers (sar_fate.hip)
void launch_basin_fate(const FateArgs& a, hipStream_t s);
void launch_basin_ladder(const FateArgs& a, hipStream_t s);

}  // namespace sar
