// sar_corr.hpp — what the two halves of the correlation dimension share (include/sar.h: sar_pairs_*, sar_runtime_pairs,
// sar_corrdim_*, sar_runtime_corrdim): the bin of a pair, bit for bit the same on the host and on the device, the folding of the
// tile-pair triangle into a rectangle, the argument blocks of k_corr_orbit and k_corr_pairs (sar_corr.hip) and their launch wrappers,
// called from sar_corr.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kCorrTile = 256;               // points per tile = lanes per workgroup of k_corr_pairs: one i point per lane
constexpr uint32_t kCorrMaxPoints = 1u << 20;     // per set
constexpr uint32_t kCorrMaxJobs = 1u << 16;
constexpr uint32_t kCorrMaxBins = 1024;
constexpr uint32_t kCorrMaxSubBits = 4;
constexpr uint32_t kCorrMaxReplicas = 32;         // copies of the LDS histogram, one per LDS bank (k_corr_pairs)
constexpr uint32_t kCorrHistLdsBytes = 64u << 10; // what the copies may take: with the 6 KiB j tile two workgroups share a CU's 160 KiB
constexpr uint32_t kDefaultCorrChunk = 1u << 18;  // workgroups per launch: 2^34 pairs, keeps one dispatch short
constexpr uint32_t kMaxCorrChunk = 1u << 30;
constexpr uint64_t kCorrPointBudget = 1ull << 24; // points in device memory at a time (24 B each): sets beyond it go in groups

// The binning of r^2 (sar_pairs_params): `base` = ((1023 + e_min) << s) - 1 and `top` = bins - 1, so that
// bin = clamp(key + 1, 0, top) with key = (bits(r^2) >> (52 - s)) - ((1023 + e_min) << s). Only the high word of r^2 is read
// (s <= 4 <= 20) and its sign bit is dropped: r^2 is a sum of squares, never negative, and a NaN (from infinite coordinates) lands
// in the overflow bin whatever sign the machine gave it.
struct CorrBinning {
    int32_t base;
    int32_t top;
    uint32_t shift;  // 20 - s
    uint32_t bins;
};

__host__ __device__ inline uint32_t corr_bin_hi(const CorrBinning& b, uint32_t hi) {
    const int32_t k = (int32_t)((hi & 0x7fffffffu) >> b.shift) - b.base;
    return (uint32_t)(k < 0 ? 0 : (k > b.top ? b.top : k));
}

// The tile pairs I <= J of nt tiles as a rectangle without holes: with m = nt | 1 (odd), the triangle of m rows has m (m + 1) / 2
// cells = (m + 1) / 2 rows of m. Cell (r, c) is the pair (r, c) for c >= r and (m - r, m - r + c) for c < r; for an even nt the
// pairs that touch tile nt (one row and one column of the larger triangle) do not exist and their workgroups return at once.
__host__ __device__ inline uint32_t corr_fold_m(uint32_t nt) { return nt | 1u; }
__host__ __device__ inline uint64_t corr_fold_cells(uint32_t nt) { return (uint64_t)corr_fold_m(nt) * ((corr_fold_m(nt) + 1u) / 2u); }
__host__ __device__ inline void corr_fold_pair(uint32_t m, uint32_t cell, uint32_t& I, uint32_t& J) {
    const uint32_t r = cell / m, c = cell % m;
    I = c >= r ? r : m - r;
    J = c >= r ? c : m - r + c;
}

// One map's state in device memory, raised by k_corr_orbit and read by k_corr_pairs (a DIVERGED set has no pairs).
struct CorrMapState {
    unsigned long long fail;      // (job << 40) | step of the first failure by (job, step), ~0: none. step is 1-based, transient included
    unsigned long long lo[3];     // sortable image of the smallest x, y, z recorded (~0: none)
    unsigned long long hi[3];     // of the largest (0: none)
};
constexpr unsigned long long kCorrNoFail = ~0ull;

// the sortable 64-bit image of a double: unsigned order == numeric order (-0.0 below +0.0). The device writes the keys with
// f64_sortable (sar_device.hpp; wave_extent, sar_tangent.hpp) — the same image, bit for bit; the host decodes them here
__host__ __device__ inline unsigned long long corr_sortable(unsigned long long bits) {
    return (bits >> 63) ? ~bits : (bits | (1ull << 63));
}
__host__ __device__ inline unsigned long long corr_unsortable(unsigned long long key) {
    return (key >> 63) ? (key & ~(1ull << 63)) : ~key;
}

struct CorrOrbitArgs {
    const double* coeffs;      // [maps of the group][30], canonicalised
    const double* starts;      // [jobs][3]
    double* points;            // [maps of the group][3][n] SoA, n = jobs * samples
    CorrMapState* state;       // [maps of the group]
    uint32_t first_map;        // the launch's first map of the group; blockIdx.y counts from it
    uint32_t jobs, samples, stride;
    uint32_t transient;
    uint32_t n;
    double bound;
};

struct CorrPairsArgs {
    const double* points;           // [sets of the group][3][n] SoA
    const CorrMapState* state;      // nullable: [sets of the group]; a set whose state has a failure is skipped
    unsigned long long* hist;       // [sets of the group][bins], zero before the first launch
    uint32_t fold_m;                // corr_fold_m(nt): a launch covers cells [first_cell, ..) of the folded triangle for sets [first_set, ..)
    uint32_t nt;                    // ceil(n / kCorrTile)
    uint32_t n, samples, theiler;   // theiler <= n
    uint32_t rep_shift;             // log2 of the LDS histogram's copies
    CorrBinning bin;
};

// The recorded orbits of maps, shared by sar_runtime_corrdim and sar_runtime_boxdim (sar_box.cpp); all in sar_corr.cpp. A group of
// maps shares rt->d_corr_points, d_corr_state and d_corr_coeffs.
struct CorrOrbitShape {
    uint32_t jobs, samples, stride, transient;
    uint64_t seed;
    double bound;
};
// the refusals of the shape (no device needed), then those of n_maps > 0 maps' coefficients and start points
int corr_check_shape(const char* where, const CorrOrbitShape& s);
int corr_check_maps(const char* where, const CorrOrbitShape& s, uint32_t n_maps, const double* coeffs_host, const double* starts_xyz_host);
// sets per group: what fits the device's point buffer
uint32_t corr_group_size(uint32_t n_sets, uint32_t n);
// grows the buffers for groups of `group` maps and uploads the start points (starts_xyz_host NULL: the stream of s.seed)
int corr_orbits_begin(sar_runtime* rt, const CorrOrbitShape& s, const double* starts_xyz_host, uint32_t group);
// one group: canonical coefficients and fresh states up, then k_corr_orbit over `maps` maps, "corr_chunk" blocks per launch, each
// launch a span of warmup_ms. Nothing is read back (read_map_group, sar_analysis.hpp).
int corr_orbits_run(sar_runtime* rt, const CorrOrbitShape& s, const double* coeffs_host /* [maps][30] */, uint32_t maps);

constexpr uint32_t kCorrMaxGridY = 65535;  // maps / sets per launch
void launch_corr_orbit(const CorrOrbitArgs& a, uint32_t n_maps, hipStream_t s);
// 0, or the hipError_t of setting the LDS attribute
int launch_corr_pairs(const CorrPairsArgs& a, uint32_t first_cell, uint32_t n_cells, uint32_t first_set, uint32_t n_sets, hipStream_t s);

}  // namespace sar
