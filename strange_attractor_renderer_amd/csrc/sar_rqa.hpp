// sar_rqa.hpp — what the two halves of the recurrence analysis share (include/sar.h: sar_recurrence_*, sar_runtime_recurrence,
// sar_runtime_recurrence_plot, sar_rqa_*, sar_runtime_rqa): the limits, the bands of diagonals and their folding, the layout of a
// set's counts in device memory, the argument block of k_rqa_diag, k_rqa_vert and k_rqa_plot (sar_rqa.hip) and their launch
// wrappers, called from sar_rqa.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_corr.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kRqaBlock = 256;              // lanes per workgroup: diagonals of a band (k_rqa_diag), columns of a tile (k_rqa_vert)
constexpr uint32_t kRqaWalk = 256;               // i points per LDS chunk of a walk
constexpr uint32_t kRqaMinBins = 2;
constexpr uint32_t kRqaMaxBins = 4096;           // B
#ifndef SAR_RQA_REPLICAS
#define SAR_RQA_REPLICAS 32                      // (A/B builds: -DSAR_RQA_REPLICAS=1 keeps one copy)
#endif
constexpr uint32_t kRqaMaxReplicas = SAR_RQA_REPLICAS;  // copies of the LDS histogram, one per LDS bank, as k_corr_pairs'
static_assert(kRqaMaxReplicas >= 1 && kRqaMaxReplicas <= 32 && (kRqaMaxReplicas & (kRqaMaxReplicas - 1)) == 0, "a power of two up to the banks of a half");
constexpr uint32_t kRqaHistLdsBytes = 64u << 10; // what the copies may take: with the 18 KiB of points two workgroups share a CU's 160 KiB
constexpr uint32_t kDefaultRqaChunk = 1u << 16;  // workgroups per launch
constexpr uint32_t kMaxRqaChunk = 1u << 30;

// The 32-bit counters in LDS. A lane walks at most two diagonals (a folded pair of bands) or one column of at most 2^20 entries, and
// a line takes at least one entry and — but for the last of a walk — one gap: a workgroup finishes at most 2 * 256 * 2^20 / 2 = 2^28
// lines, which bounds the sum of a bin's copies; it sees at most 2 * 256 * 2^20 = 2^29 recurrent entries. The spare row counts the
// entries that finish no line, at most 2 * 2^20 per copy. Nothing wraps. The sums per set are 64-bit.
static_assert(2ull * kRqaBlock * kCorrMaxPoints < (1ull << 32), "the recurrences of a workgroup fit 32 bits");

// log2 of the copies of a histogram of B + 2 rows — bins 0 .. B and the spare row — that the LDS budget holds
__host__ __device__ inline uint32_t rqa_rep_shift(uint32_t line_bins) {
    uint32_t rep = kRqaMaxReplicas, shift = 0;
    while (rep > 1u && (line_bins + 2u) * rep * 4u > kRqaHistLdsBytes) rep >>= 1;
    while ((1u << shift) < rep) ++shift;
    return shift;
}

// The diagonals k = theiler + 1 .. T - 1 of a trajectory of T points in bands of 256 neighbours; band b and band nb - 1 - b go to
// one workgroup (the middle band of an odd nb alone), so that every workgroup walks about T entries per lane.
__host__ __device__ inline uint32_t rqa_diagonals(uint32_t samples, uint32_t theiler) { return samples > theiler + 1u ? samples - theiler - 1u : 0u; }
__host__ __device__ inline uint32_t rqa_bands(uint32_t samples, uint32_t theiler) { return (rqa_diagonals(samples, theiler) + kRqaBlock - 1u) / kRqaBlock; }
__host__ __device__ inline uint32_t rqa_folded_bands(uint32_t samples, uint32_t theiler) { return (rqa_bands(samples, theiler) + 1u) / 2u; }

// A set's counts in device memory: [diag: B + 1][vert: B + 1][recurrences, diag_longest, vert_longest, unused], 64-bit each
__host__ __device__ inline uint32_t rqa_row(uint32_t line_bins) { return 2u * (line_bins + 1u) + 4u; }

struct RqaArgs {
    const double* points;        // [sets of the group][3][n] SoA
    const double* eps2;          // [sets of the group]: a set whose eps2 is not > 0 (a DIVERGED map, a fixed point) is skipped
    unsigned long long* out;     // [sets of the group][rqa_row(line_bins)], zero before the first launch
    uint32_t n, jobs, samples;   // n = jobs * samples
    uint32_t theiler;            // <= samples
    uint32_t line_bins;          // B
    uint32_t rep_shift;
    uint32_t per_job;            // workgroups per trajectory: folded bands (k_rqa_diag), column tiles (k_rqa_vert)
    uint32_t _pad;
};

struct RqaPlotArgs {
    const double* points;        // [3][samples]: one trajectory
    unsigned char* out;          // [height][width]
    uint32_t samples, theiler;
    uint32_t i0, j0, height, width;
    double eps2;
};

// workgroups [first, first + count) of the group's sets * jobs * per_job: 0, or the hipError_t of setting the LDS attribute
int launch_rqa_diag(const RqaArgs& a, uint32_t first, uint32_t count, hipStream_t s);
int launch_rqa_vert(const RqaArgs& a, uint32_t first, uint32_t count, hipStream_t s);
void launch_rqa_plot(const RqaPlotArgs& a, hipStream_t s);

}  // namespace sar
