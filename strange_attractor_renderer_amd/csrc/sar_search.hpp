// sar_search.hpp — what the host (sar_search.cpp) and the device (sar_search.hip) of the chaotic-map search share: the
// random-access candidate generator, bit for bit the same on both sides, and the kernels' argument block.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kSearchCoeffs = 30;
// candidates per launch: 28 B of survivor scratch each, and a 144-byte record per survivor. Phase 2 runs only the survivors of
// the transient (2.7 % of the default box): 2^22 candidates leave ~115 000 lanes, under two waves per SIMD of the chip.
constexpr uint32_t kDefaultSearchChunk = 1u << 22;
constexpr uint32_t kMaxSearchChunk = 1u << 30;  // the kernels' 32-bit slot arithmetic (2 n + slot, the grid) stays below 2^32
constexpr uint32_t kMaxSearchSteps = 1u << 31;  // transient / steps: the kernels' step counters advance by 16 and must not wrap

// SplitMix64's finaliser (Steele, Lea & Flood / Vigna, splitmix64.c)
__host__ __device__ inline uint64_t search_mix64(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// Coefficient j (0..29: x row, y row, z row) of candidate `index`: draw k = 30 index + j of the stream, mapped into
// [lo, hi) with a multiply and an add (span = hi - lo, computed once by the caller), -0.0 canonicalised.
__host__ __device__ inline double search_coeff(uint64_t seed, double lo, double span, uint64_t index, uint32_t j) {
    const uint64_t k = index * kSearchCoeffs + j;
    const uint64_t d = search_mix64(seed + (k + 1u) * 0x9e3779b97f4a7c15ull);
    const double u = static_cast<double>(d >> 11) * 0x1.0p-53;
    const double c = lo + span * u;
    return 0. + 1. * c;
}

// One launch chunk of sar_runtime_search; the same block goes to both kernels.
struct SearchArgs {
    uint64_t seed;
    double lo, span;              // generated candidates: lo and hi - lo
    const double* coeffs;         // nullable: the caller's [n][30] for this chunk (canonicalised), instead of generating
    uint64_t first;               // candidate index of chunk slot 0
    uint32_t n;                   // candidates in this chunk
    uint32_t transient, steps;
    uint32_t _pad;
    double start[3];
    double bound;
    uint32_t* counters;           // [0] survivors of the transient, [1] candidates that died in it
    uint32_t* surv_idx;           // [n] chunk slot of every survivor, by survivor slot
    double* surv_xyz;             // [3][n] SoA: the point after the transient, by survivor slot
    sar_search_record* records;   // [survivors] by survivor slot: the raw fields (lyapunov / ky_dim are the host's)
};

// launch wrappers (sar_search.hip)
void launch_search_screen(const SearchArgs& a, hipStream_t s);
void launch_search_lyapunov(const SearchArgs& a, uint32_t survivors, hipStream_t s);  // survivors: counters[0], read back

}  // namespace sar
