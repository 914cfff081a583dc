// sar_search.hpp — what the host (sar_search.cpp) and the device (sar_search.hip) of the chaotic-map search share: the
// random-access candidate generator, bit for bit the same on both sides, and the kernels' argument block; and SearchCoeffs, the
// one coefficient block of every analysis family (the search, the planes, the orbit diagrams, the correlation dimension, the basins, the period planes, the cycles).
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kSearchCoeffs = 30;
// One map's 30 coefficients as next_point's rows (sar_device.hpp). Per lane in VGPRs where every lane steps a map of its own (the
// search, the planes, k_corr_orbit); wave-uniform where all lanes step one — a column's block of the orbit diagrams, read through the
// constant address space (load_frame_args), and the basins' map, a kernel argument.
struct SearchCoeffs {
    double cx[10], cy[10], cz[10];
};
static_assert(sizeof(SearchCoeffs) == kSearchCoeffs * sizeof(double), "30 coefficients: the x, y, z rows of a [30] array, read as 8-byte words");
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

// Lyapunov planes (sar_runtime_plane, include/sar.h): one launch of k_plane<K> over the 8 x 8 pixel tiles
// [first_tile, first_tile + n_tiles) of the plane, tiles row-major, tiles_x of them per row.
constexpr uint32_t kPlaneTile = 8;                 // a wave covers a tile of 8 x 8 pixels
constexpr uint32_t kDefaultPlaneChunk = 1u << 20;  // pixels per launch (whole tiles): keeps one dispatch short
constexpr uint32_t kMaxPlaneChunk = 1u << 30;
constexpr uint32_t kMaxPlanePixels = 1u << 24;     // per call
struct PlaneArgs {
    double base[kSearchCoeffs];   // canonicalised
    double lo[2], span[2];        // span = hi - lo
    uint32_t axis[2];             // the swept coefficients: axis[0] along x, axis[1] along y
    uint32_t width, height, tiles_x;
    uint32_t first_tile, n_tiles;
    uint32_t transient, steps;
    uint32_t _pad;
    double start[3];
    double bound;
    sar_plane_record* records;    // [height][width]: the raw fields (lyapunov / ky_dim are the host's)
};

// value i of n along one axis: lo + span * t, t = i / (n - 1) (0 when n == 1), a divide, a multiply and an add
__host__ __device__ inline double plane_sweep(double lo, double span, uint32_t i, uint32_t n) {
    const double t = n > 1u ? (double)i / (double)(n - 1u) : 0.;
    return lo + span * t;
}
// value of coefficient j at a pixel whose swept values are v0 (axis[0]) and v1 (axis[1]); -0.0 -> +0.0
__host__ __device__ inline double plane_pick(const PlaneArgs& a, uint32_t j, double v0, double v1) {
    const double c = j == a.axis[0] ? v0 : (j == a.axis[1] ? v1 : a.base[j]);
    return 0. + 1. * c;
}
// coefficient j of pixel (x, y): column x sweeps axis[0] from lo[0]; row y sweeps axis[1] with row 0 at the high end (y up, as
// in a plot) and row height - 1 at lo[1]
__host__ __device__ inline double plane_coeff(const PlaneArgs& a, uint32_t x, uint32_t y, uint32_t j) {
    return plane_pick(a, j, plane_sweep(a.lo[0], a.span[0], x, a.width), plane_sweep(a.lo[1], a.span[1], a.height - 1u - y, a.height));
}

// the host finish (sar_search.cpp): lambda_i = (E_i ln2 + ln M_i) / folded for the first k columns, sorted descending, and with
// k = 3 the Kaplan-Yorke dimension; the other exponents and (k = 1) ky_dim are NaN, and all of them without a folded step
void lyapunov_finish(const int64_t* log2_exp, const double* mant, int k, uint32_t folded, double* lyapunov, double* ky_dim);

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
// (sar_plane.hip)
void launch_plane(const PlaneArgs& a, int k, hipStream_t s);  // k = 1 (SAR_PLANE_L1) or 3 (SAR_PLANE_SPECTRUM)
void launch_plane_colorize(const sar_plane_record* rec, uint32_t npix, int k, const PaletteParams& pal, double threshold,
                           double chaos_scale, double order_scale, void* rgba16_out, hipStream_t s);

}  // namespace sar
