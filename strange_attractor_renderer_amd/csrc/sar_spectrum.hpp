// sar_spectrum.hpp — what the two halves of the power spectra share (include/sar.h: sar_spectra_*, sar_runtime_spectra,
// sar_spectrum_*, sar_runtime_spectrum): the limits, the padded LDS index of the transform, the argument block of k_spectrum and
// k_spectrum_fold (sar_spectrum.hip) and their launch wrappers, called from sar_spectrum.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_corr.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kSpectrumBlock = 256;              // lanes per workgroup of both kernels
constexpr uint32_t kSpectrumMinLog2 = 3;              // N = 8
constexpr uint32_t kSpectrumMaxLog2 = 12;             // N = 4096: re and im take 64 KiB of LDS, two workgroups share a CU's 160 KiB
constexpr uint32_t kSpectrumMaxN = 1u << kSpectrumMaxLog2;
constexpr uint32_t kSpectrumPadLog2 = 4;              // the 16 lanes of one ds_write_b64 group
constexpr uint32_t kDefaultSpectrumChunk = 1u << 16;  // (set, job) workgroups per launch
constexpr uint32_t kMaxSpectrumChunk = 1u << 30;

// The LDS index of element i of an N = 2^log2n array. The bit-reversed store sends 16 neighbouring lanes to elements N / 16 apart:
// one more double every N / 16 elements spreads them over 16 banks. Below N = 256 nothing is padded.
#if !defined(SAR_SPECTRUM_PAD) || SAR_SPECTRUM_PAD
__host__ __device__ inline uint32_t spectrum_pad_shift(uint32_t log2n) { return log2n >= 8u ? log2n - kSpectrumPadLog2 : 31u; }
#else  // (A/B builds: no padding)
__host__ __device__ inline uint32_t spectrum_pad_shift(uint32_t) { return 31u; }
#endif
__host__ __device__ inline uint32_t spectrum_lds_doubles(uint32_t log2n) {
    const uint32_t n = 1u << log2n;
    return 2u * (n + (n >> spectrum_pad_shift(log2n)));
}
constexpr uint32_t kSpectrumMaxLdsBytes = 2u * (kSpectrumMaxN + (1u << kSpectrumPadLog2)) * 8u;

struct SpectrumArgs {
    const double* points;        // [sets of the group][3][n_points] SoA
    const CorrMapState* state;   // nullable: [sets of the group]; a set whose state has a failure is all +0.0
    const double* twiddles;      // [N / 2][2]
    const double* window;        // [N]
    double* scratch;             // [sets of the group][jobs][row]: P_j[0 .. N / 2], then E_j
    double* power;               // [sets of the group][row]: P[0 .. N / 2], then E
    uint32_t n_points;           // per set: jobs * samples
    uint32_t jobs, samples, segments;
    uint32_t log2n, hop;
    uint32_t row;                // N / 2 + 2
    uint32_t _pad;
    double inv_n;                // 1.0 / N, exact
    double proj[3];
};

// workgroups [first, first + count) of the group's sets * jobs: 0, or the hipError_t of setting the LDS attribute
int launch_spectrum(const SpectrumArgs& a, uint32_t first, uint32_t count, hipStream_t s);
void launch_spectrum_fold(const SpectrumArgs& a, uint32_t n_sets, hipStream_t s);

}  // namespace sar
