// sar_orbit.hpp — what the two halves of the orbit diagrams share (include/sar.h: sar_orbit_*, sar_runtime_orbit): the function that
// builds a column's coefficients, bit for bit the same on the host and on the device, and the argument block
// of k_orbit (sar_orbit.hip), and its launch wrapper, called from sar_orbit.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"
#include "sar_search.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kMaxOrbitWidth = 65536;
constexpr uint32_t kMaxOrbitHeight = 32768;       // a column's histogram is 4 B per bin of LDS: 128 KiB of a CU's 160 KiB
constexpr uint32_t kMaxOrbitJobs = 1024;          // a column's trajectories are the lanes of one workgroup
constexpr uint32_t kDefaultOrbitChunk = 4096;     // columns per launch: sixteen workgroups per CU, keeps one dispatch short
constexpr uint32_t kMaxOrbitChunk = 1u << 16;

// Coefficient k of column c of `width`: a + span * t, t = c / (width - 1) (0 when width == 1), span = b - a computed once by the
// caller — a divide, a multiply and an add —, -0.0 canonicalised as the search and the planes do.
__host__ __device__ inline double orbit_coeff(double a, double span, uint32_t c, uint32_t width) {
    const double t = width > 1u ? (double)c / (double)(width - 1u) : 0.;
    const double v = a + span * t;
    return 0. + 1. * v;
}

// What differs from column to column is its map: one SearchCoeffs block per column in device memory. The workgroup reads its own
// through the constant address space (load_frame_args) — scalar loads into SGPRs.
struct OrbitArgs {
    const SearchCoeffs* cols;  // [width]: every column of the call
    const double* starts;      // [jobs][3]: the start points, the same for every column
    uint32_t* count;           // [height][width]: the whole diagram; a workgroup writes every row of its column
    sar_orbit_column* stats;   // [width]
    uint32_t* max;             // the diagram's largest bin (zero before the first launch)
    uint32_t first_col;        // the launch's first column; workgroup b takes column first_col + b
    uint32_t width, height;
    uint32_t jobs;
    uint32_t transient, steps; // each <= 2^31; jobs * steps < 2^32
    double bound;
    double proj[3];
    double v_lo, scale;        // scale = height / (v_hi - v_lo)
};

int launch_orbit(const OrbitArgs& a, uint32_t n_cols, hipStream_t s);  // 0, or the hipError_t of setting the LDS attribute

}  // namespace sar
