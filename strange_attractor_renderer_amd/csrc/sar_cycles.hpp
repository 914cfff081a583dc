// sar_cycles.hpp — what the two halves of the cycles family share (include/sar.h: sar_cycles_*, sar_cycle_charpoly,
// sar_runtime_cycles): what a start finds, the argument block of the kernels of sar_cycles.hip and their launch wrappers, called
// from sar_cycles.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"
#include "sar_search.hpp"

namespace sar {

constexpr uint32_t kMaxCyclePeriod = 64;
constexpr uint32_t kMaxCycleJobs = 4096;           // a map's starts are merged in one workgroup's LDS
constexpr uint32_t kMaxCycleNewton = 1u << 16;     // jobs * max_newton, the sum of a map's iterations, stays below 2^32
constexpr uint32_t kMaxCycleCap = kMaxCycleJobs;
constexpr uint32_t kDefaultCyclesChunk = 1u << 21; // (map, start) lanes per launch: 120 B of finds each
constexpr uint32_t kMaxCyclesChunk = 1u << 30;
constexpr uint32_t kCycleMergeThreads = 256;
constexpr uint32_t kCycleLdsPerStart = 32;         // k_cycles_merge: the representative (3 doubles), the period word, the leader word
constexpr uint32_t kMaxCycleMaps = 1u << 20;       // per call

// What k_cycles_newton leaves per (map, start) for k_cycles_merge: the fields of an orbit slot where the start CONVERGED, zeros
// otherwise but for status and iterations.
struct CycleFind {
    double rep[3];
    uint32_t q;          // the minimal period; 0 where the start did not converge
    int32_t status;      // SAR_CYCLE_*
    uint32_t iterations;
    uint32_t _pad;
    double residual;
    double M[9];
};
static_assert(sizeof(CycleFind) == 120, "k_cycles_newton writes it word by word");

struct CyclesArgs {
    const SearchCoeffs* coeffs;   // [maps of the launch]: canonicalised
    const double* starts;         // [jobs][3]: the same for every map
    CycleFind* finds;             // [maps of the launch][jobs]
    sar_cycles_record* records;   // [maps of the launch]
    sar_cycle_orbit* orbits;      // [maps of the launch][cap]
    uint32_t n_maps;              // of the launch
    uint32_t jobs;
    uint32_t period, max_newton, cap;
    uint32_t _pad;
    double tol, bound, merge, same;
};

// launch wrappers (sar_cycles.hip)
void launch_cycles_newton(const CyclesArgs& a, hipStream_t s);
int launch_cycles_merge(const CyclesArgs& a, hipStream_t s);  // 0, or the hipError_t of setting the LDS attribute

}  // namespace sar
