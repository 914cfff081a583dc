// sar_flow.hpp — what the two halves of flow rendering share (include/sar.h: sar_flow_*, sar_runtime_render_flow): the limits, the
// RK4 step (one text for sar_flow_step on the host and the kernels of sar_flow.hip on the device), the block the kernels' sums
// reduce into, the argument blocks of the kernels and their launch wrappers, called from sar_flow.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kDefaultFlowChunkJobs = 1u << 17;   // jobs per launch: 2048 waves, eight per CU
constexpr uint32_t kDefaultFlowChunkSteps = 1u << 12;  // RK4 steps per job and launch (four evaluations of the polynomial each)
constexpr uint32_t kMaxFlowChunk = 1u << 24;           // either chunk: a lane's counters of one launch are 32-bit words
constexpr uint64_t kMaxFlowPlots = 0xFFFFFFFFull;      // steps_per_job / stride: what one job may add to a pixel
constexpr unsigned long long kFlowNoMin = ~0ull;       // FlowSums::lo before any point (no double has that sortable image but a NaN)

// One classical RK4 step of p' = P(p) with the fixed step h, in include/sar.h's order: h2 = h * 0.5 and h6 = h / 6.0 are the host's,
// eval(x, y, z) replaces the point by P(point) (next_point's polynomial, operand for operand). Multiplies and adds only, each its own
// IEEE operation. Returns whether the new point passes max(|x'|, |y'|, |z'|) <= bound; a NaN fails.
template <typename Eval>
__host__ __device__ inline bool flow_step(const Eval& eval, double h, double h2, double h6, double bound, double& x, double& y, double& z) {
    double k1x = x, k1y = y, k1z = z;
    eval(k1x, k1y, k1z);
    double k2x = x + h2 * k1x, k2y = y + h2 * k1y, k2z = z + h2 * k1z;
    eval(k2x, k2y, k2z);
    double k3x = x + h2 * k2x, k3y = y + h2 * k2y, k3z = z + h2 * k2z;
    eval(k3x, k3y, k3z);
    double k4x = x + h * k3x, k4y = y + h * k3y, k4z = z + h * k3z;
    eval(k4x, k4y, k4z);
    x = x + h6 * (((k1x + 2.0 * k2x) + 2.0 * k3x) + k4x);
    y = y + h6 * (((k1y + 2.0 * k2y) + 2.0 * k3y) + k4y);
    z = z + h6 * (((k1z + 2.0 * k2z) + 2.0 * k3z) + k4z);
    const double ax = x < 0. ? -x : x, ay = y < 0. ? -y : y, az = z < 0. ? -z : z;
    return (int)(ax <= bound) & (int)(ay <= bound) & (int)(az <= bound);  // every compare is false for a NaN
}

// What the workgroups of k_flow_transient and k_flow_render add into, one per call
struct FlowSums {
    unsigned long long steps;              // counted steps whose point stayed within the bound
    unsigned long long visits, outside;    // plotted points inside / outside the image
    unsigned long long count_atomics;      // run flushes: the atomic adds on count
    unsigned long long key_atomics;        // run flushes that held a depth: the key raises offered (include/sar.h)
    unsigned long long escaped_transient, escaped;  // jobs
    unsigned long long lo[3], hi[3];       // sortable images of the counted points' extent: kFlowNoMin / 0 before any
};
static_assert(sizeof(FlowSums) == 104, "seven 64-bit sums and six keys");

struct FlowArgs {
    MapParams p;                   // cfg's field and view, as render hoists them
    ColorTransformParams ct;
    double* state;                 // [3][n_jobs] SoA: every job's point between launches; x is NaN once the job has escaped
    uint32_t* count;               // the runtime's count
    unsigned long long* keys;      // [npix]: this call's keys, zero before the first launch
    FlowSums* sums;
    double h, h2, h6, bound;
    uint32_t n_jobs, n_steps, width, stride;
    uint32_t phase;                // counted steps this job has behind it, modulo stride
    int32_t plot;
};

struct FlowResolveArgs {
    const unsigned long long* keys;   // [npix]: the call's keys
    const uint32_t* count;
    unsigned long long* zkey;         // the runtime's depth keys
    double* steps;
    uint32_t* scalars;
    uint32_t npix, _pad;
};

// launch wrappers (sar_flow.hip)
void launch_flow_transient(const FlowArgs& a, hipStream_t s);
void launch_flow_render(const FlowArgs& a, hipStream_t s);
void launch_flow_resolve(const FlowResolveArgs& a, hipStream_t s);

}  // namespace sar
