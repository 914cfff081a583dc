// sar_section.hpp — what the two halves of the Poincare sections share (include/sar.h: sar_section_*, sar_runtime_section): the
// surface function g, its gradient, one counted step with the crossing test and Henon's refinement (one text for sar_section_step on
// the host and k_flow_section on the device, as flow_step is), the block the kernels' sums reduce into, the argument blocks of the
// kernels and their launch wrappers, called from sar_section.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_flow.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kMaxSectionSamples = 1u << 20;      // recorded crossings per job
constexpr uint64_t kMaxSectionCrossings = 1ull << 24;  // n_jobs * samples: what a call may record
constexpr uint32_t kSectionNone = 0xFFFFFFFFu;         // clock_step of a job without a clock crossing
constexpr uint32_t kSectionRows = 6u;                  // SectionArgs::rows

// g(p) = s . [1, x, x^2, xy, xz, y, y^2, yz, z, z^2]; d2, d6, d9 are 2 * s[2], 2 * s[6], 2 * s[9], doubled on the host (exact)
struct SectionSurface {
    double s[10];
    double d2, d6, d9;
};

// g, summed as next_point sums a row: g = s0, then g = g + t[k] * s[k + 1], left to right
__host__ __device__ inline double section_g(const SectionSurface& f, double x, double y, double z) {
    double g = f.s[0];
    g = g + x * f.s[1];
    g = g + (x * x) * f.s[2];
    g = g + (x * y) * f.s[3];
    g = g + (x * z) * f.s[4];
    g = g + y * f.s[5];
    g = g + (y * y) * f.s[6];
    g = g + (y * z) * f.s[7];
    g = g + z * f.s[8];
    g = g + (z * z) * f.s[9];
    return g;
}

__host__ __device__ inline bool section_finite(double v) {
    const double a = v < 0. ? -v : v;
    return a <= 1.7976931348623157e308;  // false for an infinity and for a NaN
}

// The right-hand side of Henon's system at p, g the independent variable: (dp/dg, dt/dg) = (P(p) * w, w), w = 1.0 / gdot,
// gdot = (gx * Px + gy * Py) + gz * Pz with the gradient of include/sar.h. One division.
template <typename Eval>
__host__ __device__ inline void section_rate(const Eval& eval, const SectionSurface& f, double x, double y, double z, double& kx, double& ky,
                                             double& kz, double& kt) {
    double px = x, py = y, pz = z;
    eval(px, py, pz);
    const double gx = ((f.s[1] + f.d2 * x) + f.s[3] * y) + f.s[4] * z;
    const double gy = ((f.s[5] + f.s[3] * x) + f.d6 * y) + f.s[7] * z;
    const double gz = ((f.s[8] + f.s[4] * x) + f.s[7] * y) + f.d9 * z;
    const double gdot = (gx * px + gy * py) + gz * pz;
    const double w = 1.0 / gdot;
    kx = px * w;
    ky = py * w;
    kz = pz * w;
    kt = w;
}

// One classical RK4 step of Henon's system from (p0, t = 0) with the step D = -g0, in flow_step's operand order: the point q on the
// surface and the time dt from p0 to it. Five divisions (D / 6.0 and four rates). Returns whether it is accepted: 0 <= dt <= h and q
// within the bound, both false for a NaN.
template <typename Eval>
__host__ __device__ inline bool section_henon(const Eval& eval, const SectionSurface& f, double h, double bound, double g0, double x, double y,
                                              double z, double& qx, double& qy, double& qz, double& dt) {
    const double D = -g0, D2 = D * 0.5, D6 = D / 6.0;
    double k1x, k1y, k1z, k1t, k2x, k2y, k2z, k2t, k3x, k3y, k3z, k3t, k4x, k4y, k4z, k4t;
    section_rate(eval, f, x, y, z, k1x, k1y, k1z, k1t);
    section_rate(eval, f, x + D2 * k1x, y + D2 * k1y, z + D2 * k1z, k2x, k2y, k2z, k2t);
    section_rate(eval, f, x + D2 * k2x, y + D2 * k2y, z + D2 * k2z, k3x, k3y, k3z, k3t);
    section_rate(eval, f, x + D * k3x, y + D * k3y, z + D * k3z, k4x, k4y, k4z, k4t);
    qx = x + D6 * (((k1x + 2.0 * k2x) + 2.0 * k3x) + k4x);
    qy = y + D6 * (((k1y + 2.0 * k2y) + 2.0 * k3y) + k4y);
    qz = z + D6 * (((k1z + 2.0 * k2z) + 2.0 * k3z) + k4z);
    dt = 0.0 + D6 * (((k1t + 2.0 * k2t) + 2.0 * k3t) + k4t);
    const double ax = qx < 0. ? -qx : qx, ay = qy < 0. ? -qy : qy, az = qz < 0. ? -qz : qz;
    return (int)(0.0 <= dt) & (int)(dt <= h) & (int)(ax <= bound) & (int)(ay <= bound) & (int)(az <= bound);
}

// One counted step of a job: p0 = (x, y, z) -> p1 by flow_step, g1 = g(p1) (g0 = g(p0) is the caller's: the previous step's g1), the
// crossing test for `direction` and, on a crossing alone, its refinement. Returns the kind: -1 escaped (p1 fails the bound test and
// no crossing is looked for), 0 no crossing, 1 Henon's step accepted, 2 rough (linear interpolation; one more division). On 1 and 2
// (qx, qy, qz) is the crossing and dt the time from p0 to it.
template <typename Eval>
__host__ __device__ inline int section_step(const Eval& eval, const SectionSurface& f, double h, double h2, double h6, double bound,
                                            int32_t direction, double g0, double& x, double& y, double& z, double& g1, double& qx, double& qy,
                                            double& qz, double& dt) {
    const double x0 = x, y0 = y, z0 = z;
    if (!flow_step(eval, h, h2, h6, bound, x, y, z)) return -1;
    g1 = section_g(f, x, y, z);
    const bool side0 = g0 >= 0., side1 = g1 >= 0.;
    const bool up = !side0 && side1, down = side0 && !side1;
    const bool wanted = (up && direction >= 0) || (down && direction <= 0);
    if (!(wanted && section_finite(g0) && section_finite(g1))) return 0;
    if (section_henon(eval, f, h, bound, g0, x0, y0, z0, qx, qy, qz, dt)) return 1;
    const double theta = g0 / (g0 - g1);
    qx = x0 + theta * (x - x0);
    qy = y0 + theta * (y - y0);
    qz = z0 + theta * (z - z0);
    dt = theta * h;
    return 2;
}

// What the workgroups of k_flow_section and k_section_plot add into, one per call
struct SectionSums {
    unsigned long long steps;                      // counted steps whose point stayed within the bound
    unsigned long long crossings, rough;           // recorded crossings; those of them that are rough
    unsigned long long clocked;                    // jobs that found their clock crossing
    unsigned long long full, escaped, escaped_transient;  // jobs
    unsigned long long visits, outside;            // k_section_plot: recorded crossings inside / outside the image
    unsigned long long lo[3], hi[3];               // sortable images of the recorded crossings' extent: kFlowNoMin / 0 before any
    unsigned long long ret_lo, ret_hi;             // of the return times, likewise
    unsigned long long residual;                   // sortable image of the largest |g(q)|; 0 before any
};
static_assert(sizeof(SectionSums) == 144, "nine 64-bit sums and nine keys");

struct SectionArgs {
    MapParams p;                   // cfg's field, as render hoists it (the view is k_section_plot's)
    SectionSurface f;
    double* state;                 // [3][n_jobs] SoA: FlowState::d_state, x NaN once the job has escaped
    double* dt_prev;               // [n_jobs]: the time from its step's p0 to the previous crossing
    uint32_t* rows;                // [kSectionRows][n_jobs]: status, found, rough, steps, clock_step, t_prev
    double* cross;                 // [n_jobs][samples][4]: a recorded crossing's q and its return time, 32 bytes
    SectionSums* sums;
    double h, h2, h6, bound;
    uint32_t n_jobs, n_steps;
    uint32_t t0;                   // counted steps every running job of this chunk has behind it
    uint32_t samples;
    int32_t direction;
    uint32_t _pad;
};

struct SectionPlotArgs {
    MapParams p;                   // cfg's view
    const double* cross;
    const uint32_t* found;         // SectionArgs::rows' row 1
    uint32_t* count;               // the runtime's count
    unsigned long long* keys;      // FlowState::d_keys
    SectionSums* sums;
    uint32_t n_jobs, samples, width, _pad;
};

// launch wrappers (sar_section.hip)
void launch_flow_section(const SectionArgs& a, hipStream_t s);
void launch_section_plot(const SectionPlotArgs& a, hipStream_t s);

}  // namespace sar
