// sar_manifold.hpp — what the two halves of the unstable-manifold family share (include/sar.h: sar_manifold_*, sar_runtime_manifold):
// the limits, the projection of a point into the view (one text for sar_manifold_pixel on the host and k_manifold on the device), a
// branch's block, the counters a branch's waves add into, the argument block of k_manifold (sar_manifold.hip) and its launch wrapper,
// called from sar_manifold.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kMaxManifoldPeriod = 128;
constexpr uint32_t kMinManifoldSamples = 2;
constexpr uint32_t kMaxManifoldSamples = 1u << 20;
constexpr uint32_t kMaxManifoldSteps = 65535;        // first = n * 4096 + branch stays below 2^28 + 2^12
constexpr uint32_t kMaxManifoldSpan = 4096;          // a lane's plots of one step; 2 k dX + L stays far inside an int
constexpr uint32_t kMaxManifoldBranches = 4096;      // the branch's 12 bits of `first`
constexpr uint32_t kMaxManifoldLanes = 1u << 26;     // per call
constexpr uint32_t kManifoldWaveSegments = 63;       // a wave's 64 points bound 63 segments; the seam point is computed twice
constexpr uint32_t kManifoldNone = 0xFFFFFFFFu;      // first[pix] of a pixel never plotted, first_long_step without a long segment
constexpr double kManifoldPlaced = 1073741824.;      // 2^30: a placed point has -2^30 <= fi, fj < 2^30, so dX, dY fit an int

// fi, fj of (x, y, z): iterate_once's projection (sar_device.hpp), operation for operation — screen_space, center_camera, the
// angle's rotation, then the two pixel coordinates — with the constants fill_map_params hoists.
__host__ __device__ inline void manifold_project(const MapParams& p, double x, double y, double z, double& fi, double& fj) {
    const double sx = p.m[0] * x + p.m[1] * y + p.m[2] * z;
    const double sy = p.m[3] * x + p.m[4] * y + p.m[5] * z;
    const double sz = p.m[6] * x + p.m[7] * y + p.m[8] * z;
    const double ax = sx + p.ccx;
    const double az = sz + p.ccy;
    const double x2 = ax * p.cos_v + az * p.sin_v;
    fi = (p.scale_adjusted_mid - x2) * p.width_scaled;
    fj = p.half_height - (sy + p.ccz) * p.width_scaled;
}

// A branch as the device reads it, wave-uniform: the fundamental domain's first end, d = b - a, and whether the domain stayed in bounds
struct ManifoldBranch {
    double a[3];
    double d[3];
    uint32_t live;   // 0: SAR_MANIFOLD_DOMAIN_ESCAPED, its waves leave at once
    uint32_t _pad;
};
static_assert(sizeof(ManifoldBranch) == 56, "load_frame_args reads it as seven 8-byte words");

// What a branch's waves add into, one per branch; the host turns it into the record
struct ManifoldSums {
    unsigned long long drawn, dead, far, longs, pixels, length_px;
    uint32_t first_long_step;   // kManifoldNone before the launch; atomicMin
    uint32_t alive_end;
};
static_assert(sizeof(ManifoldSums) == 56, "six 64-bit sums and two words");

struct ManifoldArgs {
    MapParams p;                        // cfg's map (all 30 coefficients canonicalised) and view
    const ManifoldBranch* branches;     // [n_branches]
    ManifoldSums* sums;                 // [n_branches]
    uint32_t* count;                    // [height * width], zero before the launch
    uint32_t* first;                    // [height * width], kManifoldNone before the launch
    uint32_t n_branches, samples, steps, max_span;
    uint32_t waves_per_branch;          // ceil((samples - 1) / 63)
    uint32_t width, height;
    uint32_t _pad;
    double bound;
};

inline uint32_t manifold_waves_per_branch(uint32_t samples) { return (samples - 1u + kManifoldWaveSegments - 1u) / kManifoldWaveSegments; }

// launch wrapper (sar_manifold.hip)
void launch_manifold(const ManifoldArgs& a, hipStream_t s);

}  // namespace sar
