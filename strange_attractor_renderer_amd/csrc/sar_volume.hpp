// sar_volume.hpp — what the two halves of volume rendering share (include/sar.h: sar_volume_*, sar_runtime_volume*): the limits, the
// slab of a depth (one text for sar_volume_slab on the host and k_volume_accumulate on the device), the blocks the kernels' sums
// reduce into, the argument blocks of the kernels of sar_volume.hip and their launch wrappers, called from sar_volume.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kMaxVolumeSlabs = 1024;
constexpr uint64_t kMaxVolumeVoxels = 1ull << 30;    // W * H * D: a voxel index fits 32 bits, the volume 4 GiB
constexpr uint32_t kMaxVolumeJobs = 1u << 24;
constexpr uint64_t kMaxVolumeIters = 1ull << 40;
constexpr uint32_t kDefaultVolumeChunk = 1u << 17;   // jobs per launch: 2048 waves, eight per CU
constexpr uint32_t kDefaultVolumeSteps = 1u << 16;   // counted iterations per job and launch
constexpr uint32_t kMaxVolumeChunk = 1u << 24;
constexpr uint32_t kMaxVolumeSteps = 1u << 24;       // a lane's class counters of one launch are 32-bit words
constexpr int32_t kVolumeBelow = -1, kVolumeAbove = -2, kVolumeNan = -3;
constexpr uint32_t kVolumeNoMin = 0xFFFFFFFFu;       // VolumeSums::zmin_key before any finite depth (no finite f32 has that key)

// The slab of the f32 depth zf: u = ((double)zf - z_lo) * dscale, a subtraction, then a multiplication; NaN, below 0 and at or beyond
// D are the three classes without a slab, anything else truncates to its slab.
__host__ __device__ inline int32_t volume_slab(float zf, double z_lo, double dscale, double slabs_f) {
    const double u = ((double)zf - z_lo) * dscale;
    if (u != u) return kVolumeNan;
    if (u < 0.) return kVolumeBelow;
    if (u >= slabs_f) return kVolumeAbove;
    return (int32_t)(uint32_t)u;
}

// What the accumulate kernel's workgroups and the reduction pass add into, one per call
struct VolumeSums {
    unsigned long long visits, below, above, nan;   // this call's in-bounds visits and the three classes without a slab
    unsigned long long nonempty;                    // k_volume_reduce: voxels != 0
    uint32_t vmax;                                  // k_volume_reduce: the largest voxel
    uint32_t zmin_key, zmax_key;                    // sortable images of the smallest / largest finite depth: kVolumeNoMin / 0 before
    uint32_t _pad;
};
static_assert(sizeof(VolumeSums) == 56, "five 64-bit sums and four words");

struct VolumeMarchSums {
    unsigned long long slabs_seen;
    uint32_t covered, stopped;
};
static_assert(sizeof(VolumeMarchSums) == 16, "sar_volume_march_stats' layout");

struct VolumeArgs {
    MapParams p;           // cfg's map and view, as render hoists them
    double* state;         // [3][n_jobs] SoA: every job's point, read at the start of a launch and written back at its end
    uint32_t* vol;         // [slabs][npix]
    VolumeSums* sums;
    double z_lo, dscale, slabs_f;
    uint32_t n_jobs, n_steps, width, npix;
};

struct VolumeSectionArgs {
    const uint32_t* vol;
    uint32_t* count;       // nullable: [npix]
    int32_t* nearest;      // nullable: [npix]
    uint32_t npix, k0, k1, _pad;
};

struct VolumeMarchArgs {
    const uint32_t* vol;
    ushort4* out;          // [npix]
    VolumeMarchSums* sums;
    uint32_t npix, slabs, k0, k1;
    int32_t transparent;
    int32_t _pad;
    double half, t_min, pos_lo, dpos, slabs_f;
    double bg[3];          // (double)background[c] / 65535.0, the host's division
    PaletteParams pal;
};

// launch wrappers (sar_volume.hip)
void launch_volume_warm(const VolumeArgs& a, hipStream_t s);
void launch_volume_accumulate(const VolumeArgs& a, hipStream_t s);
void launch_volume_reduce(const uint32_t* vol, size_t n, VolumeSums* sums, hipStream_t s);
void launch_volume_section(const VolumeSectionArgs& a, hipStream_t s);
void launch_volume_march(const VolumeMarchArgs& a, hipStream_t s);

}  // namespace sar
