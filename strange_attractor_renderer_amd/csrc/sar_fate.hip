// sar_fate.hip — gfx950 (MI355X) kernels of the basin probes (include/sar.h: sar_runtime_basin_fates, sar_runtime_basin_uncertainty).
//
// Both kernels run a start point exactly as k_basin_screen runs a pixel (sar_basin.hip) — the same map, a kernel argument with the x
// and y rows scalar operands and the z row pinned into VGPRs, the same bound test at every step, the same checked stepping loop —
// and then, instead of packing survivors for a union-find, read the HELD picture's table label[node] along the tail until a cell has a
// label. k_basin_fate gives a lane one point. k_basin_ladder gives a GROUP of g = 1 + 2K neighbouring lanes one base point: lane 0
// of the group runs the base point, lanes 1..K the probes base + dir * e_k, lanes K + 1..2K base - dir * e_k. A group's probes start
// within eps0 of each other, so its lanes share their fate except where a boundary passes and a wave whose lanes are all dead stops
// early — the reason k_basin_screen takes 8 x 8 tiles. The map, the probe point and the node are multiplies, adds and compares: the
// build's fused-op audit pins both kernels at 0, and a host restatement gives every field bit for bit.
//
// BOUNDS. The table has grid^3 <= 128^3 = 2^21 entries and basin_cell clamps every coordinate into [0, grid) (a NaN to 0), so
// every index basin_node returns is in range by construction, whatever the point. Every other index is a point or base-point index
// below a.n, tested before use.
// DESIGN.md section 27 has the decomposition and the counter bounds.
#include "sar_fate.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

// The held box next to the map's x and y rows would not fit the scalar file (k_basin_fate spilt 36 SGPRs into VGPR lanes): like the
// z row it is pinned into VGPRs, which are plentiful here. (The 12 it still spills are read back between two runs of the checked
// loop, not inside one.)
struct FateBox {
    double lo[3], scale[3];
};
__device__ __forceinline__ FateBox pin_box(const FateArgs& a) {
    FateBox b;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = vgpr_pin(a.box_lo[k]);
        b.scale[k] = vgpr_pin(a.scale[k]);
    }
    return b;
}

__device__ __forceinline__ uint32_t fate_node(const FateBox& b, uint32_t grid, double x, double y, double z) {
    const uint32_t cx = basin_cell(x, b.lo[0], b.scale[0], grid);
    const uint32_t cy = basin_cell(y, b.lo[1], b.scale[1], grid);
    const uint32_t cz = basin_cell(z, b.lo[2], b.scale[2], grid);
    return (cz * grid + cy) * grid + cx;  // < grid^3 <= 2^21: inside the table
}

// The fate of the lane's point (x, y, z); `valid`: the lane has one (the others step some point with the wave, are never alive and
// read nothing). A lane stops looking the table up once it has its label — `open` — but keeps stepping for the bound test: a probe
// that escapes late is DIVERGED whatever its first tail points met.
__device__ __forceinline__ sar_basin_fate run_fate(const FateArgs& a, const SearchCoeffs& c, bool valid, double x, double y, double z) {
    const double bound = a.bound;
    const FateBox box = pin_box(a);
    bool alive = valid;
    uint32_t esc = 0;
    for (CheckedSteps run(a.transient); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool in = within(x, y, z, bound);
            esc = (alive & !in) ? t + 1u : esc;
            alive = alive & in;
        }
    uint32_t label = kFateUnknown, hit = a.steps + 1u;  // (steps <= 2^31)
    bool open = alive;
    if (open) {  // tail point 0
        const uint32_t l = a.label[fate_node(box, a.grid, x, y, z)];
        if (l != kBasinEmpty) {
            label = l;
            hit = 0;
            open = false;
        }
    }
    for (CheckedSteps run(a.steps); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool in = within(x, y, z, bound);
            esc = (alive & !in) ? a.transient + t + 1u : esc;  // (transient + steps < 2^32)
            alive = alive & in;
            open = open & in;
            if (open) {  // tail point t + 1
                const uint32_t l = a.label[fate_node(box, a.grid, x, y, z)];
                if (l != kBasinEmpty) {
                    label = l;
                    hit = t + 1u;
                    open = false;
                }
            }
        }
    sar_basin_fate f;
    f.status = alive ? SAR_SEARCH_BOUNDED : SAR_SEARCH_DIVERGED;
    f.escape_step = esc;
    f.label = alive ? label : kBasinEmpty;
    f.hit = alive ? hit : 0u;
    return f;
}

__device__ __forceinline__ void store_fate(sar_basin_fate* dst, const sar_basin_fate& f) {
    uint4 rec;
    rec.x = (uint32_t)f.status;
    rec.y = f.escape_step;
    rec.z = f.label;
    rec.w = f.hit;
    *(uint4*)dst = rec;
}

// ---------------------------------------------------------------------------------------------------
// k_basin_fate — one lane per point of the launch.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basin_fate(const FateArgs a) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < a.n;
    const SearchCoeffs c = pin_z_row(a.map);
    const uint32_t at = valid ? i : 0u;  // (a.n >= 1: in bounds for every lane)
    const sar_basin_fate f = run_fate(a, c, valid, a.points[3u * at], a.points[3u * at + 1u], a.points[3u * at + 2u]);
    if (valid) store_fate(a.fates + i, f);
}

// ---------------------------------------------------------------------------------------------------
// k_basin_ladder — four waves per workgroup, floor(64 / g) groups per wave, the lanes beyond them idle. Behind the fates the base
// lane's class reaches its group by a cross-lane read, two ballots give every lane the wave's "my class is UNKNOWN" and "my class
// differs from my base's" bits, and the base lane cuts its group's + and - bits out of them: the masks it writes, and per set bit
// one LDS atomic on the workgroup's counts; then one 64-bit global atomic per non-zero entry and workgroup.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_basin_ladder(const FateArgs a) {
    __shared__ uint32_t s_count[2u * kMaxLadderLevels];  // [level][uncertain, unknown]; a workgroup holds at most 4 * 21 groups
    const uint32_t K = a.levels, g = 1u + 2u * K, per_wave = 64u / g;
    if (threadIdx.x < 2u * kMaxLadderLevels) s_count[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = blockIdx.x * 4u + (threadIdx.x >> 6);
    const uint32_t grp = lane / g, member = lane - grp * g;
    const uint32_t base = wave * per_wave + grp;  // (<= 2^20 base points a call, at most 64 idle waves: no wrap)
    const bool valid = grp < per_wave && base < a.n;
    const SearchCoeffs c = pin_z_row(a.map);
    const uint32_t at = valid ? base : 0u;  // (a.n >= 1: in bounds for every lane)
    const bool minus = member > K;
    const uint32_t level = member == 0u ? 0u : (minus ? member - K : member) - 1u;  // (< K for every member of a group; idle lanes clamp)
    const double e = a.eps[level < K ? level : 0u];
    double x = a.points[3u * at], y = a.points[3u * at + 1u], z = a.points[3u * at + 2u];
    if (member != 0u) {
        x = ladder_probe(x, a.dir[0], e, minus);
        y = ladder_probe(y, a.dir[1], e, minus);
        z = ladder_probe(z, a.dir[2], e, minus);
    }
    const sar_basin_fate f = run_fate(a, c, valid, x, y, z);
    const uint32_t cls = f.label;  // (a DIVERGED fate's label is 0xFFFFFFFF: the class)
    const uint32_t base_lane = grp * g;  // (<= 63 for the lanes of a group; an idle lane reads some lane and drops it)
    const uint32_t base_cls = __shfl(cls, (int)(base_lane & 63u), 64);
    const unsigned long long unknown_lanes = wave_ballot(valid & (cls == kFateUnknown));
    const unsigned long long differ_lanes = wave_ballot(valid & (cls != base_cls));
    if (valid && member == 0u) {
        const uint32_t all = (K < 32u ? (1u << K) : 0u) - 1u;  // K <= 31: K ones
        const unsigned long long u = unknown_lanes >> base_lane, d = differ_lanes >> base_lane;
        const uint32_t unknown_bits = (u & 1ull) ? all : (((uint32_t)(u >> 1) | (uint32_t)(u >> (1u + K))) & all);
        const uint32_t uncertain_bits = ((uint32_t)(d >> 1) | (uint32_t)(d >> (1u + K))) & all & ~unknown_bits;
        store_fate(a.fates + base, f);
        sar_basin_ladder_mask m;
        m.uncertain_bits = uncertain_bits;
        m.unknown_bits = unknown_bits;
        a.masks[base] = m;
        for (uint32_t bits = uncertain_bits; bits; bits &= bits - 1u) atomicAdd(&s_count[2u * (uint32_t)(__ffs((int)bits) - 1)], 1u);
        for (uint32_t bits = unknown_bits; bits; bits &= bits - 1u) atomicAdd(&s_count[2u * (uint32_t)(__ffs((int)bits) - 1) + 1u], 1u);
    }
    __syncthreads();
    if (threadIdx.x < 2u * K) {
        const uint32_t v = s_count[threadIdx.x];
        if (v) atomicAdd(a.counts + threadIdx.x, (unsigned long long)v);
    }
}

void launch_basin_fate(const FateArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_basin_fate, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_basin_ladder(const FateArgs& a, hipStream_t s) {
    const uint32_t per_block = 4u * ladder_groups_per_wave(a.levels);
    hipLaunchKernelGGL(k_basin_ladder, dim3((a.n + per_block - 1u) / per_block), dim3(256), 0, s, a);
}

}  // namespace sar
