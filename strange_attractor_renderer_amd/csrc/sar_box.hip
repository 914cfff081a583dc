// sar_box.hip — gfx950 (MI355X) kernels of box counting (include/sar.h: sar_runtime_boxes, sar_runtime_boxdim).
//
// A pyramid through hash tables in device memory, per set: k_box_insert, one lane per point, puts the points' cells at the finest
// level L into the set's table 0; k_box_level, launched for l = L down to 1, sums the occupancies of level l's table and inserts
// every occupied cell's parent, with the cell's occupancy, into the other table, which so becomes level l - 1's. No sort and no
// dense grid (2^48 cells at L = 16). A cell comes from one subtract, one multiply and a conversion, the logarithm of an occupancy
// is lg32 in integers (sar_box.hpp): no division, square root or logarithm, so the build's fused-op audit pins both kernels at 0 and
// a host restatement gives the same integers. DESIGN.md section 19 has the table layout, the argument that the result does not
// depend on the order of the insertions, and the resources.
#include "sar_box.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

// c_k of include/sar.h: `top` = 2^L as a double, `last` = 2^L - 1. A NaN u (none arises from what the host accepts) goes to cell 0.
__device__ __forceinline__ uint32_t box_cell(double p, double origin, double scale, double top, uint32_t last) {
    const double u = (p - origin) * scale;
    return !(u >= 0.) ? 0u : (u >= top ? last : (uint32_t)u);
}

// the 16 bits of v on every third bit: the key of a cell is spread(c_x) | spread(c_y) << 1 | spread(c_z) << 2, so that
// key >> 3 is the key of its parent
__device__ __forceinline__ unsigned long long box_spread(uint32_t v) {
    unsigned long long x = v;
    x = (x | x << 16) & 0x001f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// a key's home slot: two multiplicative rounds, the top slot_bits bits (keys of one level differ mostly in their low bits)
__device__ __forceinline__ uint32_t box_home(unsigned long long key, uint32_t slot_bits) {
    unsigned long long h = key * 0x9e3779b97f4a7c15ull;
    h ^= h >> 32;
    h *= 0xd6e8feb86659fd93ull;
    return (uint32_t)(h >> (64u - slot_bits));
}

// Adds `add` to key's occupancy in an open-addressing table with linear probing. A slot is claimed with a device-scope CAS from
// kBoxEmpty, and the lane goes on from the value the CAS RETURNS, never from a plain load: the L2s of the eight XCDs are not
// coherent (sar_basin.hip has the same concern), and a load could show an earlier, empty slot that another lane has since claimed
// for another key. A key's slot never changes once claimed, so every lane that brings the key walks the same probe sequence to the
// same slot. The walk ends after at most `slots` steps; the tables always have a free slot (slots > n >= distinct keys), and a
// walk that went round all the same raises *overflow for the host (SAR_ERR_INTERNAL). Nothing waits for another lane.
__device__ __forceinline__ void box_add(unsigned long long* keys, uint32_t* counts, uint32_t slots, uint32_t slot_bits,
                                        unsigned long long key, uint32_t add, uint32_t* overflow) {
    uint32_t slot = box_home(key, slot_bits);
    for (uint32_t step = 0; step < slots; ++step) {
        const unsigned long long old = atomicCAS(keys + slot, kBoxEmpty, key);
        if (old == kBoxEmpty || old == key) {
            atomicAdd(counts + slot, add);
            return;
        }
        slot = (slot + 1u) & (slots - 1u);
    }
    atomicOr(overflow, 1u);
}

__device__ __forceinline__ unsigned long long box_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_down(v, off);
    return v;
}

// ---------------------------------------------------------------------------------------------------
// k_box_insert — grid (ceil(n / 256), sets). Equal keys are combined within a wave before they go to memory: for up to
// kBoxCombineRounds rounds the first lane still pending broadcasts its key, a ballot counts the lanes that hold it, and they are
// settled — the leader will add their number. A fixed point or a short cycle (most of a coefficient plane) so costs a few atomics
// per wave and not n on one address; lanes still pending after the rounds add 1 each, which is the same sum. The kernel also clears
// table 1, which the first k_box_level fills (table 0 is cleared by the host before the launch).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBoxBlock) k_box_insert(const BoxArgs a) {
    const uint32_t set = a.first_set + blockIdx.y;
    const BoxCube cube = a.cubes[set];
    if (cube.skip) return;  // (the whole grid row)
    const size_t base = (size_t)set * a.slots;
    {
        unsigned long long* const k1 = a.keys + a.table_stride + base;
        uint32_t* const c1 = a.counts + a.table_stride + base;
        for (uint32_t k = blockIdx.x * kBoxBlock + threadIdx.x; k < a.slots; k += gridDim.x * kBoxBlock) {
            k1[k] = kBoxEmpty;
            c1[k] = 0u;
        }
    }
    const uint32_t i = blockIdx.x * kBoxBlock + threadIdx.x, lane = threadIdx.x & 63u;
    bool pending = i < a.n;
    unsigned long long key = 0;
    if (pending) {
        const double* const px = a.points + (size_t)set * 3u * a.n;
        const uint32_t last = (1u << a.levels) - 1u;
        const double top = (double)(1u << a.levels);
        const uint32_t cx = box_cell(px[i], cube.origin[0], cube.scale, top, last);
        const uint32_t cy = box_cell(px[(size_t)a.n + i], cube.origin[1], cube.scale, top, last);
        const uint32_t cz = box_cell(px[2u * (size_t)a.n + i], cube.origin[2], cube.scale, top, last);
        key = box_spread(cx) | (box_spread(cy) << 1) | (box_spread(cz) << 2);
    }
    uint32_t add = 1u;
    bool leads = false;
    for (uint32_t round = 0; round < kBoxCombineRounds; ++round) {
        const unsigned long long todo = __builtin_amdgcn_ballot_w64(pending);
        if (!todo) break;  // (the same in every lane)
        const uint32_t leader = (uint32_t)__builtin_ctzll(todo);
        const unsigned long long theirs = __shfl(key, (int)leader);
        const bool same = pending & (key == theirs);
        const unsigned long long group = __builtin_amdgcn_ballot_w64(same);
        if (lane == leader) {
            add = (uint32_t)__builtin_popcountll(group);
            leads = true;
        }
        pending = pending & !same;
    }
    if (leads | pending) box_add(a.keys + base, a.counts + base, a.slots, a.slot_bits, key, add, a.overflow);
}

// ---------------------------------------------------------------------------------------------------
// k_box_level — grid (min(ceil(slots / 256), kBoxLevelBlocks), sets), over the slots of level `level`'s table, table (L - level) & 1.
// Every occupied slot (key, n) adds 1, [n == 1], n^2 and n lg32(n) (skipped for n == 1: lg32(1) = 0) to the lane's sums, and — above
// level 1, whose parent is the whole cube, written by the host — adds n to key >> 3 in the other table: at most eight children meet
// on a parent, and the inserts shrink with every level. The slot is then emptied: the table is the one the NEXT launch fills. The
// sums are reduced in the wave and through LDS in the workgroup, then folded with one 64-bit atomic per non-zero sum and workgroup.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBoxBlock) k_box_level(const BoxArgs a, uint32_t level) {
    __shared__ unsigned long long s_sum[4];
    const uint32_t set = a.first_set + blockIdx.y, tid = threadIdx.x;
    if (a.cubes[set].skip) return;  // (the whole workgroup)
    const uint32_t t = (a.levels - level) & 1u;
    const size_t base = (size_t)set * a.slots, from = t * a.table_stride + base, to = (1u - t) * a.table_stride + base;
    if (tid < 4u) s_sum[tid] = 0ull;
    __syncthreads();

    unsigned long long cells = 0, singles = 0, sum_sq = 0, n_log_n = 0;
    for (uint32_t k = blockIdx.x * kBoxBlock + tid; k < a.slots; k += gridDim.x * kBoxBlock) {
        const unsigned long long key = a.keys[from + k];
        if (key == kBoxEmpty) continue;
        const uint32_t c = a.counts[from + k];
        cells += 1ull;
        singles += c == 1u ? 1ull : 0ull;
        sum_sq += (unsigned long long)c * c;
        if (c > 1u) n_log_n += (unsigned long long)c * box_lg32(c);
        if (level > 1u) box_add(a.keys + to, a.counts + to, a.slots, a.slot_bits, key >> 3, c, a.overflow);
        a.keys[from + k] = kBoxEmpty;
        a.counts[from + k] = 0u;
    }
    cells = box_wave_sum(cells);
    singles = box_wave_sum(singles);
    sum_sq = box_wave_sum(sum_sq);
    n_log_n = box_wave_sum(n_log_n);
    if ((tid & 63u) == 0u) {
        if (cells) atomicAdd(&s_sum[0], cells);
        if (singles) atomicAdd(&s_sum[1], singles);
        if (sum_sq) atomicAdd(&s_sum[2], sum_sq);
        if (n_log_n) atomicAdd(&s_sum[3], n_log_n);
    }
    __syncthreads();
    if (tid < 4u && s_sum[tid]) atomicAdd(a.sums + ((size_t)set * (a.levels + 1u) + level) * 4u + tid, s_sum[tid]);
}

void launch_box_insert(const BoxArgs& a, uint32_t n_sets, hipStream_t s) {
    hipLaunchKernelGGL(k_box_insert, dim3((a.n + kBoxBlock - 1u) / kBoxBlock, n_sets), dim3(kBoxBlock), 0, s, a);
}

void launch_box_level(const BoxArgs& a, uint32_t level, uint32_t n_sets, hipStream_t s) {
    const uint32_t blocks = (a.slots + kBoxBlock - 1u) / kBoxBlock;
    hipLaunchKernelGGL(k_box_level, dim3(blocks < kBoxLevelBlocks ? blocks : kBoxLevelBlocks, n_sets), dim3(kBoxBlock), 0, s, a, level);
}

}  // namespace sar
