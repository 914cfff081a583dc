// sar_box.hpp — what the two halves of box counting share (include/sar.h: sar_box_*, sar_runtime_boxes, sar_boxdim_*,
// sar_runtime_boxdim): the fixed-point logarithm, bit for bit the same on the host and on the device, the layout of a set's hash
// tables, the argument blocks of k_box_insert and k_box_level (sar_box.hip) and their launch wrappers, called from sar_box.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include "sar_internal.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

constexpr uint32_t kBoxMaxLevels = 16;            // 3 * 16 = 48 key bits
constexpr uint32_t kBoxMaxPoints = 1u << 20;      // per set: sum_sq <= 2^40 and n_log_n < 2^57 fit 64 bits, an occupancy fits 32
constexpr uint32_t kBoxBlock = 256;               // lanes per workgroup of both kernels
constexpr uint32_t kBoxLevelBlocks = 1024;        // workgroups of k_box_level per set at most: it strides over the slots
constexpr uint32_t kBoxCombineRounds = 8;         // leaders k_box_insert broadcasts per wave: a cycle of up to 8 points is one atomic each
constexpr uint32_t kBoxMaxSlots = 1u << 24;       // "box_slots"
constexpr uint32_t kBoxMaxGridY = 65535;          // sets per launch ("box_chunk")
constexpr uint64_t kBoxPointBudget = 1ull << 24;  // points in device memory at a time (24 B each): sets beyond it go in groups
constexpr uint64_t kBoxSlotBudget = 1ull << 25;   // slots per table of a group (12 B each, two tables)
constexpr unsigned long long kBoxEmpty = ~0ull;   // no key has more than 48 bits

// lg32(n) of include/sar.h, n >= 1: the top bit, then 32 squarings of the mantissa y in [2^63, 2^64). y * y lies in [2^126, 2^128):
// where it reaches 2^127 the fraction bit is 1 and the halved (y * y) >> 63 is the product's high word; otherwise the bit is 0 and
// (y * y) >> 63 takes the high word's low 63 bits and the low word's top bit.
__host__ __device__ inline uint64_t box_lg32(uint32_t n) {
    const uint32_t e = 31u - (uint32_t)__builtin_clz(n);
    unsigned long long y = (unsigned long long)n << (63u - e), frac = 0;
    for (int k = 0; k < 32; ++k) {
#if defined(__HIP_DEVICE_COMPILE__)
        const unsigned long long hi = __umul64hi(y, y), lo = y * y;
#else
        const unsigned __int128 sq = (unsigned __int128)y * y;
        const unsigned long long hi = (unsigned long long)(sq >> 64), lo = (unsigned long long)sq;
#endif
        const unsigned long long bit = hi >> 63;
        y = bit ? hi : ((hi << 1) | (lo >> 63));
        frac = (frac << 1) | bit;
    }
    return ((unsigned long long)e << 32) | frac;
}

// One set's cube in device memory: u = (p - origin) * scale. A set with skip != 0 (a DIVERGED map) is not counted.
struct BoxCube {
    double origin[3];
    double scale;
    uint32_t skip;
    uint32_t _pad;
};

// A group's two tables: table t of set s holds `slots` 64-bit keys at keys + t * table_stride + s * slots and as many 32-bit
// occupancies at the same index of counts. An empty slot is (kBoxEmpty, 0).
struct BoxArgs {
    const double* points;          // [sets of the group][3][n] SoA
    const BoxCube* cubes;          // [sets of the group]
    unsigned long long* keys;      // [2][sets of the group][slots]
    uint32_t* counts;              // [2][sets of the group][slots]
    size_t table_stride;           // sets of the group * slots
    unsigned long long* sums;      // [sets of the group][L + 1][4]: sar_box_level rows, zero before the first launch
    uint32_t* overflow;            // [1]: raised where a probe sequence went round its table (never, while slots > n)
    uint32_t n, slots;             // slots: a power of two > n
    uint32_t slot_bits;            // log2(slots)
    uint32_t levels;               // L
    uint32_t first_set;            // the launch's first set of the group; blockIdx.y counts from it
};

// k_box_insert fills table 0 (cleared by the host) with level L and clears table 1
void launch_box_insert(const BoxArgs& a, uint32_t n_sets, hipStream_t s);
// k_box_level at `level` (L .. 1): sums table (L - level) & 1, folds it into the other one unless level == 1, and clears what it read
void launch_box_level(const BoxArgs& a, uint32_t level, uint32_t n_sets, hipStream_t s);

}  // namespace sar
