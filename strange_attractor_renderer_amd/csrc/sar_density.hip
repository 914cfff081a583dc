// sar_density.hip — the gfx950 kernel of density estimation (sar_runtime_density, include/sar.h): a variable-radius gather stencil.
//
// k_density: a workgroup of 256 lanes owns a tile of 32 x tile_h outputs (tile_h = 8, 16 or 32; a lane owns tile_h / 8 pixels of one
// column). It stages the snapshot's counts of the tile plus an R-wide halo in LDS (a source outside the image is staged as count 0,
// which the contract skips anyway), and finds the smallest count below S among them on the way:
//   * none (every source 0 or >= S, the identity class): the tile is COPIED THROUGH. The live buffers still hold what the snapshot
//     holds, so nothing is written; the lanes only fold the statistics of their pixels. Four fifths of a typical frame is empty and
//     the bright part is identity: such a tile costs its counts, 4 of the 12 bytes per source.
//   * otherwise the steps of tile and halo and the packed weight plan follow into LDS, and each lane walks the taps of its pixels in
//     the contract's order, dy outer, dx inner — bounded by the reach of that smallest count, since a tap with d2 * cmin >= S is
//     dead for every source of the tile (d2 * c >= d2 * cmin): a wave-uniform skip of taps whose weight is 0 changes no bit.
// It is a gather: a pixel's fp64 hue sum runs in one lane in a fixed order, whatever the launch shape.
//
// LDS traffic: the 32 lanes of a half-wave read 32 consecutive counts (ds_read_b32: banks a/4 mod 32) or steps (ds_read_b64: banks
// a/4 mod 64) of ONE halo row — a lane group never spans two rows, so no row stride can make the halo rows conflict, and the rows
// need no padding. The weight W[off[d2] + c - 1] is indexed by the source's class: off[d2] is wave-uniform (a broadcast), equal
// classes broadcast, unequal ones may share a bank — the one gathered read of a tap, taken only for a source with 0 < count < S.
//
// The statistics (all integers) and the maximum fold through a wave reduction, LDS atomics and one global atomic per block and
// field. The hue is multiplies, adds and ONE division: the build's fused-op audit pins k_density at that division's expansion.
#include "sar_density.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

namespace {

__device__ inline uint32_t wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o);
        v = w < v ? w : v;
    }
    return v;
}
__device__ inline uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t w = __shfl_xor(v, o);
        v = w > v ? w : v;
    }
    return v;
}
__device__ inline uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ inline unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), o);
        const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), o);
        v += (static_cast<unsigned long long>(hi) << 32) | lo;
    }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(kDensityThreads) k_density(const DensityArgs a) {
    extern __shared__ double lds[];
    __shared__ uint32_t s_cmin;
    __shared__ unsigned long long s_sum64[2];  // mass_in, mass_q16
    __shared__ uint32_t s_sum32[4];            // covered_in, covered_out, spread, saturated
    __shared__ uint32_t s_max32[2];            // max_in, max_out

    const uint32_t tid = threadIdx.x;
    const uint32_t S = a.S, R = a.R;
    const uint32_t hw = kDensityTileW + 2u * R, hh = a.tile_h + 2u * R, n = hw * hh;
    double* l_steps = lds;                                        // [hh][hw]
    uint32_t* l_count = reinterpret_cast<uint32_t*>(lds + n);     // [hh][hw]
    uint32_t* l_plan = l_count + n;                               // [plan_words]
    const uint32_t x0 = (blockIdx.x % a.tiles_x) * kDensityTileW, y0 = (blockIdx.x / a.tiles_x) * a.tile_h;

    if (tid == 0) s_cmin = 0xFFFFFFFFu;
    if (tid < 2) s_sum64[tid] = 0ull;
    if (tid < 4) s_sum32[tid] = 0u;
    if (tid < 2) s_max32[tid] = 0u;
    __syncthreads();

    // the counts of tile and halo; the smallest one that spreads
    uint32_t cmin = 0xFFFFFFFFu;
    for (uint32_t i = tid; i < n; i += kDensityThreads) {
        const uint32_t hy = i / hw, hx = i - hy * hw;
        const uint32_t gx = x0 + hx - R, gy = y0 + hy - R;  // (wraps below 0: then >= width / height)
        uint32_t c = 0u;
        if (gx < a.width && gy < a.height) c = a.snap_count[static_cast<size_t>(gy) * a.width + gx];
        l_count[i] = c;
        cmin = (c != 0u && c < S && c < cmin) ? c : cmin;
    }
    cmin = wave_min_u32(cmin);
    if ((tid & 63u) == 0u && cmin != 0xFFFFFFFFu) atomicMin(&s_cmin, cmin);
    __syncthreads();
    cmin = s_cmin;
    const bool copy = cmin == 0xFFFFFFFFu;  // block-uniform
    uint32_t reach = 0u;
    if (!copy) {
        while (reach < R && (reach + 1u) * (reach + 1u) * cmin < S) ++reach;
        for (uint32_t i = tid; i < n; i += kDensityThreads) {
            const uint32_t hy = i / hw, hx = i - hy * hw;
            const uint32_t gx = x0 + hx - R, gy = y0 + hy - R;
            double s = 0.;
            if (gx < a.width && gy < a.height) s = a.snap_steps[static_cast<size_t>(gy) * a.width + gx];
            l_steps[i] = s;
        }
        for (uint32_t i = tid; i < a.plan_words; i += kDensityThreads) l_plan[i] = a.plan[i];
        __syncthreads();
    }

    unsigned long long mass_in = 0ull, mass_q16 = 0ull;
    uint32_t cov_in = 0u, cov_out = 0u, spread = 0u, saturated = 0u, max_in = 0u, max_out = 0u;
    const uint32_t tx = tid & 31u;
    const int r = static_cast<int>(reach);
    for (uint32_t ty = tid >> 5; ty < a.tile_h; ty += kDensityThreads / kDensityTileW) {
        const uint32_t px = x0 + tx, py = y0 + ty;
        if (px >= a.width || py >= a.height) continue;
        const uint32_t centre = (ty + R) * hw + tx + R;
        const uint32_t cin = l_count[centre];
        unsigned long long acc = static_cast<unsigned long long>(cin) << 16;  // a copied tile: the identity class, or nothing
        uint32_t cout = cin;
        if (!copy) {
            unsigned long long den = 0ull;
            double num = 0.;
            bool others = false;  // a source other than the pixel itself has entered den
            acc = 0ull;
            for (int dy = -r; dy <= r; ++dy)
                for (int dx = -r; dx <= r; ++dx) {
                    const uint32_t d2 = static_cast<uint32_t>(dx * dx + dy * dy);
                    if (d2 * cmin >= S) continue;  // wave-uniform: dead for every source of this tile (and d2 < S from here on)
                    const uint32_t idx = static_cast<uint32_t>(static_cast<int>(centre) + dy * static_cast<int>(hw) + dx);
                    const uint32_t c = l_count[idx];
                    if (c == 0u) continue;
                    uint32_t w;
                    if (c >= S) w = d2 == 0u ? 65536u : 0u;
                    else w = d2 * c < S ? l_plan[l_plan[d2] + c - 1u] : 0u;
                    if (w == 0u) continue;
                    const unsigned long long m = static_cast<unsigned long long>(w) * c;
                    acc += m;
                    const double s = l_steps[idx];
                    const unsigned long long bits = static_cast<unsigned long long>(__double_as_longlong(s));
                    if ((bits & 0x7FF0000000000000ull) != 0x7FF0000000000000ull) {  // finite
                        den += m;
                        const double ms = static_cast<double>(m) * s;
                        num = num + ms;
                        others = others | (d2 != 0u);
                    }
                }
            const unsigned long long rounded = (acc + 32768ull) >> 16;
            saturated += rounded > 0xFFFFFFFFull ? 1u : 0u;
            cout = rounded > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(rounded);
            const size_t p = static_cast<size_t>(py) * a.width + px;
            a.count[p] = cout;
            if (others) a.steps[p] = num / static_cast<double>(den);  // (else: the bits stay)
        }
        mass_in += cin;
        mass_q16 += acc;
        cov_in += cin != 0u ? 1u : 0u;
        cov_out += cout != 0u ? 1u : 0u;
        spread += (cin != 0u && cin < S) ? 1u : 0u;
        max_in = cin > max_in ? cin : max_in;
        max_out = cout > max_out ? cout : max_out;
    }

    // wave -> LDS -> one global atomic per block and field (a zero adds nothing and is not sent)
    mass_in = wave_sum_u64(mass_in);
    mass_q16 = wave_sum_u64(mass_q16);
    cov_in = wave_sum_u32(cov_in);
    cov_out = wave_sum_u32(cov_out);
    spread = wave_sum_u32(spread);
    saturated = wave_sum_u32(saturated);
    max_in = wave_max_u32(max_in);
    max_out = wave_max_u32(max_out);
    if ((tid & 63u) == 0u) {
        atomicAdd(&s_sum64[0], mass_in);
        atomicAdd(&s_sum64[1], mass_q16);
        atomicAdd(&s_sum32[0], cov_in);
        atomicAdd(&s_sum32[1], cov_out);
        atomicAdd(&s_sum32[2], spread);
        atomicAdd(&s_sum32[3], saturated);
        atomicMax(&s_max32[0], max_in);
        atomicMax(&s_max32[1], max_out);
    }
    __syncthreads();
    if (tid == 0) {
        sar_density_stats* st = &a.stats->s;
        if (s_sum64[0]) atomicAdd(reinterpret_cast<unsigned long long*>(&st->mass_in), s_sum64[0]);
        if (s_sum64[1]) atomicAdd(reinterpret_cast<unsigned long long*>(&st->mass_q16), s_sum64[1]);
        if (s_sum32[0]) atomicAdd(&st->covered_in, s_sum32[0]);
        if (s_sum32[1]) atomicAdd(&st->covered_out, s_sum32[1]);
        if (s_sum32[2]) atomicAdd(&st->spread, s_sum32[2]);
        if (s_sum32[3]) atomicAdd(&st->saturated, s_sum32[3]);
        if (s_max32[0]) atomicMax(&st->max_in, s_max32[0]);
        if (s_max32[1]) {
            atomicMax(&st->max_out, s_max32[1]);
            atomicMax(&a.scalars[SC_MAX], s_max32[1]);
        }
        atomicAdd(&a.stats->tiles, 1u);
        if (copy) atomicAdd(&a.stats->tiles_copied, 1u);
    }
}

void launch_density(const DensityArgs& a, uint32_t tiles, hipStream_t s) {
    // at most 54 KiB (tile_h 32, S = 256): below the 64 KiB a kernel may take without an attribute
    const size_t lds = density_lds_bytes(a.R, a.tile_h, a.plan_words);
    hipLaunchKernelGGL(k_density, dim3(tiles), dim3(kDensityThreads), lds, s, a);
}

}  // namespace sar
