// sar_manifold.hip — the gfx950 kernel of the unstable-manifold family (sar_runtime_manifold, include/sar.h has the contract): the
// sample points of every branch's fundamental domain stepped under the map, and at every step the line segments between neighbouring
// samples rasterised into the view's count and first images.
//
// k_manifold: one lane per sample, one wave per 63 segments of ONE branch. Wave w of a branch holds the points 63 w .. 63 w + 63: lane
// l projects its own point, takes its right neighbour's (X, Y, alive, placed) through a cross-lane read and owns segment 63 w + l;
// lane 63 owns none, and the seam point 63 w + 63 is computed again as lane 0 of wave w + 1 — the same doubles from the same index,
// so the two waves agree on it to the bit. Nothing is stored per lane and no LDS is used. cfg's MapParams come by value and are
// pinned as the single-frame kernels pin them; the branch's block is wave-uniform and read with scalar loads (load_frame_args). A
// wave whose branch is DOMAIN_ESCAPED, and the waves beyond the last branch, leave at once.
//
// A step: the bound test, the projection, the neighbour read, the classes, then the raster loop, which runs to the wave's largest
// plot count with the other lanes masked. The pixel of plot k is X0 + floor((2 k dX + L) / (2 L)): the loop carries the quotient and
// the remainder of that division and moves them by 2 dX per plot — |2 dX| <= 2 L, so one correction per plot keeps 0 <= r < 2 L —
// which is the floored division in integers without a divide. A plot inside the image is one add to count and, where a plain load
// of first shows a larger word, one atomicMin (first only falls, so a stale load can only ask for a min that was not needed). Plot 0
// of a segment is its own start pixel, and a run of neighbouring lanes that start on one pixel makes one add of the run's length:
// next to the cycle a whole wave sits on one pixel, and 63 adds to one address become one. The wave leaves the step loop when a
// ballot says none of its points is alive: its remaining segments are all dead.
//
// The counters are per-lane words (a lane's plots stay below 2^28), summed over the wave at the end and added to the branch's 64-bit
// sums with one atomic per wave and counter.
//
// Multiplies, adds, compares and ONE division (t_i), contraction off: the build's fused-op audit pins k_manifold at that division's
// expansion.
#include "sar_device.hpp"
#include "sar_manifold.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

// the sum of v over the wave's lanes (every lane calls; every lane gets it)
__device__ __forceinline__ unsigned long long wave_sum_u64(uint32_t v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// one step of the division's quotient q and remainder r by `den` as the numerator grows by `num_step`, |num_step| <= den
__device__ __forceinline__ void floor_div_advance(int& q, int& r, int num_step, int den) {
    r += num_step;
    const bool over = r >= den, under = r < 0;
    r = over ? r - den : (under ? r + den : r);
    q = over ? q + 1 : (under ? q - 1 : q);
}

__global__ void __launch_bounds__(256) k_manifold(const ManifoldArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t branch = wave / a.waves_per_branch;
    if (branch >= a.n_branches) return;  // (the whole wave; the kernel has no barrier)
    const ManifoldBranch br = load_frame_args(a.branches + branch);
    if (!br.live) return;                // DOMAIN_ESCAPED: nothing is drawn, the sums stay 0
    MapParams p = a.p;
    pin_map_params(p);

    const uint32_t samples = a.samples, steps = a.steps, max_span = a.max_span, width = a.width, height = a.height;
    const double bound = a.bound;
    const uint32_t i = (wave - branch * a.waves_per_branch) * kManifoldWaveSegments + lane;  // the lane's point
    const bool valid = i < samples;
    const bool seg = (lane < kManifoldWaveSegments) & (i + 1u < samples);  // the lane owns segment (i, i + 1)
    // the last point of the branch has no wave of its own behind it: lane 63 counts it where it is that point, and only there
    const bool counted = valid & ((lane < kManifoldWaveSegments) | (i + 1u == samples));
    uint32_t* const count = a.count;
    uint32_t* const first = a.first;

    // the lanes beyond the branch's last point take its first one, step with the others and are never alive
    const double t = (double)(valid ? i : 0u) / (double)(samples - 1u);
    double x = br.a[0] + br.d[0] * t, y = br.a[1] + br.d[1] * t, z = br.a[2] + br.d[2] * t;

    bool alive = valid;
    uint32_t n_drawn = 0, n_dead = 0, n_far = 0, n_long = 0, pixels = 0, length_px = 0, first_long = kManifoldNone, alive_end = 0;
    for (uint32_t n = 0;; ++n) {
        alive = alive & within(x, y, z, bound);
        if (!wave_ballot(alive)) {  // from here on every segment of the wave is dead
            n_dead += seg ? steps - n + 1u : 0u;
            break;
        }
        double fi, fj;
        manifold_project(p, x, y, z, fi, fj);
        const bool placed = (int)(fi >= -kManifoldPlaced) & (int)(fi < kManifoldPlaced) & (int)(fj >= -kManifoldPlaced) & (int)(fj < kManifoldPlaced);
        const int X0 = placed ? (int)floor(fi) : 0, Y0 = placed ? (int)floor(fj) : 0;
        const uint32_t flags = (alive ? 1u : 0u) | (placed ? 2u : 0u);
        const int X1 = __shfl_down(X0, 1), Y1 = __shfl_down(Y0, 1);
        const uint32_t both = flags & (uint32_t)__shfl_down((int)flags, 1);
        const int dX = X1 - X0, dY = Y1 - Y0;  // (placed points: both below 2^31 in size)
        const uint32_t adx = (uint32_t)(dX < 0 ? -dX : dX), ady = (uint32_t)(dY < 0 ? -dY : dY), L = adx > ady ? adx : ady;
        const bool is_dead = seg & !(both & 1u);
        const bool is_far = seg & ((both & 1u) != 0u) & !(both & 2u);
        const bool near = seg & (both == 3u);
        const bool is_long = near & (L > max_span), drawn = near & (L <= max_span);
        n_dead += is_dead ? 1u : 0u;
        n_far += is_far ? 1u : 0u;
        n_long += is_long ? 1u : 0u;
        n_drawn += drawn ? 1u : 0u;
        length_px += drawn ? L : 0u;
        first_long = (is_long & (first_long == kManifoldNone)) ? n : first_long;

        // the raster: `plots` pixels from (X0, Y0), the end pixel left to the next segment
        const uint32_t plots = drawn ? (L ? L : 1u) : 0u;
        const uint32_t word = n * 4096u + branch;
        const int den = drawn ? (int)(L + L) : 0, step_x = drawn ? dX + dX : 0, step_y = drawn ? dY + dY : 0;  // (|dX| <= 4096 where drawn)
        int qx = 0, qy = 0, rx = drawn ? (int)L : 0, ry = rx;
        {
            // plot 0 of every drawn segment is its own pixel (X0, Y0). Near the cycle, and wherever the samples are denser than the
            // pixels, neighbouring lanes sit on one pixel: a run of them makes ONE add of its length and one min (the word is the
            // wave's), led by its first lane. The same sums and the same minimum, so every bit stays as it is.
            const bool in0 = drawn & ((uint32_t)X0 < width) & ((uint32_t)Y0 < height);
            const uint32_t pix0 = in0 ? (uint32_t)Y0 * width + (uint32_t)X0 : kManifoldNone;  // (a pixel index stays below 2^24)
            const uint32_t before = (uint32_t)__shfl_up((int)pix0, 1);                      // (lane 0 reads itself: it leads anyway)
            const bool head = in0 & ((lane == 0u) | (before != pix0));
            const unsigned long long ends = wave_ballot(!in0 | head);  // where a run cannot go on
            if (head) {
                const unsigned long long above = (ends >> lane) >> 1;
                const uint32_t run = above ? (uint32_t)__builtin_ctzll(above) + 1u : 64u - lane;
                atomicAdd(count + pix0, run);
                if (__hip_atomic_load(first + pix0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > word) atomicMin(first + pix0, word);
            }
            pixels += in0 ? 1u : 0u;
            floor_div_advance(qx, rx, step_x, den);
            floor_div_advance(qy, ry, step_y, den);
        }
        for (uint32_t k = 1; wave_ballot(k < plots); ++k) {
            if (k < plots) {
                const int px = X0 + qx, py = Y0 + qy;
                if ((uint32_t)px < width && (uint32_t)py < height) {
                    const uint32_t pix = (uint32_t)py * width + (uint32_t)px;
                    atomicAdd(count + pix, 1u);
                    if (__hip_atomic_load(first + pix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > word) atomicMin(first + pix, word);
                    ++pixels;
                }
                floor_div_advance(qx, rx, step_x, den);
                floor_div_advance(qy, ry, step_y, den);
            }
        }

        if (n == steps) {
            alive_end = (alive & counted) ? 1u : 0u;
            break;
        }
        next_point(p, x, y, z);
    }

    // the wave's sums into the branch's (no lane left early: the returns above are wave-uniform)
    const unsigned long long s_drawn = wave_sum_u64(n_drawn), s_dead = wave_sum_u64(n_dead), s_far = wave_sum_u64(n_far);
    const unsigned long long s_long = wave_sum_u64(n_long), s_pixels = wave_sum_u64(pixels), s_length = wave_sum_u64(length_px);
    const unsigned long long s_alive = wave_sum_u64(alive_end);
    uint32_t fl = first_long;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)fl, off);
        fl = o < fl ? o : fl;
    }
    if (lane == 0u) {
        ManifoldSums* const s = a.sums + branch;
        if (s_drawn) atomicAdd(&s->drawn, s_drawn);
        if (s_dead) atomicAdd(&s->dead, s_dead);
        if (s_far) atomicAdd(&s->far, s_far);
        if (s_long) atomicAdd(&s->longs, s_long);
        if (s_pixels) atomicAdd(&s->pixels, s_pixels);
        if (s_length) atomicAdd(&s->length_px, s_length);
        if (s_alive) atomicAdd(&s->alive_end, (uint32_t)s_alive);
        if (fl != kManifoldNone) atomicMin(&s->first_long_step, fl);
    }
}

void launch_manifold(const ManifoldArgs& a, hipStream_t s) {
    const uint32_t waves = a.n_branches * a.waves_per_branch;  // a wave serves one branch
    hipLaunchKernelGGL(k_manifold, dim3((waves + 3u) / 4u), dim3(256), 0, s, a);
}

}  // namespace sar
