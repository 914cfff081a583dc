// sar_flow.hip — the gfx950 kernels of flow rendering (sar_runtime_render_flow, include/sar.h has the contract): the quadratic vector
// field p' = P(p) of the 30 coefficients, integrated by classical RK4 with a fixed step and plotted into the runtime's count, zbuf and
// steps.
//
// k_flow_transient / k_flow_render: one lane per job. A job's point lives in device memory between launches ([3][n_jobs], read and
// written as 512-byte rows per wave), so a long job is any number of short launches. A step is flow_step (sar_flow.hpp) around
// next_point — four evaluations of render's polynomial —, then the bound test: a job that fails it has escaped, its failing point is
// dropped, its saved x becomes NaN and every later launch skips it. Every stride-th counted step is plotted through project_once
// (sar_device.hpp), render's projection and bounds test.
//
// count: consecutive plotted points of a trajectory land on the same or a neighbouring pixel, so a lane keeps a run (idx, n) in
// registers and flushes ONE non-returning add of n when the pixel changes, when a plotted point falls outside the image and at the
// end of the launch. Sums commute: count does not depend on the launch shape; the atomics fall by the mean run length.
//
// depth and hue: the key of a visit is sortable(zf) << 32 | sortable((float)c), c the colour transform of this ONE step's
// displacement; the largest key of a pixel wins — the nearest depth, and at an exact depth tie the largest hue. A maximum commutes as
// well, so there are no visit ordinals, no checkpoints and no replay. Before a lane forms c (a square root) it loads the pixel's key
// relaxed and drops a visit whose depth lies below it; a run's keys merge in a register, and a flush raises the key with one atomic
// max only where a second load says it can still win. Both loads only ever spare work whose result the maximum would discard.
//
// The lanes' counters (32-bit words: a launch is at most 2^24 steps) and extents are summed over the wave, then through LDS over the
// workgroup, and thread 0 makes the few atomics. Every loop's trip count is fixed before it starts; nothing waits on another lane.
//
// k_flow_resolve: one pass over the image — a pixel whose key beats the runtime's depth (render's strict test) takes the key's depth
// and hue; the largest count raises the runtime's max.
//
// Contraction off. k_flow_transient and k_flow_resolve hold no fused fp64 op, k_flow_render the expansions of the colour transform's
// square root and of the poisson-saturne transform's two divisions and nothing else (the build's audit pins all three). No division
// in the step: h * 0.5 and h / 6.0 are the host's.
#include "sar_device.hpp"
#include "sar_flow.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

namespace {

struct FlowField {  // P(point) in place: next_point on the kernel's pinned parameters
    const MapParams& p;
    __device__ __forceinline__ void operator()(double& x, double& y, double& z) const { next_point(p, x, y, z); }
};

__device__ __forceinline__ unsigned long long flow_wave_sum(uint32_t v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
__device__ __forceinline__ unsigned long long flow_wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long flow_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

constexpr double kFlowNan = __builtin_nan("");

}  // namespace

__global__ void __launch_bounds__(256) k_flow_transient(const FlowArgs a) {
    __shared__ uint32_t s_esc[4];
    const uint32_t job = blockIdx.x * 256u + threadIdx.x;
    const bool valid = job < a.n_jobs;
    const uint32_t slot = valid ? job : 0u;  // (a lane beyond the last job reads job 0's point and runs no step)
    MapParams p = a.p;
    pin_map_params(p);
    const FlowField field{p};
    const size_t n = a.n_jobs;
    double x = a.state[slot], y = a.state[n + slot], z = a.state[2u * n + slot];
    const bool alive = valid && x == x;
    const uint32_t steps = alive ? a.n_steps : 0u;
    const double h = a.h, h2 = a.h2, h6 = a.h6, bound = a.bound;
    uint32_t esc = 0;
    for (uint32_t t = 0; t < steps; ++t) {
        if (!flow_step(field, h, h2, h6, bound, x, y, z)) {
            esc = 1;
            x = kFlowNan;
            break;
        }
    }
    if (alive) {
        a.state[job] = x;
        a.state[n + job] = y;
        a.state[2u * n + job] = z;
    }
    const unsigned long long w_esc = flow_wave_sum(esc);
    if ((threadIdx.x & 63u) == 0u) s_esc[threadIdx.x >> 6] = (uint32_t)w_esc;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const unsigned long long e = (unsigned long long)((s_esc[0] + s_esc[1]) + (s_esc[2] + s_esc[3]));
        if (e) atomicAdd(&a.sums->escaped_transient, e);
    }
}

__global__ void __launch_bounds__(256) k_flow_render(const FlowArgs a) {
    __shared__ unsigned long long s_sum[6][4];
    __shared__ unsigned long long s_ext[6][4];
    const uint32_t job = blockIdx.x * 256u + threadIdx.x;
    const bool valid = job < a.n_jobs;
    const uint32_t slot = valid ? job : 0u;
    MapParams p = a.p;
    pin_map_params(p);
    const FlowField field{p};
    const size_t n = a.n_jobs;
    double x = a.state[slot], y = a.state[n + slot], z = a.state[2u * n + slot];
    const bool alive = valid && x == x;
    const uint32_t steps = alive ? a.n_steps : 0u;
    const double h = a.h, h2 = a.h2, h6 = a.h6, bound = a.bound;
    const uint32_t width = a.width, stride = a.stride;
    const bool plot = a.plot != 0;
    uint32_t* const count = a.count;
    unsigned long long* const keys = a.keys;

    uint32_t done = 0, visits = 0, outside = 0, c_atomics = 0, k_atomics = 0, esc = 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t run_idx = 0, run_n = 0;      // the run: run_n plotted points in a row on pixel run_idx
    unsigned long long run_key = 0;       // the largest of their keys that the first load let through
    bool run_depth = false;               // one of them had a depth that is no NaN
    // one add for the run, one raise for its key (run_idx < npix: it passed the bounds test)
    auto flush = [&]() {
        __hip_atomic_fetch_add(count + run_idx, run_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++c_atomics;
        if (run_depth) {
            ++k_atomics;
            if (run_key > __hip_atomic_load(keys + run_idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
                __hip_atomic_fetch_max(keys + run_idx, run_key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        run_n = 0;
        run_key = 0;
        run_depth = false;
    };

    uint32_t k = a.phase;
    for (uint32_t t = 0; t < steps; ++t) {
        double nx = x, ny = y, nz = z;
        if (!flow_step(field, h, h2, h6, bound, nx, ny, nz)) {  // escaped: the failing point is neither plotted nor counted
            esc = 1;
            x = kFlowNan;
            break;
        }
        ++done;
        lo[0] = nx < lo[0] ? nx : lo[0];
        hi[0] = nx > hi[0] ? nx : hi[0];
        lo[1] = ny < lo[1] ? ny : lo[1];
        hi[1] = ny > hi[1] ? ny : hi[1];
        lo[2] = nz < lo[2] ? nz : lo[2];
        hi[2] = nz > hi[2] ? nz : hi[2];
        if (++k == stride) {  // counted step t of the job is plotted where (t + 1) % stride == 0
            k = 0;
            bool inb;
            uint32_t idx;
            float zf;
            project_once(p, width, nx, ny, nz, inb, idx, zf);
            if (inb) {
                ++visits;
                if (plot) {
                    if (run_n != 0u && idx != run_idx) flush();
                    run_idx = idx;
                    ++run_n;
                    zf = zf + 0.0f;  // -0.0 -> +0.0, as render's keys
                    if (zf == zf) {
                        run_depth = true;
                        const uint32_t zs = f32_sortable(zf);
                        const unsigned long long seen = __hip_atomic_load(keys + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        if (zs >= (uint32_t)(seen >> 32)) {
                            double sx, sy, sz;
                            screen_space(p, nx, ny, nz, sx, sy, sz);
                            const double c = color_transform(a.ct, nx - x, ny - y, nz - z, sx, sy, sz);
                            const unsigned long long key = ((unsigned long long)zs << 32) | (unsigned long long)f32_sortable((float)c);
                            run_key = key > run_key ? key : run_key;
                        }
                    }
                }
            } else {
                ++outside;
                if (plot && run_n != 0u) flush();
            }
        }
        x = nx;
        y = ny;
        z = nz;
    }
    if (run_n != 0u) flush();
    if (alive) {
        a.state[job] = x;
        a.state[n + job] = y;
        a.state[2u * n + job] = z;
    }

    // the lanes' words over the wave, the waves' over the workgroup, then thread 0's few atomics (no lane left early)
    const unsigned long long w_sum[6] = {flow_wave_sum(done),      flow_wave_sum(visits),    flow_wave_sum(outside),
                                         flow_wave_sum(c_atomics), flow_wave_sum(k_atomics), flow_wave_sum(esc)};
    unsigned long long w_ext[6];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w_ext[c] = flow_wave_min(done ? f64_sortable(lo[c]) : kFlowNoMin);
        w_ext[3 + c] = flow_wave_max(done ? f64_sortable(hi[c]) : 0ull);
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) {
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            s_sum[c][wave] = w_sum[c];
            s_ext[c][wave] = w_ext[c];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        FlowSums* const s = a.sums;
        unsigned long long* const dst[6] = {&s->steps, &s->visits, &s->outside, &s->count_atomics, &s->key_atomics, &s->escaped};
        for (int c = 0; c < 6; ++c) {
            const unsigned long long t = (s_sum[c][0] + s_sum[c][1]) + (s_sum[c][2] + s_sum[c][3]);
            if (t) atomicAdd(dst[c], t);
        }
        for (int c = 0; c < 3; ++c) {
            unsigned long long l = s_ext[c][0], u = s_ext[3 + c][0];
            for (int w = 1; w < 4; ++w) {
                l = s_ext[c][w] < l ? s_ext[c][w] : l;
                u = s_ext[3 + c][w] > u ? s_ext[3 + c][w] : u;
            }
            if (l != kFlowNoMin) atomicMin(&s->lo[c], l);
            if (u != 0ull) atomicMax(&s->hi[c], u);
        }
    }
}

__global__ void __launch_bounds__(256) k_flow_resolve(const FlowResolveArgs a) {
    __shared__ uint32_t s_tmp[4];
    uint32_t m = 0;
    const uint32_t stride = gridDim.x * 256u;
    for (uint32_t pix = blockIdx.x * 256u + threadIdx.x; pix < a.npix; pix += stride) {
        const uint32_t c = a.count[pix];
        m = c > m ? c : m;
        const unsigned long long key = a.keys[pix];
        if (key != 0ull) {
            const uint32_t zs = (uint32_t)(key >> 32), hue = (uint32_t)key;
            // render's strict test zf > zbuf[pix] on the floats: false against a held NaN of either sign (a negative NaN's sortable
            // image lies below -inf's, and an integer compare would let every depth replace it); -1 and below never beat the sentinel
            // (the held depth is read as the key's high dword alone: ROCm 7.2's instruction selection crashes on this compare where
            // the word is shifted out of the 64-bit load)
            typedef uint32_t __attribute__((may_alias)) u32_alias;
            const uint32_t held = reinterpret_cast<const u32_alias*>(a.zkey)[2u * (size_t)pix + 1u];
            if (sortable_f32(zs) > sortable_f32(held)) {
                a.zkey[pix] = ((unsigned long long)zs << 32) | 0xFFFFFFFFull;
                a.steps[pix] = (double)sortable_f32(hue);
            }
        }
    }
    m = block_max_u32(m, s_tmp);
    if (threadIdx.x == 0u && m) raise_scalar(&a.scalars[SC_MAX], m);
}

void launch_flow_transient(const FlowArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_flow_transient, dim3((a.n_jobs + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_flow_render(const FlowArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_flow_render, dim3((a.n_jobs + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_flow_resolve(const FlowResolveArgs& a, hipStream_t s) {
    const uint32_t blocks = (a.npix + 255u) / 256u;
    hipLaunchKernelGGL(k_flow_resolve, dim3(blocks < 2048u ? blocks : 2048u), dim3(256), 0, s, a);
}

}  // namespace sar
