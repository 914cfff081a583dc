// sar_section.hip — the gfx950 kernels of the Poincare sections of flows (sar_runtime_section, include/sar.h has the contract): the
// crossings of an RK4 trajectory with a quadric surface g = 0, each refined by one step of Henon's system, recorded with their return
// times and, on request, plotted into the runtime's frame.
//
// k_flow_section: one lane per job, as k_flow_render. Between launches a job lives in device memory as SoA rows — its point (flows'
// [3][n_jobs]), the step and the time offset of its previous crossing, what it has found — so a long job is any number of short
// launches, and nothing here depends on how the steps are cut into them: a return time is formed from two step ordinals and two
// offsets, never from an accumulated time. The loop body is section_step (sar_section.hpp): flow_step plus ONE evaluation of g — g0 is
// the previous step's g1 — and the crossing test; the refinement (four rates, five divisions, a sixth on the rough path) sits behind
// the branch that only crossing lanes enter, about one step in 75 on Lorenz at dt 0.01. A crossing after the job's first (the clock
// crossing) stores 32 bytes, q and the return time, to [job][found]: rare and scattered. A job that escapes takes NaN as its saved x,
// as in flows; a job that holds `samples` crossings is FULL, and it and an escaped one are skipped by every later launch.
//
// The lanes' counters (32-bit words: a launch is at most 2^24 steps), the extent of the recorded crossings, the extrema of the
// return times and the largest residual |g(q)| are reduced over the wave, then through LDS over the workgroup, and thread 0 makes the
// few atomics, the doubles as their sortable images. Every lane reaches the reduction: a loop ends by break alone.
//
// k_section_plot: one lane per (job, k < found): project_once (sar_device.hpp) in cfg's view, one add on count, one max on the keys
// that k_flow_resolve (sar_flow.hip, unchanged) then resolves into the frame. The key is sortable(zf) << 32 | sortable((float)r).
//
// Contraction off. k_section_plot holds no fused fp64 op, k_flow_section the expansions of its six divisions and nothing else (the
// build's audit pins both).
#include "sar_device.hpp"
#include "sar_section.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

namespace {

struct SectionField {  // P(point) in place: next_point on the kernel's pinned parameters
    const MapParams& p;
    __device__ __forceinline__ void operator()(double& x, double& y, double& z) const { next_point(p, x, y, z); }
};

__device__ __forceinline__ unsigned long long section_wave_sum(uint32_t v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
__device__ __forceinline__ unsigned long long section_wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long section_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off);
        v = o > v ? o : v;
    }
    return v;
}

constexpr double kSectionNan = __builtin_nan("");

}  // namespace

__global__ void __launch_bounds__(256) k_flow_section(const SectionArgs a) {
    __shared__ unsigned long long s_sum[7][4];
    __shared__ unsigned long long s_ext[9][4];
    const uint32_t job = blockIdx.x * 256u + threadIdx.x;
    const bool valid = job < a.n_jobs;
    const uint32_t slot = valid ? job : 0u;  // (a lane beyond the last job reads job 0's rows and runs no step)
    MapParams p = a.p;
    pin_map_params(p);
    const SectionField field{p};
    SectionSurface f = a.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) f.s[k] = vgpr_pin(f.s[k]);  // (the field's x and y rows fill the scalar file, as in the flow kernels)
    f.d2 = vgpr_pin(f.d2);
    f.d6 = vgpr_pin(f.d6);
    f.d9 = vgpr_pin(f.d9);
    const size_t n = a.n_jobs;
    uint32_t* const r_status = a.rows;
    uint32_t* const r_found = a.rows + n;
    uint32_t* const r_rough = a.rows + 2u * n;
    uint32_t* const r_steps = a.rows + 3u * n;
    uint32_t* const r_clock = a.rows + 4u * n;
    uint32_t* const r_prev = a.rows + 5u * n;

    double x = a.state[slot], y = a.state[n + slot], z = a.state[2u * n + slot];
    uint32_t status = r_status[slot];
    bool run = valid && status == (uint32_t)SAR_SECTION_SHORT;  // neither full nor escaped in an earlier launch
    uint32_t esc_t = 0;
    if (run && !(x == x)) {  // the transient's mark
        esc_t = 1;
        r_status[job] = (uint32_t)SAR_SECTION_ESCAPED_TRANSIENT;
        run = false;
    }
    uint32_t found = r_found[slot], rough = r_rough[slot], clock = r_clock[slot], t_prev = r_prev[slot];
    double dt_prev = a.dt_prev[slot];
    const uint32_t found0 = found, rough0 = rough, clock0 = clock;
    const uint32_t steps = run ? a.n_steps : 0u;
    const double h = a.h, h2 = a.h2, h6 = a.h6, bound = a.bound;
    const uint32_t samples = a.samples;
    const int32_t direction = a.direction;
    double* const out = a.cross + (size_t)slot * samples * 4u;

    uint32_t done = 0, esc = 0, full = 0;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double r_lo = INFINITY, r_hi = -INFINITY, res = 0.;
    double g0 = section_g(f, x, y, z);
    for (uint32_t t = 0; t < steps; ++t) {
        double nx = x, ny = y, nz = z, g1, qx, qy, qz, dt;
        const int kind = section_step(field, f, h, h2, h6, bound, direction, g0, nx, ny, nz, g1, qx, qy, qz, dt);
        if (kind < 0) {  // escaped: the failing point is dropped, and no crossing is looked for in its step
            esc = 1;
            x = kSectionNan;
            status = (uint32_t)SAR_SECTION_ESCAPED;
            break;
        }
        ++done;
        x = nx;
        y = ny;
        z = nz;
        g0 = g1;
        if (kind > 0) {
            const uint32_t T = a.t0 + t;
            if (clock == kSectionNone) {
                clock = T;  // the clock crossing: not recorded
            } else {
                const double r = ((double)(T - t_prev) * h + dt) - dt_prev;
                double* const o = out + (size_t)found * 4u;
                o[0] = qx;
                o[1] = qy;
                o[2] = qz;
                o[3] = r;
                ++found;
                rough += kind == 2 ? 1u : 0u;
                lo[0] = qx < lo[0] ? qx : lo[0];
                hi[0] = qx > hi[0] ? qx : hi[0];
                lo[1] = qy < lo[1] ? qy : lo[1];
                hi[1] = qy > hi[1] ? qy : hi[1];
                lo[2] = qz < lo[2] ? qz : lo[2];
                hi[2] = qz > hi[2] ? qz : hi[2];
                r_lo = r < r_lo ? r : r_lo;
                r_hi = r > r_hi ? r : r_hi;
                const double gq = section_g(f, qx, qy, qz);
                const double aq = gq < 0. ? -gq : gq;
                res = aq > res ? aq : res;
            }
            t_prev = T;
            dt_prev = dt;
            if (found == samples) {
                full = 1;
                status = (uint32_t)SAR_SECTION_FULL;
                break;
            }
        }
    }
    if (run) {
        a.state[job] = x;
        a.state[n + job] = y;
        a.state[2u * n + job] = z;
        a.dt_prev[job] = dt_prev;
        r_status[job] = status;
        r_found[job] = found;
        r_rough[job] = rough;
        r_steps[job] = a.t0 + done;
        r_clock[job] = clock;
        r_prev[job] = t_prev;
    }

    // the lanes' words over the wave, the waves' over the workgroup, then thread 0's few atomics (no lane left early)
    const uint32_t got = found - found0;
    const unsigned long long w_sum[7] = {section_wave_sum(done),
                                         section_wave_sum(got),
                                         section_wave_sum(rough - rough0),
                                         section_wave_sum(clock != clock0 ? 1u : 0u),
                                         section_wave_sum(full),
                                         section_wave_sum(esc),
                                         section_wave_sum(esc_t)};
    unsigned long long w_ext[9];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        w_ext[c] = section_wave_min(got ? f64_sortable(lo[c]) : kFlowNoMin);
        w_ext[3 + c] = section_wave_max(got ? f64_sortable(hi[c]) : 0ull);
    }
    w_ext[6] = section_wave_min(got ? f64_sortable(r_lo) : kFlowNoMin);
    w_ext[7] = section_wave_max(got ? f64_sortable(r_hi) : 0ull);
    w_ext[8] = section_wave_max(got ? f64_sortable(res) : 0ull);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) {
#pragma unroll
        for (int c = 0; c < 7; ++c) s_sum[c][wave] = w_sum[c];
#pragma unroll
        for (int c = 0; c < 9; ++c) s_ext[c][wave] = w_ext[c];
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        SectionSums* const s = a.sums;
        unsigned long long* const dst[7] = {&s->steps, &s->crossings, &s->rough, &s->clocked, &s->full, &s->escaped, &s->escaped_transient};
        for (int c = 0; c < 7; ++c) {
            const unsigned long long t = (s_sum[c][0] + s_sum[c][1]) + (s_sum[c][2] + s_sum[c][3]);
            if (t) atomicAdd(dst[c], t);
        }
        unsigned long long* const mins[4] = {&s->lo[0], &s->lo[1], &s->lo[2], &s->ret_lo};
        unsigned long long* const maxs[5] = {&s->hi[0], &s->hi[1], &s->hi[2], &s->ret_hi, &s->residual};
        const int min_at[4] = {0, 1, 2, 6}, max_at[5] = {3, 4, 5, 7, 8};
        for (int c = 0; c < 4; ++c) {
            unsigned long long l = s_ext[min_at[c]][0];
            for (int w = 1; w < 4; ++w) l = s_ext[min_at[c]][w] < l ? s_ext[min_at[c]][w] : l;
            if (l != kFlowNoMin) atomicMin(mins[c], l);
        }
        for (int c = 0; c < 5; ++c) {
            unsigned long long u = s_ext[max_at[c]][0];
            for (int w = 1; w < 4; ++w) u = s_ext[max_at[c]][w] > u ? s_ext[max_at[c]][w] : u;
            if (u != 0ull) atomicMax(maxs[c], u);
        }
    }
}

__global__ void __launch_bounds__(256) k_section_plot(const SectionPlotArgs a) {
    __shared__ uint32_t s_vis[2][4];
    MapParams p = a.p;
    pin_map_params(p);
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;  // (n_jobs * samples is at most 2^24)
    const uint32_t job = i / a.samples, k = i - job * a.samples;
    uint32_t vis = 0, outside = 0;
    if (job < a.n_jobs && k < a.found[job]) {
        const double* const c = a.cross + (size_t)i * 4u;
        bool inb;
        uint32_t idx;
        float zf;
        project_once(p, a.width, c[0], c[1], c[2], inb, idx, zf);
        if (inb) {  // idx < npix: it passed the bounds test
            vis = 1;
            __hip_atomic_fetch_add(a.count + idx, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            zf = zf + 0.0f;  // -0.0 -> +0.0, as render's keys
            if (zf == zf) {
                const unsigned long long key = ((unsigned long long)f32_sortable(zf) << 32) | (unsigned long long)f32_sortable((float)c[3]);
                __hip_atomic_fetch_max(a.keys + idx, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        } else {
            outside = 1;
        }
    }
    const unsigned long long w_vis = section_wave_sum(vis), w_out = section_wave_sum(outside);
    if ((threadIdx.x & 63u) == 0u) {
        s_vis[0][threadIdx.x >> 6] = (uint32_t)w_vis;
        s_vis[1][threadIdx.x >> 6] = (uint32_t)w_out;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const unsigned long long v = (unsigned long long)((s_vis[0][0] + s_vis[0][1]) + (s_vis[0][2] + s_vis[0][3]));
        const unsigned long long o = (unsigned long long)((s_vis[1][0] + s_vis[1][1]) + (s_vis[1][2] + s_vis[1][3]));
        if (v) atomicAdd(&a.sums->visits, v);
        if (o) atomicAdd(&a.sums->outside, o);
    }
}

void launch_flow_section(const SectionArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_flow_section, dim3((a.n_jobs + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_section_plot(const SectionPlotArgs& a, hipStream_t s) {
    const uint32_t lanes = a.n_jobs * a.samples;
    hipLaunchKernelGGL(k_section_plot, dim3((lanes + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace sar
