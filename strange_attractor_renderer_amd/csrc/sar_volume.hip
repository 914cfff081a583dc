// sar_volume.hip — the gfx950 kernels of volume rendering (sar_runtime_volume*, include/sar.h has the contract): the hit histogram
// resolved along the view ray, D slabs of width x height u32 voxels, filled by k_volume_accumulate and read by k_volume_section and
// k_volume_march.
//
// k_volume_warm / k_volume_accumulate: one lane per job. A job's point lives in device memory between launches ([3][n_jobs], read
// and written as 512-byte rows per wave), so a long job is any number of short launches: the warm-up kernel runs render's 1000
// uncounted steps, every accumulate launch n_steps counted ones. A step is iterate_once (sar_device.hpp) — next_point, screen_space,
// the projection and the bounds test are render's by construction — and, for a visit whose depth has a slab, ONE non-returning u32
// add on vol[k][j][i]. The class counters are 32-bit words per lane (a launch is at most 2^24 steps), the depth range two sortable
// keys per lane; both are summed over the wave and then over the workgroup through LDS, and thread 0 makes at most six atomics. A
// point whose x is NaN stays NaN: this and every later step passes the bounds test, lands on pixel (0, 0) and has a NaN depth, so
// the lane books the rest of the launch at once and leaves the loop. Every loop's trip count is fixed before it starts; nothing
// waits on another lane.
//
// This first version is ATOMIC-BOUND: a stored visit costs a scattered global atomic, and the chip retires about 2.1e10 of those a
// second whatever the kernel around them does (sar_iterate.hip has the measurement).
//
// k_volume_reduce: the largest voxel and the number of non-empty ones, a grid-stride pass over the volume at the end of a call.
//
// k_volume_section / k_volume_march: one lane per pixel, consecutive lanes on consecutive i, so a wave reads 256 contiguous bytes of
// every slab. The march composites front to back in fp64, in include/sar.h's order; the slabs' colours — the palette blend at the
// slab's position, three square roots — are computed once per workgroup into LDS, next to a copy of the palette's rows.
//
// Contraction off. The accumulate, warm-up, reduce and section kernels hold no fused fp64 op; k_volume_march holds the expansions of
// its divisions and the blend's square roots and nothing else (the build's audit pins all five).
#include "sar_device.hpp"
#include "sar_volume.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

namespace {

__device__ __forceinline__ unsigned long long volume_wave_sum(uint32_t v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}
__device__ __forceinline__ uint32_t volume_wave_min(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint32_t volume_wave_max(uint32_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, off);
        v = o > v ? o : v;
    }
    return v;
}

}  // namespace

__global__ void __launch_bounds__(256) k_volume_warm(const VolumeArgs a) {
    const uint32_t job = blockIdx.x * 256u + threadIdx.x;
    if (job >= a.n_jobs) return;  // (no barrier in this kernel)
    MapParams p = a.p;
    pin_map_params(p);
    const size_t n = a.n_jobs;
    double x = a.state[job], y = a.state[n + job], z = a.state[2u * n + job];
    for (int w = 0; w < 1000; ++w) next_point(p, x, y, z);  // "skip first 1000 to get good values in the attractor" (:750-752)
    a.state[job] = x;
    a.state[n + job] = y;
    a.state[2u * n + job] = z;
}

__global__ void __launch_bounds__(256) k_volume_accumulate(const VolumeArgs a) {
    __shared__ unsigned long long s_sum[4][4];
    __shared__ uint32_t s_key[2][4];
    const uint32_t job = blockIdx.x * 256u + threadIdx.x;
    const bool valid = job < a.n_jobs;
    const uint32_t slot = valid ? job : 0u;  // (a lane beyond the last job reads job 0's point and runs no step)
    MapParams p = a.p;
    pin_map_params(p);
    const size_t n = a.n_jobs;
    double x = a.state[slot], y = a.state[n + slot], z = a.state[2u * n + slot];

    const uint32_t steps = valid ? a.n_steps : 0u;
    const uint32_t width = a.width, npix = a.npix;
    const double z_lo = a.z_lo, dscale = a.dscale, slabs_f = a.slabs_f;
    uint32_t* const vol = a.vol;
    uint32_t visits = 0, below = 0, above = 0, nan = 0, kmin = kVolumeNoMin, kmax = 0;
    for (uint32_t t = 0; t < steps; ++t) {
        bool inb;
        uint32_t idx;
        float zf;
        iterate_once(p, width, x, y, z, inb, idx, zf);
        if (x != x) {  // absorbed: this step and the rest of the launch are visits of pixel (0, 0) with a NaN depth
            visits += steps - t;
            nan += steps - t;
            break;
        }
        if (inb) {
            ++visits;
            const int32_t k = volume_slab(zf, z_lo, dscale, slabs_f);
            if (k >= 0) {  // idx < npix (the bounds test), k < slabs: the voxel is inside the volume
                __hip_atomic_fetch_add(vol + ((size_t)(uint32_t)k * npix + idx), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                below += k == kVolumeBelow ? 1u : 0u;
                above += k == kVolumeAbove ? 1u : 0u;
                nan += k == kVolumeNan ? 1u : 0u;
            }
            if ((__float_as_uint(zf) & 0x7fffffffu) < 0x7f800000u) {  // finite
                const uint32_t key = f32_sortable(zf);
                kmin = key < kmin ? key : kmin;
                kmax = key > kmax ? key : kmax;
            }
        }
    }
    if (valid) {
        a.state[job] = x;
        a.state[n + job] = y;
        a.state[2u * n + job] = z;
    }

    // the lanes' words over the wave, the waves' over the workgroup, then thread 0's few atomics (no lane left early)
    const unsigned long long w_visits = volume_wave_sum(visits), w_below = volume_wave_sum(below), w_above = volume_wave_sum(above),
                             w_nan = volume_wave_sum(nan);
    const uint32_t w_min = volume_wave_min(kmin), w_max = volume_wave_max(kmax);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0u) {
        s_sum[0][wave] = w_visits;
        s_sum[1][wave] = w_below;
        s_sum[2][wave] = w_above;
        s_sum[3][wave] = w_nan;
        s_key[0][wave] = w_min;
        s_key[1][wave] = w_max;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        unsigned long long t[4];
        for (int c = 0; c < 4; ++c) t[c] = (s_sum[c][0] + s_sum[c][1]) + (s_sum[c][2] + s_sum[c][3]);
        uint32_t lo = s_key[0][0], hi = s_key[1][0];
        for (int w = 1; w < 4; ++w) {
            lo = s_key[0][w] < lo ? s_key[0][w] : lo;
            hi = s_key[1][w] > hi ? s_key[1][w] : hi;
        }
        VolumeSums* const s = a.sums;
        if (t[0]) atomicAdd(&s->visits, t[0]);
        if (t[1]) atomicAdd(&s->below, t[1]);
        if (t[2]) atomicAdd(&s->above, t[2]);
        if (t[3]) atomicAdd(&s->nan, t[3]);
        if (lo != kVolumeNoMin) atomicMin(&s->zmin_key, lo);
        if (hi != 0u) atomicMax(&s->zmax_key, hi);
    }
}

__global__ void __launch_bounds__(256) k_volume_reduce(const uint32_t* vol, size_t n, VolumeSums* sums) {
    __shared__ unsigned long long s_cnt[4];
    __shared__ uint32_t s_max[4];
    uint32_t cnt = 0, m = 0;  // (a lane sees n / (gridDim * 256) + 1 voxels: far below 2^32)
    const size_t stride = (size_t)gridDim.x * 256u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
        const uint32_t v = vol[i];
        cnt += v ? 1u : 0u;
        m = v > m ? v : m;
    }
    const unsigned long long w_cnt = volume_wave_sum(cnt);
    const uint32_t w_max = volume_wave_max(m);
    if ((threadIdx.x & 63u) == 0u) {
        s_cnt[threadIdx.x >> 6] = w_cnt;
        s_max[threadIdx.x >> 6] = w_max;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const unsigned long long c = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
        uint32_t mm = s_max[0];
        for (int w = 1; w < 4; ++w) mm = s_max[w] > mm ? s_max[w] : mm;
        if (c) atomicAdd(&sums->nonempty, c);
        if (mm) atomicMax(&sums->vmax, mm);
    }
}

__global__ void __launch_bounds__(256) k_volume_section(const VolumeSectionArgs a) {
    const uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    if (pix >= a.npix) return;
    const uint32_t* v = a.vol + ((size_t)a.k0 * a.npix + pix);
    uint32_t sum = 0;
    int32_t nearest = -1;
    for (uint32_t k = a.k0; k < a.k1; ++k, v += a.npix) {
        const uint32_t c = *v;
        sum += c;  // wraps as count does
        nearest = c ? (int32_t)k : nearest;
    }
    if (a.count) a.count[pix] = sum;
    if (a.nearest) a.nearest[pix] = nearest;
}

__global__ void __launch_bounds__(256) k_volume_march(const VolumeMarchArgs a) {
    __shared__ double s_pal[(SAR_PALETTE_MAX + 1) * 3];
    __shared__ double s_rgb[kMaxVolumeSlabs][3];
    __shared__ unsigned long long s_seen[4];
    __shared__ uint32_t s_cov[4], s_stop[4];
    const uint32_t len = a.pal.len;
    for (uint32_t e = threadIdx.x; e < (len + 1u) * 3u; e += 256u) s_pal[e] = a.pal.rgb[e / 3u][e % 3u];
    __syncthreads();
    // the colour of slab k: the palette blend at the slab's centre, v_k = pos_lo + (((double)k + 0.5) / D) * (pos_hi - pos_lo)
    for (uint32_t k = a.k0 + threadIdx.x; k < a.k1; k += 256u) {
        const double v = a.pos_lo + (((double)k + 0.5) / a.slabs_f) * a.dpos;
        double r, g, b;
        palette_blend(v, s_pal, len, r, g, b);
        s_rgb[k][0] = r;
        s_rgb[k][1] = g;
        s_rgb[k][2] = b;
    }
    __syncthreads();

    const uint32_t pix = blockIdx.x * 256u + threadIdx.x;
    const bool valid = pix < a.npix;
    const uint32_t npix = a.npix, k0 = a.k0;
    const double half = a.half, t_min = a.t_min;
    double T = 1.0, R = 0.0, G = 0.0, B = 0.0;
    uint32_t seen = 0;
    bool stopped = false;
    if (valid) {
        const uint32_t* v = a.vol + ((size_t)a.k1 * npix + pix);
        for (uint32_t k = a.k1; k > k0;) {  // front to back: slab D - 1 is nearest to the viewer
            --k;
            v -= npix;
            const uint32_t c = *v;
            if (!c) continue;
            ++seen;
            const double nd = (double)c;
            const double al = nd / (nd + half);
            const double w = T * al;
            R = R + w * s_rgb[k][0];
            G = G + w * s_rgb[k][1];
            B = B + w * s_rgb[k][2];
            T = T * (1.0 - al);
            if (T < t_min) {
                stopped = true;
                break;
            }
        }
        double c[4];
        if (a.transparent) {
            const double cover = 1.0 - T;
            const bool any = T < 1.0;
            c[0] = any ? R / cover : 0.0;
            c[1] = any ? G / cover : 0.0;
            c[2] = any ? B / cover : 0.0;
            c[3] = cover;
        } else {
            c[0] = R + T * a.bg[0];
            c[1] = G + T * a.bg[1];
            c[2] = B + T * a.bg[2];
            c[3] = 1.0;
        }
        uint16_t q[4];
#pragma unroll
        for (int ch = 0; ch < 4; ++ch) {
            double e = c[ch];
            e = e > 0. ? e : 0.;  // (NaN gives 0)
            e = e < 1. ? e : 1.;
            q[ch] = as_u16(e * 65535.0);
        }
        a.out[pix] = make_ushort4(q[0], q[1], q[2], q[3]);
    }

    const unsigned long long w_seen = volume_wave_sum(seen);
    const unsigned long long w_cov = volume_wave_sum(seen ? 1u : 0u), w_stop = volume_wave_sum(stopped ? 1u : 0u);
    if ((threadIdx.x & 63u) == 0u) {
        s_seen[threadIdx.x >> 6] = w_seen;
        s_cov[threadIdx.x >> 6] = (uint32_t)w_cov;
        s_stop[threadIdx.x >> 6] = (uint32_t)w_stop;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        const unsigned long long n_seen = (s_seen[0] + s_seen[1]) + (s_seen[2] + s_seen[3]);
        const uint32_t n_cov = (s_cov[0] + s_cov[1]) + (s_cov[2] + s_cov[3]), n_stop = (s_stop[0] + s_stop[1]) + (s_stop[2] + s_stop[3]);
        if (n_seen) atomicAdd(&a.sums->slabs_seen, n_seen);
        if (n_cov) atomicAdd(&a.sums->covered, n_cov);
        if (n_stop) atomicAdd(&a.sums->stopped, n_stop);
    }
}

void launch_volume_warm(const VolumeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_volume_warm, dim3((a.n_jobs + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_volume_accumulate(const VolumeArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_volume_accumulate, dim3((a.n_jobs + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_volume_reduce(const uint32_t* vol, size_t n, VolumeSums* sums, hipStream_t s) {
    const size_t blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(k_volume_reduce, dim3((uint32_t)(blocks < 2048u ? blocks : 2048u)), dim3(256), 0, s, vol, n, sums);
}
void launch_volume_section(const VolumeSectionArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_volume_section, dim3((a.npix + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_volume_march(const VolumeMarchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_volume_march, dim3((a.npix + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace sar
