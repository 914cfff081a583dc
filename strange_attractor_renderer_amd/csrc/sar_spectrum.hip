// sar_spectrum.hip — gfx950 (MI355X) kernels of the power spectra (include/sar.h: sar_runtime_spectra, sar_runtime_spectrum).
//
// k_spectrum<PER> is the Welch periodogram of one trajectory: a workgroup takes one (set, job), walks its segments in order and keeps
// the sum of the periodograms in registers, every bin in the lane that owns it. A segment lives in LDS as re[] and im[]: the
// plotted value v of every sample, stored where the bit reversal of its index points, the two pairwise sums (the mean and the
// energy), the taper, and log2 N stages of plain radix-2 butterflies. k_spectrum_fold adds the jobs of a set in job order. All of it
// is fp64 multiplies, adds and subtractions in the order include/sar.h states — no division, square root or logarithm, so the
// build's fused-op audit pins both kernels at 0 and a numpy restatement gives the same doubles. DESIGN.md section 25 has the LDS
// layout, the padding and the cost.
#include "sar_spectrum.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

namespace {

__device__ inline uint32_t spectrum_at(uint32_t i, uint32_t pad_shift) { return i + (i >> pad_shift); }

// tree(a) of include/sar.h over the bit-reversed re[]: a[2 i] and a[2 i + 1] lie N / 2 apart there, their sums — again in
// bit-reversed order — go to the lower half of im[], and so on down to im[0]. SQUARES: tree(a o a), the squares taken at the first
// level. Every lane returns the sum; im[] is free again behind the call.
template <bool SQUARES>
__device__ inline double spectrum_tree(const double* re, double* im, uint32_t n, uint32_t pad_shift, uint32_t tid) {
    uint32_t h = n >> 1;
    for (uint32_t j = tid; j < h; j += kSpectrumBlock) {
        const double lo = re[spectrum_at(j, pad_shift)], hi = re[spectrum_at(j + h, pad_shift)];
        im[spectrum_at(j, pad_shift)] = SQUARES ? lo * lo + hi * hi : lo + hi;
    }
    __syncthreads();
    for (h >>= 1; h >= 1u; h >>= 1) {
        for (uint32_t j = tid; j < h; j += kSpectrumBlock)
            im[spectrum_at(j, pad_shift)] = im[spectrum_at(j, pad_shift)] + im[spectrum_at(j + h, pad_shift)];
        __syncthreads();
    }
    const double sum = im[0];
    __syncthreads();
    return sum;
}

__device__ inline bool spectrum_failed(const CorrMapState* state, uint32_t set) {
    return state && __hip_atomic_load(&state[set].fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kCorrNoFail;
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// k_spectrum<PER> — grid (workgroups of the launch), workgroup `first + blockIdx.x` of the group's sets * jobs; PER = the
// butterflies of a stage per lane, N <= 512 PER. Lane t holds samples t, t + 256, ... of a segment (2 PER at most) and bins t,
// t + 256, ... of the spectrum (PER + 1 at most). The LDS is dynamic: re[], then im[], each N doubles and their padding. Global
// loads are issued a phase ahead of their use: the next segment's samples before this segment's stages, and a stage's twiddles
// — the same for every segment, but up to 12 PER of them per lane, too many to keep — before the stage in front of it.
// ---------------------------------------------------------------------------------------------------
template <uint32_t PER>
__device__ inline void spectrum_series(const SpectrumArgs& a, const double* px, const double* py, const double* pz, uint32_t at, uint32_t n,
                                       uint32_t tid, double (&v)[2u * PER]) {
#pragma unroll
    for (uint32_t r = 0; r < 2u * PER; ++r) {
        const uint32_t i = tid + r * kSpectrumBlock;
        v[r] = i < n ? (a.proj[0] * px[at + i] + a.proj[1] * py[at + i]) + a.proj[2] * pz[at + i] : 0.;
    }
}

// stage l's twiddle of every butterfly of this lane (j << shift < N / 2 whatever b is: no lane reads past the table)
template <uint32_t PER>
__device__ inline void spectrum_stage_twiddles(const double2* tw, uint32_t l, uint32_t log2n, uint32_t tid, double2 (&w)[PER]) {
    const uint32_t half = 1u << (l - 1u), shift = log2n - l;
#pragma unroll
    for (uint32_t q = 0; q < PER; ++q) w[q] = tw[((tid + q * kSpectrumBlock) & (half - 1u)) << shift];
}

template <uint32_t PER>
__global__ void __launch_bounds__(kSpectrumBlock) k_spectrum(const SpectrumArgs a, uint32_t first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char spectrum_lds[];
    const uint32_t tid = threadIdx.x, wg = first + blockIdx.x, set = wg / a.jobs, job = wg - set * a.jobs;
    if (spectrum_failed(a.state, set)) return;  // (the whole workgroup; k_spectrum_fold writes the zeros)

    const uint32_t log2n = a.log2n, n = 1u << log2n, half_n = n >> 1, ps = spectrum_pad_shift(log2n);
    double* const re = (double*)spectrum_lds;
    double* const im = re + (n + (n >> ps));
    const double* const px = a.points + (size_t)set * 3u * a.n_points + (size_t)job * a.samples;
    const double* const py = px + a.n_points;
    const double* const pz = py + a.n_points;
    const double2* const tw = (const double2*)a.twiddles;
    const double inv_n = a.inv_n;

    double acc[PER + 1u];
#pragma unroll
    for (uint32_t q = 0; q <= PER; ++q) acc[q] = 0.;
    double energy = 0.;
    double v[2u * PER];
    spectrum_series<PER>(a, px, py, pz, 0u, n, tid, v);

    for (uint32_t seg = 0; seg < a.segments; ++seg) {
        double2 w[PER];
        spectrum_stage_twiddles<PER>(tw, 1u, log2n, tid, w);
#pragma unroll
        for (uint32_t r = 0; r < 2u * PER; ++r) {
            const uint32_t i = tid + r * kSpectrumBlock;
            if (i < n) re[spectrum_at(__brev(i) >> (32u - log2n), ps)] = v[r];
        }
        __syncthreads();
        const double mean = spectrum_tree<false>(re, im, n, ps, tid) * inv_n;
#pragma unroll
        for (uint32_t r = 0; r < 2u * PER; ++r) {
            const uint32_t i = tid + r * kSpectrumBlock;
            if (i < n) re[spectrum_at(__brev(i) >> (32u - log2n), ps)] = (v[r] - mean) * a.window[i];
        }
        __syncthreads();
        energy = energy + spectrum_tree<true>(re, im, n, ps, tid);
        for (uint32_t i = tid; i < n; i += kSpectrumBlock) im[spectrum_at(i, ps)] = 0.;
        __syncthreads();
        if (seg + 1u < a.segments) spectrum_series<PER>(a, px, py, pz, (seg + 1u) * a.hop, n, tid, v);  // at + n <= samples

        // the stages len = 2, 4, .., N: butterfly b of a stage is j = b mod len / 2 of the block b / (len / 2)
        for (uint32_t l = 1; l <= log2n; ++l) {
            double2 next[PER];
            spectrum_stage_twiddles<PER>(tw, l < log2n ? l + 1u : l, log2n, tid, next);
            const uint32_t half = 1u << (l - 1u);
#pragma unroll
            for (uint32_t q = 0; q < PER; ++q) {
                const uint32_t b = tid + q * kSpectrumBlock;
                if (b < half_n) {
                    const uint32_t j = b & (half - 1u), i0 = ((b - j) << 1) + j;
                    const uint32_t lo = spectrum_at(i0, ps), hi = spectrum_at(i0 + half, ps);
                    const double wr = w[q].x, wi = w[q].y;
                    const double ur = re[lo], ui = im[lo], br = re[hi], bi = im[hi];
                    const double tr = wr * br - wi * bi, ti = wr * bi + wi * br;
                    re[lo] = ur + tr;
                    im[lo] = ui + ti;
                    re[hi] = ur - tr;
                    im[hi] = ui - ti;
                }
            }
            __syncthreads();
#pragma unroll
            for (uint32_t q = 0; q < PER; ++q) w[q] = next[q];
        }

#pragma unroll
        for (uint32_t q = 0; q <= PER; ++q) {
            const uint32_t k = tid + q * kSpectrumBlock;
            if (k <= half_n) {
                const double xr = re[spectrum_at(k, ps)], xi = im[spectrum_at(k, ps)];
                acc[q] = acc[q] + (xr * xr + xi * xi);
            }
        }
        __syncthreads();  // (the next segment writes re[])
    }

    double* const out = a.scratch + (size_t)wg * a.row;
#pragma unroll
    for (uint32_t q = 0; q <= PER; ++q) {
        const uint32_t k = tid + q * kSpectrumBlock;
        if (k <= half_n) out[k] = acc[q];
    }
    if (tid == 0u) out[half_n + 1u] = energy;
}

// ---------------------------------------------------------------------------------------------------
// k_spectrum_fold — grid (sets * blocks_per_set): one lane per entry of a set's row — the bins, then the energy — adds the jobs'
// entries in job order from +0.0.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kSpectrumBlock) k_spectrum_fold(const SpectrumArgs a, uint32_t blocks_per_set) {
    const uint32_t set = blockIdx.x / blocks_per_set, k = (blockIdx.x - set * blocks_per_set) * kSpectrumBlock + threadIdx.x;
    if (k >= a.row) return;
    double sum = 0.;
    if (!spectrum_failed(a.state, set)) {
        const double* const in = a.scratch + (size_t)set * a.jobs * a.row + k;
        for (uint32_t j = 0; j < a.jobs; ++j) sum = sum + in[(size_t)j * a.row];
    }
    a.power[(size_t)set * a.row + k] = sum;
}

template <uint32_t PER>
static int launch_spectrum_per(const SpectrumArgs& a, uint32_t first, uint32_t count, hipStream_t s) {
    // (per device and function; cheap next to a launch of whole trajectories)
    const hipError_t e = hipFuncSetAttribute((const void*)k_spectrum<PER>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSpectrumMaxLdsBytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_spectrum<PER>, dim3(count), dim3(kSpectrumBlock), spectrum_lds_doubles(a.log2n) * sizeof(double), s, a, first);
    return 0;
}

int launch_spectrum(const SpectrumArgs& a, uint32_t first, uint32_t count, hipStream_t s) {
    const uint32_t n = 1u << a.log2n;  // N <= 512 PER
    return n <= 512u ? launch_spectrum_per<1>(a, first, count, s) : n <= 1024u ? launch_spectrum_per<2>(a, first, count, s)
         : n <= 2048u ? launch_spectrum_per<4>(a, first, count, s) : launch_spectrum_per<8>(a, first, count, s);
}

void launch_spectrum_fold(const SpectrumArgs& a, uint32_t n_sets, hipStream_t s) {
    const uint32_t blocks_per_set = (a.row + kSpectrumBlock - 1u) / kSpectrumBlock;
    hipLaunchKernelGGL(k_spectrum_fold, dim3(n_sets * blocks_per_set), dim3(kSpectrumBlock), 0, s, a, blocks_per_set);
}

}  // namespace sar
