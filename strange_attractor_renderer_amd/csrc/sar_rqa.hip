// sar_rqa.hip — gfx950 (MI355X) kernels of the recurrence analysis (include/sar.h: sar_runtime_recurrence, sar_runtime_rqa,
// sar_runtime_recurrence_plot).
//
// The recurrence matrix R(i, j) = |i - j| > theiler && r2(i, j) < eps2 of a trajectory is never stored. k_rqa_diag gives a lane one
// diagonal j = i + k and k_rqa_vert one column j; the lane walks its line from end to end with the length of the run it is in in a
// register, so no run is ever cut between lanes, workgroups or launches and nothing has to be stitched: every output is a sum of
// integers or a maximum. The points of a walk come through LDS in chunks: p_i is one address for the whole wave — a broadcast —,
// p_(i + k) consecutive doubles across the lanes, 32 of them one bank row of a ds_read_b64. A finished run is one add on a
// histogram in LDS, kept in copies as k_corr_pairs keeps its own (on chaotic data most runs end at length 1, in one bin), folded
// into the set's 64-bit counts at the end. r2 = (dx dx + dy dy) + dz dz is k_corr_pairs' arithmetic: subtracts, multiplies, adds and
// a compare, so the build's fused-op audit pins the kernels at 0. DESIGN.md section 26 has the decomposition, the LDS budget and the
// counters' bounds.
#include "sar_rqa.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

typedef uint32_t __attribute__((may_alias)) rqa_lds_u32;

namespace {

// What a lane carries along a walk and the workgroup's histogram: [B + 2][R] words, row B + 1 the spare one that takes the add of
// every entry that finishes no line — no branch, so that the loads and the arithmetic of successive entries overlap.
struct RqaWalk {
    rqa_lds_u32* hist;
    uint32_t bins, rep, copy;    // B, log2 R, the lane's copy
    uint32_t run, longest, recs;

    __device__ void entry(bool rec) {
        const uint32_t l = run < bins ? run : bins;
        const uint32_t b = (!rec && run) ? l : bins + 1u;
        __hip_atomic_fetch_add(hist + ((b << rep) + copy), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        longest = run > longest ? run : longest;
        recs += rec ? 1u : 0u;
        run = rec ? run + 1u : 0u;
    }
    // the end of a line of the matrix ends a run
    __device__ void end() { entry(false); }
};

__device__ inline bool rqa_skipped(const RqaArgs& a, uint32_t set) { return !(a.eps2[set] > 0.); }

__device__ inline void rqa_hist_clear(rqa_lds_u32* hist, uint32_t words, uint32_t* totals) {
    for (uint32_t k = threadIdx.x; k < words; k += kRqaBlock) hist[k] = 0u;
    if (threadIdx.x < 2u) totals[threadIdx.x] = 0u;
}

// The workgroup's histogram into out[0 .. B], its longest run into *longest and (nullable) its recurrent entries into *recs
__device__ inline void rqa_flush(const RqaWalk& w, uint32_t* totals, unsigned long long* out, unsigned long long* longest,
                                 unsigned long long* recs) {
    __hip_atomic_fetch_max(&totals[0], w.longest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (recs) __hip_atomic_fetch_add(&totals[1], w.recs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    const uint32_t tid = threadIdx.x, copies = 1u << w.rep;
    // one 64-bit atomic per non-empty bin; a lane starts at its own copy so that the lanes of a wave read different banks
    for (uint32_t b = tid; b <= w.bins; b += kRqaBlock) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < copies; ++k) sum += w.hist[(b << w.rep) + ((k + tid) & (copies - 1u))];
        if (sum) atomicAdd(out + b, (unsigned long long)sum);
    }
    if (tid == 0u && totals[0]) atomicMax(longest, (unsigned long long)totals[0]);
    if (tid == 1u && recs && totals[1]) atomicAdd(recs, (unsigned long long)totals[1]);
}

}  // namespace

// ---------------------------------------------------------------------------------------------------
// k_rqa_diag — grid (workgroups of the launch); workgroup first + blockIdx.x is (set, job, folded band f) and takes the bands f and
// nb - 1 - f of the job's diagonals one after the other. Lane t of band b owns diagonal k = theiler + 1 + 256 b + t with its T - k
// entries R(i, i + k); the band's first diagonal is its longest. Per chunk of kRqaWalk values of i the workgroup loads p_i and the
// window p_(i + k0) .. p_(i + k0 + 255 + kRqaWalk - 1); what lies past the trajectory's end is loaded as 0 and is not recurrent.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRqaBlock) k_rqa_diag(const RqaArgs a, uint32_t first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rqa_lds[];
    __shared__ double pi[3][kRqaWalk];
    __shared__ double pj[3][kRqaWalk + kRqaBlock];
    __shared__ uint32_t totals[2];

    const uint32_t tid = threadIdx.x, wg = first + blockIdx.x;
    const uint32_t f = wg % a.per_job, job = (wg / a.per_job) % a.jobs, set = wg / a.per_job / a.jobs;
    if (rqa_skipped(a, set)) return;  // (the whole workgroup)

    RqaWalk w;
    w.hist = (rqa_lds_u32*)rqa_lds;
    w.bins = a.line_bins;
    w.rep = a.rep_shift;
    w.copy = tid & ((1u << w.rep) - 1u);
    w.run = w.longest = w.recs = 0u;
    rqa_hist_clear(w.hist, (w.bins + 2u) << w.rep, totals);

    const uint32_t T = a.samples, nb = rqa_bands(T, a.theiler);
    const double eps2 = a.eps2[set];
    const double* const px = a.points + (size_t)set * 3u * a.n + (size_t)job * T;
    const double* const py = px + a.n;
    const double* const pz = py + a.n;

    for (uint32_t half = 0; half < 2u; ++half) {
        const uint32_t band = half ? nb - 1u - f : f;
        if (half && band == f) break;  // (the middle band of an odd number; the same for the whole workgroup)
        const uint32_t k0 = a.theiler + 1u + band * kRqaBlock, k = k0 + tid;  // k0 <= T - 1 <= 2^20: no wrap
        const uint32_t len = k < T ? T - k : 0u, longest_len = T - k0;
        for (uint32_t i0 = 0; i0 < longest_len; i0 += kRqaWalk) {
            __syncthreads();  // (the histogram is clear; the last chunk has been read)
            {
                const uint32_t i = i0 + tid;
                const bool have = i < T;
                pi[0][tid] = have ? px[i] : 0.;
                pi[1][tid] = have ? py[i] : 0.;
                pi[2][tid] = have ? pz[i] : 0.;
            }
            for (uint32_t t = tid; t < kRqaWalk + kRqaBlock; t += kRqaBlock) {
                const uint32_t j = i0 + k0 + t;
                const bool have = j < T;
                pj[0][t] = have ? px[j] : 0.;
                pj[1][t] = have ? py[j] : 0.;
                pj[2][t] = have ? pz[j] : 0.;
            }
            __syncthreads();
            const uint32_t cnt = longest_len - i0 < kRqaWalk ? longest_len - i0 : kRqaWalk;
            for (uint32_t ii = 0; ii < cnt; ++ii) {
                const double dx = pj[0][ii + tid] - pi[0][ii], dy = pj[1][ii + tid] - pi[1][ii], dz = pj[2][ii + tid] - pi[2][ii];
                const double r2 = (dx * dx + dy * dy) + dz * dz;
                w.entry((i0 + ii < len) & (r2 < eps2));
            }
        }
        w.end();
    }
    unsigned long long* const out = a.out + (size_t)set * rqa_row(w.bins);
    rqa_flush(w, totals, out, out + 2u * (w.bins + 1u) + 1u, out + 2u * (w.bins + 1u));
}

// ---------------------------------------------------------------------------------------------------
// k_rqa_vert — grid (workgroups of the launch); workgroup first + blockIdx.x is (set, job, column tile). Lane t owns column
// j = 256 tile + t with p_j in registers and walks i = 0 .. T - 1 over the full matrix; the Theiler band's entries are zeros and
// cut a run. A column past the trajectory's end (the last tile's tail) has no recurrent entry.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRqaBlock) k_rqa_vert(const RqaArgs a, uint32_t first) {
    extern __shared__ __attribute__((aligned(16))) unsigned char rqa_lds[];
    __shared__ double pi[3][kRqaWalk];
    __shared__ uint32_t totals[2];

    const uint32_t tid = threadIdx.x, wg = first + blockIdx.x;
    const uint32_t tile = wg % a.per_job, job = (wg / a.per_job) % a.jobs, set = wg / a.per_job / a.jobs;
    if (rqa_skipped(a, set)) return;  // (the whole workgroup)

    RqaWalk w;
    w.hist = (rqa_lds_u32*)rqa_lds;
    w.bins = a.line_bins;
    w.rep = a.rep_shift;
    w.copy = tid & ((1u << w.rep) - 1u);
    w.run = w.longest = w.recs = 0u;
    rqa_hist_clear(w.hist, (w.bins + 2u) << w.rep, totals);

    const uint32_t T = a.samples, theiler = a.theiler;
    const double eps2 = a.eps2[set];
    const double* const px = a.points + (size_t)set * 3u * a.n + (size_t)job * T;
    const double* const py = px + a.n;
    const double* const pz = py + a.n;
    const uint32_t j = tile * kRqaBlock + tid;
    const bool valid = j < T;
    const double xj = valid ? px[j] : 0., yj = valid ? py[j] : 0., zj = valid ? pz[j] : 0.;

    for (uint32_t i0 = 0; i0 < T; i0 += kRqaWalk) {
        __syncthreads();  // (the histogram is clear; the last chunk has been read)
        {
            const uint32_t i = i0 + tid;
            const bool have = i < T;
            pi[0][tid] = have ? px[i] : 0.;
            pi[1][tid] = have ? py[i] : 0.;
            pi[2][tid] = have ? pz[i] : 0.;
        }
        __syncthreads();
        const uint32_t cnt = T - i0 < kRqaWalk ? T - i0 : kRqaWalk;
        for (uint32_t ii = 0; ii < cnt; ++ii) {
            const uint32_t i = i0 + ii, gap = i > j ? i - j : j - i;
            const double dx = xj - pi[0][ii], dy = yj - pi[1][ii], dz = zj - pi[2][ii];
            const double r2 = (dx * dx + dy * dy) + dz * dz;
            w.entry(valid & (gap > theiler) & (r2 < eps2));
        }
    }
    w.end();
    unsigned long long* const out = a.out + (size_t)set * rqa_row(w.bins);
    rqa_flush(w, totals, out + (w.bins + 1u), out + 2u * (w.bins + 1u) + 2u, nullptr);
}

// ---------------------------------------------------------------------------------------------------
// k_rqa_plot — one lane per entry of a height x width window of one trajectory's matrix: row y is i = i0 + y, column x is j = j0 + x.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kRqaBlock) k_rqa_plot(const RqaPlotArgs a) {
    const uint32_t at = blockIdx.x * kRqaBlock + threadIdx.x;  // height * width <= 2^24
    if (at >= a.height * a.width) return;
    const uint32_t y = at / a.width, i = a.i0 + y, j = a.j0 + (at - y * a.width), T = a.samples;  // i, j < T: the host's check
    const double* const px = a.points;
    const double* const py = px + T;
    const double* const pz = py + T;
    const double dx = px[j] - px[i], dy = py[j] - py[i], dz = pz[j] - pz[i];
    const double r2 = (dx * dx + dy * dy) + dz * dz;
    const uint32_t gap = i > j ? i - j : j - i;
    a.out[at] = (unsigned char)(((gap > a.theiler) & (r2 < a.eps2)) ? 1u : 0u);
}

template <typename Kernel>
static int launch_rqa_walk(Kernel kernel, const RqaArgs& a, uint32_t first, uint32_t count, hipStream_t s) {
    // (per device and function; cheap next to a launch of whole walks)
    const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRqaHistLdsBytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kernel, dim3(count), dim3(kRqaBlock), ((a.line_bins + 2u) << a.rep_shift) * 4u, s, a, first);
    return 0;
}

int launch_rqa_diag(const RqaArgs& a, uint32_t first, uint32_t count, hipStream_t s) { return launch_rqa_walk(k_rqa_diag, a, first, count, s); }
int launch_rqa_vert(const RqaArgs& a, uint32_t first, uint32_t count, hipStream_t s) { return launch_rqa_walk(k_rqa_vert, a, first, count, s); }

void launch_rqa_plot(const RqaPlotArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_rqa_plot, dim3((a.height * a.width + kRqaBlock - 1u) / kRqaBlock), dim3(kRqaBlock), 0, s, a);
}

}  // namespace sar
