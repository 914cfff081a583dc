// sar_corr.hip — gfx950 (MI355X) kernels of the correlation dimension (include/sar.h: sar_runtime_pairs, sar_runtime_corrdim).
//
// k_corr_orbit records the point sets: one lane per (map, job), the map's coefficients per lane as in k_search_lyapunov. k_corr_pairs
// is the all-pairs pass: a workgroup takes one pair of 256-point tiles I <= J of one set, keeps its i points in registers, one per
// lane, streams the j tile through LDS — every lane reads the same j point, a broadcast —, and counts the bin of each r^2 into a
// histogram in LDS, folded into the set's 64-bit histogram at the end. The bin comes from the bits of r^2: only subtracts,
// multiplies, adds and integer operations, no division, square root or logarithm, so the build's fused-op audit pins both kernels
// at 0 and a host restatement gives the same integers. DESIGN.md section 16 has the histogram layout, the LDS budget and resources.
#include "sar_corr.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

typedef uint32_t __attribute__((may_alias)) corr_lds_u32;

// ---------------------------------------------------------------------------------------------------
// k_corr_orbit — grid (ceil(jobs / 256), maps). A job runs `transient` steps, then `samples` times `stride` steps and a recorded
// point. The first point outside the bound box ends the job and lowers the map's failure key to (job, step); a wave whose lanes are
// all dead stops (CheckedSteps). Points go SoA into device memory at index job * samples + sample; the extent of
// the points recorded by live jobs moves the map's sortable minima and maxima, one atomic per wave and bound.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_corr_orbit(const CorrOrbitArgs a) {
    const uint32_t map = a.first_map + blockIdx.y, job = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = job < a.jobs;
    SearchCoeffs c;
    load_coeffs(a.coeffs + (size_t)map * kSearchCoeffs, c);
    double x = 0., y = 0., z = 0.;
    if (valid) {
        x = a.starts[3u * job];
        y = a.starts[3u * job + 1u];
        z = a.starts[3u * job + 2u];
    }
    const double bound = a.bound;
    bool alive = valid;
    unsigned long long fail = 0;  // the 1-based step of this job's failure
    for (CheckedSteps run(a.transient); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool ok = within(x, y, z, bound);
            fail = (alive & !ok) ? (unsigned long long)t + 1ull : fail;
            alive = alive & ok;
        }
    double* const px = a.points + (size_t)map * 3u * a.n;
    double* const py = px + a.n;
    double* const pz = py + a.n;
    const size_t at = (size_t)job * a.samples;
    const uint32_t total = a.stride * a.samples;  // <= 2^31
    uint32_t left = a.stride, sample = 0;
    double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
    for (CheckedSteps run(total); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool ok = within(x, y, z, bound);
            fail = (alive & !ok) ? (unsigned long long)a.transient + t + 1ull : fail;
            alive = alive & ok;
            if (--left == 0u) {  // (the same step in every lane)
                left = a.stride;
                if (valid) {
                    px[at + sample] = x;
                    py[at + sample] = y;
                    pz[at + sample] = z;
                }
                lo[0] = (alive & (x < lo[0])) ? x : lo[0];
                hi[0] = (alive & (x > hi[0])) ? x : hi[0];
                lo[1] = (alive & (y < lo[1])) ? y : lo[1];
                hi[1] = (alive & (y > hi[1])) ? y : hi[1];
                lo[2] = (alive & (z < lo[2])) ? z : lo[2];
                hi[2] = (alive & (z > hi[2])) ? z : hi[2];
                ++sample;
            }
        }
    CorrMapState* const st = a.state + map;
    if (valid & !alive) atomicMin(&st->fail, ((unsigned long long)job << 40) | fail);
#pragma unroll
    for (int k = 0; k < 3; ++k) wave_extent(lo[k], hi[k], &st->lo[k], &st->hi[k]);
}

// ---------------------------------------------------------------------------------------------------
// k_corr_pairs — grid (cells of the folded tile-pair triangle, sets). The LDS histogram is kept in R = 2^rep_shift copies laid out
// [bin][R]: lane l adds to copy l % R, so with R = 32 every lane of a 32-lane half owns an LDS bank — no two lanes of a half ever
// meet on an address or on a bank, however many pairs share a bin (on an attractor most pairs fall into the few top bins). A copy
// is a plain sum, so the count of a bin is the sum of its copies whatever R is. One more row, [bins][R], takes the adds of the pairs
// that do not count (j <= i, the Theiler window) and is never read.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kCorrTile) k_corr_pairs(const CorrPairsArgs a, uint32_t first_cell, uint32_t first_set) {
    extern __shared__ __attribute__((aligned(16))) unsigned char corr_lds[];
    __shared__ double tj[3][kCorrTile + 2];  // (the loop reads one point ahead: entry kCorrTile is read and never used)

    const uint32_t tid = threadIdx.x, set = first_set + blockIdx.y;
    uint32_t I, J;
    corr_fold_pair(a.fold_m, first_cell + blockIdx.x, I, J);
    if (J >= a.nt) return;  // (the whole workgroup; I <= J)
    if (a.state && __hip_atomic_load(&a.state[set].fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != kCorrNoFail) return;

    corr_lds_u32* const hist = (corr_lds_u32*)corr_lds;
    const uint32_t bins = a.bin.bins, rep = a.rep_shift, words = (bins + 1u) << rep;  // row `bins` takes the pairs that do not count
    for (uint32_t k = tid; k < words; k += kCorrTile) hist[k] = 0u;

    const uint32_t n = a.n;
    const double* const px = a.points + (size_t)set * 3u * n;
    const double* const py = px + n;
    const double* const pz = py + n;
    const uint32_t i = I * kCorrTile + tid, j0 = J * kCorrTile, jt = j0 + tid;
    double xi = 0., yi = 0., zi = 0.;
    uint32_t skip_hi = 0xffffffffu;  // pair (i, j) counts for j > skip_hi: past i itself and past the Theiler window of i's trajectory
    if (i < n) {
        xi = px[i];
        yi = py[i];
        zi = pz[i];
        const uint32_t last = (i / a.samples + 1u) * a.samples - 1u, reach = i + a.theiler;  // (theiler <= n <= 2^20: no wrap)
        skip_hi = reach < last ? reach : last;
    }
    const bool have = jt < n;
    tj[0][tid] = have ? px[jt] : 0.;
    tj[1][tid] = have ? py[jt] : 0.;
    tj[2][tid] = have ? pz[jt] : 0.;
    __syncthreads();

    const uint32_t jn = n - j0 < kCorrTile ? n - j0 : kCorrTile;
    const uint32_t copy = tid & ((1u << rep) - 1u);
    const CorrBinning bin = a.bin;
    double xn = tj[0][0], yn = tj[1][0], zn = tj[2][0];
    for (uint32_t jj = 0; jj < jn; ++jj) {
        const double dx = xn - xi, dy = yn - yi, dz = zn - zi;
        xn = tj[0][jj + 1u];  // the next j point is on its way while this one is binned
        yn = tj[1][jj + 1u];
        zn = tj[2][jj + 1u];
        const double r2 = (dx * dx + dy * dy) + dz * dz;
        // (no branch: a skipped pair adds to the lane's own word of the spare row, so that the loads and the arithmetic of
        // successive j overlap instead of each waiting behind an exec-mask test)
        uint32_t hi = (uint32_t)__double2hiint(r2);
        asm volatile("" : "+v"(hi));  // (r2 is computed for every pair: the compiler would put it behind the test otherwise)
        const uint32_t b = j0 + jj > skip_hi ? corr_bin_hi(bin, hi) : bins;
        __hip_atomic_fetch_add(hist + ((b << rep) + copy), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();

    // one 64-bit atomic per non-empty bin; a lane starts at its own copy so that the lanes of a wave read different banks
    unsigned long long* const out = a.hist + (size_t)set * bins;
    for (uint32_t b = tid; b < bins; b += kCorrTile) {
        uint32_t sum = 0;
        for (uint32_t k = 0; k < (1u << rep); ++k) sum += hist[(b << rep) + ((k + tid) & ((1u << rep) - 1u))];
        if (sum) atomicAdd(out + b, (unsigned long long)sum);
    }
}

void launch_corr_orbit(const CorrOrbitArgs& a, uint32_t n_maps, hipStream_t s) {
    hipLaunchKernelGGL(k_corr_orbit, dim3((a.jobs + 255u) / 256u, n_maps), dim3(256), 0, s, a);
}

int launch_corr_pairs(const CorrPairsArgs& a, uint32_t first_cell, uint32_t n_cells, uint32_t first_set, uint32_t n_sets, hipStream_t s) {
    // (per device and function; cheap next to a launch of whole tile pairs)
    const hipError_t e = hipFuncSetAttribute((const void*)k_corr_pairs, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kCorrHistLdsBytes);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_corr_pairs, dim3(n_cells, n_sets), dim3(kCorrTile), ((a.bin.bins + 1u) << a.rep_shift) * 4u, s, a, first_cell, first_set);
    return 0;
}

}  // namespace sar
