// sar_orbit.hip — gfx950 (MI355X) kernel of the orbit diagrams (include/sar.h: sar_runtime_orbit): k_orbit takes ONE column — one map
// of the family — from its start points to its histogram in ONE workgroup, a trajectory per lane. The column's 30 coefficients are
// wave-uniform: the workgroup reads its block with scalar loads, the x and y rows stay scalar operands and the z row is pinned into
// VGPRs (pin_z_row, sar_tangent.hpp). The histogram is `height` u32 words of dynamic LDS and every hit one LDS add; nothing is scattered
// to device memory. Only multiplies, adds and compares: no division, square root or logarithm, so the build's fused-op audit pins
// this kernel at 0 and a host restatement gives the same counts bit for bit. DESIGN.md section 15 has the LDS budget and resources.
#include "sar_orbit.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

typedef uint32_t __attribute__((may_alias)) lds_u32;

enum : uint32_t { OR_DEAD_T = 0, OR_DEAD_L = 1, OR_ALIVE = 2, OR_OCCUPIED = 3, OR_MAX = 4, OR_COUNT = 5 };
constexpr uint32_t kOrbitWaves = kMaxOrbitJobs / 64u;

__global__ void __launch_bounds__(kMaxOrbitJobs) k_orbit(const OrbitArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char o_lds[];
    __shared__ uint32_t s_u32[kOrbitWaves][OR_COUNT];
    __shared__ unsigned long long s_u64[kOrbitWaves][2];  // hits, misses
    __shared__ double s_f64[kOrbitWaves][2];              // vmin, vmax

    const uint32_t tid = threadIdx.x, col = a.first_col + blockIdx.x, height = a.height;
    if (col >= a.width) return;  // (the whole workgroup: the host launches no such column)
    const SearchCoeffs c = pin_z_row(load_frame_args(a.cols + col));

    lds_u32* const hist = (lds_u32*)o_lds;
    for (uint32_t r = tid; r < height; r += blockDim.x) hist[r] = 0u;
    __syncthreads();

    // the lanes beyond `jobs` (the block is whole waves) step some point with the others; they are never alive
    const bool valid = tid < a.jobs;
    double x = 0., y = 0., z = 0.;
    if (valid) {
        x = a.starts[3u * tid];
        y = a.starts[3u * tid + 1u];
        z = a.starts[3u * tid + 2u];
    }
    const double bound = a.bound;

    // the transient: a lane is dead once its point leaves the bound box; a wave stops once its lanes all have
    bool alive = valid;
    for (CheckedSteps run(a.transient); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            alive = alive & within(x, y, z, bound);
        }
    const bool survived = alive;

    // the counted steps: advance, test the box, then the visit
    const double p0 = a.proj[0], p1 = a.proj[1], p2 = a.proj[2], v_lo = a.v_lo, scale = a.scale, hf = (double)height;
    const uint32_t top = height - 1u;
    uint32_t hits = 0, misses = 0;  // per lane: at most `steps` <= 2^31
    double vmin = __builtin_inf(), vmax = -__builtin_inf();
    for (CheckedSteps run(a.steps); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            alive = alive & within(x, y, z, bound);
            const double v = (p0 * x + p1 * y) + p2 * z;
            const double u = (v - v_lo) * scale;
            const bool hit = alive & (u >= 0.) & (u < hf);
            vmin = (alive & (v < vmin)) ? v : vmin;
            vmax = (alive & (v > vmax)) ? v : vmax;
            if (hit) {  // 0 <= u < height: the bin is in range
                __hip_atomic_fetch_add(hist + (top - (uint32_t)u), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                ++hits;
            }
            misses += (alive & !hit) ? 1u : 0u;
        }
    __syncthreads();

    // ---- the tail: every row of the column (zeros included: the diagram needs no memset), and the column's scalars ---------------
    uint32_t occupied = 0, m = 0;
    for (uint32_t r = tid; r < height; r += blockDim.x) {
        const uint32_t n = hist[r];
        a.count[(size_t)r * a.width + col] = n;
        occupied += n ? 1u : 0u;
        m = n > m ? n : m;
    }
    uint32_t dead_t = (valid & !survived) ? 1u : 0u, dead_l = (survived & !alive) ? 1u : 0u, live = alive ? 1u : 0u;
    unsigned long long h64 = hits, m64 = misses;
    for (int off = 32; off > 0; off >>= 1) {
        const uint32_t om = __shfl_down(m, off);
        const double on = __shfl_down(vmin, off), ox = __shfl_down(vmax, off);
        m = om > m ? om : m;
        vmin = on < vmin ? on : vmin;
        vmax = ox > vmax ? ox : vmax;
        occupied += __shfl_down(occupied, off);
        dead_t += __shfl_down(dead_t, off);
        dead_l += __shfl_down(dead_l, off);
        live += __shfl_down(live, off);
        h64 += __shfl_down(h64, off);
        m64 += __shfl_down(m64, off);
    }
    const uint32_t wave = tid >> 6;
    if ((tid & 63u) == 0u) {
        s_u32[wave][OR_DEAD_T] = dead_t;
        s_u32[wave][OR_DEAD_L] = dead_l;
        s_u32[wave][OR_ALIVE] = live;
        s_u32[wave][OR_OCCUPIED] = occupied;
        s_u32[wave][OR_MAX] = m;
        s_u64[wave][0] = h64;
        s_u64[wave][1] = m64;
        s_f64[wave][0] = vmin;
        s_f64[wave][1] = vmax;
    }
    __syncthreads();
    if (tid == 0) {
        sar_orbit_column st;
        st.dead_transient = st.dead_late = st.alive = st.occupied = st.max = st._pad = 0u;
        st.hits = st.misses = 0ull;
        st.vmin = __builtin_inf();
        st.vmax = -__builtin_inf();
        for (uint32_t w = 0; w < (blockDim.x >> 6); ++w) {
            st.dead_transient += s_u32[w][OR_DEAD_T];
            st.dead_late += s_u32[w][OR_DEAD_L];
            st.alive += s_u32[w][OR_ALIVE];
            st.occupied += s_u32[w][OR_OCCUPIED];
            st.max = s_u32[w][OR_MAX] > st.max ? s_u32[w][OR_MAX] : st.max;
            st.hits += s_u64[w][0];
            st.misses += s_u64[w][1];
            st.vmin = s_f64[w][0] < st.vmin ? s_f64[w][0] : st.vmin;
            st.vmax = s_f64[w][1] > st.vmax ? s_f64[w][1] : st.vmax;
        }
        a.stats[col] = st;
        if (st.max) raise_scalar(a.max, st.max);  // one atomic per column at most
    }
}

int launch_orbit(const OrbitArgs& a, uint32_t n_cols, hipStream_t s) {
    // (per device and function; cheap next to a launch of whole columns)
    const hipError_t e = hipFuncSetAttribute((const void*)k_orbit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(kMaxOrbitHeight * 4u));
    if (e != hipSuccess) return (int)e;
    const uint32_t block = (a.jobs + 63u) / 64u * 64u;  // the column's jobs, rounded up to whole waves
    hipLaunchKernelGGL(k_orbit, dim3(n_cols), dim3(block), a.height * 4u, s, a);  // 4 B per bin, not a fixed size: short diagrams
    return 0;                                                                      // put several columns on a CU
}

}  // namespace sar
