// sar_cycles.hip — gfx950 kernels of the cycles family (sar_runtime_cycles, include/sar.h has the contract): fixed points and periodic
// orbits of maps by Newton's method on F^p(x) - x, and the merge of what the starts find.
//
// k_cycles_newton: one lane per (map, start). A wave's 64 lanes belong to one map, so the map's 30 coefficients are wave-uniform: the
// wave reads its block with scalar loads, the x and y rows stay scalar operands and the z row is pinned into VGPRs (pin_z_row); the
// lanes beyond `jobs` of a map's last wave idle. A Newton iteration is p steps of the map carrying M <- J M, the residual, the
// adjugate of A = M - I and three divisions; the loop leaves when a ballot says no lane of the wave is still running, and a lane that
// has finished steps on with its wave, masked: nothing it computes from then on reaches x, its status or its iteration count. Passes
// 1 and 2 (minimal period and representative, then M and the residual at the representative) recompute the orbit instead of keeping
// p points, and run only where the wave holds a CONVERGED lane. Every lane writes its CycleFind to device memory.
//
// k_cycles_merge: one workgroup per map. The representatives and periods of the map's starts go into dynamic LDS with a word for
// the leader, 32 B per start, 128 KiB at 4096 starts; the leader search runs over the earlier starts, heads are resolved by following
// leaders (leader(j) <= j: the chain ends), hits are counted with LDS adds, and the orbit table is compacted in head order. Compares,
// differences and integers: no multiply, so nothing to fuse.
//
// Multiplies, adds, subtractions, three divisions and compares, contraction off: every field is bit-identical to a host restatement;
// the build's fused-op audit pins k_cycles_newton at the three divisions' expansions and k_cycles_merge at 0.
#include "sar_cycles.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

typedef uint32_t __attribute__((may_alias)) lds_u32;
typedef double __attribute__((may_alias)) lds_f64;

constexpr uint32_t kCycleNone = 0xFFFFFFFFu;

__device__ __forceinline__ double max3_abs(double a, double b, double c) {
    const double fa = __builtin_fabs(a), fb = __builtin_fabs(b), fc = __builtin_fabs(c);
    const double ab = fa > fb ? fa : fb;
    return ab > fc ? ab : fc;
}

// One step at (x, y, z) carrying the columns m[k] of the product: m <- J(x, y, z) m with tangent_eval's Jacobian rows and its
// V = J Q, then the point through next_point.
__device__ __forceinline__ void cycle_step(const SearchCoeffs& c, double& x, double& y, double& z, double (&m)[3][3]) {
    const double x2 = x + x, y2 = y + y, z2 = z + z;
    const double jxx = ((c.cx[1] + x2 * c.cx[2]) + y * c.cx[3]) + z * c.cx[4];
    const double jxy = ((x * c.cx[3] + c.cx[5]) + y2 * c.cx[6]) + z * c.cx[7];
    const double jxz = ((x * c.cx[4] + y * c.cx[7]) + c.cx[8]) + z2 * c.cx[9];
    const double jyx = ((c.cy[1] + x2 * c.cy[2]) + y * c.cy[3]) + z * c.cy[4];
    const double jyy = ((x * c.cy[3] + c.cy[5]) + y2 * c.cy[6]) + z * c.cy[7];
    const double jyz = ((x * c.cy[4] + y * c.cy[7]) + c.cy[8]) + z2 * c.cy[9];
    const double jzx = ((c.cz[1] + x2 * c.cz[2]) + y * c.cz[3]) + z * c.cz[4];
    const double jzy = ((x * c.cz[3] + c.cz[5]) + y2 * c.cz[6]) + z * c.cz[7];
    const double jzz = ((x * c.cz[4] + y * c.cz[7]) + c.cz[8]) + z2 * c.cz[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v0 = (jxx * m[k][0] + jxy * m[k][1]) + jxz * m[k][2];
        const double v1 = (jyx * m[k][0] + jyy * m[k][1]) + jyz * m[k][2];
        const double v2 = (jzx * m[k][0] + jzy * m[k][1]) + jzz * m[k][2];
        m[k][0] = v0;
        m[k][1] = v1;
        m[k][2] = v2;
    }
    next_point(c, x, y, z);
}

__device__ __forceinline__ void cycle_identity(double (&m)[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int r = 0; r < 3; ++r) m[k][r] = k == r ? 1. : 0.;
}

__global__ void __launch_bounds__(256) k_cycles_newton(const CyclesArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));
    const uint32_t waves_per_map = (a.jobs + 63u) / 64u;
    const uint32_t map = wave / waves_per_map;
    if (map >= a.n_maps) return;  // (the whole wave; the kernel has no barrier)
    const uint32_t job = (wave - map * waves_per_map) * 64u + lane;
    const bool valid = job < a.jobs;
    const SearchCoeffs c = pin_z_row(load_frame_args(a.coeffs + map));
    const uint32_t period = a.period, max_newton = a.max_newton;
    const double tol = a.tol, bound = a.bound, same = a.same;

    // the lanes beyond `jobs` take the origin and step it with the others; they never run and write nothing
    double x = 0., y = 0., z = 0.;
    if (valid) {
        x = a.starts[3u * job];
        y = a.starts[3u * job + 1u];
        z = a.starts[3u * job + 2u];
    }

    // ---- Newton: iteration n at (x, y, z) --------------------------------------------------------------------------------------
    bool running = valid;
    int32_t status = SAR_CYCLE_NOT_CONVERGED;
    uint32_t iterations = 0;
    for (uint32_t n = 0; n <= max_newton; ++n) {
        if (!wave_ballot(running)) break;
        double px = x, py = y, pz = z, m[3][3];
        cycle_identity(m);
        bool inb = true;
        for (uint32_t k = 0; k < period; ++k) {
            cycle_step(c, px, py, pz, m);
            inb = inb & within(px, py, pz, bound);
        }
        const double r0 = px - x, r1 = py - y, r2 = pz - z;
        const double res = max3_abs(r0, r1, r2);
        // A = M - I, row-major a b c / d e f / g h i (m[k][r] is row r of column k)
        const double aa = m[0][0] - 1., ab = m[1][0], ac = m[2][0];
        const double ad = m[0][1], ae = m[1][1] - 1., af = m[2][1];
        const double ag = m[0][2], ah = m[1][2], ai = m[2][2] - 1.;
        const double c00 = ae * ai - af * ah, c01 = af * ag - ad * ai, c02 = ad * ah - ae * ag;
        const double c10 = ac * ah - ab * ai, c11 = aa * ai - ac * ag, c12 = ab * ag - aa * ah;
        const double c20 = ab * af - ac * ae, c21 = ac * ad - aa * af, c22 = aa * ae - ab * ad;
        const double det = (aa * c00 + ab * c01) + ac * c02;
        const double n0 = (c00 * r0 + c10 * r1) + c20 * r2;
        const double n1 = (c01 * r0 + c11 * r1) + c21 * r2;
        const double n2 = (c02 * r0 + c12 * r1) + c22 * r2;
        const bool esc = !inb, conv = inb & (res <= tol), last = n == max_newton;
        const bool sing = (det == 0.) | !(__builtin_fabs(det) < __builtin_inf());
        const bool stop = esc | conv | last | sing;
        const int32_t code = esc ? SAR_CYCLE_ESCAPED : (conv ? SAR_CYCLE_CONVERGED : (last ? SAR_CYCLE_NOT_CONVERGED : SAR_CYCLE_SINGULAR));
        const bool ended = running & stop;
        status = ended ? code : status;
        iterations = ended ? n : iterations;
        running = running & !stop;
        const double ux = x - n0 / det, uy = y - n1 / det, uz = z - n2 / det;
        x = running ? ux : x;
        y = running ? uy : y;
        z = running ? uz : z;
    }

    // ---- passes 1 and 2, where the wave holds a CONVERGED lane; the other lanes go along masked --------------------------------
    const bool converged = valid & (status == SAR_CYCLE_CONVERGED);
    uint32_t q = period;
    double repx = x, repy = y, repz = z, residual = 0., m[3][3];
    cycle_identity(m);
    if (wave_ballot(converged)) {
        double px = x, py = y, pz = z;
        bool found = false;
        for (uint32_t k = 1; k <= period; ++k) {
            next_point(c, px, py, pz);
            const double d = max3_abs(px - x, py - y, pz - z);
            const bool hit = !found & (period % k == 0u) & (d <= same);
            q = hit ? k : q;
            found = found | hit;
            const bool less = (px < repx) | ((px == repx) & ((py < repy) | ((py == repy) & (pz < repz))));
            const bool take = !found & less & (k < period);
            repx = take ? px : repx;
            repy = take ? py : repy;
            repz = take ? pz : repz;
        }
        px = repx, py = repy, pz = repz;
        for (uint32_t k = 0; k < period; ++k) {
            if (!wave_ballot(converged & (k < q))) break;
            double nx = px, ny = py, nz = pz, nm[3][3];
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 3; ++r) nm[j][r] = m[j][r];
            cycle_step(c, nx, ny, nz, nm);
            const bool go = k < q;
            px = go ? nx : px;
            py = go ? ny : py;
            pz = go ? nz : pz;
#pragma unroll
            for (int j = 0; j < 3; ++j)
#pragma unroll
                for (int r = 0; r < 3; ++r) m[j][r] = go ? nm[j][r] : m[j][r];
        }
        residual = max3_abs(px - repx, py - repy, pz - repz);
    }

    if (!valid) return;
    CycleFind f;
    f.rep[0] = converged ? repx : 0.;
    f.rep[1] = converged ? repy : 0.;
    f.rep[2] = converged ? repz : 0.;
    f.q = converged ? q : 0u;
    f.status = status;
    f.iterations = iterations;
    f._pad = 0u;
    f.residual = converged ? residual : 0.;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int j = 0; j < 3; ++j) f.M[3 * r + j] = converged ? m[j][r] : 0.;  // row r, column j
    a.finds[(size_t)map * a.jobs + job] = f;
}

// ---------------------------------------------------------------------------------------------------
// k_cycles_merge — include/sar.h: "Merge, per map, over the starts in order".
// ---------------------------------------------------------------------------------------------------
enum : uint32_t { CM_STATUS0 = 0, CM_HEADS = 4, CM_HITS_LOST = 5, CM_ITERATIONS = 6, CM_COUNT = 8 };

__global__ void __launch_bounds__(kCycleMergeThreads) k_cycles_merge(const CyclesArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char c_lds[];
    __shared__ uint32_t s_cnt[CM_COUNT];
    __shared__ uint32_t s_chunk[kCycleMergeThreads];

    const uint32_t tid = threadIdx.x, map = blockIdx.x, jobs = a.jobs, cap = a.cap;
    const CycleFind* const f = a.finds + (size_t)map * jobs;
    lds_f64* const rx = (lds_f64*)c_lds;
    lds_f64* const ry = rx + jobs;
    lds_f64* const rz = ry + jobs;
    lds_u32* const qw = (lds_u32*)(rz + jobs);
    lds_u32* const lead = qw + jobs;
    const double merge = a.merge;

    if (tid < CM_COUNT) s_cnt[tid] = 0u;
    __syncthreads();
    for (uint32_t j = tid; j < jobs; j += kCycleMergeThreads) {
        rx[j] = f[j].rep[0];
        ry[j] = f[j].rep[1];
        rz[j] = f[j].rep[2];
        qw[j] = f[j].q;
        __hip_atomic_fetch_add(&s_cnt[CM_STATUS0 + (uint32_t)f[j].status], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&s_cnt[CM_ITERATIONS], f[j].iterations, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();

    // the leader of start j: the first CONVERGED i <= j of its period within `merge` of it (j itself at the latest)
    for (uint32_t j = tid; j < jobs; j += kCycleMergeThreads) {
        const uint32_t q = qw[j];
        uint32_t l = kCycleNone;
        if (q) {
            const double x = rx[j], y = ry[j], z = rz[j];
            l = j;
            for (uint32_t i = 0; i < j; ++i)
                if (qw[i] == q && max3_abs(rx[i] - x, ry[i] - y, rz[i] - z) <= merge) {
                    l = i;
                    break;
                }
        }
        lead[j] = l;
    }
    __syncthreads();

    // the representatives are done with: their first 8 B per start now hold the hits (a word) and the head (a word)
    lds_u32* const hits = (lds_u32*)c_lds;
    lds_u32* const head = hits + jobs;
    for (uint32_t j = tid; j < jobs; j += kCycleMergeThreads) hits[j] = 0u;
    __syncthreads();
    for (uint32_t j = tid; j < jobs; j += kCycleMergeThreads) {
        uint32_t h = lead[j];
        if (h != kCycleNone) {
            for (uint32_t l = lead[h]; l != h; l = lead[h]) h = l;  // leader(h) <= h, and a head leads itself
            __hip_atomic_fetch_add(&hits[h], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        head[j] = h;
    }
    __syncthreads();

    // heads in index order: a thread counts the heads of its run of consecutive starts, then places them behind the runs before it
    const uint32_t run = (jobs + kCycleMergeThreads - 1u) / kCycleMergeThreads;
    const uint32_t j0 = tid * run < jobs ? tid * run : jobs, j1 = j0 + run < jobs ? j0 + run : jobs;
    uint32_t mine = 0;
    for (uint32_t j = j0; j < j1; ++j) mine += head[j] == j ? 1u : 0u;
    s_chunk[tid] = mine;
    __syncthreads();
    uint32_t slot = 0;
    for (uint32_t t = 0; t < tid; ++t) slot += s_chunk[t];
    sar_cycle_orbit* const orbits = a.orbits + (size_t)map * cap;
    uint32_t lost = 0;
    for (uint32_t j = j0; j < j1; ++j) {
        if (head[j] != j) continue;
        if (slot < cap) {
            const CycleFind& g = f[j];
            sar_cycle_orbit o;
            o.rep[0] = g.rep[0];
            o.rep[1] = g.rep[1];
            o.rep[2] = g.rep[2];
            o.period = g.q;
            o.head = j;
            o.hits = hits[j];
            o.newton = g.iterations;
            o.residual = g.residual;
#pragma unroll
            for (int k = 0; k < 9; ++k) o.M[k] = g.M[k];
            orbits[slot] = o;
        } else {
            lost += hits[j];
        }
        ++slot;
    }
    if (mine) __hip_atomic_fetch_add(&s_cnt[CM_HEADS], mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (lost) __hip_atomic_fetch_add(&s_cnt[CM_HITS_LOST], lost, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();

    const uint32_t heads = s_cnt[CM_HEADS], kept = heads < cap ? heads : cap;
    for (uint32_t s = kept + tid; s < cap; s += kCycleMergeThreads) {  // the unused slots: zero
        sar_cycle_orbit o;
        o.rep[0] = o.rep[1] = o.rep[2] = o.residual = 0.;
        o.period = o.head = o.hits = o.newton = 0u;
#pragma unroll
        for (int k = 0; k < 9; ++k) o.M[k] = 0.;
        orbits[s] = o;
    }
    if (tid == 0) {
        sar_cycles_record r;
        r.converged = s_cnt[CM_STATUS0 + SAR_CYCLE_CONVERGED];
        r.escaped = s_cnt[CM_STATUS0 + SAR_CYCLE_ESCAPED];
        r.singular = s_cnt[CM_STATUS0 + SAR_CYCLE_SINGULAR];
        r.not_converged = s_cnt[CM_STATUS0 + SAR_CYCLE_NOT_CONVERGED];
        r.n_orbits = kept;
        r.orbits_lost = heads - kept;
        r.hits_lost = s_cnt[CM_HITS_LOST];
        r._pad = 0u;
        r.newton_iterations = s_cnt[CM_ITERATIONS];  // (jobs * max_newton <= 2^28)
        a.records[map] = r;
    }
}

void launch_cycles_newton(const CyclesArgs& a, hipStream_t s) {
    const uint32_t waves = a.n_maps * ((a.jobs + 63u) / 64u);  // a wave serves one map
    hipLaunchKernelGGL(k_cycles_newton, dim3((waves + 3u) / 4u), dim3(256), 0, s, a);
}

int launch_cycles_merge(const CyclesArgs& a, hipStream_t s) {
    // (per device and function; cheap next to a launch of whole maps)
    const hipError_t e = hipFuncSetAttribute((const void*)k_cycles_merge, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kMaxCycleJobs * kCycleLdsPerStart));
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(k_cycles_merge, dim3(a.n_maps), dim3(kCycleMergeThreads), a.jobs * kCycleLdsPerStart, s, a);
    return 0;
}

}  // namespace sar
