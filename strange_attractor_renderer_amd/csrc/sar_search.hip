// sar_search.hip — gfx950 kernels of the chaotic-map search (sar_runtime_search, include/sar.h): one lane per candidate.
//
// k_search_screen runs the transient of every candidate of a chunk and packs the survivors; k_search_lyapunov carries each
// survivor's tangent space through `steps` more steps (Jacobian, modified Gram-Schmidt, exact log-free accumulation of the
// norms) and writes one record per survivor slot. The coefficients differ per lane, so they live in VGPRs (SearchCoeffs),
// not in the wave-uniform MapParams of the render kernels; the map itself is next_point, the same template the render
// kernels instantiate, so the operation order is the reference's. Only multiply, add, divide, sqrt and frexp: the records
// are bit-identical to a host restatement (the build's fused-op audit holds the screen kernel to zero v_fma_f64 and the
// Lyapunov kernel to its sqrt / divide expansions).
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

__device__ __forceinline__ void search_load_coeffs(const SearchArgs& a, uint32_t slot, SearchCoeffs& c) {
    if (a.coeffs) {
        load_coeffs(a.coeffs + (size_t)slot * kSearchCoeffs, c);
    } else {
        const uint64_t index = a.first + slot;
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            c.cx[k] = search_coeff(a.seed, a.lo, a.span, index, k);
            c.cy[k] = search_coeff(a.seed, a.lo, a.span, index, 10 + k);
            c.cz[k] = search_coeff(a.seed, a.lo, a.span, index, 20 + k);
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// k_search_screen — phase 1: `transient` steps from the common start point; a lane is dead once its point leaves the
// bound box. A wave whose lanes are all dead stops (CheckedSteps). Survivors are appended with one atomic
// per wave; their order depends on which wave lands first, the results do not (records carry the candidate index).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_search_screen(const SearchArgs a) {
    const uint32_t slot = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = slot < a.n;
    SearchCoeffs c;
    search_load_coeffs(a, valid ? slot : 0u, c);
    double x = a.start[0], y = a.start[1], z = a.start[2];
    const double bound = a.bound;
    bool alive = valid;
    for (CheckedSteps run(a.transient); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            alive = alive & within(x, y, z, bound);
        }
    const unsigned long long dm = wave_ballot(valid && !alive);
    if ((threadIdx.x & 63u) == 0u && dm) atomicAdd(&a.counters[1], (uint32_t)__popcll(dm));
    const uint32_t s = wave_append(alive, &a.counters[0]);
    if (alive) {
        a.surv_idx[s] = slot;
        a.surv_xyz[s] = x;
        a.surv_xyz[a.n + s] = y;
        a.surv_xyz[2u * a.n + s] = z;
    }
}

// ---------------------------------------------------------------------------------------------------
// k_search_lyapunov — phase 2, one lane per survivor slot: `steps` steps of the map with the tangent space Q (columns q1..q3,
// the identity at first). Per step: J at p, V = J Q, modified Gram-Schmidt, the norms folded as M *= n, (M, e) = frexp(M),
// E += e (exact: no log on the device), then p = next_point(p) and the raw bounds. The first norm that is not positive and
// finite ends the lane (DEGENERATE for zero, DIVERGED otherwise), then a point outside the bound box (DIVERGED); a failing
// step is neither folded nor bounded. The kernel keeps its own text of the stepping loop and of the tangent step: through
// CheckedSteps alone it ran 4 % slower, through the planes' TangentStep 5 % (profiles/r08_refactor_ab.txt).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_search_lyapunov(const SearchArgs a) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= a.counters[0]) return;
    const uint32_t slot = a.surv_idx[s];
    SearchCoeffs c;
    search_load_coeffs(a, slot, c);
    double x = a.surv_xyz[s], y = a.surv_xyz[a.n + s], z = a.surv_xyz[2u * a.n + s];
    const double bound = a.bound;
    double q1x = 1., q1y = 0., q1z = 0.;
    double q2x = 0., q2y = 1., q2z = 0.;
    double q3x = 0., q3y = 0., q3z = 1.;
    double m1 = 1., m2 = 1., m3 = 1.;
    long long e1 = 0, e2 = 0, e3 = 0;
    double b[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b[2 * k] = __builtin_inf();
        b[2 * k + 1] = -__builtin_inf();
    }
    int status = SAR_SEARCH_BOUNDED;
    uint32_t done = a.steps;
    bool active = true;
    for (uint32_t t0 = 0, t1; t0 < a.steps; t0 = t1) {  // (t1 <= steps: the counter never wraps)
        if (!wave_ballot(active)) break;
        t1 = a.steps - t0 < kSearchCheck ? a.steps : t0 + kSearchCheck;
        for (uint32_t t = t0; t < t1; ++t) {
            if (!active) continue;
            // the Jacobian at p, row by row (d/dx, d/dy, d/dz of the x, y, z sums)
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
            // V = J Q
            double v1x = (jxx * q1x + jxy * q1y) + jxz * q1z;
            double v1y = (jyx * q1x + jyy * q1y) + jyz * q1z;
            double v1z = (jzx * q1x + jzy * q1y) + jzz * q1z;
            double v2x = (jxx * q2x + jxy * q2y) + jxz * q2z;
            double v2y = (jyx * q2x + jyy * q2y) + jyz * q2z;
            double v2z = (jzx * q2x + jzy * q2y) + jzz * q2z;
            double v3x = (jxx * q3x + jxy * q3y) + jxz * q3z;
            double v3y = (jyx * q3x + jyy * q3y) + jyz * q3z;
            double v3z = (jzx * q3x + jzy * q3y) + jzz * q3z;
            // modified Gram-Schmidt
            const double n1 = normalise(v1x, v1y, v1z);
            reject(v1x, v1y, v1z, v2x, v2y, v2z);
            const double n2 = normalise(v2x, v2y, v2z);
            reject(v1x, v1y, v1z, v3x, v3y, v3z);
            reject(v2x, v2y, v2z, v3x, v3y, v3z);
            const double n3 = normalise(v3x, v3y, v3z);
            double nx = x, ny = y, nz = z;
            next_point(c, nx, ny, nz);
            int st = norm_status(n1);
            if (st == SAR_SEARCH_BOUNDED) st = norm_status(n2);
            if (st == SAR_SEARCH_BOUNDED) st = norm_status(n3);
            if (st == SAR_SEARCH_BOUNDED && !within(nx, ny, nz, bound)) st = SAR_SEARCH_DIVERGED;
            if (st != SAR_SEARCH_BOUNDED) {
                status = st;
                done = t + 1u;
                active = false;
                continue;
            }
            int e;
            m1 = frexp(m1 * n1, &e);
            e1 += e;
            m2 = frexp(m2 * n2, &e);
            e2 += e;
            m3 = frexp(m3 * n3, &e);
            e3 += e;
            x = nx;
            y = ny;
            z = nz;
            b[0] = x < b[0] ? x : b[0];
            b[1] = x > b[1] ? x : b[1];
            b[2] = y < b[2] ? y : b[2];
            b[3] = y > b[3] ? y : b[3];
            b[4] = z < b[4] ? z : b[4];
            b[5] = z > b[5] ? z : b[5];
            q1x = v1x; q1y = v1y; q1z = v1z;
            q2x = v2x; q2y = v2y; q2z = v2z;
            q3x = v3x; q3y = v3y; q3z = v3z;
        }
    }
    sar_search_record* r = a.records + s;
    r->candidate = a.first + slot;
    r->status = status;
    r->steps_done = done;
    r->log2_exp[0] = e1;
    r->log2_exp[1] = e2;
    r->log2_exp[2] = e3;
    r->mant[0] = m1;
    r->mant[1] = m2;
    r->mant[2] = m3;
#pragma unroll
    for (int k = 0; k < 6; ++k) r->extent[k] = b[k];
}

void launch_search_screen(const SearchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_search_screen, dim3((a.n + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_search_lyapunov(const SearchArgs& a, uint32_t survivors, hipStream_t s) {
    hipLaunchKernelGGL(k_search_lyapunov, dim3((survivors + 255u) / 256u), dim3(256), 0, s, a);
}

}  // namespace sar
