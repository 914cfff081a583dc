// sar_tangent.hpp — the device code the chaotic-map search (sar_search.hip) and the Lyapunov planes (sar_plane.hip) share:
// per-lane coefficients, the bound test and one step of the map carrying its tangent space. Only multiply, add, divide, sqrt and
// frexp: the raw fields both kernels write are bit-identical to a host restatement.
#pragma once

#include "sar_device.hpp"
#include "sar_search.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

struct SearchCoeffs {
    double cx[10], cy[10], cz[10];
};

constexpr uint32_t kSearchCheck = 16;  // steps between two tests for a wave whose lanes are all done

__device__ __forceinline__ bool within(double x, double y, double z, double bound) {
    // `&` of the three compares: no branch; NaN compares false
    return (int)(__builtin_fabs(x) <= bound) & (int)(__builtin_fabs(y) <= bound) & (int)(__builtin_fabs(z) <= bound);
}

// the status a norm gives a step: a positive finite norm passes (0), exactly zero is DEGENERATE, inf / NaN is DIVERGED
__device__ __forceinline__ int norm_status(double n) {
    return n == 0. ? SAR_SEARCH_DEGENERATE : (n < __builtin_inf() ? SAR_SEARCH_BOUNDED : SAR_SEARCH_DIVERGED);
}

// v <- v * (1 / n), n = |v| = sqrt((vx^2 + vy^2) + vz^2)
__device__ __forceinline__ double normalise(double& vx, double& vy, double& vz) {
    const double n = sqrt((vx * vx + vy * vy) + vz * vz);
    const double r = 1.0 / n;
    vx = vx * r;
    vy = vy * r;
    vz = vz * r;
    return n;
}

// v <- v - (q . v) q
__device__ __forceinline__ void reject(double qx, double qy, double qz, double& vx, double& vy, double& vz) {
    const double d = (qx * vx + qy * vy) + qz * vz;
    vx = vx - d * qx;
    vy = vy - d * qy;
    vz = vz - d * qz;
}

// One step of the map at p = (x, y, z) with the first K columns of the tangent frame Q (K = 3: the whole space; K = 1: q1
// alone, which is the first column of K = 3 to the bit), in two halves. tangent_eval: J at p, V = J Q, modified Gram-Schmidt of
// V's columns in the order 1..K, p' = next_point(p), and the step's status — that of the first norm that is not positive and
// finite (DEGENERATE for zero, DIVERGED otherwise), then DIVERGED for a p' outside the bound box. tangent_fold, for a BOUNDED step
// only: M_k *= n_k, (M_k, e) = frexp(M_k), E_k += e, p = p'; the caller then takes V as the new Q. A failing step changes nothing.
template <int K>
struct TangentStep {
    double v[K][3];
    double n[K];
    double nx, ny, nz;
    int status;
};

template <int K>
__device__ __forceinline__ void tangent_eval(const SearchCoeffs& c, double bound, double x, double y, double z, const double (&q)[K][3],
                                             TangentStep<K>& s) {
    static_assert(K == 1 || K == 3, "the frame is q1 or the whole space");
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
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s.v[k][0] = (jxx * q[k][0] + jxy * q[k][1]) + jxz * q[k][2];
        s.v[k][1] = (jyx * q[k][0] + jyy * q[k][1]) + jyz * q[k][2];
        s.v[k][2] = (jzx * q[k][0] + jzy * q[k][1]) + jzz * q[k][2];
    }
    // modified Gram-Schmidt
    s.n[0] = normalise(s.v[0][0], s.v[0][1], s.v[0][2]);
    if constexpr (K == 3) {
        reject(s.v[0][0], s.v[0][1], s.v[0][2], s.v[1][0], s.v[1][1], s.v[1][2]);
        s.n[1] = normalise(s.v[1][0], s.v[1][1], s.v[1][2]);
        reject(s.v[0][0], s.v[0][1], s.v[0][2], s.v[2][0], s.v[2][1], s.v[2][2]);
        reject(s.v[1][0], s.v[1][1], s.v[1][2], s.v[2][0], s.v[2][1], s.v[2][2]);
        s.n[2] = normalise(s.v[2][0], s.v[2][1], s.v[2][2]);
    }
    s.nx = x;
    s.ny = y;
    s.nz = z;
    next_point(c, s.nx, s.ny, s.nz);
    int st = norm_status(s.n[0]);
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (st == SAR_SEARCH_BOUNDED) st = norm_status(s.n[k]);
    if (st == SAR_SEARCH_BOUNDED && !within(s.nx, s.ny, s.nz, bound)) st = SAR_SEARCH_DIVERGED;
    s.status = st;
}

template <int K>
__device__ __forceinline__ void tangent_fold(const TangentStep<K>& s, double& x, double& y, double& z, double (&m)[K], long long (&e)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        int ek;
        m[k] = frexp(m[k] * s.n[k], &ek);
        e[k] += ek;
    }
    x = s.nx;
    y = s.ny;
    z = s.nz;
}

template <int K>
__device__ __forceinline__ void tangent_take(const TangentStep<K>& s, double (&q)[K][3]) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        q[k][0] = s.v[k][0];
        q[k][1] = s.v[k][1];
        q[k][2] = s.v[k][2];
    }
}

}  // namespace sar
