// sar_tangent.hpp — the device code behind the analysis kernels (sar_search.hip, sar_plane.hip, sar_orbit.hip, sar_corr.hip,
// sar_basin.hip, sar_period.hip, sar_cycles.hip, sar_manifold.hip, sar_ftle.hip): the coefficient block's loads, the bound test, the checked stepping loop, one step of the map carrying its tangent
// space (the planes'; k_search_lyapunov keeps its own text of the step and of the loop), the wave's survivor pack, the tile-to-pixel mapping and the extent fold. Only multiply,
// add, divide, sqrt and frexp: the raw fields the kernels write are bit-identical to a host restatement.
#pragma once

#include "sar_device.hpp"
#include "sar_search.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

// the three rows of a [30] array, per lane
__device__ __forceinline__ void load_coeffs(const double* src, SearchCoeffs& c) {
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        c.cx[k] = src[k];
        c.cy[k] = src[10 + k];
        c.cz[k] = src[20 + k];
    }
}

// A wave-uniform map (a kernel argument, or read through the constant address space): 60 SGPRs of coefficients would not fit next
// to the other arguments. The x and y rows stay scalar operands and the z row is pinned into VGPRs (pin_map_params's split).
__device__ __forceinline__ SearchCoeffs pin_z_row(SearchCoeffs c) {
#pragma unroll
    for (int k = 0; k < 10; ++k) c.cz[k] = vgpr_pin(c.cz[k]);
    return c;
}

constexpr uint32_t kSearchCheck = 16;  // steps between two tests for a wave whose lanes are all done

// The checked stepping loop: steps t = 0 .. n - 1 in runs of kSearchCheck; before each run the wave stops if none of its lanes is
// live any more. The loop's body stays in the kernel, between the braces of
//     for (CheckedSteps run(n); run.next(live);)
//         for (uint32_t t = run.t0; t < run.t1; ++t) { ... }
// and clears the flag; a lane that is not live steps on with the others, and the body masks it. (Not a function taking the body as a
// closure: that form costs k_search_screen 24 VGPRs and an occupancy class. k_search_lyapunov alone writes the loop out: it ran
// 4 % slower through this struct.)
struct CheckedSteps {
    uint32_t n, t0 = 0, t1 = 0;  // the run in hand is [t0, t1)
    __device__ __forceinline__ explicit CheckedSteps(uint32_t steps) : n(steps) {}
    __device__ __forceinline__ bool next(bool live) {
        t0 = t1;
        if (t0 >= n || !wave_ballot(live)) return false;
        t1 = n - t0 < kSearchCheck ? n : t0 + kSearchCheck;  // (n <= 2^31 and t1 <= n: the counter never wraps)
        return true;
    }
};

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

// The wave appends its `keep` lanes to a list whose length is *counter, with one atomicAdd per wave (every lane of the wave calls):
// a keep lane's slot. Which wave lands first decides the order of the list, nothing else.
__device__ __forceinline__ uint32_t wave_append(bool keep, uint32_t* counter) {
    const unsigned long long lm = wave_ballot(keep);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(lm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)lm, 0u));
    uint32_t base = 0;
    if ((threadIdx.x & 63u) == 0u && lm) base = atomicAdd(counter, (uint32_t)__popcll(lm));
    return __builtin_amdgcn_readfirstlane(base) + rank;
}

// A workgroup of four waves, a wave per 8 x 8 tile of a width x height plane (tiles row-major, tiles_x per row), over the launch's
// tiles [first_tile, first_tile + n_tiles): the lane's pixel. The lanes of a partial tile and of a tile beyond the launch are not
// valid: they step with the others and write nothing.
struct TilePixel {
    uint32_t px, py;
    bool valid;
};
__device__ __forceinline__ TilePixel tile_pixel(uint32_t first_tile, uint32_t n_tiles, uint32_t tiles_x, uint32_t width, uint32_t height) {
    const uint32_t slot_tile = blockIdx.x * 4u + (threadIdx.x >> 6), tile = first_tile + slot_tile;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t ty = tile / tiles_x, tx = tile - ty * tiles_x;
    TilePixel p;
    p.px = tx * kPlaneTile + (lane & 7u);
    p.py = ty * kPlaneTile + (lane >> 3);
    p.valid = slot_tile < n_tiles && p.px < width && p.py < height;
    return p;
}

// One coordinate's extent over the wave, on the sortable 64-bit image (unsigned order == numeric order): the fold of the lanes'
// lo / hi and one atomicMin / atomicMax per wave. A lane with nothing to report passes +inf / -inf. f64_sortable is
// corr_sortable (sar_corr.hpp) on the double's bits: the host reads these keys back with corr_unsortable.
__device__ __forceinline__ void wave_extent(double lo, double hi, unsigned long long* lo_key, unsigned long long* hi_key) {
    unsigned long long l = f64_sortable(lo), h = f64_sortable(hi);
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long ol = __shfl_down(l, off), oh = __shfl_down(h, off);
        l = ol < l ? ol : l;
        h = oh > h ? oh : h;
    }
    if ((threadIdx.x & 63u) == 0u) {
        atomicMin(lo_key, l);
        atomicMax(hi_key, h);
    }
}

}  // namespace sar
