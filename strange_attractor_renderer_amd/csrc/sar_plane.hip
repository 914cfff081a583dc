// sar_plane.hip — gfx950 kernels of the Lyapunov planes (sar_runtime_plane, include/sar.h): one lane per pixel.
//
// k_plane<K> fuses the search's two phases for one map per lane: the transient with the bound test, then the tangent phase
// k_search_lyapunov runs (sar_tangent.hpp) over the first K columns of the tangent frame (K = 3: the search's; K = 1: its first
// column). A wave covers an 8 x 8 tile of the plane, not a row segment: neighbouring pixels tend to share their fate, so the lanes of
// a wave tend to finish together, and the wave stops once they all have (CheckedSteps). The coefficients are
// built once per lane from the plane's base and the two swept values (plane_pick: unrolled selects, no runtime-indexed array) and
// then live in VGPRs as the search's do. Only multiply, add, divide, sqrt and frexp: the raw fields are bit-identical to a host
// restatement (the build's fused-op audit pins the sqrt / divide expansions).
//
// k_plane_colorize turns the records still on the device into RGBA16 (include/sar.h: sar_plane_colors).
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

template <int K>
__global__ void __launch_bounds__(256) k_plane(const PlaneArgs a) {
    const TilePixel tp = tile_pixel(a.first_tile, a.n_tiles, a.tiles_x, a.width, a.height);
    const uint32_t px = tp.px, py = tp.py;
    const bool valid = tp.valid;
    // the lanes of a partial tile build some map and step it with the others; they are never active and write nothing
    const double v0 = plane_sweep(a.lo[0], a.span[0], px, a.width);
    const double v1 = plane_sweep(a.lo[1], a.span[1], a.height - 1u - py, a.height);
    SearchCoeffs c;
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        c.cx[k] = plane_pick(a, k, v0, v1);
        c.cy[k] = plane_pick(a, 10 + k, v0, v1);
        c.cz[k] = plane_pick(a, 20 + k, v0, v1);
    }
    double x = a.start[0], y = a.start[1], z = a.start[2];
    const double bound = a.bound;
    // the transient: a lane is dead once its point leaves the bound box (transient_done: that step)
    bool alive = valid;
    uint32_t tdone = a.transient;
    for (CheckedSteps run(a.transient); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool in = within(x, y, z, bound);
            tdone = alive && !in ? t + 1u : tdone;
            alive = alive & in;
        }
    // the tangent phase, for the survivors
    double q[K][3], m[K];
    long long e[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        q[k][0] = k == 0 ? 1. : 0.;
        q[k][1] = k == 1 ? 1. : 0.;
        q[k][2] = k == 2 ? 1. : 0.;
        m[k] = 1.;
        e[k] = 0;
    }
    int status = alive ? SAR_SEARCH_BOUNDED : SAR_SEARCH_DIVERGED;
    uint32_t done = alive ? a.steps : 0u;
    bool active = alive;
    for (CheckedSteps run(a.steps); run.next(active);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            if (!active) continue;
            TangentStep<K> s;
            tangent_eval<K>(c, bound, x, y, z, q, s);
            if (s.status != SAR_SEARCH_BOUNDED) {
                status = s.status;
                done = t + 1u;
                active = false;
                continue;
            }
            tangent_fold<K>(s, x, y, z, m, e);
            tangent_take<K>(s, q);
        }
    if (!valid) return;
    sar_plane_record* r = a.records + ((size_t)py * a.width + px);
    r->status = status;
    r->transient_done = tdone;
    r->steps_done = done;
    r->_pad = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {  // (L1: columns 2 and 3 hold E = 0, M = 1)
        r->log2_exp[k] = 0;
        r->mant[k] = 1.;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        r->log2_exp[k] = e[k];
        r->mant[k] = m[k];
    }
}

// lambda_1 of a record with `folded` steps, from its raw fields (the host finish's expression; the device's log)
template <int K>
__device__ __forceinline__ double plane_lambda1(const sar_plane_record& r, uint32_t folded) {
    double l = ((double)r.log2_exp[0] * 0.6931471805599453 + log(r.mant[0])) / folded;
#pragma unroll
    for (int k = 1; k < K; ++k) {
        const double lk = ((double)r.log2_exp[k] * 0.6931471805599453 + log(r.mant[k])) / folded;
        l = lk > l ? lk : l;
    }
    return l;
}

template <int K>
__global__ void __launch_bounds__(256) k_plane_colorize(const sar_plane_record* rec, uint32_t npix, const PaletteParams pal,
                                                        double threshold, double chaos_scale, double order_scale, ushort4* out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const sar_plane_record& r = rec[p];
    ushort4 o;
    o.x = o.y = o.z = 0;
    o.w = 65535;
    if (r.status == SAR_SEARCH_DIVERGED) {
        o.w = 0;
    } else if (r.status == SAR_SEARCH_BOUNDED && r.steps_done != 0u) {
        const double l1 = plane_lambda1<K>(r, r.steps_done);
        if (l1 >= threshold) {
            double red, green, blue;  // the palette at (lambda_1 - threshold) / chaos_scale
            palette_blend((l1 - threshold) / chaos_scale, &pal.rgb[0][0], pal.len, red, green, blue);
            o.x = as_u16(red * 65535.);
            o.y = as_u16(green * 65535.);
            o.z = as_u16(blue * 65535.);
        } else {
            const double f = 1. - (threshold - l1) / order_scale;
            const double g = 0.5 * (f > 0. ? f : 0.);
            o.x = o.y = o.z = as_u16(g * 65535.);
        }
    }
    out[p] = o;
}

void launch_plane(const PlaneArgs& a, int k, hipStream_t s) {
    const dim3 grid((a.n_tiles + 3u) / 4u);  // four waves per workgroup, a tile each
    if (k == SAR_PLANE_SPECTRUM) hipLaunchKernelGGL(k_plane<3>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_plane<1>, grid, dim3(256), 0, s, a);
}

void launch_plane_colorize(const sar_plane_record* rec, uint32_t npix, int k, const PaletteParams& pal, double threshold,
                           double chaos_scale, double order_scale, void* rgba16_out, hipStream_t s) {
    const dim3 grid((npix + 255u) / 256u);
    if (k == SAR_PLANE_SPECTRUM)
        hipLaunchKernelGGL(k_plane_colorize<3>, grid, dim3(256), 0, s, rec, npix, pal, threshold, chaos_scale, order_scale, (ushort4*)rgba16_out);
    else
        hipLaunchKernelGGL(k_plane_colorize<1>, grid, dim3(256), 0, s, rec, npix, pal, threshold, chaos_scale, order_scale, (ushort4*)rgba16_out);
}

}  // namespace sar
