// sar_period.hip — gfx950 kernels of the period planes (sar_runtime_period, include/sar.h): one lane per pixel.
//
// k_period<LIST> runs a pixel's map through the planes' transient, keeps the point it ends on as the reference r, and steps on until
// the orbit first comes back to within eps of r in the max norm: that step's number is the pixel's period. A wave covers an 8 x 8
// tile of the plane as in k_plane — neighbours tend to share their period — and leaves the return loop once every lane has
// returned or left the bound box (CheckedSteps): a tile of settled pixels pays its longest period rounded up to 16 steps, only a
// chaotic one pays max_period. LIST = false builds the lane's coefficients from the plane's base and the two swept values
// (plane_sweep / plane_pick, two divisions); LIST = true loads the caller's 30 doubles. The map, the differences, the absolute
// values and the compares are multiplies, adds and selects: no LDS, no atomics, no scratch, and every field of the records,
// `residual` included, is bit-identical to a host restatement (the build's fused-op audit pins the kernels at the two divisions'
// expansions and at 0).
//
// k_period_colorize turns the records still on the device into RGBA16 (include/sar.h: sar_period_colors).
#include "sar_period.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

// (five waves per SIMD: 96 VGPRs. Left alone the allocator takes 98 for the sweep form, one allocation granule and one wave more.)
template <bool LIST>
__global__ void __launch_bounds__(256, 5) k_period(const PeriodArgs a) {
    const PlaneArgs& pl = a.plane;
    const TilePixel tp = tile_pixel(pl.first_tile, pl.n_tiles, pl.tiles_x, pl.width, pl.height);
    const uint32_t px = tp.px, py = tp.py;
    const bool valid = tp.valid;
    // the lanes of a partial tile take some map (LIST: pixel 0's, in bounds) and step it with the others; they are never alive and
    // write nothing
    SearchCoeffs c;
    if constexpr (LIST) {
        load_coeffs(a.coeffs + (valid ? (size_t)py * pl.width + px : (size_t)0) * kSearchCoeffs, c);
#pragma unroll
        for (int k = 0; k < 10; ++k) {  // -0.0 -> +0.0, as plane_pick does
            c.cx[k] = 0. + 1. * c.cx[k];
            c.cy[k] = 0. + 1. * c.cy[k];
            c.cz[k] = 0. + 1. * c.cz[k];
        }
    } else {
        const double v0 = plane_sweep(pl.lo[0], pl.span[0], px, pl.width);
        const double v1 = plane_sweep(pl.lo[1], pl.span[1], pl.height - 1u - py, pl.height);
#pragma unroll
        for (int k = 0; k < 10; ++k) {
            c.cx[k] = plane_pick(pl, k, v0, v1);
            c.cy[k] = plane_pick(pl, 10 + k, v0, v1);
            c.cz[k] = plane_pick(pl, 20 + k, v0, v1);
        }
    }
    double x = pl.start[0], y = pl.start[1], z = pl.start[2];
    const double bound = pl.bound, eps = a.eps;
    // the transient: a lane is dead once its point leaves the bound box (transient_done: that step)
    bool alive = valid;
    uint32_t tdone = pl.transient;
    for (CheckedSteps run(pl.transient); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool in = within(x, y, z, bound);
            tdone = alive && !in ? t + 1u : tdone;
            alive = alive & in;
        }
    // the return: step k = t + 1 from the reference point. A lane that has returned or left the box steps on with its wave and is
    // masked: whatever it computes from then on, NaN included, reaches neither done nor res
    const double rx = x, ry = y, rz = z;
    bool found = false;
    uint32_t done = alive ? pl.steps : 0u;  // the step a lane stopped at: its period where it has returned
    double res = __builtin_nan("");
    for (CheckedSteps run(pl.steps); run.next(alive & !found);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool live = alive & !found;
            const bool in = within(x, y, z, bound);
            const double dx = __builtin_fabs(x - rx), dy = __builtin_fabs(y - ry), dz = __builtin_fabs(z - rz);
            const double dxy = dx > dy ? dx : dy;
            const double d = dxy > dz ? dxy : dz;  // (finite for a live lane inside the box: no NaN to order)
            const bool hit = live & in & (d <= eps);
            const bool out = live & !in;
            res = hit ? d : res;
            done = (hit | out) ? t + 1u : done;
            found = found | hit;
            alive = alive & !out;
        }
    if (!valid) return;
    sar_period_record* r = a.records + ((size_t)py * pl.width + px);
    r->status = alive ? SAR_SEARCH_BOUNDED : SAR_SEARCH_DIVERGED;
    r->period = found ? done : 0u;
    r->transient_done = tdone;
    r->steps_done = done;
    r->residual = res;
}

// ---------------------------------------------------------------------------------------------------
// k_period_colorize — include/sar.h: sar_period_colors. One division, the palette's position of period p among `colours` slots, and
// the three square roots of the palette blend; no logarithm.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_period_colorize(const sar_period_record* rec, uint32_t npix, const PaletteParams pal,
                                                         uint32_t colours, ushort4* out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const int32_t status = rec[p].status;
    const uint32_t period = rec[p].period;
    ushort4 o;
    o.x = o.y = o.z = 0;
    o.w = status == SAR_SEARCH_DIVERGED ? 0 : 65535;
    if (status == SAR_SEARCH_BOUNDED && period != 0u) {
        const double q = ((double)((period - 1u) % colours) + 0.5) / (double)colours;
        double r, g, b;
        palette_blend(q, &pal.rgb[0][0], pal.len, r, g, b);
        o.x = as_u16(r * 65535.);
        o.y = as_u16(g * 65535.);
        o.z = as_u16(b * 65535.);
    }
    out[p] = o;
}

void launch_period(const PeriodArgs& a, bool list, hipStream_t s) {
    const dim3 grid((a.plane.n_tiles + 3u) / 4u);  // four waves per workgroup, a tile each
    if (list) hipLaunchKernelGGL(k_period<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_period<false>, grid, dim3(256), 0, s, a);
}

void launch_period_colorize(const sar_period_record* rec, uint32_t npix, const PaletteParams& pal, uint32_t colours, void* rgba16_out,
                            hipStream_t s) {
    hipLaunchKernelGGL(k_period_colorize, dim3((npix + 255u) / 256u), dim3(256), 0, s, rec, npix, pal, colours, (ushort4*)rgba16_out);
}

}  // namespace sar
