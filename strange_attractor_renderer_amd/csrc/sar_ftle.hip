// sar_ftle.hip — gfx950 (MI355X) kernels of the FTLE maps (include/sar.h: sar_runtime_ftle, sar_runtime_ftle_colorize).
//
// k_ftle_flow carries every pixel of a launch through N steps of the map — one lane per start point, a wave per 8 x 8 tile as in
// k_basin_screen, because neighbours share their fate — and writes its fate and its end point; k_ftle_gram, ONE launch over the whole
// picture behind every band of the first, takes the differences between the end points of a pixel's four neighbours and writes their
// Gram entries and the flags. The two passes are not fused: a tile's neighbours live in other waves and in other launches, and the
// kernel boundary is what makes their stores visible across the XCDs. All lanes step ONE map: its 30 coefficients are kernel
// arguments, the x and y rows scalar operands and the z row pinned into VGPRs (pin_z_row, sar_tangent.hpp). Both kernels are
// multiplies, adds, subtractions and compares: no division, square root or logarithm, so the build's fused-op audit pins them at 0
// and a host restatement gives the same records bit for bit. k_ftle_colorize has one logarithm, two divisions and three square roots.
// DESIGN.md section 24 has the argument for finite differences and the resources.
#include "sar_ftle.hpp"
#include "sar_tangent.hpp"

#pragma STDC FP_CONTRACT OFF
#pragma clang fp contract(off)

namespace sar {

// ---------------------------------------------------------------------------------------------------
// k_ftle_flow — `steps` steps from the pixel's start point (the basins': basin_start over the tables tu[], tv[]); a lane is dead once
// its point leaves the bound box (escape_step: that step, 1-based), and a wave whose lanes are all dead stops (CheckedSteps). A dead
// lane steps on with the others, so its point is no property of the pixel: a DIVERGED record's end is 0. The lanes of a partial tile
// step some point with the others; they are never alive and write nothing.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ftle_flow(const FtleArgs a) {
    const TilePixel tp = tile_pixel(a.first_tile, a.n_tiles, a.tiles_x, a.width, a.height);
    const uint32_t px = tp.px, py = tp.py;
    const bool valid = tp.valid;
    const SearchCoeffs c = pin_z_row(a.map);
    const double tu = a.tu[px < a.width ? px : a.width - 1u], tv = a.tv[py < a.height ? py : a.height - 1u];  // (in bounds for every lane)
    double x = basin_start(a.origin[0], a.du[0], a.dv[0], tu, tv);
    double y = basin_start(a.origin[1], a.du[1], a.dv[1], tu, tv);
    double z = basin_start(a.origin[2], a.du[2], a.dv[2], tu, tv);
    const double bound = a.bound;
    bool alive = valid;
    uint32_t esc = 0;
    for (CheckedSteps run(a.steps); run.next(alive);)
        for (uint32_t t = run.t0; t < run.t1; ++t) {
            next_point(c, x, y, z);
            const bool in = within(x, y, z, bound);
            esc = (alive & !in) ? t + 1u : esc;  // (steps <= 2^31)
            alive = alive & in;
        }
    if (!valid) return;
    sar_ftle_pixel* r = a.pixels + ((size_t)py * a.width + px);  // (valid: px < width and py < height)
    r->status = alive ? SAR_SEARCH_BOUNDED : SAR_SEARCH_DIVERGED;
    r->escape_step = esc;
    r->end[0] = alive ? x : 0.;
    r->end[1] = alive ? y : 0.;
    r->end[2] = alive ? z : 0.;
}

// The difference d of a BOUNDED pixel `self` along one axis, from its neighbour on the plus side and the one on the minus side
// (nullptr: outside the picture), and the axis' flags. A neighbour that is not usable is replaced by the pixel itself: both usable
// (e+ - e-) * 0.5, one usable e+ - e or e - e-, none e - e = +0 (e is finite: it passed the bound test).
__device__ __forceinline__ uint32_t ftle_axis(const sar_ftle_pixel& self, const sar_ftle_pixel* plus, const sar_ftle_pixel* minus,
                                              uint32_t one_sided, uint32_t none, double (&d)[3]) {
    const bool up = plus && plus->status == SAR_SEARCH_BOUNDED, um = minus && minus->status == SAR_SEARCH_BOUNDED;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double e = self.end[k];
        const double hi = up ? plus->end[k] : e, lo = um ? minus->end[k] : e;
        const double diff = hi - lo;
        d[k] = (up & um) ? diff * 0.5 : diff;
    }
    uint32_t flags = ((plus && !up) || (minus && !um)) ? SAR_FTLE_EDGE : 0u;
    flags |= (up != um) ? one_sided : 0u;
    flags |= (!up & !um) ? none : 0u;
    return flags;
}

// ---------------------------------------------------------------------------------------------------
// k_ftle_gram — behind the kernel boundary every band's records are visible. Lane p reads pixel p's record and, for a BOUNDED pixel,
// its four neighbours' status and end points, and writes flags, g11, g12 and g22 (zero for a DIVERGED pixel). It reads only the
// fields k_ftle_flow wrote and writes only its own: no lane reads what another lane of this launch writes.
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ftle_gram(const FtleArgs a) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= a.width * a.height) return;  // (width * height <= 2^24)
    const uint32_t y = p / a.width, x = p - y * a.width;
    sar_ftle_pixel* r = a.pixels + p;
    uint32_t flags = 0;
    double g11 = 0., g12 = 0., g22 = 0.;
    if (r->status == SAR_SEARCH_BOUNDED) {
        double u[3], v[3];
        flags = ftle_axis(*r, x + 1u < a.width ? r + 1 : nullptr, x > 0u ? r - 1 : nullptr, SAR_FTLE_ONE_SIDED_U, SAR_FTLE_NO_U, u);
        flags |= ftle_axis(*r, y > 0u ? r - a.width : nullptr, y + 1u < a.height ? r + a.width : nullptr, SAR_FTLE_ONE_SIDED_V, SAR_FTLE_NO_V, v);
        g11 = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
        g12 = (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2];
        g22 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    }
    r->flags = flags;
    r->_pad = 0;
    r->g11 = g11;
    r->g12 = g12;
    r->g22 = g22;
}

// ---------------------------------------------------------------------------------------------------
// k_ftle_colorize — include/sar.h: sar_ftle_colors. stretch2[] is the host finish's, uploaded behind the call; ftle is taken from it
// here with the device's log. One division serves both kinds of pixel: e / (e + fade) of an escaped one (k_basin_colorize's grey),
// (ftle - lo) / span of a bounded one, the palette's position (palette_blend).
// ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_ftle_colorize(const sar_ftle_pixel* pixels, const double* stretch2, uint32_t npix,
                                                       const PaletteParams pal, double two_n, double lo, double span, double fade,
                                                       ushort4* out) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const bool escaped = pixels[p].status != SAR_SEARCH_BOUNDED;
    const bool edge = (pixels[p].flags & SAR_FTLE_EDGE) != 0u;
    const double e = (double)pixels[p].escape_step;
    const double f = log(stretch2[p]) / two_n;
    const bool finite = __builtin_fabs(f) < __builtin_inf();  // (false for NaN)
    const double num = escaped ? e : f - lo;
    const double den = escaped ? e + fade : span;
    const double q = num / den;
    ushort4 o;
    o.x = o.y = o.z = 0;
    o.w = 65535;
    if (escaped) {
        const double g = 0.5 * q;
        o.x = o.y = o.z = as_u16(g * 65535.);
    } else if (edge) {
        o.x = o.y = o.z = 65535;
    } else if (finite) {
        double r, g, b;
        palette_blend(q, &pal.rgb[0][0], pal.len, r, g, b);
        o.x = as_u16(r * 65535.);
        o.y = as_u16(g * 65535.);
        o.z = as_u16(b * 65535.);
    }
    out[p] = o;
}

void launch_ftle_flow(const FtleArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_ftle_flow, dim3((a.n_tiles + 3u) / 4u), dim3(256), 0, s, a);  // four waves per workgroup, a tile each
}
void launch_ftle_gram(const FtleArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(k_ftle_gram, dim3((a.width * a.height + 255u) / 256u), dim3(256), 0, s, a);
}
void launch_ftle_colorize(const sar_ftle_pixel* pixels, const double* stretch2, uint32_t npix, const PaletteParams& pal, double two_n,
                          double lo, double span, double fade, void* rgba16_out, hipStream_t s) {
    hipLaunchKernelGGL(k_ftle_colorize, dim3((npix + 255u) / 256u), dim3(256), 0, s, pixels, stretch2, npix, pal, two_n, lo, span, fade,
                       (ushort4*)rgba16_out);
}

}  // namespace sar
