// sar_ftle.cpp — the host half of the FTLE maps (include/sar.h: sar_ftle_*, sar_runtime_ftle, sar_runtime_ftle_colorize): the
// checks, the plane's two parameter tables, the chunked launches of k_ftle_flow and the one launch of k_ftle_gram (sar_ftle.hip), and
// — one loop over the pixels — the finish of every record (stretch2, ftle) and the statistics.
//
// Built with -ffp-contract=off: sar_ftle_start must produce the doubles the kernels start from, and the finish is held bit for bit
// by a restatement.
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_ftle.hpp"

using namespace sar;

namespace {

// The plane's metric: the Gram entries of its steps per pixel hu = du / (width - 1), hv = dv / (height - 1) (an axis of one pixel
// has none: its entries stay 0 and are never read), and A = det M.
struct FtleMetric {
    double m11 = 0., m12 = 0., m22 = 0., A = 0.;
};

FtleMetric ftle_metric(const sar_ftle_params* p) {
    double hu[3] = {0., 0., 0.}, hv[3] = {0., 0., 0.};
    for (int k = 0; k < 3; ++k) {
        if (p->width > 1u) hu[k] = p->du[k] / static_cast<double>(p->width - 1u);
        if (p->height > 1u) hv[k] = p->dv[k] / static_cast<double>(p->height - 1u);
    }
    FtleMetric m;
    m.m11 = (hu[0] * hu[0] + hu[1] * hu[1]) + hu[2] * hu[2];
    m.m12 = (hu[0] * hv[0] + hu[1] * hv[1]) + hu[2] * hv[2];
    m.m22 = (hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2];
    m.A = m.m11 * m.m22 - m.m12 * m.m12;
    return m;
}

int check_ftle(const sar_ftle_params* p, const char* where) {
    if (!p) { set_error("%s: the FTLE parameters are NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_plane_size(where, p->width, p->height));
    SAR_TRY(check_steps(where, 0, p->steps));
    if (!p->steps) { set_error("%s: steps must be 1 to 2^31 (0)", where); return SAR_ERR_INVALID; }
    if (p->chunk > kMaxFtleChunk) { set_error("%s: chunk must be at most 2^30 pixels (%u)", where, p->chunk); return SAR_ERR_INVALID; }
    for (uint32_t k = 0; k < kSearchCoeffs; ++k)
        if (!std::isfinite(p->coeffs[k])) {
            set_error("%s: the map's coefficients must be finite (entry %u)", where, k);
            return SAR_ERR_INVALID;
        }
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k]) || !std::isfinite(p->du[k]) || !std::isfinite(p->dv[k])) {
            set_error("%s: the plane's origin, du and dv must be finite", where);
            return SAR_ERR_INVALID;
        }
    SAR_TRY(check_bound(where, p->bound));
    const FtleMetric m = ftle_metric(p);
    if (p->width > 1u && m.m11 == 0.) { set_error("%s: du is zero (or its square underflows) over %u columns", where, p->width); return SAR_ERR_INVALID; }
    if (p->height > 1u && m.m22 == 0.) { set_error("%s: dv is zero (or its square underflows) over %u rows", where, p->height); return SAR_ERR_INVALID; }
    if (p->width > 1u && p->height > 1u && !(m.A > 0. && std::isfinite(m.A))) {
        set_error("%s: du and dv must span a plane (the determinant of their Gram matrix is not positive and finite)", where);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

// include/sar.h's host finish of one record, in its order of operations
void ftle_finish(sar_ftle_pixel& r, const FtleMetric& m, double two_n) {
    const bool no_u = (r.flags & SAR_FTLE_NO_U) != 0u, no_v = (r.flags & SAR_FTLE_NO_V) != 0u;
    double s = std::numeric_limits<double>::quiet_NaN();
    if (r.status == SAR_SEARCH_BOUNDED && !no_u && !no_v) {
        const double B = (r.g11 * m.m22 + r.g22 * m.m11) - 2. * (r.g12 * m.m12);
        const double C = r.g11 * r.g22 - r.g12 * r.g12;
        double disc = B * B - 4. * (m.A * C);
        disc = disc > 0. ? disc : 0.;  // (a NaN too)
        s = (B + std::sqrt(disc)) / (2. * m.A);
    } else if (r.status == SAR_SEARCH_BOUNDED && !no_u) {
        s = r.g11 / m.m11;
    } else if (r.status == SAR_SEARCH_BOUNDED && !no_v) {
        s = r.g22 / m.m22;
    }
    r.stretch2 = s;
    r.ftle = std::log(s) / two_n;
}

}  // namespace

extern "C" {

int sar_ftle_params_default(sar_ftle_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->origin[0] = out->origin[1] = -1.;
    out->du[0] = 2.;
    out->dv[1] = 2.;
    out->width = out->height = 256;
    out->steps = 16;
    out->bound = 1e6;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_ftle_start(const sar_ftle_params* p, uint32_t x, uint32_t y, double out3[3]) try {
    SAR_TRY(check_ftle(p, "sar_ftle_start"));
    if (!out3 || x >= p->width || y >= p->height) return SAR_ERR_INVALID;
    const double tu = basin_param(x, p->width), tv = basin_param(p->height - 1u - y, p->height);
    for (int k = 0; k < 3; ++k) out3[k] = basin_start(p->origin[k], p->du[k], p->dv[k], tu, tv);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_ftle(sar_runtime* rt, const sar_ftle_params* p, sar_ftle_pixel* pixels_out_host, sar_ftle_stats* stats_out) try {
    SAR_TRY(check_ftle(p, "sar_runtime_ftle"));  // (no device needed to refuse the parameters)
    if (!rt || !pixels_out_host) { set_error("sar_runtime_ftle: the runtime or the pixel buffer is NULL"); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_ftle_flow, resolve_ms = k_ftle_gram (sar_timing)
    rt->ftle.width = rt->ftle.height = 0;  // no FTLE map until this one is whole
    const uint32_t width = p->width, height = p->height, npix = width * height;
    const TileBands bands = tile_bands(width, height, p->chunk ? p->chunk : kDefaultFtleChunk);

    // the plane's parameters, one division per column and per row (basin_param)
    std::vector<double> t(static_cast<size_t>(width) + height);
    for (uint32_t x = 0; x < width; ++x) t[x] = basin_param(x, width);
    for (uint32_t y = 0; y < height; ++y) t[width + y] = basin_param(height - 1u - y, height);
    HIP_TRY(rt->ftle.d_t.grow(nullptr, t.size()));
    HIP_TRY(rt->ftle.d_pix.grow(nullptr, npix));
    HIP_TRY(rt->ftle.d_stretch2.grow(nullptr, npix));
    HIP_TRY(hipMemcpyAsync(rt->ftle.d_t, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream));

    FtleArgs a;
    std::memset(&a, 0, sizeof(a));
    canonical_coeffs(p->coeffs, 10, a.map.cx);
    canonical_coeffs(p->coeffs + 10, 10, a.map.cy);
    canonical_coeffs(p->coeffs + 20, 10, a.map.cz);
    for (int k = 0; k < 3; ++k) {
        a.origin[k] = p->origin[k];
        a.du[k] = p->du[k];
        a.dv[k] = p->dv[k];
    }
    a.bound = p->bound;
    a.tu = rt->ftle.d_t;
    a.tv = rt->ftle.d_t + width;
    a.pixels = rt->ftle.d_pix;
    a.width = width;
    a.height = height;
    a.tiles_x = bands.tiles_x;
    a.steps = p->steps;
    SAR_TRY(for_tile_bands(bands, [&](uint32_t first, uint32_t n) -> int {
        a.first_tile = first;
        a.n_tiles = n;
        return timed_launch(rt, rt->tm.iter, [&] { launch_ftle_flow(a, rt->stream); });
    }));
    SAR_TRY(timed_launch(rt, rt->tm.fold, [&] { launch_ftle_gram(a, rt->stream); }));
    HIP_TRY(hipMemcpyAsync(pixels_out_host, rt->ftle.d_pix, static_cast<size_t>(npix) * sizeof(sar_ftle_pixel), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));

    // the finish and the statistics
    const FtleMetric m = ftle_metric(p);
    const double two_n = 2. * static_cast<double>(p->steps);
    sar_ftle_stats st;
    std::memset(&st, 0, sizeof(st));
    st.pixels = npix;
    st.ftle_min = HUGE_VAL;
    st.ftle_max = -HUGE_VAL;
    std::vector<double> stretch2(npix);
    for (uint32_t i = 0; i < npix; ++i) {
        sar_ftle_pixel& r = pixels_out_host[i];
        ftle_finish(r, m, two_n);
        stretch2[i] = r.stretch2;
        ++(r.status == SAR_SEARCH_BOUNDED ? st.bounded : st.escaped);
        if (r.flags & SAR_FTLE_EDGE) ++st.edge;
        if (r.flags & (SAR_FTLE_ONE_SIDED_U | SAR_FTLE_ONE_SIDED_V)) ++st.one_sided;
        if ((r.flags & SAR_FTLE_NO_U) && (r.flags & SAR_FTLE_NO_V)) ++st.isolated;
        if (std::isfinite(r.ftle)) {
            st.ftle_min = r.ftle < st.ftle_min ? r.ftle : st.ftle_min;
            st.ftle_max = r.ftle > st.ftle_max ? r.ftle : st.ftle_max;
        }
    }
    // stretch2 goes back for the colorize
    HIP_TRY(hipMemcpyAsync(rt->ftle.d_stretch2, stretch2.data(), static_cast<size_t>(npix) * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->ftle.width = width;
    rt->ftle.height = height;
    rt->ftle.steps = p->steps;
    if (stats_out) *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_ftle_colors_default(sar_ftle_colors* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->hi = 1.;
    out->fade = 32.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_ftle_colorize(const sar_config* cfg, sar_runtime* rt, const sar_ftle_colors* colors, uint16_t* rgba16_out_host) try {
    if (!cfg || !rt || !rgba16_out_host) return SAR_ERR_INVALID;
    const sar_ftle_colors c = given_or_default(colors, sar_ftle_colors_default);
    if (!std::isfinite(c.lo) || !std::isfinite(c.hi) || !(c.lo < c.hi) || !std::isfinite(c.hi - c.lo)) {
        set_error("sar_runtime_ftle_colorize: lo and hi must be finite with lo < hi and a finite hi - lo");
        return SAR_ERR_INVALID;
    }
    if (!(c.fade > 0.) || !std::isfinite(c.fade)) {
        set_error("sar_runtime_ftle_colorize: the fade must be positive and finite");
        return SAR_ERR_INVALID;
    }
    return colorize_tail("sar_runtime_ftle_colorize", "FTLE map", "sar_runtime_ftle", cfg, rt, rt->ftle.width, rt->ftle.height,
                         rt->ftle.d_rgba, rgba16_out_host, [&](uint32_t npix, uint16_t* rgba) {
                             launch_ftle_colorize(rt->ftle.d_pix, rt->ftle.d_stretch2, npix, palette_params(cfg),
                                                  2. * static_cast<double>(rt->ftle.steps), c.lo, c.hi - c.lo, c.fade, rgba, rt->stream);
                         });
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
