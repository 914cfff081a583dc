// sar_period.cpp — the host half of the period planes (include/sar.h: sar_period_*, sar_runtime_period,
// sar_runtime_period_colorize): the checks, the upload of a caller's coefficient list, the banded launches of k_period
// (sar_period.hip), the statistics, and the colours.
//
// Built with -ffp-contract=off: sar_period_coeffs must produce the device's doubles.
#include <cmath>
#include <cstring>

#include "sar_analysis.hpp"
#include "sar_period.hpp"

using namespace sar;

namespace {

// the size, the run and the tolerance: what both forms need
int check_period(const sar_period_params* p, const char* where) {
    if (!p) { set_error("%s: the parameters are NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_plane_size(where, p->width, p->height));
    SAR_TRY(check_bound(where, p->bound));
    SAR_TRY(check_steps(where, p->transient, p->max_period));
    if (!p->max_period) {
        set_error("%s: max_period must be 1 to 2^31", where);
        return SAR_ERR_INVALID;
    }
    if (!(p->eps >= 0.) || !std::isfinite(p->eps)) {
        set_error("%s: eps must be finite and not negative", where);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

// the axes and their ranges: the sweep form alone
int check_period_sweep(const sar_period_params* p, const char* where) {
    SAR_TRY(check_sweep_axes(where, p->axis));
    return check_sweep_ranges(where, p->lo, p->hi);
}

// the kernels' view of a checked plane (the list form ignores base, axis, lo and span)
PeriodArgs period_args(const sar_period_params* p) {
    PeriodArgs a;
    std::memset(&a, 0, sizeof(a));
    a.plane = sweep_args(p->base, p->axis, p->lo, p->hi, p->width, p->height, p->transient, p->max_period, p->start, p->bound);
    a.eps = p->eps;
    return a;
}

}  // namespace

extern "C" {

int sar_period_params_default(sar_period_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->axis[0] = 0;
    out->axis[1] = 1;
    out->lo[0] = out->lo[1] = -1.2;
    out->hi[0] = out->hi[1] = 1.2;
    out->width = out->height = 256;
    out->start[0] = out->start[1] = out->start[2] = 0.05;
    out->transient = 2000;
    out->max_period = 256;
    out->bound = 1e6;
    out->eps = 1e-9;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_period_coeffs(const sar_period_params* p, uint32_t x, uint32_t y, double out30[30]) try {
    SAR_TRY(check_period(p, "sar_period_coeffs"));
    SAR_TRY(check_period_sweep(p, "sar_period_coeffs"));
    return sweep_coeffs(period_args(p).plane, x, y, out30);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_period(sar_runtime* rt, const sar_period_params* p, const double* coeffs_host, sar_period_record* out_host,
                       sar_period_stats* stats_out) try {
    SAR_TRY(check_period(p, "sar_runtime_period"));  // (no device needed to refuse the parameters)
    if (!coeffs_host) SAR_TRY(check_period_sweep(p, "sar_runtime_period"));
    if (!rt || !out_host) { set_error("sar_runtime_period: the runtime or the record buffer is NULL"); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_period (sar_timing)
    rt->period.width = rt->period.height = 0;  // no period plane until this one is whole
    const uint32_t npix = p->width * p->height;
    HIP_TRY(rt->period.d_rec.grow(nullptr, npix));
    PeriodArgs a = period_args(p);
    a.records = rt->period.d_rec;
    if (coeffs_host) {
        const size_t n = static_cast<size_t>(npix) * kSearchCoeffs;
        HIP_TRY(rt->period.d_coeffs.grow(nullptr, n));
        HIP_TRY(hipMemcpyAsync(rt->period.d_coeffs, coeffs_host, n * sizeof(double), hipMemcpyHostToDevice, rt->stream));
        a.coeffs = rt->period.d_coeffs;
    }
    SAR_TRY(for_tile_bands(tile_bands(p->width, p->height, rt->opt.period_chunk ? rt->opt.period_chunk : kDefaultPeriodChunk), [&](uint32_t first, uint32_t n) {
        a.plane.first_tile = first;
        a.plane.n_tiles = n;
        return timed_launch(rt, rt->tm.iter, [&] { launch_period(a, coeffs_host != nullptr, rt->stream); });
    }));
    HIP_TRY(hipMemcpyAsync(out_host, rt->period.d_rec, static_cast<size_t>(npix) * sizeof(sar_period_record), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (the caller's coefficient list has been read, too)
    sar_period_stats st;
    std::memset(&st, 0, sizeof(st));
    st.pixels = npix;
    for (uint32_t i = 0; i < npix; ++i) {
        const sar_period_record& r = out_host[i];
        if (r.status != SAR_SEARCH_BOUNDED) ++(r.steps_done ? st.diverged_late : st.diverged_transient);
        else ++(r.period ? st.periodic : st.aperiodic);
        if (r.period > st.max_period_found) st.max_period_found = r.period;
    }
    rt->period.width = p->width;
    rt->period.height = p->height;
    if (stats_out) *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_period_colors_default(sar_period_colors* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->colours = 16;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_period_colorize(const sar_config* cfg, sar_runtime* rt, const sar_period_colors* colors, uint16_t* rgba16_out_host) try {
    if (!cfg || !rt || !rgba16_out_host) return SAR_ERR_INVALID;
    const sar_period_colors c = given_or_default(colors, sar_period_colors_default);
    if (!c.colours) {
        set_error("sar_runtime_period_colorize: colours must be at least 1");
        return SAR_ERR_INVALID;
    }
    return colorize_tail("sar_runtime_period_colorize", "period plane", "sar_runtime_period", cfg, rt, rt->period.width, rt->period.height,
                         rt->period.d_rgba, rgba16_out_host, [&](uint32_t npix, uint16_t* rgba) {
                             launch_period_colorize(rt->period.d_rec, npix, palette_params(cfg), c.colours, rgba, rt->stream);
                         });
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
