// sar_plane.cpp — the host half of the Lyapunov planes (include/sar.h: sar_plane_*, sar_runtime_plane, sar_runtime_plane_colorize):
// the checks, the banded launches of k_plane (sar_plane.hip), the search's finish of the records, and their colours.
//
// Built with -ffp-contract=off: sar_plane_coeffs must produce the device's doubles.
#include <cmath>
#include <cstring>

#include "sar_analysis.hpp"
#include "sar_search.hpp"

using namespace sar;

namespace {

int check_plane(const sar_plane_params* p, const char* where) {
    if (!p) return SAR_ERR_INVALID;
    SAR_TRY(check_sweep_axes(where, p->axis));
    SAR_TRY(check_plane_size(where, p->width, p->height));
    SAR_TRY(check_sweep_ranges(where, p->lo, p->hi));
    SAR_TRY(check_bound(where, p->bound));
    SAR_TRY(check_steps(where, p->transient, p->steps));
    if (p->mode != SAR_PLANE_L1 && p->mode != SAR_PLANE_SPECTRUM) {
        set_error("%s: mode must be SAR_PLANE_L1 or SAR_PLANE_SPECTRUM (%d)", where, p->mode);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

PlaneArgs plane_args(const sar_plane_params* p) {
    return sweep_args(p->base, p->axis, p->lo, p->hi, p->width, p->height, p->transient, p->steps, p->start, p->bound);
}

}  // namespace

extern "C" {

int sar_plane_params_default(sar_plane_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->axis[0] = 0;
    out->axis[1] = 1;
    out->lo[0] = out->lo[1] = -1.2;
    out->hi[0] = out->hi[1] = 1.2;
    out->width = out->height = 256;
    out->start[0] = out->start[1] = out->start[2] = 0.05;
    out->transient = 1000;
    out->steps = 20000;
    out->bound = 1e6;
    out->mode = SAR_PLANE_L1;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_plane_coeffs(const sar_plane_params* p, uint32_t x, uint32_t y, double out30[30]) try {
    SAR_TRY(check_plane(p, "sar_plane_coeffs"));
    return sweep_coeffs(plane_args(p), x, y, out30);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_plane(sar_runtime* rt, const sar_plane_params* p, sar_plane_record* out_host, sar_plane_stats* stats_out) try {
    SAR_TRY(check_plane(p, "sar_runtime_plane"));  // (no device needed to refuse the parameters)
    if (!rt || !out_host) return SAR_ERR_INVALID;
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_plane (sar_timing)
    rt->plane.width = rt->plane.height = 0;  // no plane until this one is whole
    const uint32_t npix = p->width * p->height;
    HIP_TRY(rt->plane.d_rec.grow(nullptr, npix));
    PlaneArgs a = plane_args(p);
    a.records = rt->plane.d_rec;
    SAR_TRY(for_tile_bands(tile_bands(p->width, p->height, rt->opt.plane_chunk ? rt->opt.plane_chunk : kDefaultPlaneChunk), [&](uint32_t first, uint32_t n) {
        a.first_tile = first;
        a.n_tiles = n;
        return timed_launch(rt, rt->tm.iter, [&] { launch_plane(a, p->mode, rt->stream); });
    }));
    HIP_TRY(hipMemcpyAsync(out_host, rt->plane.d_rec, static_cast<size_t>(npix) * sizeof(sar_plane_record), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    sar_plane_stats st;
    std::memset(&st, 0, sizeof(st));
    st.pixels = npix;
    for (uint32_t i = 0; i < npix; ++i) {
        sar_plane_record& r = out_host[i];
        // folded steps: every one of a BOUNDED record, all but the failing one otherwise, none for a death in the transient
        const uint32_t folded = r.status == SAR_SEARCH_BOUNDED ? r.steps_done : (r.steps_done ? r.steps_done - 1u : 0u);
        lyapunov_finish(r.log2_exp, r.mant, p->mode, folded, r.lyapunov, &r.ky_dim);
        if (r.status == SAR_SEARCH_BOUNDED) ++st.bounded;
        else if (r.status == SAR_SEARCH_DEGENERATE) ++st.degenerate;
        else if (r.steps_done) ++st.diverged_late;
        else ++st.diverged_transient;
    }
    rt->plane.width = p->width;
    rt->plane.height = p->height;
    rt->plane.mode = p->mode;
    if (stats_out) *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_plane_colors_default(sar_plane_colors* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->threshold = 0.;
    out->chaos_scale = 0.25;
    out->order_scale = 1.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_plane_colorize(const sar_config* cfg, sar_runtime* rt, const sar_plane_colors* colors, uint16_t* rgba16_out_host) try {
    if (!cfg || !rt || !rgba16_out_host) return SAR_ERR_INVALID;
    const sar_plane_colors c = given_or_default(colors, sar_plane_colors_default);
    if (!std::isfinite(c.threshold) || !(c.chaos_scale > 0.) || !std::isfinite(c.chaos_scale) || !(c.order_scale > 0.) ||
        !std::isfinite(c.order_scale)) {
        set_error("sar_runtime_plane_colorize: threshold must be finite, chaos_scale and order_scale positive and finite");
        return SAR_ERR_INVALID;
    }
    return colorize_tail("sar_runtime_plane_colorize", "plane", "sar_runtime_plane", cfg, rt, rt->plane.width, rt->plane.height, rt->plane.d_rgba,
                         rgba16_out_host, [&](uint32_t npix, uint16_t* rgba) {
                             launch_plane_colorize(rt->plane.d_rec, npix, rt->plane.mode, palette_params(cfg), c.threshold, c.chaos_scale,
                                                   c.order_scale, rgba, rt->stream);
                         });
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
