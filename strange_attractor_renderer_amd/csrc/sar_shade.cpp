// sar_shade.cpp — the host half of shaded rendering (include/sar.h: sar_shade_params_default, sar_shade, sar_shade_device): the
// checks, the host constants of the contract (the light and half vectors, the reciprocal distances, the tap count, the window's span),
// the launch of k_shade (sar_shade.hip) and the statistics.
//
// Built with -ffp-contract=off: every constant is one IEEE operation after another, as the restatement has them.
#include <cmath>
#include <cstring>

#include "sar_analysis.hpp"
#include "sar_shade.hpp"

using namespace sar;

namespace {

bool weight_ok(double v) { return std::isfinite(v) && v >= 0.; }

int check_shade(const sar_shade_params* p, const char* where) {
    if (!std::isfinite(p->light[0]) || !std::isfinite(p->light[1]) || !std::isfinite(p->light[2]) ||
        (p->light[0] == 0. && p->light[1] == 0. && p->light[2] == 0.)) {
        set_error("%s: the light must be finite and not all zero (%g, %g, %g)", where, p->light[0], p->light[1], p->light[2]);
        return SAR_ERR_INVALID;
    }
    const struct { const char* name; double v; } weights[] = {
        {"ambient", p->ambient}, {"diffuse", p->diffuse}, {"specular", p->specular},
        {"ao_strength", p->ao_strength}, {"ao_range", p->ao_range}, {"smooth_range", p->smooth_range}};
    for (const auto& w : weights)
        if (!weight_ok(w.v)) { set_error("%s: %s must be finite and not negative (%g)", where, w.name, w.v); return SAR_ERR_INVALID; }
    if (p->shininess_log2 > kShadeMaxShininessLog2) {
        set_error("%s: shininess_log2 must be 0 to %u (%u)", where, kShadeMaxShininessLog2, p->shininess_log2);
        return SAR_ERR_INVALID;
    }
    if (p->ao_radius > kShadeMaxRadius) {
        set_error("%s: ao_radius must be 0 to %u (%u)", where, kShadeMaxRadius, p->ao_radius);
        return SAR_ERR_INVALID;
    }
    if (p->smooth != 0 && p->smooth != 1) { set_error("%s: smooth must be 0 or 1 (%d)", where, p->smooth); return SAR_ERR_INVALID; }
    if (p->has_window != 0 && p->has_window != 1) { set_error("%s: has_window must be 0 or 1 (%d)", where, p->has_window); return SAR_ERR_INVALID; }
    if (p->has_window) {  // what sar_runtime_hold_color_range asks of a record
        const sar_color_range& w = p->window;
        const double span = w.hi - w.lo;
        if (!std::isfinite(w.pos_lo) || !std::isfinite(w.pos_hi) ||
            (w.applied && !(std::isfinite(w.lo) && std::isfinite(w.hi) && span > 0. && std::isfinite(span)))) {
            set_error("%s: colour range: a window needs finite palette positions and, if applied, finite lo < hi with a finite span "
                      "(got [%g, %g] -> [%g, %g])", where, w.lo, w.hi, w.pos_lo, w.pos_hi);
            return SAR_ERR_INVALID;
        }
    }
    return SAR_OK;
}

// out = v / |v| with |v| = sqrt((x x + y y) + z z), a division per component whatever the length is; returns the length
double normalised(const double v[3], double out[3]) {
    const double len = std::sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    for (int i = 0; i < 3; ++i) out[i] = v[i] / len;
    return len;
}

// out: the caller's image. host_image: it is host memory — k_shade writes rt->rb.d_rgba, made behind the refusals, and the caller reads
// it back; otherwise it is device memory and k_shade writes it.
int shade_launch(const sar_config* cfg, sar_runtime* rt, const sar_shade_params* params, sar_shade_stats* stats_out, void* out,
                 bool host_image, const char* where) {
    const sar_shade_params p = given_or_default(params, sar_shade_params_default);
    SAR_TRY(check_shade(&p, where));  // (no device needed to refuse the parameters)
    SAR_TRY(validate(cfg));
    const double k = static_cast<double>(cfg->width) * cfg->scale;
    if (!std::isfinite(k) || !(k > 0.)) {
        set_error("%s: width * scale must be finite and positive (%g)", where, k);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(check_cfg_matches(cfg, rt));
    if (!out) { set_error("%s: the output image is NULL", where); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    if (host_image) {
        HIP_TRY(rt->rb.d_rgba.grow(rt, static_cast<size_t>(rt->npix) * 8));
        SAR_TRY(rt->rb.wait_last_copy(rt->stream));
        out = rt->rb.d_rgba;
    }
    HIP_TRY(rt->shade.d_stats.grow(nullptr, 1));  // a plain allocation made on first use, freed with the runtime

    ShadeArgs a;
    std::memset(&a, 0, sizeof(a));
    a.key = rt->d_key;
    a.count = rt->d_count;
    a.steps = rt->d_steps;
    a.out = static_cast<ushort4*>(out);
    a.stats = rt->shade.d_stats;
    a.width = rt->W;
    a.height = rt->H;
    a.tiles_x = (rt->W + kShadeTileW - 1u) / kShadeTileW;
    a.R = p.ao_radius;
    a.Rz = p.ao_radius ? p.ao_radius : 1u;
    a.min_count = p.min_count;
    a.shininess_log2 = p.shininess_log2;
    a.smooth = p.smooth;
    for (int i = 0; i < 3; ++i) a.background[i] = p.background[i];
    a.background[3] = cfg->transparent ? 0 : 65535;
    a.k = k;
    normalised(p.light, a.L);  // (finite and not all zero, but its squares may underflow to 0 or overflow: L is then what IEEE gives)
    const double h[3] = {a.L[0], a.L[1], a.L[2] + 1.0};
    a.spec_on = normalised(h, a.H) == 0. ? 0 : 1;  // (a length of 0: the light (0, 0, -1); H is then not read)
    a.ambient = p.ambient;
    a.diffuse = p.diffuse;
    a.specular = p.specular;
    a.ao_strength = p.ao_strength;
    a.ao_range = p.ao_range;
    a.smooth_range = p.smooth_range;
    if (p.has_window && p.window.applied) {
        a.window = 1;
        a.w_lo = p.window.lo;
        a.w_span = p.window.hi - p.window.lo;
        a.w_pos_lo = p.window.pos_lo;
        a.w_dpos = p.window.pos_hi - p.window.pos_lo;
    }
    const int r = static_cast<int>(a.R);
    for (int dy = -r; dy <= r; ++dy)
        for (int dx = -r; dx <= r; ++dx) {
            const int d2 = dx * dx + dy * dy;
            if (d2 == 0 || d2 > r * r) continue;
            ++a.taps;
            a.inv_d[d2] = 1.0 / std::sqrt(static_cast<double>(d2));
        }
    a.pal = palette_params(cfg);

    const uint32_t tiles = a.tiles_x * ((rt->H + kShadeTileH - 1u) / kShadeTileH);
    HIP_TRY(hipMemsetAsync(rt->shade.d_stats, 0, sizeof(sar_shade_stats), rt->stream));
    rt->tm.single_begin(rt->tm.colorize_span, rt->stream);
    launch_shade(a, tiles, rt->stream);
    rt->tm.single_end(rt->tm.colorize_span, rt->tm.colorize_timed, rt->stream);
    HIP_TRY(hipGetLastError());
    if (stats_out) {
        HIP_TRY(hipMemcpyAsync(stats_out, rt->shade.d_stats, sizeof(sar_shade_stats), hipMemcpyDeviceToHost, rt->stream));
        HIP_TRY(hipStreamSynchronize(rt->stream));
    }
    return SAR_OK;
}

}  // namespace

extern "C" {

int sar_shade_params_default(sar_shade_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->light[0] = -0.5;
    out->light[1] = -0.7;
    out->light[2] = 0.6;
    out->ambient = 0.25;
    out->diffuse = 0.75;
    out->specular = 0.25;
    out->ao_strength = 1.0;
    out->ao_range = 12.0;
    out->smooth_range = 2.0;
    out->shininess_log2 = 5;
    out->ao_radius = 6;
    out->smooth = 1;
    out->min_count = 1;
    out->window.pos_hi = 1.0;  // (the window is off: has_window 0)
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_shade_device(const sar_config* cfg, sar_runtime* rt, const sar_shade_params* params, sar_shade_stats* stats_out,
                     void* rgba_out_dev) try {
    return shade_launch(cfg, rt, params, stats_out, rgba_out_dev, false, "sar_shade_device");
} catch (...) { return sar::abi_caught(); }

int sar_shade(const sar_config* cfg, sar_runtime* rt, const sar_shade_params* params, sar_shade_stats* stats_out,
              uint16_t* rgba_out_host) try {
    SAR_TRY(shade_launch(cfg, rt, params, nullptr, rgba_out_host, true, "sar_shade"));
    HIP_TRY(hipMemcpyAsync(rgba_out_host, rt->rb.d_rgba, static_cast<size_t>(rt->npix) * 8, hipMemcpyDeviceToHost, rt->stream));
    if (stats_out) HIP_TRY(hipMemcpyAsync(stats_out, rt->shade.d_stats, sizeof(sar_shade_stats), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
