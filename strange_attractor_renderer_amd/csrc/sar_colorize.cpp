// sar_colorize.cpp — colorize: the Gas run with auto exposure and auto colour range, the Depth colorize, the image conversion and export
// into the runtime's own buffers, and the read-back with its tickets. Host logic only; the arithmetic is in sar_image.hip and sar_select.hip.
#include <cmath>
#include <cstring>

#include "sar_plan.hpp"

using namespace sar;

int sar::validate_exposure(const sar_exposure_params* p) {
    if (!p) { set_error("exposure parameters are NULL"); return SAR_ERR_INVALID; }
    if (!(0. <= p->q_black && p->q_black <= p->q_white && p->q_white <= 1.)) {
        set_error("exposure: need 0 <= q_black <= q_white <= 1 (got %g, %g)", p->q_black, p->q_white);
        return SAR_ERR_INVALID;
    }
    if (!std::isfinite(p->level_black) || !std::isfinite(p->level_white) || !(p->level_black < p->level_white)) {
        set_error("exposure: need finite levels with level_black < level_white (got %g, %g)", p->level_black, p->level_white);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

int sar::validate_color_range(const sar_color_range_params* p) {
    if (!p) { set_error("colour range parameters are NULL"); return SAR_ERR_INVALID; }
    if (!(0. <= p->q_lo && p->q_lo <= p->q_hi && p->q_hi <= 1.)) {
        set_error("colour range: need 0 <= q_lo <= q_hi <= 1 (got %g, %g)", p->q_lo, p->q_hi);
        return SAR_ERR_INVALID;
    }
    if (!std::isfinite(p->pos_lo) || !std::isfinite(p->pos_hi)) {
        set_error("colour range: need finite palette positions (got %g, %g)", p->pos_lo, p->pos_hi);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

PaletteParams sar::palette_params(const sar_config* cfg) {
    PaletteParams pal;
    std::memset(&pal, 0, sizeof(pal));
    pal.len = cfg->palette_len;
    for (uint32_t k = 0; k < cfg->palette_len; ++k)
        for (int ch = 0; ch < 3; ++ch) pal.rgb[k][ch] = cfg->palette_rgb[k][ch];
    for (int ch = 0; ch < 3; ++ch)  // Palette::new duplicates the last entry (:416-418)
        pal.rgb[cfg->palette_len][ch] = cfg->palette_rgb[cfg->palette_len - 1][ch];
    return pal;
}

namespace {

// the select scratch and record(s) of a runtime for one consumer (sar_internal.hpp: SelectState): made on first use, the histograms
// zeroed once (every scan kernel clears what it read)
template <typename Rec>
int ensure_select(sar_runtime* rt, DevBuf<uint32_t>& scratch, uint32_t words, DevBuf<Rec>& rec, size_t n_rec) {
    if (scratch && rec) return SAR_OK;
    HIP_TRY(scratch.grow(nullptr, words));
    HIP_TRY(rec.grow(nullptr, n_rec));
    HIP_TRY(hipMemsetAsync(scratch, 0, words * sizeof(uint32_t), rt->stream));
    return SAR_OK;
}

// what follows a select's launches: after a launch error, whatever ran may have left a histogram dirty — the next call starts from
// fresh scratch
template <typename Scratch>
int select_launched(uint32_t n, sar_runtime* const* rts, Scratch scratch, const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SAR_OK;
    for (uint32_t i = 0; i < n; ++i) scratch(rts[i]).release();
    set_error("%s launch: %s", what, hipGetErrorString(e));
    return SAR_ERR_HIP;
}

// Select + solve of frame i = (cfgs[i], rts[i], params[i]) into rts[i]'s record: ONE set of launches on rts[0]'s stream for
// runtimes on one device and stream with one image size (the caller's to check). Enqueues only.
int enqueue_exposure(uint32_t n, const sar_config* const* cfgs, sar_runtime* const* rts, const sar_exposure_params* const* params) {
    sar_runtime* lead = rts[0];
    ExpoBatch t;
    std::memset(&t, 0, sizeof(t));
    t.lut = lead->d_lnlut;
    t.lut_len = kLnLutEntries;
    for (uint32_t i = 0; i < n; ++i) {
        SAR_TRY(ensure_select(rts[i], rts[i]->expo.d_scratch, kExpoScratchWords, rts[i]->expo.d_rec, 1));
        ExpoBatch::Frame& f = t.f[i];
        f.count = rts[i]->d_count;
        f.scalars = rts[i]->d_scalars;
        f.hist = rts[i]->expo.d_scratch;
        f.rec = rts[i]->expo.d_rec;
        f.q[0] = params[i]->q_black;
        f.q[1] = params[i]->q_white;
        f.level[0] = params[i]->level_black;
        f.level[1] = params[i]->level_white;
        f.cfg_offset = cfgs[i]->brightness_offset;
        f.cfg_factor = cfgs[i]->brightness_factor;
    }
    launch_exposure(t, n, lead->npix, lead->stream);
    return select_launched(n, rts, [](sar_runtime* rt) -> DevBuf<uint32_t>& { return rt->expo.d_scratch; }, "exposure");
}

// The same for the colour range of frame i = (rts[i], params[i]), into rts[i]'s measured record.
int enqueue_color_range(uint32_t n, sar_runtime* const* rts, const sar_color_range_params* const* params) {
    sar_runtime* lead = rts[0];
    CrBatch t;
    std::memset(&t, 0, sizeof(t));
    for (uint32_t i = 0; i < n; ++i) {
        SAR_TRY(ensure_select(rts[i], rts[i]->crange.d_scratch, kCrScratchWords, rts[i]->crange.d_rec, 2));  // (the measured record, the held one)
        CrBatch::Frame& f = t.f[i];
        f.count = rts[i]->d_count;
        f.steps = rts[i]->d_steps;
        f.hist = rts[i]->crange.d_scratch;
        f.rec = rts[i]->crange.d_rec;
        f.q[0] = params[i]->q_lo;
        f.q[1] = params[i]->q_hi;
        f.pos[0] = params[i]->pos_lo;
        f.pos[1] = params[i]->pos_hi;
    }
    launch_color_range(t, n, lead->npix, lead->stream);
    return select_launched(n, rts, [](sar_runtime* rt) -> DevBuf<uint32_t>& { return rt->crange.d_scratch; }, "colour range");
}

// ONE Gas colorize launch of pixels [first, first + n) of frame i = (cfgs[i], rts[i]) into outs[i], for m runtimes on rts[0]'s device,
// stream and image size, with one palette and alpha rule, one exposure mode and one colour-range mode (the caller's to check). With the
// exposure mode on, the run's exposure goes first and every frame takes its constants from its own record; off, from cfgs[0]. With the
// colour range measured, the run's select goes first as well; measured or held, every frame colours through its own record. Enqueues only.
int colorize_gas_run(uint32_t m, const sar_config* const* cfgs, sar_runtime* const* rts, void* const* outs, uint32_t first, uint32_t n) {
    sar_runtime* lead = rts[0];
    if (lead->expo.on) {
        const sar_exposure_params* params[kMaxBatchFrames];
        for (uint32_t i = 0; i < m; ++i) params[i] = &rts[i]->expo.params;
        SAR_TRY(enqueue_exposure(m, cfgs, rts, params));
    }
    if (lead->crange.mode == kCrMeasure) {
        const sar_color_range_params* params[kMaxBatchFrames];
        for (uint32_t i = 0; i < m; ++i) params[i] = &rts[i]->crange.params;
        SAR_TRY(enqueue_color_range(m, rts, params));
    }
    ColorizeBatch t;
    ColorizeWindows w;
    std::memset(&t, 0, sizeof(t));
    std::memset(&w, 0, sizeof(w));
    for (uint32_t i = 0; i < m; ++i) {
        t.f[i] = {rts[i]->d_count + first, rts[i]->d_steps + first, rts[i]->d_scalars, rts[i]->expo.on ? rts[i]->expo.d_rec.get() : nullptr, outs[i]};
        if (rts[i]->crange.mode != kCrOff) w.win[i] = rts[i]->crange.d_rec.get() + (rts[i]->crange.mode == kCrHold ? 1 : 0);
    }
    const sar_config* c0 = cfgs[0];
    launch_colorize_gas(t, lead->crange.mode != kCrOff ? &w : nullptr, m, lead->d_lnlut, kLnLutEntries, palette_params(c0), c0->brightness_offset,
                        c0->brightness_factor, c0->transparent ? 1 : 0, n, lead->stream);
    ++lead->colorize_launches;
    return SAR_OK;
}

}  // namespace

int sar::colorize_range(const sar_config* cfg, sar_runtime* rt, uint32_t first, uint32_t n, void* out_dev, bool global_scalars) {
    HIP_TRY(hipSetDevice(rt->device));
    if (first > rt->npix || n > rt->npix - first) { set_error("colorize: pixel range out of bounds"); return SAR_ERR_RANGE; }
    if (rt->expo.on && global_scalars) {
        set_error("colorize of a pixel range with auto exposure on: the quantiles are the whole image's (sar_runtime_set_exposure NULL)");
        return SAR_ERR_INVALID;
    }
    if (rt->crange.mode != kCrOff && global_scalars) {
        set_error("colorize of a pixel range with a colour range on: its quantiles are the whole image's (sar_runtime_set_color_range / "
                  "sar_runtime_hold_color_range NULL)");
        return SAR_ERR_INVALID;
    }
    rt->tm.single_begin(rt->tm.colorize_span, rt->stream);
    if (cfg->render_kind == SAR_RENDER_GAS) {
        const int st = n ? colorize_gas_run(1, &cfg, &rt, &out_dev, first, n) : SAR_OK;
        if (st != SAR_OK) {  // (the span begun above is closed: a timed runtime never holds half a span)
            rt->tm.single_end(rt->tm.colorize_span, rt->tm.colorize_timed, rt->stream);
            return st;
        }
    } else if (global_scalars) {
        if (n) launch_colorize_depth_range(rt->d_key + first, rt->d_scalars, n, out_dev, rt->stream);
        if (n) ++rt->colorize_launches;
    } else {
        launch_colorize_depth(rt->d_key + first, rt->d_scalars, n, out_dev, rt->stream);
        ++rt->colorize_launches;
    }
    rt->tm.single_end(rt->tm.colorize_span, rt->tm.colorize_timed, rt->stream);
    HIP_TRY(hipGetLastError());
    return SAR_OK;
}

static int do_colorize(const sar_config* cfg, sar_runtime* rt, void* out_dev) { return colorize_range(cfg, rt, 0, rt->npix, out_dev, false); }

static int ensure_rgba(sar_runtime* rt) {
    HIP_TRY(rt->rb.d_rgba.grow(rt, static_cast<size_t>(rt->npix) * 8));
    return SAR_OK;
}

extern "C" {

int sar_colorize_device(const sar_config* cfg, sar_runtime* rt, void* rgba_out_dev) try {
    SAR_TRY(check_cfg_matches(cfg, rt));
    if (!rgba_out_dev) return SAR_ERR_INVALID;
    return do_colorize(cfg, rt, rgba_out_dev);
} catch (...) { return sar::abi_caught(); }

int sar_colorize_device_batch(uint32_t n, const sar_config* const* cfgs, sar_runtime* const* rts, void* const* rgba_out_dev) try {
    if (n && (!cfgs || !rts || !rgba_out_dev)) return SAR_ERR_INVALID;
    for (uint32_t i = 0; i < n; ++i) {
        if (!cfgs[i] || !rts[i] || !rgba_out_dev[i]) return SAR_ERR_INVALID;
        SAR_TRY(check_cfg_matches(cfgs[i], rts[i]));
    }
    for (uint32_t first = 0; first < n;) {
        // runs of Gas frames of one palette, brightness and alpha rule on one device, stream and image size: ONE launch
        const sar_config* c0 = cfgs[first];
        sar_runtime* lead = rts[first];
        // (with auto exposure on, every frame's constants come from its own record: they need not agree — but the mode must)
        auto same_colours = [&](const sar_config* c, const sar_runtime* rt) {
            return c->render_kind == SAR_RENDER_GAS && c->palette_len == c0->palette_len && c->transparent == c0->transparent &&
                   rt->expo.on == lead->expo.on && rt->crange.mode == lead->crange.mode &&
                   (lead->expo.on || (std::memcmp(&c->brightness_offset, &c0->brightness_offset, sizeof(double)) == 0 &&
                                      std::memcmp(&c->brightness_factor, &c0->brightness_factor, sizeof(double)) == 0)) &&
                   std::memcmp(c->palette_rgb, c0->palette_rgb, sizeof(double) * 3 * c0->palette_len) == 0;
        };
        // (a runtime listed twice in one exposure run would give two frames of the launch ONE select scratch: with the mode on, a run
        // ends before a runtime it already holds — the repeat starts the next run, behind this one on the same stream. The colour
        // range's select has one scratch per runtime as well)
        auto fresh = [&](uint32_t i) {
            if (!lead->expo.on && lead->crange.mode != kCrMeasure) return true;
            for (uint32_t j = first; j < i; ++j)
                if (rts[j] == rts[i]) return false;
            return true;
        };
        const uint32_t m = c0->render_kind == SAR_RENDER_GAS && !lead->tm.timing ? run_length(n, rts, first, [&](uint32_t i) {
            return !rts[i]->tm.timing && same_colours(cfgs[i], rts[i]) && fresh(i);  // (a timed runtime records its own span)
        }) : 1;
        if (m == 1) {
            SAR_TRY(do_colorize(c0, lead, rgba_out_dev[first]));
        } else {
            HIP_TRY(hipSetDevice(lead->device));
            SAR_TRY(colorize_gas_run(m, cfgs + first, rts + first, rgba_out_dev + first, 0, lead->npix));
            HIP_TRY(hipGetLastError());
        }
        first += m;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_colorize(const sar_config* cfg, sar_runtime* rt, uint16_t* rgba_out_host) try {
    SAR_TRY(check_cfg_matches(cfg, rt));
    if (!rgba_out_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    SAR_TRY(ensure_rgba(rt));
    SAR_TRY(rt->rb.wait_last_copy(rt->stream));
    SAR_TRY(do_colorize(cfg, rt, rt->rb.d_rgba));
    HIP_TRY(hipMemcpyAsync(rgba_out_host, rt->rb.d_rgba, static_cast<size_t>(rt->npix) * 8, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_exposure_params_default(sar_exposure_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    out->q_black = 0.;
    out->q_white = 0.995;
    out->level_black = 0.;
    out->level_white = 1.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_exposure(const sar_config* cfg, sar_runtime* rt, const sar_exposure_params* params, sar_exposure* out) try {
    SAR_TRY(check_cfg_matches(cfg, rt));
    if (!out) { set_error("sar_runtime_exposure: NULL output"); return SAR_ERR_INVALID; }
    sar_exposure_params defaults;
    sar_exposure_params_default(&defaults);
    const sar_exposure_params* p = params ? params : &defaults;
    SAR_TRY(validate_exposure(p));
    HIP_TRY(hipSetDevice(rt->device));
    SAR_TRY(enqueue_exposure(1, &cfg, &rt, &p));
    HIP_TRY(hipMemcpyAsync(out, rt->expo.d_rec, sizeof(sar_exposure), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_exposure(sar_runtime* rt, const sar_exposure_params* params) try {
    if (params) SAR_TRY(validate_exposure(params));  // (first: bad parameters are refused whatever the handle)
    if (!rt) { set_error("sar_runtime_set_exposure: runtime is NULL"); return SAR_ERR_INVALID; }
    if (params) rt->expo.params = *params;
    rt->expo.on = params != nullptr;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_color_range_params_default(sar_color_range_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    out->q_lo = 0.01;
    out->q_hi = 0.99;
    out->pos_lo = 0.;
    out->pos_hi = 1.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_color_range(const sar_config* cfg, sar_runtime* rt, const sar_color_range_params* params, sar_color_range* out) try {
    sar_color_range_params defaults;
    sar_color_range_params_default(&defaults);
    const sar_color_range_params* p = params ? params : &defaults;
    SAR_TRY(validate_color_range(p));  // (first: bad parameters are refused whatever the handles)
    SAR_TRY(check_cfg_matches(cfg, rt));
    if (!out) { set_error("sar_runtime_color_range: NULL output"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    SAR_TRY(enqueue_color_range(1, &rt, &p));
    HIP_TRY(hipMemcpyAsync(out, rt->crange.d_rec, sizeof(sar_color_range), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_color_range(sar_runtime* rt, const sar_color_range_params* params) try {
    if (params) SAR_TRY(validate_color_range(params));  // (first: bad parameters are refused whatever the handle)
    if (!rt) { set_error("sar_runtime_set_color_range: runtime is NULL"); return SAR_ERR_INVALID; }
    if (params) rt->crange.params = *params;
    if (params) rt->crange.mode = kCrMeasure;
    else if (rt->crange.mode == kCrMeasure) rt->crange.mode = kCrOff;  // (NULL ends the mode, not a hold)
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_hold_color_range(sar_runtime* rt, const sar_color_range* range) try {
    if (range) {
        const double span = range->hi - range->lo;
        if (!std::isfinite(range->pos_lo) || !std::isfinite(range->pos_hi) ||
            (range->applied && !(std::isfinite(range->lo) && std::isfinite(range->hi) && span > 0. && std::isfinite(span)))) {
            set_error("colour range: a held window needs finite palette positions and, if applied, finite lo < hi with a finite span "
                      "(got [%g, %g] -> [%g, %g])", range->lo, range->hi, range->pos_lo, range->pos_hi);
            return SAR_ERR_INVALID;
        }
    }
    if (!rt) { set_error("sar_runtime_hold_color_range: runtime is NULL"); return SAR_ERR_INVALID; }
    if (!range) {
        if (rt->crange.mode == kCrHold) rt->crange.mode = kCrOff;
        return SAR_OK;
    }
    HIP_TRY(hipSetDevice(rt->device));
    SAR_TRY(ensure_select(rt, rt->crange.d_scratch, kCrScratchWords, rt->crange.d_rec, 2));
    // (behind every colorize that still reads the record it replaces; the wait: `range` is the caller's)
    HIP_TRY(hipMemcpyAsync(rt->crange.d_rec.get() + 1, range, sizeof(sar_color_range), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->crange.mode = kCrHold;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_color_range_to_velocity(const sar_config* in, const sar_color_range* range, sar_config* out) try {
    if (!in || !range || !out) { set_error("sar_color_range_to_velocity: NULL argument"); return SAR_ERR_INVALID; }
    if (in->color_transform != SAR_CT_ADJUSTED_VELOCITY) {
        set_error("sar_color_range_to_velocity: the config's colour transform is not SAR_CT_ADJUSTED_VELOCITY");
        return SAR_ERR_INVALID;
    }
    if (range->pos_lo != 0. || range->pos_hi != 1.) {
        set_error("sar_color_range_to_velocity: needs the palette positions (0, 1), got (%g, %g)", range->pos_lo, range->pos_hi);
        return SAR_ERR_INVALID;
    }
    sar_config c = *in;
    if (range->applied) {
        const double span = range->hi - range->lo;
        c.ct_offset = in->ct_offset - range->lo / in->ct_factor;
        c.ct_factor = in->ct_factor / span;
        if (!(span > 0.) || !std::isfinite(span) || in->ct_factor == 0. || !std::isfinite(c.ct_offset) || !std::isfinite(c.ct_factor)) {
            set_error("sar_color_range_to_velocity: window [%g, %g] with ct_factor %g gives no finite constants", range->lo, range->hi, in->ct_factor);
            return SAR_ERR_INVALID;
        }
    }
    *out = c;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_image_convert_device(sar_runtime* rt, const void* rgba16_dev, int format, void* out_dev) try {
    if (!rt || !rgba16_dev || !out_dev) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    if (format == SAR_FMT_RGBA16) {
        HIP_TRY(hipMemcpyAsync(out_dev, rgba16_dev, static_cast<size_t>(rt->npix) * 8, hipMemcpyDeviceToDevice, rt->stream));
        return SAR_OK;
    }
    if (launch_convert(rgba16_dev, format, out_dev, rt->npix, rt->stream) != 0) {
        set_error("unknown image format %d", format);
        return SAR_ERR_INVALID;
    }
    HIP_TRY(hipGetLastError());
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

// colorize + the CLI's conversion into the runtime's own buffers (d_rgba, d_export), on the launch stream; remembers where the
// image lies and how long it is
static int enqueue_colorize_convert(const sar_config* cfg, sar_runtime* rt, int format) {
    SAR_TRY(check_cfg_matches(cfg, rt));
    const size_t bytes = sar_image_bytes(format, rt->W, rt->H);
    if (bytes == 0) { set_error("sar_colorize_format: bad format"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    SAR_TRY(ensure_rgba(rt));
    SAR_TRY(rt->rb.wait_last_copy(rt->stream));
    SAR_TRY(do_colorize(cfg, rt, rt->rb.d_rgba));
    rt->rb.export_src = rt->rb.d_rgba;
    if (format != SAR_FMT_RGBA16) {
        HIP_TRY(rt->rb.d_export.grow(rt, static_cast<size_t>(rt->npix) * 6));  // largest converted format
        SAR_TRY(sar_image_convert_device(rt, rt->rb.d_rgba, format, rt->rb.d_export));
        rt->rb.export_src = rt->rb.d_export;
    }
    rt->rb.export_bytes = bytes;
    return SAR_OK;
}

// the read-back of that image: on the launch stream, or — the async form — on the copy stream behind an event, so that the next
// frame's kernels do not queue behind 20-30 MB over PCIe (d_rgba / d_export are written again only behind this copy's event)
static int enqueue_read_image(sar_runtime* rt, void* out_host, bool own_copy_stream) {
    if (!out_host || !rt->rb.export_src) { set_error("read-back: NULL output, or no colorized image to read"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    if (!own_copy_stream || rt->opt.readback_inline) {
        HIP_TRY(hipMemcpyAsync(out_host, rt->rb.export_src, rt->rb.export_bytes, hipMemcpyDeviceToHost, rt->stream));
        return SAR_OK;
    }
    SAR_TRY(rt->rb.ensure_copy_stream());
    HIP_TRY(rt->rb.img_ready.ensure(hipEventDisableTiming));
    HIP_TRY(hipEventRecord(rt->rb.img_ready, rt->stream));
    HIP_TRY(hipStreamWaitEvent(rt->rb.copy_stream, rt->rb.img_ready, 0));
    HIP_TRY(hipMemcpyAsync(out_host, rt->rb.export_src, rt->rb.export_bytes, hipMemcpyDeviceToHost, rt->rb.copy_stream));
    return SAR_OK;
}

static int ticket_for_read(sar_runtime* rt, uint64_t* ticket_out) {
    Event& ev = rt->rb.img_events[rt->rb.img_next % 8];
    HIP_TRY(ev.ensure(hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev, rt->opt.readback_inline ? rt->stream : rt->rb.copy_stream));
    rt->rb.copy_in_flight = !rt->opt.readback_inline;
    *ticket_out = rt->rb.img_next++;
    return SAR_OK;
}

int sar_colorize_format(const sar_config* cfg, sar_runtime* rt, int format, void* out_host) try {
    if (!out_host) { set_error("sar_colorize_format: NULL output"); return SAR_ERR_INVALID; }
    SAR_TRY(enqueue_colorize_convert(cfg, rt, format));
    SAR_TRY(enqueue_read_image(rt, out_host, false));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_colorize_format_async(const sar_config* cfg, sar_runtime* rt, int format, void* out_host, uint64_t* ticket_out) try {
    if (out_host && !ticket_out) { set_error("sar_colorize_format_async: NULL ticket"); return SAR_ERR_INVALID; }
    SAR_TRY(enqueue_colorize_convert(cfg, rt, format));
    if (!out_host) return SAR_OK;  // the image stays in device memory: sar_runtime_read_image_async fetches it
    SAR_TRY(enqueue_read_image(rt, out_host, true));
    return ticket_for_read(rt, ticket_out);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_read_image_async(sar_runtime* rt, void* out_host, uint64_t* ticket_out) try {
    if (!rt || !ticket_out) { set_error("sar_runtime_read_image_async: NULL argument"); return SAR_ERR_INVALID; }
    SAR_TRY(enqueue_read_image(rt, out_host, true));
    return ticket_for_read(rt, ticket_out);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_image_done(sar_runtime* rt, uint64_t ticket, int* done_out) try {
    if (!rt || !done_out || ticket >= rt->rb.img_next) { set_error("sar_runtime_image_done: no such ticket"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    const hipError_t e = hipEventQuery(rt->rb.img_events[ticket % 8]);
    if (e != hipSuccess && e != hipErrorNotReady) HIP_TRY(e);
    *done_out = e == hipSuccess ? 1 : 0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_wait_image(sar_runtime* rt, uint64_t ticket) try {
    if (!rt || ticket >= rt->rb.img_next) { set_error("sar_runtime_wait_image: no such ticket"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipEventSynchronize(rt->rb.img_events[ticket % 8]));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_colorize_range_device(const sar_config* cfg, sar_runtime* rt, uint32_t first_px, uint32_t n_px, void* rgba_out_dev) try {
    SAR_TRY(check_cfg_matches(cfg, rt));
    if (!rgba_out_dev) return SAR_ERR_INVALID;
    return colorize_range(cfg, rt, first_px, n_px, rgba_out_dev, true);
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
