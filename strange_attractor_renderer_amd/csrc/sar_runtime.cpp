// sar_runtime.cpp — the C ABI of the Runtime (include/sar.h): life cycle, reset, merge, colorize and image export, read-back
// accessors, timing and the tuning options. The render call itself is sar_render.cpp, its planning sar_plan.cpp, the multi-device
// ParallelRenderer sar_multi.cpp, the exchange of the one-process-per-GPU path sar_exchange.cpp.
//
// Host logic only (allocation, argument blocks, stream ordering); all arithmetic on image data happens in the kernel files
// (sar_iterate.hip, sar_accumulate.hip, sar_image.hip, sar_select.hip). There is no CPU fallback: without a HIP device every entry point
// that touches a runtime returns SAR_ERR_NO_DEVICE.
#include <sys/mman.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "sar_plan.hpp"
#include "sar_search.hpp"

using namespace sar;

namespace {

// ln(k+1) for k < kLnLutEntries, computed once per process with the host libm — the same function
// the oracle (and the reference, through Rust's f64::ln) calls on this machine.
const double* host_ln_lut() {
    static std::vector<double> lut;
    static std::once_flag once;
    std::call_once(once, [] {
        lut.resize(kLnLutEntries);
        for (uint32_t k = 0; k < kLnLutEntries; ++k) lut[k] = std::log(static_cast<double>(k + 1u));
    });
    return lut.data();
}

// The table in device memory: ONE per device, shared by every runtime there (read-only; it used to be 8 MiB of allocation and
// upload per runtime — 0.35 ms of each of a sweep's sixteen), released with the device's last runtime.
struct DeviceLnLut {
    std::mutex mu;
    double* table = nullptr;
    int refs = 0;
} g_lnlut[64];

int acquire_ln_lut(sar_runtime* rt) {
    if (rt->device < 0 || rt->device >= 64) { set_error("device %d: this library addresses devices 0..63", rt->device); return SAR_ERR_INVALID; }
    DeviceLnLut& d = g_lnlut[rt->device];
    std::lock_guard<std::mutex> lock(d.mu);
    if (!d.table) {
        double* t = nullptr;
        if (hipMalloc(&t, kLnLutEntries * sizeof(double)) != hipSuccess) return SAR_ERR_OOM;
        // (a blocking copy: the table is complete before any stream of any runtime can read it)
        if (hipMemcpy(t, host_ln_lut(), kLnLutEntries * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { hipFree(t); return SAR_ERR_HIP; }
        d.table = t;
    }
    ++d.refs;
    rt->d_lnlut = d.table;
    return SAR_OK;
}

void release_ln_lut(sar_runtime* rt) {
    if (!rt->d_lnlut || rt->device < 0 || rt->device >= 64) return;
    DeviceLnLut& d = g_lnlut[rt->device];
    std::lock_guard<std::mutex> lock(d.mu);
    if (--d.refs == 0) {
        hipFree(d.table);
        d.table = nullptr;
    }
    rt->d_lnlut = nullptr;
}

std::mutex g_group_mu;  // the reference counts of the frame groups

constexpr size_t kSlabAlign = 256;
size_t slab_round(size_t bytes) { return (bytes + kSlabAlign - 1) & ~(kSlabAlign - 1); }

}  // namespace

void* sar::slab_carve(sar_runtime* rt, bool host, size_t bytes) {
    char* base = host ? rt->hsub : rt->sub.get();
    const size_t size = host ? rt->hsub_bytes : rt->sub.cap();
    size_t& used = host ? rt->hsub_used : rt->sub_used;
    const size_t need = slab_round(bytes ? bytes : 1);
    if (!base || need > size - used) return nullptr;
    used += need;
    return base + used - need;
}

namespace {

int alloc_image_buffers(sar_runtime* rt, uint32_t w, uint32_t h) {
    const uint64_t npix64 = static_cast<uint64_t>(w) * h;
    if (w == 0 || h == 0) { set_error("zero image dimension"); return SAR_ERR_INVALID; }
    if (npix64 > 0x7fffffffull) { set_error("width*height exceeds 2^31-1"); return SAR_ERR_RANGE; }
    // allocate first, commit on full success: a failed grow leaves the runtime as it was (old size, old buffers)
    DevBuf<uint32_t> count;
    DevBuf<unsigned long long> key;
    DevBuf<double> steps;
    hipError_t e = count.grow(rt, npix64);
    if (e == hipSuccess) e = key.grow(rt, npix64);
    if (e == hipSuccess) e = steps.grow(rt, npix64);
    if (e != hipSuccess) {
        set_error("image buffers for %ux%u: %s", w, h, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SAR_ERR_OOM : SAR_ERR_HIP;
    }
    rt->d_count = std::move(count);  // (each frees the buffer of the old size)
    rt->d_key = std::move(key);
    rt->d_steps = std::move(steps);
    rt->d_scratch_count.release();
    rt->d_scratch_key.release();
    rt->d_rgba.release();
    rt->d_export.release();
    rt->d_ztmp.release();
    rt->d_zhint.release();
    rt->export_src = nullptr;
    rt->copies = 0;
    rt->W = w;
    rt->H = h;
    rt->npix = static_cast<uint32_t>(npix64);
    return SAR_OK;
}

}  // namespace

int sar::clear_hints(sar_runtime* rt) {
    // hints are lower bounds of depths already accumulated; anything that can lower zbuf voids them (kWideHintEmpty: what they are
    // cleared to; only the arrays a launch has written since the last clear: a batched frame whose XCDs share one array leaves seven
    // untouched)
    const size_t entries = kHintStride(rt->npix) * rt->hint_copies_used;
    if (rt->d_zhint && rt->zhint_bytes == 4 && entries)
        HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rt->d_zhint.get()), static_cast<int>(kWideHintEmpty), entries, rt->stream));
    else if (rt->d_zhint && entries)
        HIP_TRY(hipMemsetAsync(rt->d_zhint, 0, entries * rt->zhint_bytes, rt->stream));
    rt->hint_copies_used = 0;
    rt->hint_range_set = false;  // empty hints: the next launch may measure the view's depth range anew
    return SAR_OK;
}

namespace {

// Runtime::reset of m runtimes on rts[0]'s device, stream and image size in ONE launch. The hints go with the buffers (clear_hints:
// what they are cleared to, and which of them); from here on they count as empty.
int do_reset(uint32_t m, sar_runtime* const* rts) {
    ResetBatch t;
    std::memset(&t, 0, sizeof(t));
    for (uint32_t i = 0; i < m; ++i) {
        sar_runtime* rt = rts[i];
        const size_t entries = rt->d_zhint ? kHintStride(rt->npix) * rt->hint_copies_used : 0;
        const bool wide = rt->zhint_bytes == 4;
        t.f[i] = {rt->d_count, rt->d_key, rt->d_steps, rt->d_scalars, static_cast<uint32_t*>(rt->d_zhint.get()),
                  static_cast<uint32_t>(wide ? entries : entries / 2u) /* (kHintStride is even) */, wide ? kWideHintEmpty : 0u};
        rt->hint_copies_used = 0;
        rt->hint_range_set = false;
    }
    launch_reset(t, m, rts[0]->npix, rts[0]->stream);
    HIP_TRY(hipGetLastError());
    return SAR_OK;
}

// the frames from `first` on that go through ONE launch: runtimes that share rts[first]'s device, stream and image size, at most
// kMaxBatchFrames, for as long as `also` holds for the next frame
template <typename Also>
uint32_t run_length(uint32_t n, sar_runtime* const* rts, uint32_t first, Also also) {
    const sar_runtime* lead = rts[first];
    uint32_t m = 1;
    while (first + m < n && m < kMaxBatchFrames && rts[first + m]->device == lead->device && rts[first + m]->stream == lead->stream &&
           rts[first + m]->npix == lead->npix && also(first + m)) ++m;
    return m;
}

}  // namespace

void sar::span_begin(sar_runtime* rt, std::vector<Span>& spans, size_t& used) {
    if (!rt->timing) return;
    if (used == spans.size()) {
        spans.emplace_back();
        spans.back().a.ensure(hipEventDefault);
        spans.back().b.ensure(hipEventDefault);
    }
    hipEventRecord(spans[used].a, rt->stream);
}
void sar::span_end(sar_runtime* rt, std::vector<Span>& spans, size_t& used) {
    if (!rt->timing) return;
    hipEventRecord(spans[used].b, rt->stream);
    ++used;
}
void sar::single_begin(sar_runtime* rt, Span& s) {
    if (!rt->timing) return;
    s.a.ensure(hipEventDefault);
    s.b.ensure(hipEventDefault);
    hipEventRecord(s.a, rt->stream);
}
void sar::single_end(sar_runtime* rt, Span& s, bool& flag) {
    if (!rt->timing) return;
    hipEventRecord(s.b, rt->stream);
    flag = true;
}

int sar::check_cfg_matches(const sar_config* cfg, const sar_runtime* rt) {
    SAR_TRY(validate(cfg));
    if (!rt) { set_error("runtime is NULL"); return SAR_ERR_INVALID; }
    if (cfg->width != rt->W || cfg->height != rt->H) {
        set_error("config is %ux%u but the runtime holds %ux%u", cfg->width, cfg->height, rt->W, rt->H);
        return SAR_ERR_DIM_MISMATCH;
    }
    return SAR_OK;
}

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

namespace sar {

PaletteParams palette_params(const sar_config* cfg) {
    PaletteParams pal;
    std::memset(&pal, 0, sizeof(pal));
    pal.len = cfg->palette_len;
    for (uint32_t k = 0; k < cfg->palette_len; ++k)
        for (int ch = 0; ch < 3; ++ch) pal.rgb[k][ch] = cfg->palette_rgb[k][ch];
    for (int ch = 0; ch < 3; ++ch)  // Palette::new duplicates the last entry (:416-418)
        pal.rgb[cfg->palette_len][ch] = cfg->palette_rgb[cfg->palette_len - 1][ch];
    return pal;
}

}  // namespace sar

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
int select_launched(uint32_t n, sar_runtime* const* rts, DevBuf<uint32_t> sar_runtime::*scratch, const char* what) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return SAR_OK;
    for (uint32_t i = 0; i < n; ++i) (rts[i]->*scratch).release();
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
        SAR_TRY(ensure_select(rts[i], rts[i]->d_expo, kExpoScratchWords, rts[i]->d_expo_rec, 1));
        ExpoBatch::Frame& f = t.f[i];
        f.count = rts[i]->d_count;
        f.scalars = rts[i]->d_scalars;
        f.hist = rts[i]->d_expo;
        f.rec = rts[i]->d_expo_rec;
        f.q[0] = params[i]->q_black;
        f.q[1] = params[i]->q_white;
        f.level[0] = params[i]->level_black;
        f.level[1] = params[i]->level_white;
        f.cfg_offset = cfgs[i]->brightness_offset;
        f.cfg_factor = cfgs[i]->brightness_factor;
    }
    launch_exposure(t, n, lead->npix, lead->stream);
    return select_launched(n, rts, &sar_runtime::d_expo, "exposure");
}

// The same for the colour range of frame i = (rts[i], params[i]), into rts[i]'s measured record.
int enqueue_color_range(uint32_t n, sar_runtime* const* rts, const sar_color_range_params* const* params) {
    sar_runtime* lead = rts[0];
    CrBatch t;
    std::memset(&t, 0, sizeof(t));
    for (uint32_t i = 0; i < n; ++i) {
        SAR_TRY(ensure_select(rts[i], rts[i]->d_crange, kCrScratchWords, rts[i]->d_crange_rec, 2));  // (the measured record, the held one)
        CrBatch::Frame& f = t.f[i];
        f.count = rts[i]->d_count;
        f.steps = rts[i]->d_steps;
        f.hist = rts[i]->d_crange;
        f.rec = rts[i]->d_crange_rec;
        f.q[0] = params[i]->q_lo;
        f.q[1] = params[i]->q_hi;
        f.pos[0] = params[i]->pos_lo;
        f.pos[1] = params[i]->pos_hi;
    }
    launch_color_range(t, n, lead->npix, lead->stream);
    return select_launched(n, rts, &sar_runtime::d_crange, "colour range");
}

// ONE Gas colorize launch of pixels [first, first + n) of frame i = (cfgs[i], rts[i]) into outs[i], for m runtimes on rts[0]'s device,
// stream and image size, with one palette and alpha rule, one exposure mode and one colour-range mode (the caller's to check). With the
// exposure mode on, the run's exposure goes first and every frame takes its constants from its own record; off, from cfgs[0]. With the
// colour range measured, the run's select goes first as well; measured or held, every frame colours through its own record. Enqueues only.
int colorize_gas_run(uint32_t m, const sar_config* const* cfgs, sar_runtime* const* rts, void* const* outs, uint32_t first, uint32_t n) {
    sar_runtime* lead = rts[0];
    if (lead->expo_on) {
        const sar_exposure_params* params[kMaxBatchFrames];
        for (uint32_t i = 0; i < m; ++i) params[i] = &rts[i]->expo_params;
        SAR_TRY(enqueue_exposure(m, cfgs, rts, params));
    }
    if (lead->crange_mode == kCrMeasure) {
        const sar_color_range_params* params[kMaxBatchFrames];
        for (uint32_t i = 0; i < m; ++i) params[i] = &rts[i]->crange_params;
        SAR_TRY(enqueue_color_range(m, rts, params));
    }
    ColorizeBatch t;
    ColorizeWindows w;
    std::memset(&t, 0, sizeof(t));
    std::memset(&w, 0, sizeof(w));
    for (uint32_t i = 0; i < m; ++i) {
        t.f[i] = {rts[i]->d_count + first, rts[i]->d_steps + first, rts[i]->d_scalars, rts[i]->expo_on ? rts[i]->d_expo_rec.get() : nullptr, outs[i]};
        if (rts[i]->crange_mode != kCrOff) w.win[i] = rts[i]->d_crange_rec.get() + (rts[i]->crange_mode == kCrHold ? 1 : 0);
    }
    const sar_config* c0 = cfgs[0];
    launch_colorize_gas(t, lead->crange_mode != kCrOff ? &w : nullptr, m, lead->d_lnlut, kLnLutEntries, palette_params(c0), c0->brightness_offset,
                        c0->brightness_factor, c0->transparent ? 1 : 0, n, lead->stream);
    ++lead->colorize_launches;
    return SAR_OK;
}

}  // namespace

int sar::colorize_range(const sar_config* cfg, sar_runtime* rt, uint32_t first, uint32_t n, void* out_dev, bool global_scalars) {
    HIP_TRY(hipSetDevice(rt->device));
    if (first > rt->npix || n > rt->npix - first) { set_error("colorize: pixel range out of bounds"); return SAR_ERR_RANGE; }
    if (rt->expo_on && global_scalars) {
        set_error("colorize of a pixel range with auto exposure on: the quantiles are the whole image's (sar_runtime_set_exposure NULL)");
        return SAR_ERR_INVALID;
    }
    if (rt->crange_mode != kCrOff && global_scalars) {
        set_error("colorize of a pixel range with a colour range on: its quantiles are the whole image's (sar_runtime_set_color_range / "
                  "sar_runtime_hold_color_range NULL)");
        return SAR_ERR_INVALID;
    }
    single_begin(rt, rt->colorize_span);
    if (cfg->render_kind == SAR_RENDER_GAS) {
        const int st = n ? colorize_gas_run(1, &cfg, &rt, &out_dev, first, n) : SAR_OK;
        if (st != SAR_OK) {  // (the span begun above is closed: a timed runtime never holds half a span)
            single_end(rt, rt->colorize_span, rt->colorize_timed);
            return st;
        }
    } else if (global_scalars) {
        if (n) launch_colorize_depth_range(rt->d_key + first, rt->d_scalars, n, out_dev, rt->stream);
        if (n) ++rt->colorize_launches;
    } else {
        launch_colorize_depth(rt->d_key + first, rt->d_scalars, n, out_dev, rt->stream);
        ++rt->colorize_launches;
    }
    single_end(rt, rt->colorize_span, rt->colorize_timed);
    HIP_TRY(hipGetLastError());
    return SAR_OK;
}

namespace {

int do_colorize(const sar_config* cfg, sar_runtime* rt, void* out_dev) { return colorize_range(cfg, rt, 0, rt->npix, out_dev, false); }

int check_device(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device available (this library has no CPU fallback)");
        return SAR_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= ndev) { set_error("device %d out of range (%d devices)", device, ndev); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(device));
    return SAR_OK;
}

// Streams, events, the persistent buffers and the reset state of a new runtime (enqueued on its stream; the caller waits). A
// runtime of a frame group runs on the group's streams and draws its memory from the group's allocations.
int init_runtime(sar_runtime* rt, const sar_config* cfg, int device) {
    rt->device = device;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) rt->sm_count = static_cast<uint32_t>(prop.multiProcessorCount);
    if (rt->group) {
        rt->stream = rt->group->stream;
        rt->copy_stream = rt->group->copy_stream;
    } else {
        if (rt->own_stream.ensure(hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return SAR_ERR_HIP; }
        rt->stream = rt->own_stream;
    }
    if (rt->starts_copied.ensure(hipEventDisableTiming) != hipSuccess) return SAR_ERR_HIP;
    if (rt->d_scalars.grow(rt, SC_COUNT) != hipSuccess) return SAR_ERR_OOM;
    SAR_TRY(acquire_ln_lut(rt));
    SAR_TRY(alloc_image_buffers(rt, cfg->width, cfg->height));
    SAR_TRY(do_reset(1, &rt));
    rt->rng.seed(cfg->seed);
    return SAR_OK;
}

// the last runtime of a group takes the group's streams and allocations with it (force: a group no runtime ever joined)
void release_group(RuntimeGroup* g, bool force) {
    {
        std::lock_guard<std::mutex> lock(g_group_mu);
        if (!force && --g->refs > 0) return;
    }
    hipSetDevice(g->device);
    delete g;
}

}  // namespace

sar_runtime::~sar_runtime() {
    // (a borrowed copy stream as well: a read-back may still read d_export)
    for (hipStream_t s : {stream, static_cast<hipStream_t>(side), copy_stream, static_cast<hipStream_t>(upload_stream)})
        if (s) hipStreamSynchronize(s);
    release_ln_lut(this);
}

namespace {

// Device and page-locked bytes ONE runtime of a frame group holds once it renders frames like cfg in batches of n: the persistent
// buffers, the scratch, one array of depth hints, the record arena, checkpoints, warm-up sets, start points, the colorized and the
// converted image. An estimate with slack — what it misses is allocated separately.
void group_bytes_per_runtime(const sar_config* cfg, sar_runtime* probe, uint32_t n, size_t& dev_bytes, size_t& host_bytes) {
    const size_t npix = probe->npix;
    size_t dev = 0, host = 0, items = 0;
    auto add = [&](size_t b) { dev += slab_round(b); ++items; };
    add(SC_COUNT * sizeof(uint32_t));
    add(npix * 4); add(npix * 8); add(npix * 8);  // count, key, steps
    add(npix * 8);                                // colorized image
    add(npix * 6);                                // converted image
    const uint32_t n_jobs = cfg->jobs_total;
    const uint64_t iters = n_jobs ? cfg->iterations / n_jobs : 0;
    LaunchPlan pl;
    if (n_jobs && iters && iters <= kMaxChunkOrdinals && plan_launch(cfg, probe, n_jobs, iters, pl, n) == SAR_OK && pl.binned) {
        add(npix * 8);                                                                            // depth keys of a launch
        add(npix * 4 * pl.splits);                                                                // partial histograms (batched launches)
        add((npix / 2048 + 1) * 4);                                                               // segment flags
        add((npix + 2) * pl.hint_bytes * (n >= 3u ? 1u : 8u));                                    // depth hints
        add(static_cast<size_t>(pl.arena_waves) * pl.chunks_per_wave * chunk_bytes(pl.R));        // record arena
        add(static_cast<size_t>(pl.max_waves) * pl.geo.bins * 4);                                 // list heads
        add(static_cast<size_t>(pl.n_ckpt) * 3 * pl.chunk_jobs * 8);                              // checkpoints
        for (int set = 0; set < 2; ++set) { add(static_cast<size_t>(pl.chunk_jobs) * 24); add(static_cast<size_t>(pl.chunk_jobs) * 4); }  // warm-up sets
        add((static_cast<size_t>(n_jobs) * 3 + 2) * 8);                                           // start points
        host += slab_round((static_cast<size_t>(n_jobs) * 3 + 2) * 8);
    }
    dev += slab_round(sizeof(BatchFrame) * kMaxBatchFrames);                                      // (a leader's argument table)
    host += slab_round(sizeof(BatchFrame) * kMaxBatchFrames * kBatchRing);
    dev_bytes = dev + 16 * kSlabAlign;   // the handful of counters
    host_bytes = host + 4 * kSlabAlign;
    (void)items;
}

int ensure_rgba(sar_runtime* rt) {
    HIP_TRY(rt->d_rgba.grow(rt, static_cast<size_t>(rt->npix) * 8));
    return SAR_OK;
}

}  // namespace

extern "C" {

int sar_device_count(int* out_count) try {
    if (!out_count) return SAR_ERR_INVALID;
    int n = 0;
    const hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *out_count = 0;
        set_error("hipGetDeviceCount: %s", hipGetErrorString(e));
        return SAR_ERR_NO_DEVICE;
    }
    *out_count = n;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_device_pci_bus_id(int device, char* out, size_t cap) try {
    if (!out || cap < 16) return SAR_ERR_INVALID;
    out[0] = 0;
    if (hipDeviceGetPCIBusId(out, static_cast<int>(cap), device) != hipSuccess) {
        set_error("hipDeviceGetPCIBusId(%d) failed", device);
        return SAR_ERR_NO_DEVICE;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_new(const sar_config* cfg, int device, sar_runtime** out) try {
    if (!out) return SAR_ERR_INVALID;
    *out = nullptr;
    SAR_TRY(validate(cfg));
    SAR_TRY(check_device(device));
    sar_runtime* rt = new (std::nothrow) sar_runtime();
    if (!rt) return SAR_ERR_OOM;
    const int st = init_runtime(rt, cfg, device);
    if (st != SAR_OK) { sar_runtime_free(rt); return st; }
    if (hipStreamSynchronize(rt->stream) != hipSuccess) { sar_runtime_free(rt); return SAR_ERR_HIP; }
    *out = rt;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_new_group(const sar_config* cfg, int device, uint32_t n, sar_runtime** out) try {
    if (!out || n == 0 || n > kMaxBatchFrames) { set_error("sar_runtime_new_group: 1..%u runtimes", kMaxBatchFrames); return SAR_ERR_INVALID; }
    for (uint32_t i = 0; i < n; ++i) out[i] = nullptr;
    SAR_TRY(validate(cfg));
    SAR_TRY(check_device(device));
    RuntimeGroup* g = new (std::nothrow) RuntimeGroup();
    if (!g) return SAR_ERR_OOM;
    g->device = device;
    auto fail = [&](int code) {
        bool any = false;
        for (uint32_t i = 0; i < n; ++i)
            if (out[i]) { any = true; sar_runtime_free(out[i]); out[i] = nullptr; }  // (the last one releases the group)
        if (!any) release_group(g, true);
        return code;
    };
    if (g->stream.ensure(hipStreamNonBlocking) != hipSuccess || g->copy_stream.ensure(hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return fail(SAR_ERR_HIP); }
    // what one runtime of the group will hold for frames like cfg in batches of n (the plan its first batched launch will make;
    // a need the estimate misses is served by hipMalloc as before)
    size_t dev_bytes = 0, host_bytes = 0;
    {
        sar_runtime probe;
        probe.device = device;
        probe.W = cfg->width; probe.H = cfg->height;
        probe.npix = static_cast<uint32_t>(static_cast<uint64_t>(cfg->width) * cfg->height);
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) probe.sm_count = static_cast<uint32_t>(prop.multiProcessorCount);
        group_bytes_per_runtime(cfg, &probe, n, dev_bytes, host_bytes);
    }
    if (g->hslab.grow(nullptr, host_bytes * n) != hipSuccess) (void)hipGetLastError();
    for (uint32_t i = 0; i < n; ++i) {
        sar_runtime* rt = new (std::nothrow) sar_runtime();
        if (!rt) return fail(SAR_ERR_OOM);
        rt->group = g;
        { std::lock_guard<std::mutex> lock(g_group_mu); ++g->refs; }
        out[i] = rt;
        // (one allocation per runtime, not one for the group: see sar_runtime_impl.hpp; beyond 4 GiB the buffers stay separate)
        if (dev_bytes > (4ull << 30) || rt->sub.grow(nullptr, dev_bytes) != hipSuccess) (void)hipGetLastError();
        if (g->hslab) { rt->hsub = g->hslab + host_bytes * i; rt->hsub_bytes = host_bytes; }
        rt->single_hint_array = n >= 3u;  // (batches of three frames or more deal their frames to the XCDs)
        const int st = init_runtime(rt, cfg, device);
        if (st != SAR_OK) return fail(st);
    }
    if (hipStreamSynchronize(g->stream) != hipSuccess) return fail(SAR_ERR_HIP);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_free(sar_runtime* rt) try {
    if (!rt) return SAR_OK;
    hipSetDevice(rt->device);
    RuntimeGroup* g = rt->group;
    delete rt;
    if (g) release_group(g, false);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_reset(sar_runtime* rt) try {
    if (!rt) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    return do_reset(1, &rt);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_reset_batch(uint32_t n, sar_runtime* const* rts) try {
    if (n && !rts) return SAR_ERR_INVALID;
    for (uint32_t i = 0; i < n; ++i)
        if (!rts[i]) return SAR_ERR_INVALID;
    for (uint32_t first = 0; first < n;) {
        const uint32_t m = run_length(n, rts, first, [](uint32_t) { return true; });
        HIP_TRY(hipSetDevice(rts[first]->device));
        SAR_TRY(do_reset(m, rts + first));
        first += m;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_width_height(sar_runtime* rt, uint32_t width, uint32_t height) try {
    if (!rt) return SAR_ERR_INVALID;
    if (rt->W == width && rt->H == height) return SAR_OK;  // :668
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    SAR_TRY(alloc_image_buffers(rt, width, height));
    return do_reset(1, &rt);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_seed(sar_runtime* rt, uint64_t seed) try {
    if (!rt) return SAR_ERR_INVALID;
    rt->rng.seed(seed);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_merge(sar_runtime* dst, const sar_runtime* src) try {
    if (!dst || !src) return SAR_ERR_INVALID;
    if (dst->W != src->W || dst->H != src->H) {  // assert_eq! in the reference (:709-710)
        set_error("merge: %ux%u vs %ux%u", dst->W, dst->H, src->W, src->H);
        return SAR_ERR_DIM_MISMATCH;
    }
    if (dst->device != src->device) { set_error("merge: runtimes live on different devices; use the exchange API"); return SAR_ERR_INVALID; }
    if (dst == src) { set_error("merge: dst and src are the same runtime"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(dst->device));
    if (src->stream != dst->stream) HIP_TRY(hipStreamSynchronize(src->stream));
    single_begin(dst, dst->merge_span);
    launch_merge(dst->d_count, dst->d_key, dst->d_steps, src->d_count, src->d_key, src->d_steps, dst->npix,
                 dst->d_scalars, dst->stream);
    single_end(dst, dst->merge_span, dst->merge_timed);
    HIP_TRY(hipGetLastError());
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_synchronize(sar_runtime* rt) try {
    if (!rt) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    if (rt->copy_stream) HIP_TRY(hipStreamSynchronize(rt->copy_stream));  // the read-backs of async frames
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_dims(const sar_runtime* rt, uint32_t* width, uint32_t* height) try {
    if (!rt || !width || !height) return SAR_ERR_INVALID;
    *width = rt->W;
    *height = rt->H;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_stream(sar_runtime* rt, void* hip_stream) try {
    if (!rt) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    if (rt->copy_stream) HIP_TRY(hipStreamSynchronize(rt->copy_stream));
    if (rt->upload_stream) HIP_TRY(hipStreamSynchronize(rt->upload_stream));
    rt->own_stream.release();
    rt->stream = static_cast<hipStream_t>(hip_stream);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_get_copy_stream(sar_runtime* rt, void** hip_stream_out) try {
    if (!rt || !hip_stream_out) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    if (!rt->copy_stream) {
        HIP_TRY(rt->own_copy_stream.ensure(hipStreamNonBlocking));
        rt->copy_stream = rt->own_copy_stream;
    }
    *hip_stream_out = rt->copy_stream;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_copy_stream(sar_runtime* rt, void* hip_stream) try {
    if (!rt || !hip_stream) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    if (rt->copy_stream) HIP_TRY(hipStreamSynchronize(rt->copy_stream));
    rt->own_copy_stream.release();
    rt->copy_stream = static_cast<hipStream_t>(hip_stream);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_get_stream(const sar_runtime* rt, void** hip_stream_out) try {
    if (!rt || !hip_stream_out) return SAR_ERR_INVALID;
    *hip_stream_out = rt->stream;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

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
                   rt->expo_on == lead->expo_on && rt->crange_mode == lead->crange_mode &&
                   (lead->expo_on || (std::memcmp(&c->brightness_offset, &c0->brightness_offset, sizeof(double)) == 0 &&
                                      std::memcmp(&c->brightness_factor, &c0->brightness_factor, sizeof(double)) == 0)) &&
                   std::memcmp(c->palette_rgb, c0->palette_rgb, sizeof(double) * 3 * c0->palette_len) == 0;
        };
        // (a runtime listed twice in one exposure run would give two frames of the launch ONE select scratch: with the mode on, a run
        // ends before a runtime it already holds — the repeat starts the next run, behind this one on the same stream. The colour
        // range's select has one scratch per runtime as well)
        auto fresh = [&](uint32_t i) {
            if (!lead->expo_on && lead->crange_mode != kCrMeasure) return true;
            for (uint32_t j = first; j < i; ++j)
                if (rts[j] == rts[i]) return false;
            return true;
        };
        const uint32_t m = c0->render_kind == SAR_RENDER_GAS && !lead->timing ? run_length(n, rts, first, [&](uint32_t i) {
            return !rts[i]->timing && same_colours(cfgs[i], rts[i]) && fresh(i);  // (a timed runtime records its own span)
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
    if (rt->copy_in_flight) {  // an async frame's read-back still reads d_rgba
        HIP_TRY(hipStreamWaitEvent(rt->stream, rt->img_events[(rt->img_next - 1) % 8], 0));
        rt->copy_in_flight = false;
    }
    SAR_TRY(do_colorize(cfg, rt, rt->d_rgba));
    HIP_TRY(hipMemcpyAsync(rgba_out_host, rt->d_rgba, static_cast<size_t>(rt->npix) * 8, hipMemcpyDeviceToHost, rt->stream));
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
    HIP_TRY(hipMemcpyAsync(out, rt->d_expo_rec, sizeof(sar_exposure), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_exposure(sar_runtime* rt, const sar_exposure_params* params) try {
    if (params) SAR_TRY(validate_exposure(params));  // (first: bad parameters are refused whatever the handle)
    if (!rt) { set_error("sar_runtime_set_exposure: runtime is NULL"); return SAR_ERR_INVALID; }
    if (params) rt->expo_params = *params;
    rt->expo_on = params != nullptr;
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
    HIP_TRY(hipMemcpyAsync(out, rt->d_crange_rec, sizeof(sar_color_range), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_color_range(sar_runtime* rt, const sar_color_range_params* params) try {
    if (params) SAR_TRY(validate_color_range(params));  // (first: bad parameters are refused whatever the handle)
    if (!rt) { set_error("sar_runtime_set_color_range: runtime is NULL"); return SAR_ERR_INVALID; }
    if (params) rt->crange_params = *params;
    if (params) rt->crange_mode = kCrMeasure;
    else if (rt->crange_mode == kCrMeasure) rt->crange_mode = kCrOff;  // (NULL ends the mode, not a hold)
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
        if (rt->crange_mode == kCrHold) rt->crange_mode = kCrOff;
        return SAR_OK;
    }
    HIP_TRY(hipSetDevice(rt->device));
    SAR_TRY(ensure_select(rt, rt->d_crange, kCrScratchWords, rt->d_crange_rec, 2));
    // (behind every colorize that still reads the record it replaces; the wait: `range` is the caller's)
    HIP_TRY(hipMemcpyAsync(rt->d_crange_rec.get() + 1, range, sizeof(sar_color_range), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->crange_mode = kCrHold;
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

int sar_runtime_extent(const sar_config* cfg, sar_runtime* rt, uint32_t n_jobs, uint64_t iters_per_job,
                       const double* starts_xyz_host, double* out12) try {
    if (!cfg || !rt || !out12 || n_jobs == 0) return SAR_ERR_INVALID;
    SAR_TRY(sar_config_validate(cfg));
    HIP_TRY(hipSetDevice(rt->device));
    std::vector<double> soa(static_cast<size_t>(n_jobs) * 3);
    for (uint32_t k = 0; k < n_jobs; ++k) {
        double p0[3];
        if (starts_xyz_host) std::memcpy(p0, starts_xyz_host + 3 * static_cast<size_t>(k), sizeof(p0));
        else rt->rng.start_point(p0);  // :748
        soa[k] = p0[0];
        soa[n_jobs + static_cast<size_t>(k)] = p0[1];
        soa[2 * static_cast<size_t>(n_jobs) + k] = p0[2];
    }
    const uint32_t blocks = (n_jobs + 255u) / 256u;
    DevBuf<double> d_starts, d_out;
    HIP_TRY(d_starts.grow(nullptr, soa.size()));
    if (d_out.grow(nullptr, static_cast<size_t>(blocks) * 12) != hipSuccess) {
        set_error("out of device memory");
        return SAR_ERR_OOM;
    }
    MapParams mp;
    std::memset(&mp, 0, sizeof(mp));
    fill_map_params(*cfg, mp);
    std::vector<double> part(static_cast<size_t>(blocks) * 12);
    hipError_t e = hipMemcpyAsync(d_starts, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream);
    if (e == hipSuccess) {
        launch_extent(mp, d_starts, n_jobs, iters_per_job, d_out, rt->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(part.data(), d_out, part.size() * sizeof(double), hipMemcpyDeviceToHost, rt->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(rt->stream);
    d_starts.release();
    d_out.release();
    if (e != hipSuccess) { set_error("sar_runtime_extent: %s", hipGetErrorString(e)); return SAR_ERR_HIP; }
    for (int k = 0; k < 12; ++k) {
        double v = part[k];
        for (uint32_t b = 1; b < blocks; ++b) {
            const double o = part[static_cast<size_t>(b) * 12 + k];
            v = (k & 1) ? (o > v ? o : v) : (o < v ? o : v);
        }
        out12[k] = v;
    }
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
    if (rt->copy_in_flight) {  // the last async frame's read-back still reads d_rgba / d_export
        HIP_TRY(hipStreamWaitEvent(rt->stream, rt->img_events[(rt->img_next - 1) % 8], 0));
        rt->copy_in_flight = false;
    }
    SAR_TRY(do_colorize(cfg, rt, rt->d_rgba));
    rt->export_src = rt->d_rgba;
    if (format != SAR_FMT_RGBA16) {
        HIP_TRY(rt->d_export.grow(rt, static_cast<size_t>(rt->npix) * 6));  // largest converted format
        SAR_TRY(sar_image_convert_device(rt, rt->d_rgba, format, rt->d_export));
        rt->export_src = rt->d_export;
    }
    rt->export_bytes = bytes;
    return SAR_OK;
}

// the read-back of that image: on the launch stream, or — the async form — on the copy stream behind an event, so that the next
// frame's kernels do not queue behind 20-30 MB over PCIe (d_rgba / d_export are written again only behind this copy's event)
static int enqueue_read_image(sar_runtime* rt, void* out_host, bool own_copy_stream) {
    if (!out_host || !rt->export_src) { set_error("read-back: NULL output, or no colorized image to read"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    if (!own_copy_stream || rt->readback_inline) {
        HIP_TRY(hipMemcpyAsync(out_host, rt->export_src, rt->export_bytes, hipMemcpyDeviceToHost, rt->stream));
        return SAR_OK;
    }
    if (!rt->copy_stream) {
        HIP_TRY(rt->own_copy_stream.ensure(hipStreamNonBlocking));
        rt->copy_stream = rt->own_copy_stream;
    }
    HIP_TRY(rt->img_ready.ensure(hipEventDisableTiming));
    HIP_TRY(hipEventRecord(rt->img_ready, rt->stream));
    HIP_TRY(hipStreamWaitEvent(rt->copy_stream, rt->img_ready, 0));
    HIP_TRY(hipMemcpyAsync(out_host, rt->export_src, rt->export_bytes, hipMemcpyDeviceToHost, rt->copy_stream));
    return SAR_OK;
}

static int ticket_for_read(sar_runtime* rt, uint64_t* ticket_out) {
    Event& ev = rt->img_events[rt->img_next % 8];
    HIP_TRY(ev.ensure(hipEventDisableTiming));
    HIP_TRY(hipEventRecord(ev, rt->readback_inline ? rt->stream : rt->copy_stream));
    rt->copy_in_flight = !rt->readback_inline;
    *ticket_out = rt->img_next++;
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
    if (!rt || !done_out || ticket >= rt->img_next) { set_error("sar_runtime_image_done: no such ticket"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    const hipError_t e = hipEventQuery(rt->img_events[ticket % 8]);
    if (e != hipSuccess && e != hipErrorNotReady) HIP_TRY(e);
    *done_out = e == hipSuccess ? 1 : 0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_wait_image(sar_runtime* rt, uint64_t ticket) try {
    if (!rt || ticket >= rt->img_next) { set_error("sar_runtime_wait_image: no such ticket"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipEventSynchronize(rt->img_events[ticket % 8]));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

// Page-locked host memory for the read-backs. hipHostMalloc page-locks 4 KiB page by 4 KiB page (1.0-1.4 ms per 21.6 MB image on
// most boxes of the pool, 3-4 on some: 33-100 ms of a sweep's set-up); an anonymous mapping that asks for transparent huge pages,
// touched once and then registered with the HIP runtime, is the same memory to a copy and takes 0.4 of the time (tools/ubench/
// alloc_cost.py: 352 MiB in 20 ms against 48-55). Large blocks go that way; what fails on the way falls back to hipHostMalloc.
}  // extern "C" (an unnamed namespace inside it gives its variables C names with EXTERNAL linkage: two copies of this library in
   // one process — the product and the test-suite's hooks build, loaded RTLD_GLOBAL — would share them, and construct and destroy
   // them twice)

namespace {
struct MappedBlock { void* p; size_t bytes; };
std::mutex g_mapped_mu;
std::vector<MappedBlock> g_mapped;
constexpr size_t kHugePage = 2u << 20;

size_t mapped_len(size_t bytes) { return (bytes + kHugePage - 1) & ~(kHugePage - 1); }

// An anonymous mapping of len bytes on a 2 MiB boundary, asked to be huge pages, every page touched — no HIP call in here.
char* map_and_touch(size_t len) {
    // (over-map by one huge page so that the block can start on a 2 MiB boundary: only aligned ranges get huge pages)
    char* raw = static_cast<char*>(mmap(nullptr, len + kHugePage, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0));
    if (raw == MAP_FAILED) return nullptr;
    char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(raw) + kHugePage - 1) & ~static_cast<uintptr_t>(kHugePage - 1));
    if (p > raw) munmap(raw, static_cast<size_t>(p - raw));
    if (p + len < raw + len + kHugePage) munmap(p + len, static_cast<size_t>(raw + len + kHugePage - (p + len)));
    madvise(p, len, MADV_HUGEPAGE);                       // (advice: refused or unavailable, the pages are small ones)
    for (size_t off = 0; off < len; off += 4096) p[off] = 0;  // first touch: the pages exist before they are locked
    return p;
}

// Blocks announced by sar_host_reserve: helper threads map and touch them ahead of their sar_host_alloc (zeroing fresh pages is
// nine tenths of what page-locking an image costs, and needs no HIP call: the helpers never contend for the HIP runtime's locks,
// which is what made page-locking itself on a helper thread slower — profiles/dead_ends.md, Round 6).
struct HostReserve {
    static constexpr int kHelpers = 3;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<char*> ready;   // mapped + touched, not registered
    size_t len = 0;            // their size (a multiple of 2 MiB)
    uint32_t pending = 0;      // blocks nobody has started on yet
    int working = 0;           // helper threads alive
    std::vector<std::thread> helpers;
    ~HostReserve() { drop(); }
    void drop() {
        std::unique_lock<std::mutex> lock(mu);
        pending = 0;
        cv.wait(lock, [&] { return working == 0; });
        for (char* p : ready) munmap(p, len);
        ready.clear();
        lock.unlock();
        for (std::thread& t : helpers)
            if (t.joinable()) t.join();
        helpers.clear();
    }
    void work(uint64_t generation_len) {
        std::unique_lock<std::mutex> lock(mu);
        while (pending) {
            --pending;
            lock.unlock();
            char* p = map_and_touch(generation_len);
            lock.lock();
            if (!p) { pending = 0; break; }
            ready.push_back(p);
            cv.notify_all();
        }
        --working;
        cv.notify_all();
    }
    // a touched block of `want` bytes, or nullptr (none announced: the caller maps its own)
    char* take(size_t want) {
        std::unique_lock<std::mutex> lock(mu);
        if (want != len) return nullptr;
        cv.wait(lock, [&] { return !ready.empty() || working == 0; });
        if (ready.empty()) return nullptr;
        char* p = ready.front();
        ready.pop_front();
        return p;
    }
} g_reserve;

void* map_and_register(size_t bytes) {
    const size_t len = mapped_len(bytes);
    char* p = g_reserve.take(len);
    if (!p) p = map_and_touch(len);
    if (!p) return nullptr;
    if (hipHostRegister(p, len, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();
        munmap(p, len);
        return nullptr;
    }
    std::lock_guard<std::mutex> lock(g_mapped_mu);
    g_mapped.push_back({p, len});
    return p;
}
}  // namespace

extern "C" {

int sar_host_reserve(size_t bytes, uint32_t count) try {
    static std::mutex one_at_a_time;                    // (announcements from several threads follow each other)
    std::lock_guard<std::mutex> serial(one_at_a_time);
    g_reserve.drop();                                   // what an earlier announcement left goes first (its helpers have ended)
    if (bytes < (4u << 20) || count == 0) return SAR_OK;  // (smaller blocks are hipHostMalloc'ed: nothing to prepare)
    if (count > 4096u) { set_error("sar_host_reserve: at most 4096 blocks"); return SAR_ERR_RANGE; }
    std::lock_guard<std::mutex> lock(g_reserve.mu);
    g_reserve.len = mapped_len(bytes);
    g_reserve.pending = count;
    const size_t len = g_reserve.len;
    const int n = count < static_cast<uint32_t>(HostReserve::kHelpers) ? static_cast<int>(count) : HostReserve::kHelpers;
    g_reserve.working = n;
    for (int i = 0; i < n; ++i) g_reserve.helpers.emplace_back([len] { g_reserve.work(len); });
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_host_alloc(size_t bytes, void** out) try {
    if (!out || bytes == 0) { set_error("sar_host_alloc: NULL output or zero size"); return SAR_ERR_INVALID; }
#ifndef SAR_EXPERIMENT_HOST_ALLOC_PLAIN  // (A/B timing only)
    if (bytes >= (4u << 20)) {
        *out = map_and_register(bytes);
        if (*out) return SAR_OK;
    }
#endif
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocDefault));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_host_free(void* p) try {
    if (!p) return SAR_OK;
    size_t mapped = 0;
    {
        std::lock_guard<std::mutex> lock(g_mapped_mu);
        for (size_t k = 0; k < g_mapped.size(); ++k)
            if (g_mapped[k].p == p) { mapped = g_mapped[k].bytes; g_mapped.erase(g_mapped.begin() + static_cast<long>(k)); break; }
    }
    if (mapped) {
        HIP_TRY(hipHostUnregister(p));
        munmap(p, mapped);
        return SAR_OK;
    }
    HIP_TRY(hipHostFree(p));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_count(sar_runtime* rt, uint32_t* out_host) try {
    if (!rt || !out_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipMemcpyAsync(out_host, rt->d_count, static_cast<size_t>(rt->npix) * 4, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_steps(sar_runtime* rt, double* out_host) try {
    if (!rt || !out_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipMemcpyAsync(out_host, rt->d_steps, static_cast<size_t>(rt->npix) * 8, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_zbuf(sar_runtime* rt, float* out_host) try {
    if (!rt || !out_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(rt->d_ztmp.grow(rt, rt->npix));
    launch_zbuf_out(rt->d_key, rt->d_ztmp, rt->npix, rt->stream);
    HIP_TRY(hipMemcpyAsync(out_host, rt->d_ztmp, static_cast<size_t>(rt->npix) * 4, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_max(sar_runtime* rt, uint32_t* out_max) try {
    if (!rt || !out_max) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    uint32_t sc[SC_COUNT];
    HIP_TRY(hipMemcpyAsync(sc, rt->d_scalars, sizeof(sc), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    *out_max = sc[SC_WRAP] ? 0xFFFFFFFFu : sc[SC_MAX];
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_load(sar_runtime* rt, const uint32_t* count_host, const double* steps_host,
                     const float* zbuf_host, uint32_t max) try {
    if (!rt || !count_host || !steps_host || !zbuf_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(rt->d_ztmp.grow(rt, rt->npix));
    HIP_TRY(hipMemcpyAsync(rt->d_count, count_host, static_cast<size_t>(rt->npix) * 4, hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(rt->d_steps, steps_host, static_cast<size_t>(rt->npix) * 8, hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(rt->d_ztmp, zbuf_host, static_cast<size_t>(rt->npix) * 4, hipMemcpyHostToDevice, rt->stream));
    launch_zbuf_in(rt->d_ztmp, rt->d_key, rt->npix, rt->stream);
    SAR_TRY(clear_hints(rt));
    uint32_t sc[SC_COUNT] = {0};
    sc[SC_MAX] = max;
    HIP_TRY(hipMemcpyAsync(rt->d_scalars, sc, sizeof(sc), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_colorize_range_device(const sar_config* cfg, sar_runtime* rt, uint32_t first_px, uint32_t n_px, void* rgba_out_dev) try {
    SAR_TRY(check_cfg_matches(cfg, rt));
    if (!rgba_out_dev) return SAR_ERR_INVALID;
    return colorize_range(cfg, rt, first_px, n_px, rgba_out_dev, true);
} catch (...) { return sar::abi_caught(); }

// ---- measurement --------------------------------------------------------------------------------------

int sar_runtime_enable_timing(sar_runtime* rt, int enabled) try {
    if (!rt) return SAR_ERR_INVALID;
    rt->timing = enabled != 0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_last_timing(sar_runtime* rt, sar_timing* out) try {
    if (!rt || !out) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    std::memset(out, 0, sizeof(*out));
    float ms = 0.f;
    for (size_t k = 0; k < rt->iter_used; ++k)
        if (hipEventElapsedTime(&ms, rt->iter_spans[k].a, rt->iter_spans[k].b) == hipSuccess) out->iterate_ms += ms;
    for (size_t k = 0; k < rt->fold_used; ++k)
        if (hipEventElapsedTime(&ms, rt->fold_spans[k].a, rt->fold_spans[k].b) == hipSuccess) out->resolve_ms += ms;
    for (size_t k = 0; k < rt->warm_used; ++k)
        if (hipEventElapsedTime(&ms, rt->warm_spans[k].a, rt->warm_spans[k].b) == hipSuccess) out->warmup_ms += ms;
    if (rt->colorize_timed && hipEventElapsedTime(&ms, rt->colorize_span.a, rt->colorize_span.b) == hipSuccess) out->colorize_ms = ms;
    if (rt->merge_timed && hipEventElapsedTime(&ms, rt->merge_span.a, rt->merge_span.b) == hipSuccess) out->merge_ms = ms;
    out->iterate_launches = static_cast<uint32_t>(rt->iter_used);
    if (rt->d_nan_count) {  // cumulative statistic of the binned path; cleared by reading
        unsigned long long sent = 0, passed = 0;
        HIP_TRY(hipMemcpy(&sent, rt->d_nan_count + 1, sizeof(sent), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(rt->d_nan_count + 1, 0, sizeof(sent)));
        HIP_TRY(hipMemcpy(&passed, rt->d_nan_count + 14, sizeof(passed), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(rt->d_nan_count + 14, 0, sizeof(passed)));
        out->depth_candidates = passed;
#ifdef SAR_EXPERIMENT_PROF
        unsigned long long seg[11];
        HIP_TRY(hipMemcpy(seg, rt->d_nan_count + 2, sizeof(seg), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(rt->d_nan_count + 2, 0, sizeof(seg)));
        const double tot = static_cast<double>(seg[0] + seg[1] + seg[2] + seg[3]);
        if (tot > 0)
            std::fprintf(stderr, "[prof] wave-cycles: map+projection %.1f%%  place_visit %.1f%%  depth %.1f%%  stores+requests %.1f%%  (total %.3g)\n",
                         100. * seg[0] / tot, 100. * seg[1] / tot, 100. * seg[2] / tot, 100. * seg[3] / tot, tot);
        const double ptot = static_cast<double>(seg[4] + seg[5]);
        double ctot = 0;
        for (int i = 6; i < 11; ++i) ctot += static_cast<double>(seg[i]);
        if (ptot > 0 && ctot > 0)
            std::fprintf(stderr, "[prof-split] producer: map+projection+hand-over %.1f%%  barrier %.1f%% (total %.4g) | consumer: barrier %.1f%%  hand-over read %.1f%%  "
                                 "place_visit %.1f%%  depth settle %.1f%%  slot+hint request %.1f%% (total %.4g)\n",
                         100. * seg[4] / ptot, 100. * seg[5] / ptot, ptot, 100. * seg[6] / ctot, 100. * seg[7] / ctot, 100. * seg[8] / ctot,
                         100. * seg[9] / ctot, 100. * seg[10] / ctot, ctot);
        unsigned long long dp[3];
        HIP_TRY(hipMemcpy(dp, rt->d_nan_count + 13, sizeof(dp), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset(rt->d_nan_count + 13, 0, sizeof(unsigned long long)));
        HIP_TRY(hipMemset(rt->d_nan_count + 15, 0, sizeof(unsigned long long)));
        if (ctot > 0)
            std::fprintf(stderr, "[prof-depth] of the consumer's time (memory drained at each mark): stage 2 (key wait, atomic, hint store, drain) %.1f%%  "
                                 "stage 1 (compare, key load, drain) %.1f%%\n", 100. * dp[0] / ctot, 100. * dp[2] / ctot);
#endif
        out->depth_atomics = sent;
    }
    out->iterations_counted = rt->last_iterations;
    if (rt->timing_accumulate) {
        rt->last_iterations = 0;
        rt->iter_used = 0;
        rt->fold_used = 0;
        rt->warm_used = 0;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_option(sar_runtime* rt, const char* name, uint64_t value) try {
    if (!rt || !name) return SAR_ERR_INVALID;
    const uint32_t v = static_cast<uint32_t>(value);
    if (!std::strcmp(name, "block_threads")) {
        if (v == 0) { rt->block_threads = kDefaultBlock; return SAR_OK; }
        if (v % 64 || v > 256) { set_error("block_threads must be 64, 128, 192 or 256"); return SAR_ERR_INVALID; }
        rt->block_threads = v;
    } else if (!std::strcmp(name, "checkpoint_stride")) {
        rt->ckpt_stride = v ? v : kDefaultCkptStride;
    } else if (!std::strcmp(name, "hint_bits")) {
        if (v && v != 16 && v != 32) { set_error("hint_bits must be 16 or 32"); return SAR_ERR_INVALID; }
        rt->hint_bits = v;
    } else if (!std::strcmp(name, "split_waves")) {
        if (v > 2) { set_error("split_waves must be 0, 1 or 2"); return SAR_ERR_INVALID; }
        rt->split_waves = v;
    } else if (!std::strcmp(name, "search_chunk")) {
        if (value > kMaxSearchChunk) { set_error("search_chunk must be at most 2^30 candidates"); return SAR_ERR_INVALID; }
        rt->search_chunk = v;
    } else if (!std::strcmp(name, "plane_chunk")) {
        if (value > kMaxPlaneChunk) { set_error("plane_chunk must be at most 2^30 pixels"); return SAR_ERR_INVALID; }
        rt->plane_chunk = v;
    } else if (!std::strcmp(name, "gallery_chunk")) {
        if (value > kMaxGalleryChunk) { set_error("gallery_chunk must be at most 2^16 tiles"); return SAR_ERR_INVALID; }
        rt->gallery_chunk = v;
    } else if (!std::strcmp(name, "orbit_chunk")) {
        if (value > kMaxOrbitChunk) { set_error("orbit_chunk must be at most 2^16 columns"); return SAR_ERR_INVALID; }
        rt->orbit_chunk = v;
    } else if (!std::strcmp(name, "corr_chunk")) {
        if (value > kMaxCorrChunk) { set_error("corr_chunk must be at most 2^30 workgroups"); return SAR_ERR_INVALID; }
        rt->corr_chunk = v;
    } else if (!std::strcmp(name, "box_chunk")) {
        if (value > kBoxMaxGridY) { set_error("box_chunk must be at most 65535 sets"); return SAR_ERR_INVALID; }
        rt->box_chunk = v;
    } else if (!std::strcmp(name, "box_slots")) {
        if (value > kBoxMaxSlots || (value & (value - 1u)) || value == 1u) { set_error("box_slots must be 0 (automatic) or a power of two from 2 to 2^24"); return SAR_ERR_INVALID; }
        rt->box_slots = v;
    } else if (!std::strcmp(name, "basin_chunk")) {
        if (value > kMaxBasinChunk) { set_error("basin_chunk must be at most 2^30 pixels"); return SAR_ERR_INVALID; }
        rt->basin_chunk = v;
    } else if (!std::strcmp(name, "period_chunk")) {
        if (value > kMaxPeriodChunk) { set_error("period_chunk must be at most 2^30 pixels"); return SAR_ERR_INVALID; }
        rt->period_chunk = v;
    } else if (!std::strcmp(name, "cycles_chunk")) {
        if (value > kMaxCyclesChunk) { set_error("cycles_chunk must be at most 2^30 lanes"); return SAR_ERR_INVALID; }
        rt->cycles_chunk = v;
    } else if (!std::strcmp(name, "density_tile")) {
        if (v && v != 8 && v != 16 && v != 32) { set_error("density_tile must be 8, 16 or 32"); return SAR_ERR_INVALID; }
        rt->density_tile = v;
    } else if (!std::strcmp(name, "tail_overlap")) {
        if (v > 1) { set_error("tail_overlap must be 0 or 1"); return SAR_ERR_INVALID; }
        rt->tail_overlap = v;
    } else if (!std::strcmp(name, "timing_accumulate")) {
        rt->timing_accumulate = v != 0;
        rt->last_iterations = 0;
        rt->iter_used = 0;
        rt->fold_used = 0;
        rt->warm_used = 0;
    } else {
        set_error("unknown option '%s' (the A/B and test options live behind sar_runtime_set_test_option: include/sar_test_hooks.h)", name);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
