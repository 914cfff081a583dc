// sar_runtime.cpp — the C ABI of the Runtime (include/sar.h): life cycle and frame groups, the ln table, reset, merge, streams,
// extent, load and the read-back accessors, timing and the tuning options. Colorize, image export and their read-back are
// sar_colorize.cpp, the page-locked allocator sar_hostmem.cpp, the render call itself sar_render.cpp, its planning sar_plan.cpp, the
// multi-device ParallelRenderer sar_multi.cpp, the exchange of the one-process-per-GPU path sar_exchange.cpp.
//
// Host logic only (allocation, argument blocks, stream ordering); all arithmetic on image data happens in the kernel files
// (sar_iterate.hip, sar_accumulate.hip, sar_image.hip, sar_select.hip). There is no CPU fallback: without a HIP device every entry point
// that touches a runtime returns SAR_ERR_NO_DEVICE.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "sar_plan.hpp"
#include "sar_search.hpp"

using namespace sar;

int sar::check_cfg_matches(const sar_config* cfg, const sar_runtime* rt) {
    SAR_TRY(validate(cfg));
    if (!rt) { set_error("runtime is NULL"); return SAR_ERR_INVALID; }
    if (cfg->width != rt->W || cfg->height != rt->H) {
        set_error("config is %ux%u but the runtime holds %ux%u", cfg->width, cfg->height, rt->W, rt->H);
        return SAR_ERR_DIM_MISMATCH;
    }
    return SAR_OK;
}

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
    rt->rb.d_rgba.release();
    rt->rb.d_export.release();
    rt->d_ztmp.release();
    rt->hints.d_zhint.release();
    rt->rb.export_src = nullptr;
    rt->copies = 0;
    rt->W = w;
    rt->H = h;
    rt->npix = static_cast<uint32_t>(npix64);
    return SAR_OK;
}

// Runtime::reset of m runtimes on rts[0]'s device, stream and image size in ONE launch. The hints go with the buffers (Hints: what they
// are cleared to, and which of them); from here on they count as empty.
int do_reset(uint32_t m, sar_runtime* const* rts) {
    ResetBatch t;
    std::memset(&t, 0, sizeof(t));
    for (uint32_t i = 0; i < m; ++i) {
        sar_runtime* rt = rts[i];
        const size_t entries = rt->hints.entries_used(rt->npix);
        t.f[i] = {rt->d_count, rt->d_key, rt->d_steps, rt->d_scalars, static_cast<uint32_t*>(rt->hints.d_zhint.get()),
                  static_cast<uint32_t>(rt->hints.zhint_bytes == 4 ? entries : entries / 2u) /* (kHintStride is even) */, rt->hints.empty_value()};
        rt->hints.mark_cleared();
    }
    launch_reset(t, m, rts[0]->npix, rts[0]->stream);
    HIP_TRY(hipGetLastError());
    return SAR_OK;
}

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
        rt->rb.copy_stream = rt->group->copy_stream;
    } else {
        if (rt->own_stream.ensure(hipStreamNonBlocking) != hipSuccess) { set_error("hipStreamCreate failed"); return SAR_ERR_HIP; }
        rt->stream = rt->own_stream;
    }
    if (rt->starts.starts_copied.ensure(hipEventDisableTiming) != hipSuccess) return SAR_ERR_HIP;
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

// `bytes` of device memory into the caller's buffer, behind what the runtime's stream holds; waits
int read_back(sar_runtime* rt, void* out_host, const void* src, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(out_host, src, bytes, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
}

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

}  // namespace

sar_runtime::~sar_runtime() {
    // (a borrowed copy stream as well: a read-back may still read d_export)
    for (hipStream_t s : {stream, static_cast<hipStream_t>(side), rb.copy_stream, static_cast<hipStream_t>(upload_stream)})
        if (s) hipStreamSynchronize(s);
    release_ln_lut(this);
}

namespace {

// the stable options (include/sar.h): {name, field, rule, wide, a, b, size of the set, the set, refusal}
constexpr OptionRule kOptions[] = {
    {"block_threads", &Options::block_threads, OptionRule::kOneOf, false, 0, 0, 5, {0, 64, 128, 192, 256}, "block_threads must be 64, 128, 192 or 256"},
    {"checkpoint_stride", &Options::ckpt_stride, OptionRule::kAny, false, 0, 0, 0, {}, nullptr},
    {"hint_bits", &Options::hint_bits, OptionRule::kOneOf, false, 0, 0, 3, {0, 16, 32}, "hint_bits must be 16 or 32"},
    {"split_waves", &Options::split_waves, OptionRule::kAtMost, false, 2, 0, 0, {}, "split_waves must be 0, 1 or 2"},
    {"search_chunk", &Options::search_chunk, OptionRule::kAtMost, true, kMaxSearchChunk, 0, 0, {}, "search_chunk must be at most 2^30 candidates"},
    {"plane_chunk", &Options::plane_chunk, OptionRule::kAtMost, true, kMaxPlaneChunk, 0, 0, {}, "plane_chunk must be at most 2^30 pixels"},
    {"gallery_chunk", &Options::gallery_chunk, OptionRule::kAtMost, true, kMaxGalleryChunk, 0, 0, {}, "gallery_chunk must be at most 2^16 tiles"},
    {"orbit_chunk", &Options::orbit_chunk, OptionRule::kAtMost, true, kMaxOrbitChunk, 0, 0, {}, "orbit_chunk must be at most 2^16 columns"},
    {"corr_chunk", &Options::corr_chunk, OptionRule::kAtMost, true, kMaxCorrChunk, 0, 0, {}, "corr_chunk must be at most 2^30 workgroups"},
    {"box_chunk", &Options::box_chunk, OptionRule::kAtMost, true, kBoxMaxGridY, 0, 0, {}, "box_chunk must be at most 65535 sets"},
    {"box_slots", &Options::box_slots, OptionRule::kPow2, true, 2, kBoxMaxSlots, 0, {}, "box_slots must be 0 (automatic) or a power of two from 2 to 2^24"},
    {"basin_chunk", &Options::basin_chunk, OptionRule::kAtMost, true, kMaxBasinChunk, 0, 0, {}, "basin_chunk must be at most 2^30 pixels"},
    {"period_chunk", &Options::period_chunk, OptionRule::kAtMost, true, kMaxPeriodChunk, 0, 0, {}, "period_chunk must be at most 2^30 pixels"},
    {"cycles_chunk", &Options::cycles_chunk, OptionRule::kAtMost, true, kMaxCyclesChunk, 0, 0, {}, "cycles_chunk must be at most 2^30 lanes"},
    {"density_tile", &Options::density_tile, OptionRule::kOneOf, false, 0, 0, 4, {0, 8, 16, 32}, "density_tile must be 8, 16 or 32"},
    {"volume_chunk", &Options::volume_chunk, OptionRule::kAtMost, true, kMaxVolumeChunk, 0, 0, {}, "volume_chunk must be at most 2^24 jobs"},
    {"volume_steps", &Options::volume_steps, OptionRule::kAtMost, true, kMaxVolumeSteps, 0, 0, {}, "volume_steps must be at most 2^24 iterations"},
    {"tail_overlap", &Options::tail_overlap, OptionRule::kAtMost, false, 1, 0, 0, {}, "tail_overlap must be 0 or 1"},
    {"timing_accumulate", nullptr, OptionRule::kCustom, false, 0, 0, 0, {}, nullptr},  // (Timing's, and it restarts the spans)
};

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
        probe.opt = Options();  // (the plan of a runtime with default options)
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
        // (one allocation per runtime, not one for the group: see Slab; beyond 4 GiB the buffers stay separate)
        if (dev_bytes > (4ull << 30) || rt->slab.sub.grow(nullptr, dev_bytes) != hipSuccess) (void)hipGetLastError();
        if (g->hslab) { rt->slab.hsub = g->hslab + host_bytes * i; rt->slab.hsub_bytes = host_bytes; }
        rt->hints.single_hint_array = n >= 3u;  // (batches of three frames or more deal their frames to the XCDs)
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
    rt->volume.drop();  // (a held volume is the old size's)
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
    dst->tm.single_begin(dst->tm.merge_span, dst->stream);
    launch_merge(dst->d_count, dst->d_key, dst->d_steps, src->d_count, src->d_key, src->d_steps, dst->npix,
                 dst->d_scalars, dst->stream);
    dst->tm.single_end(dst->tm.merge_span, dst->tm.merge_timed, dst->stream);
    HIP_TRY(hipGetLastError());
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_synchronize(sar_runtime* rt) try {
    if (!rt) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    if (rt->rb.copy_stream) HIP_TRY(hipStreamSynchronize(rt->rb.copy_stream));  // the read-backs of async frames
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
    if (rt->rb.copy_stream) HIP_TRY(hipStreamSynchronize(rt->rb.copy_stream));
    if (rt->upload_stream) HIP_TRY(hipStreamSynchronize(rt->upload_stream));
    rt->own_stream.release();
    rt->stream = static_cast<hipStream_t>(hip_stream);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_get_copy_stream(sar_runtime* rt, void** hip_stream_out) try {
    if (!rt || !hip_stream_out) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    SAR_TRY(rt->rb.ensure_copy_stream());
    *hip_stream_out = rt->rb.copy_stream;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_copy_stream(sar_runtime* rt, void* hip_stream) try {
    if (!rt || !hip_stream) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    if (rt->rb.copy_stream) HIP_TRY(hipStreamSynchronize(rt->rb.copy_stream));
    rt->rb.own_copy_stream.release();
    rt->rb.copy_stream = static_cast<hipStream_t>(hip_stream);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_get_stream(const sar_runtime* rt, void** hip_stream_out) try {
    if (!rt || !hip_stream_out) return SAR_ERR_INVALID;
    *hip_stream_out = rt->stream;
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

int sar_runtime_count(sar_runtime* rt, uint32_t* out_host) try {
    if (!rt || !out_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    return read_back(rt, out_host, rt->d_count, static_cast<size_t>(rt->npix) * 4);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_steps(sar_runtime* rt, double* out_host) try {
    if (!rt || !out_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    return read_back(rt, out_host, rt->d_steps, static_cast<size_t>(rt->npix) * 8);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_zbuf(sar_runtime* rt, float* out_host) try {
    if (!rt || !out_host) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(rt->d_ztmp.grow(rt, rt->npix));
    launch_zbuf_out(rt->d_key, rt->d_ztmp, rt->npix, rt->stream);
    return read_back(rt, out_host, rt->d_ztmp, static_cast<size_t>(rt->npix) * 4);
} catch (...) { return sar::abi_caught(); }

int sar_runtime_max(sar_runtime* rt, uint32_t* out_max) try {
    if (!rt || !out_max) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    uint32_t sc[SC_COUNT];
    SAR_TRY(read_back(rt, sc, rt->d_scalars, sizeof(sc)));
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
    SAR_TRY(rt->hints.clear(rt->npix, rt->stream));
    uint32_t sc[SC_COUNT] = {0};
    sc[SC_MAX] = max;
    HIP_TRY(hipMemcpyAsync(rt->d_scalars, sc, sizeof(sc), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

// ---- measurement --------------------------------------------------------------------------------------

int sar_runtime_enable_timing(sar_runtime* rt, int enabled) try {
    if (!rt) return SAR_ERR_INVALID;
    rt->tm.timing = enabled != 0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_last_timing(sar_runtime* rt, sar_timing* out) try {
    if (!rt || !out) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    std::memset(out, 0, sizeof(*out));
    float ms = 0.f;
    Timing& tm = rt->tm;
    auto sum = [&ms](const SpanList& l) {
        float total = 0.f;
        for (size_t k = 0; k < l.used; ++k)
            if (hipEventElapsedTime(&ms, l.spans[k].a, l.spans[k].b) == hipSuccess) total += ms;
        return total;
    };
    out->iterate_ms = sum(tm.iter);
    out->resolve_ms = sum(tm.fold);
    out->warmup_ms = sum(tm.warm);
    if (rt->tm.colorize_timed && hipEventElapsedTime(&ms, rt->tm.colorize_span.a, rt->tm.colorize_span.b) == hipSuccess) out->colorize_ms = ms;
    if (rt->tm.merge_timed && hipEventElapsedTime(&ms, rt->tm.merge_span.a, rt->tm.merge_span.b) == hipSuccess) out->merge_ms = ms;
    out->iterate_launches = static_cast<uint32_t>(tm.iter.used);
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
    out->iterations_counted = rt->tm.last_iterations;
    if (tm.timing_accumulate) tm.restart();
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_set_option(sar_runtime* rt, const char* name, uint64_t value) try {
    if (!rt || !name) return SAR_ERR_INVALID;
    int status = SAR_OK;
    const OptionRule* row = set_option_from(kOptions, sizeof(kOptions) / sizeof(kOptions[0]), rt->opt, name, value,
                                            "unknown option '%s' (the A/B and test options live behind sar_runtime_set_test_option: include/sar_test_hooks.h)", status);
    if (status != SAR_OK) return status;
    // what is more than a rule: 0 stands for the default, and a change of mode starts the spans afresh
    if (row->field == &Options::block_threads && rt->opt.block_threads == 0) rt->opt.block_threads = kDefaultBlock;
    if (row->field == &Options::ckpt_stride && rt->opt.ckpt_stride == 0) rt->opt.ckpt_stride = kDefaultCkptStride;
    if (row->kind == OptionRule::kCustom) {  // timing_accumulate
        rt->tm.timing_accumulate = static_cast<uint32_t>(value) != 0;
        rt->tm.restart();
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"

