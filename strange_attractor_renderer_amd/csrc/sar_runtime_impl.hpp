// sar_runtime_impl.hpp — the private layout of sar_runtime: owned buffers and handles, one plain struct per piece of launch state, each
// with the ONE copy of the protocol over its fields, and the few internals of sar_runtime.cpp and sar_colorize.cpp that the multi-device
// ParallelRenderer (sar_multi.cpp) and the analysis entry points (sar_analysis.hpp) build on. Host only; not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "sar_basin.hpp"
#include "sar_box.hpp"
#include "sar_corr.hpp"
#include "sar_cycles.hpp"
#include "sar_density.hpp"
#include "sar_fate.hpp"
#include "sar_flow.hpp"
#include "sar_ftle.hpp"
#include "sar_gallery.hpp"
#include "sar_launch.hpp"
#include "sar_manifold.hpp"
#include "sar_orbit.hpp"
#include "sar_period.hpp"
#include "sar_rqa.hpp"
#include "sar_section.hpp"
#include "sar_spectrum.hpp"
#include "sar_volume.hpp"

struct sar_runtime;

namespace sar {

// Memory of `rt`'s slab (Slab::carve) while that lasts; nullptr when the request does not fit.
void* slab_carve(sar_runtime* rt, bool host, size_t bytes);

template <typename T> struct ElemSize { static constexpr size_t value = sizeof(T); };
template <> struct ElemSize<void> { static constexpr size_t value = 1; };

// An owned buffer of cap() elements of T in device memory (Host = false) or page-locked host memory. grow() takes it from `rt`'s
// slab while that lasts, from hipMalloc / hipHostMalloc otherwise (`flags`: hipExtMallocWithFlags' / hipHostMalloc's). Slab memory
// is never freed here: it goes with the runtime / the group. Contents do not survive a grow.
template <typename T, bool Host>
class Buf {
public:
    Buf() = default;
    Buf(Buf&& o) noexcept { swap(o); }
    Buf& operator=(Buf&& o) noexcept {  // (frees what it held at once)
        release();
        swap(o);
        return *this;
    }
    ~Buf() { release(); }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t cap() const { return cap_; }
    void release() {
        if (p_ && !slab_) (void)(Host ? hipHostFree(p_) : hipFree(p_));
        p_ = nullptr;
        cap_ = 0;
        slab_ = false;
    }
    hipError_t grow(sar_runtime* rt, size_t n, unsigned flags = 0) {
        if (n <= cap_) return hipSuccess;
        release();
        const size_t bytes = n * ElemSize<T>::value;
        void* p = rt ? slab_carve(rt, Host, bytes) : nullptr;
        slab_ = p != nullptr;
        const hipError_t e = slab_ ? hipSuccess
                           : Host  ? hipHostMalloc(&p, bytes, flags)
                           : flags ? hipExtMallocWithFlags(&p, bytes, flags)
                                   : hipMalloc(&p, bytes);
        if (e != hipSuccess) return e;
        p_ = static_cast<T*>(p);
        cap_ = n;
        return hipSuccess;
    }

private:
    void swap(Buf& o) noexcept { std::swap(p_, o.p_); std::swap(cap_, o.cap_); std::swap(slab_, o.slab_); }
    T* p_ = nullptr;
    size_t cap_ = 0;
    bool slab_ = false;
};
template <typename T> using DevBuf = Buf<T, false>;
template <typename T> using HostBuf = Buf<T, true>;

// An owned HIP event / stream: created with `flags` on the first ensure(), destroyed with its owner.
template <typename H, hipError_t (*Create)(H*, unsigned), hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept { std::swap(h_, o.h_); }
    Handle& operator=(Handle&& o) noexcept {
        release();
        std::swap(h_, o.h_);
        return *this;
    }
    ~Handle() { release(); }
    operator H() const { return h_; }
    hipError_t ensure(unsigned flags) { return h_ ? hipSuccess : Create(&h_, flags); }
    void release() {
        if (h_) Destroy(h_);
        h_ = nullptr;
    }

private:
    H h_ = nullptr;
};
using Event = Handle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;

struct Span {
    Event a, b;
};

#ifndef SAR_TAIL_OVERLAP_DEFAULT  // (A/B timing only: a variant build whose runtimes start with the depth resolve beside the accumulate)
#define SAR_TAIL_OVERLAP_DEFAULT 0
#endif

constexpr uint32_t kDefaultBlock = 256;
// iterations between trajectory checkpoints: k_depth_resolve replays on average half a stride per new depth winner (32: the 4096^2
// share -1.3 %, a sequence frame -2 %, 2048^2 -0.5 % against 64; 16 costs the iterate kernel more than the fold saves)
constexpr uint32_t kDefaultCkptStride = 32;
constexpr uint32_t kBatchRing = 8;               // page-locked copies of a batch's argument table in flight
constexpr uint64_t kCkptBytesCap = 24ull << 30;  // checkpoint + record-arena scratch per launch chunk (HBM is 288 GB)

// What the runtimes of a frame group (sar_runtime_new_group: the frames of one batched launch) share — the launch stream, the
// read-back stream and one page-locked allocation for their start points.
struct RuntimeGroup {
    int refs = 0;  // runtimes alive
    int device = 0;
    Stream stream, copy_stream;
    HostBuf<char> hslab;
    ~RuntimeGroup() {
        if (stream) hipStreamSynchronize(stream);
        if (copy_stream) hipStreamSynchronize(copy_stream);
    }
};

}  // namespace sar

#define HIP_TRY(expr)                                                                 \
    do {                                                                              \
        hipError_t e_ = (expr);                                                       \
        if (e_ != hipSuccess) {                                                       \
            sar::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
            return (e_ == hipErrorOutOfMemory) ? SAR_ERR_OOM : SAR_ERR_HIP;           \
        }                                                                             \
    } while (0)

#define SAR_TRY(expr)                    \
    do {                                 \
        int s_ = (expr);                 \
        if (s_ != SAR_OK) return s_;     \
    } while (0)

namespace sar {

// The memory of a runtime of a frame group: `sub` is ONE device allocation of this runtime its buffers are carved from (sized from
// the plan of the frames the group was made for: some twenty hipMalloc / hipFree calls less per runtime — a hipFree costs 0.16 ms;
// one allocation for the WHOLE group, 10 GB, took between 0.3 ms and two seconds on the same box), `hsub` its share of the group's
// page-locked allocation. A bump allocator: 256-byte granules handed out front to back and never reused (what does not fit comes
// from hipMalloc / hipHostMalloc).
constexpr size_t kSlabAlign = 256;
inline size_t slab_round(size_t bytes) { return (bytes + kSlabAlign - 1) & ~(kSlabAlign - 1); }
struct Slab {
    DevBuf<char> sub;
    size_t sub_used = 0;
    char* hsub = nullptr;
    size_t hsub_bytes = 0, hsub_used = 0;
    void* carve(bool host, size_t bytes) {
        char* base = host ? hsub : sub.get();
        const size_t size = host ? hsub_bytes : sub.cap();
        size_t& used = host ? hsub_used : sub_used;
        const size_t need = slab_round(bytes ? bytes : 1);
        if (!base || need > size - used) return nullptr;
        used += need;
        return base + used - need;
    }
};

// Every option of sar_runtime_set_option (include/sar.h) and sar_runtime_set_test_option (include/sar_test_hooks.h) but
// timing_accumulate (Timing's). A default-constructed Options is "a runtime with default options".
struct Options {
    uint32_t block_threads = kDefaultBlock;
    uint32_t ckpt_stride = kDefaultCkptStride;
    uint32_t bins_mode = 0;         // "path": 0 default (binned when eligible), 1 one global atomic per visit, 3 LDS-binned records or an error
    uint32_t debug_chunk_jobs = 0;  // test hook: cap on jobs per launch chunk (0 = none)
    uint64_t max_ordinals = 0;      // test hook: visits one launch may order (0 = 2^32-2); longer jobs run as segments
    uint32_t bin_shift = 0;         // 0 = automatic
    uint32_t bin_interleave = 0;    // 0 = automatic, 1 = bins of consecutive pixels, 2 = interleaved bins (BinMap)
    uint32_t splits = 0;            // 0 = automatic
    uint32_t acc_threads = 0;       // threads per k_bin_accumulate block (0 = automatic)
    uint32_t split_waves = 0;       // 2: the iterate kernel as producer / consumer wave pairs (k_iterate_split) where it applies
    uint32_t acc_lists = 0;         // (bin, wave) lists a lane group of k_bin_accumulate walks at the same time: 1, 4 (0 = automatic)
    uint32_t chunk_records = 0;     // records per chunk: 12 / 20 / 28 / 60 (0 = automatic)
    uint32_t hint_bits = 0;         // 0 = by image size, 16, 32
    uint32_t depth_park = kDepthParkAuto;  // test option: the park window of k_iterate_split's consumer (0, 2, 4, 8); automatic = by hint type
    uint32_t hint_tile = 0;         // 0 = narrow hints of power-of-two-wide images in 8 x 8 tiles, 1 = always row-major
    uint32_t hint_shared = 0;       // 0 = automatic, 1 = one hint array per XCD, 2 = one array for the whole chip
    uint32_t tail_overlap = SAR_TAIL_OVERLAP_DEFAULT;  // 1 = the depth resolve runs on the side stream beside the accumulate kernel
                                    // (measured slower on 2048^2: profiles/r07_tail_overlap_ab.txt), 0 = behind it on the launch stream
    uint32_t chunk_ahead = 0;       // 2 = a call of several launch chunks does not run its next chunk's warm-up ahead (A/B)
    uint32_t readback_inline = 0;   // 1 = async read-backs stay on the launch stream (A/B)
    uint32_t batch_starts = 0;      // how a batched launch gets its start points: 0 = the warm-up kernel reads the page-locked staging
                                    // buffer itself (no copy), 1 = copied on the upload stream, 2 = copied on the launch stream
    uint32_t batch_warm = 0;        // the warm-up of a batched launch: 0 = two phases when the last launch lost a tenth of its jobs, 1 = one phase, 2 = two
    uint32_t batch_chain = 0;       // 1 = the iterate kernels of this device's batches are NOT chained one behind the other (A/B)
    uint32_t batch_xcd = 0;         // 1 = the frames of a batch are NOT dealt to the XCDs (every frame runs on all eight: A/B)
    uint32_t search_chunk = 0;      // candidates per chunk (0 = kDefaultSearchChunk)
    uint32_t plane_chunk = 0;       // pixels per launch (0 = kDefaultPlaneChunk)
    uint32_t gallery_chunk = 0;     // tiles per launch (0 = kDefaultGalleryChunk)
    uint32_t orbit_chunk = 0;       // columns per launch (0 = kDefaultOrbitChunk)
    uint32_t corr_chunk = 0;        // workgroups per launch (0 = kDefaultCorrChunk)
    uint32_t corr_replicas = 0;     // test hook: copies of k_corr_pairs' LDS histogram (0 = automatic)
    uint32_t box_chunk = 0;         // sets per launch (0 = kBoxMaxGridY)
    uint32_t box_slots = 0;         // slots per table (0 = the smallest power of two >= 2 n)
    uint32_t basin_chunk = 0;       // pixels per launch (0 = kDefaultBasinChunk)
    uint32_t period_chunk = 0;      // pixels per launch (0 = kDefaultPeriodChunk)
    uint32_t cycles_chunk = 0;      // (map, start) lanes per launch (0 = kDefaultCyclesChunk)
    uint32_t density_tile = 0;      // rows of a workgroup's tile, 8 / 16 / 32 (0 = kDensityDefaultTileH)
    uint32_t volume_chunk = 0;      // jobs per launch (0 = kDefaultVolumeChunk)
    uint32_t volume_steps = 0;      // counted iterations per job and launch (0 = kDefaultVolumeSteps)
};

// One row of an option table: the name, where the value goes, the rule it must pass and what a refusal says. The rules are the few
// that occur: any value; any value, stored as 0 / 1; value <= a; value one of set[0 .. n_set); 0 or a power of two in [a, b]; and
// kCustom, no field and no rule here: the caller's own few lines (it gets the row, so the name is known). `wide`: the rule reads the
// caller's 64-bit value, not its low 32 bits (what is stored is the low 32 bits either way).
struct OptionRule {
    enum Kind : uint8_t { kAny, kBool, kAtMost, kOneOf, kPow2, kCustom };
    const char* name;
    uint32_t Options::* field;
    Kind kind;
    bool wide;
    uint64_t a, b;
    uint32_t n_set, set[6];
    const char* refusal;
};
// Looks `name` up in table[0 .. n), checks `value` against the row's rule and stores it: the row and status SAR_OK. A name that is not
// there (nullptr, the text is `unknown` with the name) and a value the rule refuses leave SAR_ERR_INVALID and a text in sar_last_error.
inline const OptionRule* set_option_from(const OptionRule* table, size_t n, Options& opt, const char* name, uint64_t value, const char* unknown,
                                         int& status) {
    const OptionRule* r = table;
    while (r != table + n && std::strcmp(name, r->name)) ++r;
    status = SAR_ERR_INVALID;
    if (r == table + n) { set_error(unknown, name); return nullptr; }
    const uint32_t v = static_cast<uint32_t>(value);
    const uint64_t x = r->wide ? value : v;
    bool ok = r->kind != OptionRule::kOneOf;
    if (r->kind == OptionRule::kAtMost) ok = x <= r->a;
    if (r->kind == OptionRule::kPow2) ok = x <= r->b && !(x & (x - 1u)) && (x == 0 || x >= r->a);
    for (uint32_t i = 0; i < r->n_set; ++i) ok = ok || x == r->set[i];
    status = ok ? SAR_OK : SAR_ERR_INVALID;
    if (!ok) set_error("%s", r->refusal);
    else if (r->field) opt.*r->field = r->kind == OptionRule::kBool ? (v ? 1u : 0u) : v;
    return r;
}

// Survivor statistics of the last launch, copied back lazily (never waited for): the next render call sizes its staging for the lanes
// that will really be busy (solar-sail loses 38 % of its jobs in the warm-up).
struct Survivors {
    HostBuf<uint32_t> h_active;
    Event active_copied;
    bool on_side = false;        // the copy in flight was enqueued on the side stream (an announced launch)
    bool pending = false;
    uint32_t jobs_launched = 0;
    double fraction = 1.0;
    bool known = false;          // a launch has reported its survivors (until then the fraction is the optimistic default)
    void poll() {  // takes the copy in, if it has arrived
        if (!pending || hipEventQuery(active_copied) != hipSuccess) return;
        pending = false;
        if (jobs_launched) { fraction = static_cast<double>(*h_active) / jobs_launched; known = true; }
    }
    // Enqueues the copy of a launch of `jobs` jobs on `s` and records its event, unless one is still in flight; a failure only means no
    // statistics. `mark`: the single-frame launch says which stream `s` is, the batched launch leaves on_side as it finds it.
    enum Mark { kOnLaunchStream, kOnSideStream, kUnmarked };
    void enqueue_copy(const uint32_t* d_active, hipStream_t s, uint32_t jobs, Mark mark) {
        if (pending) return;
        if (hipMemcpyAsync(h_active, d_active, sizeof(uint32_t), hipMemcpyDeviceToHost, s) != hipSuccess || hipEventRecord(active_copied, s) != hipSuccess) return;
        pending = true;
        if (mark != kUnmarked) on_side = mark == kOnSideStream;
        jobs_launched = jobs;
    }
    // an announced launch's copy reads d_active on the side stream: whoever overwrites the counters on `s` before it was seen to finish waits
    int join(hipStream_t s) {
        if (pending && on_side) HIP_TRY(hipStreamWaitEvent(s, active_copied, 0));
        return SAR_OK;
    }
};

// The packed post-warm-up points, the job list and the survivor counters ([4]: survivors, pad, iterations of the jobs that died in the
// warm-up as a u64) of the binned path, twice. The warm-up of an ANNOUNCED render call (sar_runtime_prefetch_device) runs ahead on the
// side stream, under the current frame's accumulate / fold / colorize, into the second set; the announced call swaps the sets. The two
// depth ranges a warm-up measures for the narrow hints ({~sortable(min z), sortable(max z)}: what they quantise, HintQuant) do not swap.
struct WarmSet {
    DevBuf<double> d_warm, d_warm_alt;
    DevBuf<uint32_t> d_joblist, d_joblist_alt;
    DevBuf<uint32_t> d_active, d_active_alt;
    DevBuf<uint32_t> d_hint_range, d_hint_range_alt;
    void swap() { std::swap(d_warm, d_warm_alt); std::swap(d_joblist, d_joblist_alt); std::swap(d_active, d_active_alt); }
    // Room for m jobs in the second set. What wrote it last ran on `side` (absent: nothing did); what read it last — it was the current
    // set before the last swap — may be an iterate kernel still in flight on `launch`: both end first (rare: only while the sets grow).
    int grow_ahead(sar_runtime* rt, uint32_t m, hipStream_t side, hipStream_t launch) {
        if (m <= d_joblist_alt.cap()) return SAR_OK;
        if (side) HIP_TRY(hipStreamSynchronize(side));
        HIP_TRY(hipStreamSynchronize(launch));
        d_warm_alt.release(), d_joblist_alt.release();
        HIP_TRY(d_warm_alt.grow(rt, static_cast<size_t>(m) * 3));
        HIP_TRY(d_joblist_alt.grow(rt, m));
        return SAR_OK;
    }
};

// Start points: the page-locked staging buffer, its copy in device memory, and the converted points of an announced call (NOT one of
// the sets that swap). `starts_copied` fires when whatever reads h_starts — an upload, or a batch's kernel that reads it in place — is
// done. Start points of a batched launch are uploaded on the leader's upload stream, behind the last kernel that read d_starts
// (`starts_consumed`, recorded by whatever launched it): the upload of batch k+1 runs under batch k.
struct Starts {
    HostBuf<double> h_starts;
    DevBuf<double> d_starts, d_starts_alt;
    Event starts_copied;
    bool starts_pending = false;
    Event starts_consumed;
    bool starts_consumed_recorded = false;
    int wait_host_buffer() {  // before the host writes h_starts: the previous call's reader is done
        if (starts_pending) HIP_TRY(hipEventSynchronize(starts_copied));
        starts_pending = false;
        return SAR_OK;
    }
    int host_buffer_read_by(hipStream_t s) {  // what is enqueued on `s` so far reads h_starts; nothing behind it does
        HIP_TRY(hipEventRecord(starts_copied, s));
        starts_pending = true;
        return SAR_OK;
    }
};

// Per-XCD depth hints of the binned path: lower bounds of depths already accumulated; anything that can lower zbuf voids them.
struct Hints {
    DevBuf<void> d_zhint;
    uint32_t zhint_bytes = 0;        // bytes per hint of the current allocation (2 or 4)
    uint32_t copies_used = 8;        // of the eight per-XCD arrays, how many [0, n) a launch has written since they were last cleared
                                     // (a launch whose XCDs share ONE array writes array 0 only): what a clear clears
    uint32_t copies_alloc = 0;       // arrays the allocation holds: 8, or 1 where every launch so far shared one array (a runtime of
                                     // a frame group — its frames are dealt to XCDs of their own —, an image beyond 200 MB of hints)
    bool single_hint_array = false;  // a runtime of a frame group: its launches share ONE hint array whatever their form
    bool hint_range_set = false;     // the narrow hints' depth range was measured since the hints were last cleared (the quantiser
                                     // must not change under them)
    // what a clear covers — only the arrays a launch has written since the last one: a batched frame whose XCDs share one array
    // leaves seven untouched — and the value it writes (kWideHintEmpty: what wide hints are cleared to)
    size_t entries_used(uint32_t npix) const { return d_zhint ? kHintStride(npix) * copies_used : 0; }
    uint32_t empty_value() const { return zhint_bytes == 4 ? kWideHintEmpty : 0u; }
    void mark_cleared() { copies_used = 0; hint_range_set = false; }  // empty from here on: the next launch may measure the depth range anew
    int clear(uint32_t npix, hipStream_t s) {
        const size_t entries = entries_used(npix);
        if (entries && zhint_bytes == 4)
            HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d_zhint.get()), static_cast<int>(kWideHintEmpty), entries, s));
        else if (entries)
            HIP_TRY(hipMemsetAsync(d_zhint, 0, entries * zhint_bytes, s));
        mark_cleared();
        return SAR_OK;
    }
    // whether this launch, with hints of hint_bytes, fixes the narrow hints' quantiser: the first since they were cleared, and marks it
    bool claims_range(uint32_t hint_bytes) {
        if (hint_bytes != 2 || hint_range_set) return false;
        return hint_range_set = true;
    }
};

struct SpanList { std::vector<Span> spans; size_t used = 0; };

// Device-side timing of a runtime's launches (sar_runtime_enable_timing): one span per launch of the last render call — or, with
// the option timing_accumulate, of every render call since sar_runtime_last_timing read them.
struct Timing {
    bool timing = false, timing_accumulate = false;
    SpanList iter, fold, warm;
    Span colorize_span, merge_span;
    bool colorize_timed = false, merge_timed = false;
    uint64_t last_iterations = 0;
    void restart() { last_iterations = 0; iter.used = fold.used = warm.used = 0; }
    void restart_unless_accumulating() { if (!timing_accumulate) restart(); }
    void single_begin(Span& sp, hipStream_t s) {
        if (!timing) return;
        (void)sp.a.ensure(hipEventDefault);  // (made on first use)
        (void)sp.b.ensure(hipEventDefault);
        (void)hipEventRecord(sp.a, s);
    }
    void span_begin(SpanList& l, hipStream_t s) {
        if (!timing) return;
        if (l.used == l.spans.size()) l.spans.emplace_back();
        single_begin(l.spans[l.used], s);
    }
    void span_end(SpanList& l, hipStream_t s) {
        if (!timing) return;
        (void)hipEventRecord(l.spans[l.used].b, s);
        ++l.used;
    }
    void single_end(Span& sp, bool& flag, hipStream_t s) {
        if (!timing) return;
        (void)hipEventRecord(sp.b, s);
        flag = true;
    }
};

// The colorized image, its converted form and their read-back. The read-back of an async frame runs on its own stream (the copy
// engine), behind `img_ready`: the launch stream goes on with the next frame at once, and waits for the last read-back only before
// it writes d_rgba / d_export again. copy_stream is the runtime's own (own_copy_stream), its group's or a borrowed one.
struct Readback {
    DevBuf<void> d_rgba;
    DevBuf<void> d_export;             // converted image of sar_colorize_format (<= 6 bytes per pixel)
    const void* export_src = nullptr;  // where the last sar_colorize_format* left its image (d_rgba or d_export) and how long it is:
    size_t export_bytes = 0;           // what a read-back copies
    Event img_events[8];               // sar_colorize_format_async tickets (ticket t is event t % 8: a later recording on the
    uint64_t img_next = 0;             // same stream completes no earlier, so waiting for it is always sufficient)
    hipStream_t copy_stream = nullptr;
    Stream own_copy_stream;
    Event img_ready;
    bool copy_in_flight = false;
    int ensure_copy_stream() {
        if (!copy_stream) HIP_TRY(own_copy_stream.ensure(hipStreamNonBlocking));
        if (!copy_stream) copy_stream = own_copy_stream;
        return SAR_OK;
    }
    int wait_last_copy(hipStream_t s) {  // before `s` writes d_rgba / d_export: the last async frame's read-back may still read them
        if (copy_in_flight) HIP_TRY(hipStreamWaitEvent(s, img_events[(img_next - 1) % 8], 0));
        copy_in_flight = false;
        return SAR_OK;
    }
};

// The warm-up that runs ahead (sar_render.cpp: warmup_ahead) and the events it meets the launch stream through.
struct Prefetch {
    bool valid = false;
    MapParams p;
    uint32_t n_jobs = 0, m = 0, width = 0;
    uint64_t iters = 0;
    const double* starts = nullptr;
    bool range_measured = false;
    Event iter_done, pf_done;
    bool iter_done_recorded = false;
    hipEvent_t prefetch_after = nullptr;  // set around sar_runtime_prefetch_device by the multi-device renderer: the side stream
                                          // waits for it (the upload of the announced points) instead of the host
    uint32_t prefetch_used = 0;           // statistic: launches that found their warm-up done
};

// Batched launches (sar_batch.cpp). As the LEADER of a batch: the table of per-frame argument blocks in device memory and the
// page-locked ring it is uploaded from (entry k % kBatchRing is free again once batch_copied[k % kBatchRing] has fired). As any
// member: the event its own stream and the leader's stream meet through when they differ.
struct Batch {
    DevBuf<BatchFrame> d_batch;
    HostBuf<BatchFrame> h_batch;
    Event batch_copied[kBatchRing];
    uint64_t batch_next = 0;
    Event batch_join;
    uint32_t batches_launched = 0;  // statistic: batched launches this runtime led
};

// ---- the analysis families: the scratch of one launch chunk and what the last call left, plain allocations (not the group slab: it
// never reclaims) made on first use, kept for the next call and freed with the runtime ----

struct SearchState {  // sar_runtime_search (sar_search.cpp)
    DevBuf<uint32_t> d_counters;       // [2] survivors, deaths in the transient
    DevBuf<uint32_t> d_idx;            // [chunk]
    DevBuf<double> d_xyz;              // [3][chunk]
    DevBuf<double> d_coeffs;           // [chunk][30] the caller's coefficient sets
    DevBuf<sar_search_record> d_rec;   // [survivors of the largest phase 2 so far]
};
struct PlaneState {  // sar_runtime_plane (sar_plane.cpp): the records of the last plane stay on the device for sar_runtime_plane_colorize
    DevBuf<sar_plane_record> d_rec;    // [width * height of the largest plane so far]
    DevBuf<uint16_t> d_rgba;           // [4 * width * height]: sar_runtime_plane_colorize's image
    uint32_t width = 0, height = 0;    // the last plane; 0: none (or its call failed)
    int32_t mode = 0;
};
struct GalleryState {  // sar_runtime_gallery (sar_gallery.cpp): every tile's argument block and statistics, the atlas, the points after
                       // the warm-up and the raw tiles of one launch chunk
    DevBuf<GalleryTile> d_tiles;         // [n]
    DevBuf<sar_gallery_stats> d_stats;   // [n]
    DevBuf<double> d_starts;             // [jobs][3]
    DevBuf<double> d_warm;               // [chunk][3][jobs]
    DevBuf<uint32_t> d_count;            // [chunk][tile pixels]
    DevBuf<float> d_zbuf;
    DevBuf<double> d_steps;
    DevBuf<uint16_t> d_atlas;            // [4 * atlas pixels]
};
struct OrbitState {  // sar_runtime_orbit (sar_orbit.cpp): every column's coefficient block and statistics, the diagram and its max
    DevBuf<SearchCoeffs> d_cols;         // [width]
    DevBuf<sar_orbit_column> d_stats;    // [width]
    DevBuf<double> d_starts;             // [jobs][3]
    DevBuf<uint32_t> d_count;            // [height][width]
    DevBuf<uint32_t> d_max;              // [1]
};
struct CorrState {  // sar_runtime_pairs / sar_runtime_corrdim (sar_corr.cpp): one group of sets
    DevBuf<double> d_points;                // [sets of a group][3][n] (box counting reads them too)
    DevBuf<CorrMapState> d_state;           // [maps of a group]
    DevBuf<unsigned long long> d_hist;      // [sets of a group][bins]
    DevBuf<double> d_coeffs;                // [maps of a group][30]
    DevBuf<double> d_starts;                // [jobs][3]
};
struct BoxState {  // sar_runtime_boxes / sar_runtime_boxdim (sar_box.cpp): one group of sets (the points are CorrState's)
    DevBuf<BoxCube> d_cubes;                // [sets of a group]
    DevBuf<unsigned long long> d_keys;      // [2][sets of a group][slots]
    DevBuf<uint32_t> d_counts;              // [2][sets of a group][slots]
    DevBuf<unsigned long long> d_sums;      // [sets of a group][L + 1][4]
    DevBuf<uint32_t> d_overflow;            // [1]
};
struct SpectrumState {  // sar_runtime_spectra / sar_runtime_spectrum (sar_spectrum.cpp): one group of sets (the points are CorrState's)
    DevBuf<double> d_tables;                // [N / 2][2] twiddles, then [N] window
    DevBuf<double> d_scratch;               // [sets of a group][jobs][N / 2 + 2]: every job's spectrum, then its energy
    DevBuf<double> d_power;                 // [sets of a group][N / 2 + 2]: the folded spectrum, then the energy
};
struct RqaState {  // sar_runtime_recurrence / sar_runtime_rqa / sar_runtime_recurrence_plot (sar_rqa.cpp): one group of sets (the points are CorrState's)
    DevBuf<unsigned long long> d_out;       // [sets of a group][rqa_row(B)]: both histograms, then the recurrences and the longest lines
    DevBuf<double> d_eps2;                  // [sets of a group]
    DevBuf<unsigned char> d_plot;           // [height][width]
};
struct BasinState {  // sar_runtime_basin (sar_basin.cpp): records, labels and image stay for sar_runtime_basin_colorize
    DevBuf<double> d_t;                     // [width + height]: tu, then tv
    DevBuf<sar_basin_pixel> d_pix;          // [width * height]
    DevBuf<uint32_t> d_label;               // [width * height]: the host's labels
    DevBuf<uint32_t> d_last;                // [width * height]: the node of a survivor's last tail point
    DevBuf<uint32_t> d_counter;             // [1]
    DevBuf<uint32_t> d_surv_pix;            // [pixels of a launch]
    DevBuf<double> d_surv_xyz;              // [3][pixels of a launch]
    DevBuf<uint32_t> d_parent;              // [grid^3]
    DevBuf<uint32_t> d_node_root;           // [grid^3]
    DevBuf<unsigned long long> d_extent;    // [6]
    DevBuf<uint16_t> d_rgba;                // [4 * width * height]: sar_runtime_basin_colorize's image
    uint32_t width = 0, height = 0;         // the last basin picture; 0: none (or its call failed)
    uint32_t attractors = 0;
    // the HELD picture of the basin probes (sar_fate.cpp: sar_runtime_basin_fates / sar_runtime_basin_uncertainty): the last basin
    // call's map, steps, bound and box, if that call succeeded, and its table of the cells' labels — the host's copy, and the
    // device's, which the first probe call uploads
    bool held = false, label_uploaded = false;
    SearchCoeffs held_map{};                // canonicalised
    double held_box_lo[3] = {0., 0., 0.}, held_scale[3] = {0., 0., 0.}, held_bound = 0.;
    uint32_t held_transient = 0, held_steps = 0, held_grid = 0;
    std::vector<uint32_t> h_node_label;     // [grid^3]: a cell's attractor label, kBasinEmpty where no tail went
    DevBuf<uint32_t> d_node_label;          // [grid^3]
    DevBuf<double> d_probe;                 // [points of a launch][3] / [base points of a call][3]
    DevBuf<sar_basin_fate> d_fates;         // [points of a launch] / [base points of a call]
    DevBuf<sar_basin_ladder_mask> d_masks;  // [base points of a call]
    DevBuf<unsigned long long> d_levels;    // [kMaxLadderLevels][2]: uncertain, unknown per level
};
struct FtleState {  // sar_runtime_ftle (sar_ftle.cpp): the records and the finished stretch2 stay for sar_runtime_ftle_colorize
    DevBuf<double> d_t;                     // [width + height]: tu, then tv
    DevBuf<sar_ftle_pixel> d_pix;           // [width * height]: the device's fields (stretch2 / ftle are the host's)
    DevBuf<double> d_stretch2;              // [width * height]: the host finish's stretch2
    DevBuf<uint16_t> d_rgba;                // [4 * width * height]: sar_runtime_ftle_colorize's image
    uint32_t width = 0, height = 0;         // the last FTLE map; 0: none (or its call failed)
    uint32_t steps = 0;                     // its N
};
struct PeriodState {  // sar_runtime_period (sar_period.cpp): the records stay for sar_runtime_period_colorize
    DevBuf<sar_period_record> d_rec;        // [width * height of the largest period plane so far]
    DevBuf<double> d_coeffs;                // [width * height][30]: the caller's list of the list form
    DevBuf<uint16_t> d_rgba;                // [4 * width * height]: sar_runtime_period_colorize's image
    uint32_t width = 0, height = 0;         // the last period plane; 0: none (or its call failed)
};
struct CyclesState {  // sar_runtime_cycles (sar_cycles.cpp)
    DevBuf<SearchCoeffs> d_coeffs;          // [n_maps]
    DevBuf<double> d_starts;                // [jobs][3]
    DevBuf<CycleFind> d_finds;              // [maps of a launch][jobs]
    DevBuf<sar_cycles_record> d_rec;        // [maps of a launch]
    DevBuf<sar_cycle_orbit> d_orbits;       // [maps of a launch][cap]
};
struct ManifoldState {  // sar_runtime_manifold (sar_manifold.cpp): the family's own images, not the runtime's
    DevBuf<ManifoldBranch> d_branches;      // [n_branches]
    DevBuf<ManifoldSums> d_sums;            // [n_branches]
    DevBuf<uint32_t> d_count;               // [width * height of the largest call so far]
    DevBuf<uint32_t> d_first;               // [width * height of the largest call so far]
};
struct DensityState {  // sar_runtime_density (sar_density.cpp)
    DevBuf<char> d_snap;                    // [12 * npix]: the snapshot k_density reads (steps, then count)
    DevBuf<DensityDeviceStats> d_stats;     // the block its statistics reduce into
    DevBuf<uint32_t> d_plan;                // [kDensityPlanMaxWords]: the weight plan of the last `samples`
    std::map<uint32_t, std::vector<uint32_t>> h_plans;  // by S: what d_plan is uploaded from (an upload may read it after the call
                                            // returns, so a plan once made stays with the runtime)
    uint32_t plan_samples = 0;              // the S of d_plan; 0: none
};
struct VolumeState {  // sar_runtime_volume* (sar_volume.cpp): the HELD volume, the family's own memory, and what it was made with
    DevBuf<uint32_t> d_vol;                 // [slabs][height][width]
    DevBuf<double> d_state;                 // [3][jobs of a launch]: the jobs' points between launches
    DevBuf<VolumeSums> d_sums;              // the block a call's sums reduce into
    DevBuf<VolumeMarchSums> d_march;        // the block k_volume_march's statistics reduce into
    DevBuf<uint32_t> d_section;             // [2][width * height]: k_volume_section's count, then its nearest
    bool held = false;                      // the last sar_runtime_volume succeeded and nothing has dropped its volume since
    uint32_t width = 0, height = 0, slabs = 0;
    double z_lo = 0., z_hi = 0.;
    sar_volume_stats stats{};
    void drop() { held = false; d_vol.release(); }  // (the stream must have been waited for)
};
struct FlowState {  // sar_runtime_render_flow (sar_flow.cpp): the scratch of one call; the frame it plots into is the runtime's
    DevBuf<double> d_state;                 // [3][jobs of a launch]: the jobs' points between launches, x NaN once escaped
    DevBuf<FlowSums> d_sums;                // the block a call's sums reduce into
    DevBuf<unsigned long long> d_keys;      // [width * height]: a call's depth-and-hue keys, zeroed per call
};
struct SectionState {  // sar_runtime_section (sar_section.cpp): the scratch of one chunk; the point rows, the transient's sums and the keys are FlowState's
    DevBuf<uint32_t> d_rows;                // [kSectionRows][jobs of a launch]: status, found, rough, steps, clock_step, t_prev
    DevBuf<double> d_dt_prev;               // [jobs of a launch]: the previous crossing's time offset within its step
    DevBuf<double> d_cross;                 // [jobs of a launch][samples][4]: the recorded crossings and their return times
    DevBuf<SectionSums> d_sums;             // the block a call's sums reduce into
};
struct ShadeState {  // sar_shade (sar_shade.cpp)
    DevBuf<sar_shade_stats> d_stats;        // the block k_shade's statistics reduce into
};
// auto exposure (sar_runtime_set_exposure) and auto colour range (sar_runtime_set_color_range / sar_runtime_hold_color_range): the
// mode, and the select scratch + record(s) of sar_select.hip's kernels
struct ExposureState {
    bool on = false;
    sar_exposure_params params{};
    DevBuf<uint32_t> d_scratch;             // [kExpoScratchWords]: histograms (zero between calls) + SelectState
    DevBuf<sar_exposure> d_rec;
};
struct ColorRangeState {
    int32_t mode = kCrOff;
    sar_color_range_params params{};
    DevBuf<uint32_t> d_scratch;             // [kCrScratchWords]: histograms (zero between calls) + SelectState
    DevBuf<sar_color_range> d_rec;          // [2]: the measured record, the held one
};

}  // namespace sar

struct sar_runtime {
    int device = 0;
    // frame group (nullptr: a runtime of its own) and this runtime's memory out of the group's. Destruction order: the slab is
    // declared before every buffer, so it goes after them.
    sar::RuntimeGroup* group = nullptr;
    sar::Slab slab;
    // The launch stream: the runtime's own, its group's, or one borrowed by sar_runtime_set_stream (a batch points it at the
    // leader's for the length of the call). own_stream owns the first kind.
    hipStream_t stream = nullptr;
    sar::Stream own_stream;
    sar::Stream side;                  // announced warm-ups, and the depth resolve that runs beside the accumulate kernel
    sar::Event depth_done;             // a launch chunk's depth resolve on the side stream: the launch stream waits for it behind the accumulate
    sar::Stream upload_stream;         // a batch leader's: the start points of the next batch (Starts)
    uint32_t W = 0, H = 0, npix = 0, sm_count = 0;

    // persistent state (Runtime, reference src/lib.rs:631-646)
    sar::DevBuf<uint32_t> d_count;            // count
    sar::DevBuf<unsigned long long> d_key;    // hi: sortable(zbuf), lo: 0xFFFFFFFF between launches
    sar::DevBuf<double> d_steps;              // steps
    sar::DevBuf<uint32_t> d_scalars;          // max + flags + depth range
    sar::Rng rng;

    // scratch bins the iterate kernel accumulates into (zero between launches)
    uint32_t copies = 0;      // scratch_count copies: 1 on the one-atomic-per-visit path, 0 on the binned path, `splits` in a batched launch
    sar::DevBuf<uint32_t> d_scratch_count;
    sar::DevBuf<unsigned long long> d_scratch_key;
    sar::DevBuf<uint32_t> d_seg_any;   // batched launches: [npix / 2048 + 1] 2048-pixel segments with a count in the current launch
    sar::DevBuf<float> d_ztmp;
    // binned path: per-wave record arenas, list heads, NaN iteration counter, trajectory checkpoints
    sar::DevBuf<void> d_arena;
    sar::DevBuf<uint32_t> d_heads;
    sar::DevBuf<unsigned long long> d_nan_count;
    sar::DevBuf<double> d_ckpt;
    double* d_lnlut = nullptr;  // the device's shared table (acquire_ln_lut)

    sar::Options opt;
    sar::Hints hints;
    sar::Starts starts;
    sar::WarmSet warm;
    sar::Prefetch pf;
    sar::Survivors surv;
    sar::Readback rb;
    sar::Batch batch;
    sar::Timing tm;
    sar::SearchState search;
    sar::PlaneState plane;
    sar::GalleryState gallery;
    sar::OrbitState orbit;
    sar::CorrState corr;
    sar::BoxState box;
    sar::SpectrumState spectrum;
    sar::RqaState rqa;
    sar::BasinState basin;
    sar::FtleState ftle;
    sar::PeriodState period;
    sar::CyclesState cycles;
    sar::ManifoldState manifold;
    sar::DensityState density;
    sar::ShadeState shade;
    sar::VolumeState volume;
    sar::FlowState flow;
    sar::SectionState section;
    sar::ExposureState expo;
    sar::ColorRangeState crange;
    char last_launch[256] = {0};     // sar_runtime_describe_last_launch
    uint32_t last_chunks = 0;
    uint64_t colorize_launches = 0;  // statistic: colorize kernels this runtime enqueued, alone or as a batch's leader (test hooks)

    ~sar_runtime();  // waits for the runtime's streams; the members then free themselves
};

inline void* sar::slab_carve(sar_runtime* rt, bool host, size_t bytes) { return rt->slab.carve(host, bytes); }

namespace sar {

// sar_runtime.cpp
int check_cfg_matches(const sar_config* cfg, const sar_runtime* rt);
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

// sar_render.cpp
void fill_map_params(const sar_config& cfg, MapParams& p);      // render's hoisted constants (:755-764)
void fill_ct_params(const sar_config& cfg, ColorTransformParams& ct);
// Runs n_jobs trajectories of `iters` counted iterations each into rt (sequential job-major semantics); `starts` is
// [n_jobs][3] in host memory, or in device memory with starts_on_device. Enqueues only.
int render_chunked(const sar_config* cfg, sar_runtime* rt, uint32_t n_jobs, uint64_t iters, const double* starts,
                   bool starts_on_device = false);

// sar_colorize.cpp
// colorize of the pixel range [first, first + n) into out_dev (n * 8 bytes). global_scalars: the scalars (max, depth
// range) already hold the values of the WHOLE image (sliced multi-GPU colorize); otherwise the depth range is folded
// over the range first, as colorize does (:877-882).
int colorize_range(const sar_config* cfg, sar_runtime* rt, uint32_t first, uint32_t n, void* out_dev, bool global_scalars);
int validate_exposure(const sar_exposure_params* p);
int validate_color_range(const sar_color_range_params* p);
PaletteParams palette_params(const sar_config* cfg);  // Palette::new (:413-418): the entries, the last one duplicated

}  // namespace sar
