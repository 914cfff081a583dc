// sar_runtime_impl.hpp — the private layout of sar_runtime, the few internals of sar_runtime.cpp that the multi-device
// ParallelRenderer (sar_multi.cpp) and the analysis entry points (sar_analysis.hpp) build on. Not part of the ABI.
#pragma once

#include <hip/hip_runtime.h>

#include <map>
#include <utility>
#include <vector>

#include "sar_basin.hpp"
#include "sar_box.hpp"
#include "sar_corr.hpp"
#include "sar_cycles.hpp"
#include "sar_density.hpp"
#include "sar_gallery.hpp"
#include "sar_launch.hpp"
#include "sar_orbit.hpp"
#include "sar_period.hpp"

struct sar_runtime;

namespace sar {

// Memory of `rt`'s slab (host: of its share of its group's page-locked slab) while that lasts, in 256-byte granules handed out
// front to back and never reused; nullptr when the request does not fit.
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

struct sar_runtime {
    int device = 0;
    // frame group (nullptr: a runtime of its own). `sub` is ONE device allocation of this runtime its buffers are carved from
    // (sized from the plan of the frames the group was made for: some twenty hipMalloc / hipFree calls less per runtime — a hipFree
    // costs 0.16 ms; one allocation for the WHOLE group, 10 GB, took between 0.3 ms and two seconds on the same box), `hsub` its
    // share of the group's page-locked allocation; both handed out front to back by slab_carve and never reused (what
    // does not fit comes from hipMalloc / hipHostMalloc). Declared before every buffer: it goes after them.
    sar::RuntimeGroup* group = nullptr;
    sar::DevBuf<char> sub;
    size_t sub_used = 0;
    char* hsub = nullptr;
    size_t hsub_bytes = 0, hsub_used = 0;
    // The launch stream: the runtime's own, its group's, or one borrowed by sar_runtime_set_stream (a batch points it at the
    // leader's for the length of the call). own_stream owns the first kind.
    hipStream_t stream = nullptr;
    sar::Stream own_stream;
    uint32_t W = 0, H = 0, npix = 0;
    uint32_t sm_count = 0;

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

    // binned path: per-wave record arenas, list heads, per-XCD depth hints, NaN iteration counter
    sar::DevBuf<void> d_arena;
    sar::DevBuf<uint32_t> d_heads;
    sar::DevBuf<void> d_zhint;
    uint32_t zhint_bytes = 0;        // bytes per hint of the current allocation (2 or 4)
    uint32_t hint_copies_used = 8;   // of the eight per-XCD arrays, how many [0, n) a launch has written since they were last
                                     // cleared (a launch whose XCDs share ONE array writes array 0 only): what clear_hints clears
    uint32_t hint_copies_alloc = 0;  // arrays the allocation holds: 8, or 1 where every launch so far shared one array (a runtime of
                                     // a frame group — its frames are dealt to XCDs of their own —, an image beyond 200 MB of hints)
    bool single_hint_array = false;  // a runtime of a frame group: its launches share ONE hint array whatever their form
    uint32_t hint_bits = 0;          // option: 0 = by image size, 16, 32
    uint32_t depth_park = sar::kDepthParkAuto;  // test option: the park window of k_iterate_split's consumer (0, 2, 4, 8); automatic = by hint type
    uint32_t hint_tile = 0;          // option: 0 = narrow hints of power-of-two-wide images in 8 x 8 tiles, 1 = always row-major
    uint32_t hint_shared = 0;        // option: 0 = automatic, 1 = one hint array per XCD, 2 = one array for the whole chip
    sar::DevBuf<unsigned long long> d_nan_count;
    sar::DevBuf<uint32_t> d_hint_range;   // {~sortable(min z), sortable(max z)}: what the narrow depth hints quantise (HintQuant)
    bool hint_range_set = false;        // measured since the hints were last cleared (the quantiser must not change under them)

    // staging
    sar::HostBuf<double> h_starts;
    sar::DevBuf<double> d_starts;
    sar::DevBuf<double> d_warm;        // binned path: packed post-warm-up points, job list, survivor count
    sar::DevBuf<uint32_t> d_joblist;
    sar::DevBuf<uint32_t> d_active;    // [4]: survivors, pad, iterations of the jobs that died in the warm-up (u64)
    // The warm-up of an ANNOUNCED render call (sar_runtime_prefetch_device) runs ahead on a side stream, under the current
    // frame's accumulate / fold / colorize, into a second set of these buffers; the announced call swaps the sets
    // (d_starts_alt does not swap).
    sar::DevBuf<double> d_warm_alt;
    sar::DevBuf<uint32_t> d_joblist_alt;
    sar::DevBuf<uint32_t> d_active_alt;
    sar::DevBuf<uint32_t> d_hint_range_alt;
    sar::DevBuf<double> d_starts_alt;
    sar::Stream side;
    sar::Event iter_done, pf_done;
    sar::Event depth_done;                // the depth resolve of a launch chunk, on the side stream: the launch stream waits for it
                                          // behind the accumulate kernel
    uint32_t tail_overlap = SAR_TAIL_OVERLAP_DEFAULT;  // option: 1 = the depth resolve runs on the side stream beside the accumulate kernel
                                          // (measured slower on 2048^2: profiles/r07_tail_overlap_ab.txt), 0 = behind it on the launch stream
    hipEvent_t prefetch_after = nullptr;  // set around sar_runtime_prefetch_device by the multi-device renderer: the side stream
                                          // waits for it (the upload of the announced points) instead of the host
    bool iter_done_recorded = false;
    struct Prefetch {
        bool valid = false;
        sar::MapParams p;
        uint32_t n_jobs = 0, m = 0, width = 0;
        uint64_t iters = 0;
        const double* starts = nullptr;
        bool range_measured = false;
    } pf;
    uint32_t prefetch_used = 0;      // statistic: launches that found their warm-up done
    uint32_t chunk_ahead = 0;        // option: 2 = a call of several launch chunks does not run its next chunk's warm-up ahead (A/B)
    sar::Event img_events[8];        // sar_colorize_format_async tickets (ticket t is event t % 8: a later recording on the
    uint64_t img_next = 0;           // same stream completes no earlier, so waiting for it is always sufficient)
    // The read-back of an async frame runs on its own stream (the copy engine), behind `img_ready`: the launch stream goes on
    // with the next frame at once, and waits for the last read-back only before it writes d_rgba / d_export again.
    // copy_stream is the runtime's own (own_copy_stream), its group's or a borrowed one.
    hipStream_t copy_stream = nullptr;
    sar::Stream own_copy_stream;
    sar::Event img_ready;
    bool copy_in_flight = false;
    uint32_t readback_inline = 0;    // option: 1 = async read-backs stay on the launch stream (A/B)
    uint32_t batch_starts = 0;       // option: how a batched launch gets its start points: 0 = the warm-up kernel reads the page-locked
                                     // staging buffer itself (no copy), 1 = copied on the upload stream, 2 = copied on the launch stream
    // Start points of a batched launch are uploaded on the leader's upload stream, behind the last kernel that read d_starts
    // (`starts_consumed`, recorded by whatever launched it): the upload of batch k+1 runs under batch k.
    sar::Stream upload_stream;
    sar::Event starts_consumed;
    bool starts_consumed_recorded = false;
    char last_launch[256] = {0};     // sar_runtime_describe_last_launch
    sar::DevBuf<uint32_t> d_seg_any;   // batched launches: [npix / 2048 + 1] 2048-pixel segments with a count in the current launch
    uint32_t last_chunks = 0;
    // survivor statistics of the last launch, copied back lazily (never waited for): the next render call sizes its
    // staging for the lanes that will really be busy (solar-sail loses 38 % of its jobs in the warm-up)
    sar::HostBuf<uint32_t> h_active;
    sar::Event active_copied;
    bool active_copy_on_side = false;     // the copy in flight was enqueued on the side stream (an announced launch)
    bool active_pending = false;
    uint32_t active_jobs_launched = 0;
    double survivor_fraction = 1.0;
    bool survivors_known = false;    // a launch has reported its survivors (until then the fraction is the optimistic default)
    sar::Event starts_copied;
    bool starts_pending = false;
    sar::DevBuf<double> d_ckpt;
    double* d_lnlut = nullptr;  // the device's shared table (acquire_ln_lut)
    sar::DevBuf<void> d_rgba;
    sar::DevBuf<void> d_export;  // converted image of sar_colorize_format (<= 6 bytes per pixel)
    const void* export_src = nullptr;  // where the last sar_colorize_format* left its image (d_rgba or d_export) and how long it is:
    size_t export_bytes = 0;           // what a read-back copies
    sar::DevBuf<float> d_ztmp;

    // batched launches (sar_batch.cpp). As the LEADER of a batch: the table of per-frame argument blocks in device memory and
    // the page-locked ring it is uploaded from (entry k % kBatchRing is free again once batch_copied[k % kBatchRing] has fired).
    // As any member: the event its own stream and the leader's stream meet through when they differ.
    sar::DevBuf<sar::BatchFrame> d_batch;
    sar::HostBuf<sar::BatchFrame> h_batch;
    sar::Event batch_copied[sar::kBatchRing];
    uint64_t batch_next = 0;
    sar::Event batch_join;
    uint32_t batches_launched = 0;   // statistic: batched launches this runtime led
    uint32_t batch_warm = 0;         // option: the warm-up of a batched launch: 0 = two phases when the last launch lost a tenth of its jobs, 1 = one phase, 2 = two
    uint32_t batch_chain = 0;        // option: 1 = the iterate kernels of this device's batches are NOT chained one behind the other (A/B)
    uint32_t batch_xcd = 0;          // option: 1 = the frames of a batch are NOT dealt to the XCDs (every frame runs on all eight: A/B)

    // sar_runtime_search (sar_search.cpp): the scratch of one launch chunk, plain allocations (not the group slab: it never
    // reclaims), kept for the next call and freed with the runtime
    uint32_t search_chunk = 0;                     // option: candidates per chunk (0 = kDefaultSearchChunk)
    sar::DevBuf<uint32_t> d_search_counters;       // [2] survivors, deaths in the transient
    sar::DevBuf<uint32_t> d_search_idx;            // [chunk]
    sar::DevBuf<double> d_search_xyz;              // [3][chunk]
    sar::DevBuf<double> d_search_coeffs;           // [chunk][30] the caller's coefficient sets
    sar::DevBuf<sar_search_record> d_search_rec;   // [survivors of the largest phase 2 so far]

    // sar_runtime_plane (sar_plane.cpp): the records of the last plane stay on the device for sar_runtime_plane_colorize; plain
    // allocations (not the group slab), kept for the next call and freed with the runtime
    uint32_t plane_chunk = 0;                      // option: pixels per launch (0 = kDefaultPlaneChunk)
    sar::DevBuf<sar_plane_record> d_plane_rec;     // [width * height of the largest plane so far]
    sar::DevBuf<uint16_t> d_plane_rgba;            // [4 * width * height]: sar_runtime_plane_colorize's image
    uint32_t plane_width = 0, plane_height = 0;    // the last plane; 0: none (or its call failed)
    int32_t plane_mode = 0;

    // sar_runtime_gallery (sar_gallery.cpp): every tile's argument block and statistics, the atlas, and the scratch of one launch
    // chunk — the points after the warm-up and the raw tiles; plain allocations (not the group slab), kept for the next call and
    // freed with the runtime
    uint32_t gallery_chunk = 0;                    // option: tiles per launch (0 = kDefaultGalleryChunk)
    sar::DevBuf<sar::GalleryTile> d_gal_tiles;     // [n]
    sar::DevBuf<sar_gallery_stats> d_gal_stats;    // [n]
    sar::DevBuf<double> d_gal_starts;              // [jobs][3]
    sar::DevBuf<double> d_gal_warm;                // [chunk][3][jobs]
    sar::DevBuf<uint32_t> d_gal_count;             // [chunk][tile pixels]
    sar::DevBuf<float> d_gal_zbuf;
    sar::DevBuf<double> d_gal_steps;
    sar::DevBuf<uint16_t> d_gal_atlas;             // [4 * atlas pixels]

    // sar_runtime_orbit (sar_orbit.cpp): every column's coefficient block and statistics, the start points, the diagram and its max;
    // plain allocations (not the group slab), kept for the next call and freed with the runtime
    uint32_t orbit_chunk = 0;                      // option: columns per launch (0 = kDefaultOrbitChunk)
    sar::DevBuf<sar::SearchCoeffs> d_orbit_cols;   // [width]
    sar::DevBuf<sar_orbit_column> d_orbit_stats;   // [width]
    sar::DevBuf<double> d_orbit_starts;            // [jobs][3]
    sar::DevBuf<uint32_t> d_orbit_count;           // [height][width]
    sar::DevBuf<uint32_t> d_orbit_max;             // [1]

    // sar_runtime_pairs / sar_runtime_corrdim (sar_corr.cpp): the points, states and histograms of one group of sets, the maps'
    // coefficients and the start points; plain allocations (not the group slab), kept for the next call and freed with the runtime
    uint32_t corr_chunk = 0;                          // option: workgroups per launch (0 = kDefaultCorrChunk)
    uint32_t corr_replicas = 0;                       // test hook: copies of k_corr_pairs' LDS histogram (0 = automatic)
    sar::DevBuf<double> d_corr_points;                // [sets of a group][3][n]
    sar::DevBuf<sar::CorrMapState> d_corr_state;      // [maps of a group]
    sar::DevBuf<unsigned long long> d_corr_hist;      // [sets of a group][bins]
    sar::DevBuf<double> d_corr_coeffs;                // [maps of a group][30]
    sar::DevBuf<double> d_corr_starts;                // [jobs][3]

    // sar_runtime_boxes / sar_runtime_boxdim (sar_box.cpp): the cubes, the two hash tables per set and the level sums of one group of
    // sets (the points are d_corr_points); plain allocations (not the group slab), kept for the next call and freed with the runtime
    uint32_t box_chunk = 0;                           // option: sets per launch (0 = kBoxMaxGridY)
    uint32_t box_slots = 0;                           // option: slots per table (0 = the smallest power of two >= 2 n)
    sar::DevBuf<sar::BoxCube> d_box_cubes;            // [sets of a group]
    sar::DevBuf<unsigned long long> d_box_keys;       // [2][sets of a group][slots]
    sar::DevBuf<uint32_t> d_box_counts;               // [2][sets of a group][slots]
    sar::DevBuf<unsigned long long> d_box_sums;       // [sets of a group][L + 1][4]
    sar::DevBuf<uint32_t> d_box_overflow;             // [1]

    // sar_runtime_basin (sar_basin.cpp): the plane's parameter tables, the records, labels and image of the last basin picture (they
    // stay for sar_runtime_basin_colorize), the survivor list of one launch, the union-find over the grid and the extent; plain
    // allocations (not the group slab), kept for the next call and freed with the runtime
    uint32_t basin_chunk = 0;                         // option: pixels per launch (0 = kDefaultBasinChunk)
    sar::DevBuf<double> d_basin_t;                    // [width + height]: tu, then tv
    sar::DevBuf<sar_basin_pixel> d_basin_pix;         // [width * height]
    sar::DevBuf<uint32_t> d_basin_label;              // [width * height]: the host's labels
    sar::DevBuf<uint32_t> d_basin_last;               // [width * height]: the node of a survivor's last tail point
    sar::DevBuf<uint32_t> d_basin_counter;            // [1]
    sar::DevBuf<uint32_t> d_basin_surv_pix;           // [pixels of a launch]
    sar::DevBuf<double> d_basin_surv_xyz;             // [3][pixels of a launch]
    sar::DevBuf<uint32_t> d_basin_parent;             // [grid^3]
    sar::DevBuf<uint32_t> d_basin_node_root;          // [grid^3]
    sar::DevBuf<unsigned long long> d_basin_extent;   // [6]
    sar::DevBuf<uint16_t> d_basin_rgba;               // [4 * width * height]: sar_runtime_basin_colorize's image
    uint32_t basin_width = 0, basin_height = 0;       // the last basin picture; 0: none (or its call failed)
    uint32_t basin_attractors = 0;

    // sar_runtime_period (sar_period.cpp): the records of the last period plane stay on the device for sar_runtime_period_colorize;
    // the caller's coefficient list of the list form; plain allocations (not the group slab), kept for the next call and freed with
    // the runtime
    uint32_t period_chunk = 0;                        // option: pixels per launch (0 = kDefaultPeriodChunk)
    sar::DevBuf<sar_period_record> d_period_rec;      // [width * height of the largest period plane so far]
    sar::DevBuf<double> d_period_coeffs;              // [width * height][30]
    sar::DevBuf<uint16_t> d_period_rgba;              // [4 * width * height]: sar_runtime_period_colorize's image
    uint32_t period_width = 0, period_height = 0;     // the last period plane; 0: none (or its call failed)

    // sar_runtime_cycles (sar_cycles.cpp): the maps' coefficient blocks, the start points, and of one launch what the starts found, the
    // records and the orbit slots; plain allocations (not the group slab), kept for the next call and freed with the runtime
    uint32_t cycles_chunk = 0;                        // option: (map, start) lanes per launch (0 = kDefaultCyclesChunk)
    sar::DevBuf<sar::SearchCoeffs> d_cycles_coeffs;   // [n_maps]
    sar::DevBuf<double> d_cycles_starts;              // [jobs][3]
    sar::DevBuf<sar::CycleFind> d_cycles_finds;       // [maps of a launch][jobs]
    sar::DevBuf<sar_cycles_record> d_cycles_rec;      // [maps of a launch]
    sar::DevBuf<sar_cycle_orbit> d_cycles_orbits;     // [maps of a launch][cap]

    // auto exposure (sar_runtime_set_exposure): the mode, and the select scratch + record of sar_select.hip's kernels —
    // plain allocations made on first use (not the group slab), kept for the next call and freed with the runtime
    bool expo_on = false;
    sar_exposure_params expo_params{};
    sar::DevBuf<uint32_t> d_expo;        // [kExpoScratchWords]: histograms (zero between calls) + SelectState
    sar::DevBuf<sar_exposure> d_expo_rec;
    // auto colour range (sar_runtime_set_color_range / sar_runtime_hold_color_range): the same
    int32_t crange_mode = sar::kCrOff;
    sar_color_range_params crange_params{};
    sar::DevBuf<uint32_t> d_crange;             // [kCrScratchWords]: histograms (zero between calls) + SelectState
    sar::DevBuf<sar_color_range> d_crange_rec;  // [2]: the measured record, the held one
    // density estimation (sar_runtime_density, sar_density.cpp): the snapshot k_density reads (steps, then count: 12 bytes per pixel),
    // the block its statistics reduce into and the weight plan of the last `samples`; plain allocations made on first use (not the
    // group slab), kept for the next call and freed with the runtime
    uint32_t density_tile = 0;                        // option: rows of a workgroup's tile, 8 / 16 / 32 (0 = kDensityDefaultTileH)
    sar::DevBuf<char> d_density_snap;                 // [12 * npix]
    sar::DevBuf<sar::DensityDeviceStats> d_density_stats;
    sar::DevBuf<uint32_t> d_density_plan;             // [kDensityPlanMaxWords]
    std::map<uint32_t, std::vector<uint32_t>> h_density_plans;  // by S: what d_density_plan is uploaded from (an upload may read it after
                                                      // the call returns, so a plan once made stays with the runtime)
    uint32_t density_plan_samples = 0;                // the S of d_density_plan; 0: none
    // shaded rendering (sar_shade, sar_shade.cpp): the block k_shade's statistics reduce into; a plain allocation made on first use
    sar::DevBuf<sar_shade_stats> d_shade_stats;
    uint64_t colorize_launches = 0;      // statistic: colorize kernels this runtime enqueued, alone or as a batch's leader (test hooks)

    // tuning
    uint32_t block_threads = sar::kDefaultBlock;
    uint32_t ckpt_stride = sar::kDefaultCkptStride;
    uint32_t bins_mode = 0;     // 0 default (binned when eligible), 1 one global atomic per visit, 3 LDS-binned records or an error
    bool timing_accumulate = false;  // spans of successive render calls add up until sar_runtime_last_timing reads them
    uint32_t debug_chunk_jobs = 0;  // test hook: cap on jobs per launch chunk (0 = none)
    uint64_t max_ordinals = 0;      // test hook: visits one launch may order (0 = 2^32-2); longer jobs run as segments
    uint32_t bin_shift = 0;         // 0 = automatic
    uint32_t bin_interleave = 0;    // 0 = automatic, 1 = bins of consecutive pixels, 2 = interleaved bins (BinMap)
    uint32_t splits = 0;            // 0 = automatic
    uint32_t acc_threads = 0;       // threads per k_bin_accumulate block (0 = automatic)
    uint32_t split_waves = 0;       // 2: the iterate kernel as producer / consumer wave pairs (k_iterate_split) where it applies
    uint32_t acc_lists = 0;         // (bin, wave) lists a lane group of k_bin_accumulate walks at the same time: 1, 4 (0 = automatic)
    uint32_t chunk_records = 0;     // records per chunk: 12 / 20 / 28 / 60 (0 = automatic)

    // timing
    bool timing = false;
    std::vector<sar::Span> iter_spans, fold_spans, warm_spans;
    size_t iter_used = 0, fold_used = 0, warm_used = 0;
    sar::Span colorize_span, merge_span;
    bool colorize_timed = false, merge_timed = false;
    uint64_t last_iterations = 0;

    ~sar_runtime();  // waits for the runtime's streams; the members then free themselves
};


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

// sar_runtime.cpp
int clear_hints(sar_runtime* rt);  // hints are lower bounds of depths already accumulated; anything that can lower zbuf voids them
void span_begin(sar_runtime* rt, std::vector<Span>& spans, size_t& used);
void span_end(sar_runtime* rt, std::vector<Span>& spans, size_t& used);
void single_begin(sar_runtime* rt, Span& s);
void single_end(sar_runtime* rt, Span& s, bool& flag);

// sar_render.cpp
void fill_map_params(const sar_config& cfg, MapParams& p);      // render's hoisted constants (:755-764)
void fill_ct_params(const sar_config& cfg, ColorTransformParams& ct);

// Runs n_jobs trajectories of `iters` counted iterations each into rt (sequential job-major semantics); `starts` is
// [n_jobs][3] in host memory, or in device memory with starts_on_device. Enqueues only.
int render_chunked(const sar_config* cfg, sar_runtime* rt, uint32_t n_jobs, uint64_t iters, const double* starts,
                   bool starts_on_device = false);
// colorize of the pixel range [first, first + n) into out_dev (n * 8 bytes). global_scalars: the scalars (max, depth
// range) already hold the values of the WHOLE image (sliced multi-GPU colorize); otherwise the depth range is folded
// over the range first, as colorize does (:877-882).
int colorize_range(const sar_config* cfg, sar_runtime* rt, uint32_t first, uint32_t n, void* out_dev, bool global_scalars);
int check_cfg_matches(const sar_config* cfg, const sar_runtime* rt);
int validate_exposure(const sar_exposure_params* p);
int validate_color_range(const sar_color_range_params* p);
PaletteParams palette_params(const sar_config* cfg);  // Palette::new (:413-418): the entries, the last one duplicated

}  // namespace sar
