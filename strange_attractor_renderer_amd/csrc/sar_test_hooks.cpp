// sar_test_hooks.cpp — the A/B and test options of a runtime (include/sar_test_hooks.h). NOT part of libsar_hip.so: this file is
// linked only into the hooks build the test-suite and the A/B tools load (tests/hooks/libsar_hip_hooks.so: the product's own object
// files plus this one), so that the shipped library's ABI is include/sar.h and nothing else.
#include <cmath>
#include <cstring>
#include <limits>
#include <new>
#include <stdexcept>

#include "../../include/sar_test_hooks.h"
#include "sar_plan.hpp"

using namespace sar;

namespace {

// the A/B and test options: {name, field, rule, wide, a, b, size of the set, the set, refusal} (debug_throw needs no runtime and is
// served before the table)
constexpr OptionRule kTestOptions[] = {
    {"path", &Options::bins_mode, OptionRule::kOneOf, false, 0, 0, 3, {0, 1, 3}, "path must be 0 (automatic), 1 (one global atomic per visit) or 3 (LDS-binned records)"},
    {"bin_shift", &Options::bin_shift, OptionRule::kOneOf, false, 0, 0, 6, {0, 12, 13, 14, 15, 16}, "bin_shift must be 12..16"},
    {"bin_interleave", &Options::bin_interleave, OptionRule::kAtMost, false, 2, 0, 0, {}, "bin_interleave must be 0 (automatic), 1 (consecutive-pixel bins) or 2 (interleaved bins)"},
    {"splits", &Options::splits, OptionRule::kAtMost, false, 16, 0, 0, {}, "splits must be 1..16"},
    {"chunk_records", &Options::chunk_records, OptionRule::kOneOf, false, 0, 0, 5, {0, 12, 20, 28, 60}, "chunk_records must be 12, 20, 28 or 60"},
    {"depth_park", &Options::depth_park, OptionRule::kOneOf, false, 0, 0, 4, {0, 2, 4, 8}, "depth_park must be 0 (stage 2 in every step), 2, 4 or 8 (steps a stage-1 passer may wait in its lane)"},
    {"hint_tile", &Options::hint_tile, OptionRule::kAtMost, false, 1, 0, 0, {}, "hint_tile must be 0 (automatic) or 1 (row-major hints)"},
    {"acc_lists", &Options::acc_lists, OptionRule::kOneOf, false, 0, 0, 3, {0, 1, 4}, "acc_lists must be 0 (automatic), 1 or 4"},
    {"hint_shared", &Options::hint_shared, OptionRule::kAtMost, false, 2, 0, 0, {}, "hint_shared must be 0, 1 or 2"},
    {"readback_inline", &Options::readback_inline, OptionRule::kBool, false, 0, 0, 0, {}, nullptr},
    {"batch_starts", &Options::batch_starts, OptionRule::kAtMost, false, 3, 0, 0, {}, "batch_starts must be 0 (automatic), 1 (upload stream), 2 (launch stream) or 3 (read in place)"},
    {"batch_warm", &Options::batch_warm, OptionRule::kAtMost, false, 2, 0, 0, {}, "batch_warm must be 0 (automatic), 1 (one phase) or 2 (two phases)"},
    {"batch_chain", &Options::batch_chain, OptionRule::kBool, false, 0, 0, 0, {}, nullptr},
    {"batch_xcd", &Options::batch_xcd, OptionRule::kAtMost, false, 1, 0, 0, {}, "batch_xcd must be 0 (frames dealt to the XCDs) or 1 (every frame on all XCDs)"},
    {"chunk_ahead", &Options::chunk_ahead, OptionRule::kAtMost, false, 2, 0, 0, {}, "chunk_ahead must be 0, 1 or 2"},
    {"acc_threads", &Options::acc_threads, OptionRule::kOneOf, false, 0, 0, 4, {0, 256, 512, 1024}, "acc_threads must be 256, 512 or 1024"},
    {"corr_replicas", &Options::corr_replicas, OptionRule::kPow2, false, 1, kCorrMaxReplicas, 0, {}, "corr_replicas must be 0 (automatic) or a power of two up to 32"},
    {"debug_chunk_jobs", &Options::debug_chunk_jobs, OptionRule::kAny, false, 0, 0, 0, {}, nullptr},
    {"debug_max_ordinals", nullptr, OptionRule::kCustom, false, 0, 0, 0, {}, nullptr},  // (64 bits, clamped)
};

}  // namespace

extern "C" {

int sar_runtime_set_test_option(sar_runtime* rt, const char* name, uint64_t value) try {
    if (name && !std::strcmp(name, "debug_throw")) {  // (no runtime needed) what an exception inside an entry point becomes at the ABI
        if (value == 1) throw std::bad_alloc();
        if (value == 2) throw std::runtime_error("thrown on request");
        if (value == 3) throw 42;
        return SAR_OK;
    }
    if (!rt || !name) return SAR_ERR_INVALID;
    const uint32_t tile_before = rt->opt.hint_tile;
    int status = SAR_OK;
    const OptionRule* row = set_option_from(kTestOptions, sizeof(kTestOptions) / sizeof(kTestOptions[0]), rt->opt, name, value,
                                            "unknown test option '%s'", status);
    if (status != SAR_OK) return status;
    if (row->field == &Options::hint_tile && rt->opt.hint_tile != tile_before && rt->hints.d_zhint) {  // another layout: the old hints mean nothing
        rt->opt.hint_tile = tile_before;  // (the option changes once they are cleared)
        HIP_TRY(hipSetDevice(rt->device));
        SAR_TRY(rt->hints.clear(rt->npix, rt->stream));
        rt->opt.hint_tile = static_cast<uint32_t>(value);
    }
    if (row->kind == OptionRule::kCustom)  // debug_max_ordinals: visits one launch may order
        rt->opt.max_ordinals = value > kMaxChunkOrdinals ? kMaxChunkOrdinals : value;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

// The individual spans a runtime holds (timing_accumulate: one per launch of every render call since they were last read), in
// launch order: which = 0 iterate, 1 accumulate + fold, 2 warm-up. Synchronises the runtime's stream; clears nothing.
int sar_runtime_debug_spans(sar_runtime* rt, uint32_t which, float* out_ms, uint32_t cap, uint32_t* out_n) try {
    if (!rt || !out_n || which > 2u) return SAR_ERR_INVALID;
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    const SpanList& l = which == 0u ? rt->tm.iter : which == 1u ? rt->tm.fold : rt->tm.warm;
    *out_n = static_cast<uint32_t>(l.used);
    for (size_t k = 0; k < l.used && k < cap && out_ms; ++k) {
        float ms = 0.f;
        out_ms[k] = hipEventElapsedTime(&ms, l.spans[k].a, l.spans[k].b) == hipSuccess ? ms : -1.f;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_debug_colorize_launches(const sar_runtime* rt, uint64_t* out) try {
    if (!rt || !out) return SAR_ERR_INVALID;
    *out = rt->colorize_launches;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

// A volume from the caller's voxels (include/sar_test_hooks.h): sar_runtime_volume's checks, memory and order of events, with an upload
// where that call has its launches. nonempty and vmax are k_volume_reduce's, as after any call; the visits are the voxels' sum.
int sar_runtime_debug_volume_load(sar_runtime* rt, uint32_t slabs, double z_lo, double z_hi, const uint32_t* vol_host) try {
    const char* const where = "sar_runtime_debug_volume_load";
    if (!rt || !vol_host) { set_error("%s: the runtime or the voxels' pointer is NULL", where); return SAR_ERR_INVALID; }
    if (slabs < 1 || slabs > kMaxVolumeSlabs) {  // (check_volume_params' conditions: that function is local to sar_volume.cpp)
        set_error("%s: slabs must be 1 to %u (%u)", where, kMaxVolumeSlabs, slabs);
        return SAR_ERR_INVALID;
    }
    const double span = z_hi - z_lo;
    const double dscale = static_cast<double>(slabs) / span;
    if (!std::isfinite(z_lo) || !std::isfinite(z_hi) || !(span > 0.) || !std::isfinite(dscale)) {
        set_error("%s: z_lo and z_hi must be finite with z_hi - z_lo positive and slabs / (z_hi - z_lo) finite (%g, %g)", where, z_lo, z_hi);
        return SAR_ERR_INVALID;
    }
    const uint64_t voxels = static_cast<uint64_t>(rt->W) * rt->H * slabs;
    if (!voxels || voxels > kMaxVolumeVoxels) {
        set_error("%s: width * height * slabs must be 1 to 2^30 voxels (%llu)", where, static_cast<unsigned long long>(voxels));
        return SAR_ERR_INVALID;
    }
    HIP_TRY(hipSetDevice(rt->device));
    VolumeState& v = rt->volume;
    // (what can fail for want of room comes before the held volume is touched: a refusal leaves it as it was)
    HIP_TRY(v.d_sums.grow(nullptr, 1));
    if (voxels > v.d_vol.cap()) {
        DevBuf<uint32_t> fresh;
        HIP_TRY(fresh.grow(nullptr, voxels));
        HIP_TRY(hipStreamSynchronize(rt->stream));  // (a march of the volume that goes may still run)
        v.drop();
        v.d_vol = std::move(fresh);
    }
    v.held = false;  // from here on a failure leaves no volume held
    HIP_TRY(hipMemcpyAsync(v.d_vol, vol_host, voxels * sizeof(uint32_t), hipMemcpyHostToDevice, rt->stream));
    VolumeSums zero;
    std::memset(&zero, 0, sizeof(zero));
    zero.zmin_key = kVolumeNoMin;
    HIP_TRY(hipMemcpyAsync(v.d_sums, &zero, sizeof(zero), hipMemcpyHostToDevice, rt->stream));
    launch_volume_reduce(v.d_vol, voxels, v.d_sums, rt->stream);
    HIP_TRY(hipGetLastError());
    VolumeSums s;
    HIP_TRY(hipMemcpyAsync(&s, v.d_sums, sizeof(s), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (the caller's voxels and `zero` have been read)

    unsigned long long sum = 0;
    for (uint64_t i = 0; i < voxels; ++i) sum += vol_host[i];
    sar_volume_stats st;
    std::memset(&st, 0, sizeof(st));
    st.visits = sum;
    st.stored = sum;
    st.z_min = std::numeric_limits<float>::infinity();   // no depth is known
    st.z_max = -std::numeric_limits<float>::infinity();
    st.nonempty = s.nonempty;
    st.vmax = s.vmax;
    v.stats = st;
    v.width = rt->W;
    v.height = rt->H;
    v.slabs = slabs;
    v.z_lo = z_lo;
    v.z_hi = z_hi;
    v.held = true;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

// The statistics the runtime keeps for its held volume: what the next add = 1 call continues.
int sar_runtime_debug_volume_stats(const sar_runtime* rt, sar_volume_stats* out) try {
    const char* const where = "sar_runtime_debug_volume_stats";
    if (!rt || !out) { set_error("%s: the runtime or the output is NULL", where); return SAR_ERR_INVALID; }
    if (!rt->volume.held) { set_error("%s: the runtime holds no volume", where); return SAR_ERR_INVALID; }
    *out = rt->volume.stats;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

// The kernels' own logarithm on the caller's arguments (include/sar_test_hooks.h): an upload, k_debug_log with the runtime's table and a
// read-back, all on the runtime's stream; the two buffers are this call's and go with it.
int sar_runtime_debug_device_log(sar_runtime* rt, uint32_t kind, const void* in, uint32_t n, double* out) try {
    const char* const where = "sar_runtime_debug_device_log";
    if (!rt || !in || !out) { set_error("%s: the runtime, the arguments' or the results' pointer is NULL", where); return SAR_ERR_INVALID; }
    if (kind > 1u) { set_error("%s: kind must be 0 (log of doubles) or 1 (ln_u32 of u32) (%u)", where, kind); return SAR_ERR_INVALID; }
    if (n < 1u || n > (1u << 20)) { set_error("%s: n must be 1 to 2^20 (%u)", where, n); return SAR_ERR_INVALID; }
    if (!rt->d_lnlut) { set_error("%s: the runtime holds no logarithm table", where); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    const size_t in_bytes = static_cast<size_t>(n) * (kind ? sizeof(uint32_t) : sizeof(double));
    DevBuf<char> d_in;
    DevBuf<double> d_out;
    HIP_TRY(d_in.grow(nullptr, in_bytes));
    HIP_TRY(d_out.grow(nullptr, n));
    HIP_TRY(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, rt->stream));
    launch_debug_log(kind, d_in, n, rt->d_lnlut, kLnLutEntries, d_out, rt->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, d_out, static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (the buffers are free to go)
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
