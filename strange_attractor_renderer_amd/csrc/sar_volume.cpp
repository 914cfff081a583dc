// sar_volume.cpp — the host half of volume rendering (include/sar.h: sar_volume_*, sar_runtime_volume*): the checks with the family's
// own refusal texts, the held volume and its statistics, the launches of sar_volume.hip's kernels — the warm-up, then the counted
// iterations in launches of "volume_chunk" jobs by "volume_steps" steps —, the section, the march and the read-backs.
//
// Built with -ffp-contract=off: dscale, the march's half count, dpos and the background's three divisions are one IEEE operation
// each, as the restatement has them, and sar_volume_slab must give what k_volume_accumulate's lanes compute.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_volume.hpp"

using namespace sar;

namespace {

int check_volume_params(const sar_volume_params& p, const char* where) {
    if (p.slabs < 1 || p.slabs > kMaxVolumeSlabs) {
        set_error("%s: slabs must be 1 to %u (%u)", where, kMaxVolumeSlabs, p.slabs);
        return SAR_ERR_INVALID;
    }
    const double span = p.z_hi - p.z_lo;
    const double dscale = static_cast<double>(p.slabs) / span;
    if (!std::isfinite(p.z_lo) || !std::isfinite(p.z_hi) || !(span > 0.) || !std::isfinite(dscale)) {
        set_error("%s: z_lo and z_hi must be finite with z_hi - z_lo positive and slabs / (z_hi - z_lo) finite (%g, %g)", where, p.z_lo, p.z_hi);
        return SAR_ERR_INVALID;
    }
    if (p.add != 0 && p.add != 1) { set_error("%s: add must be 0 or 1 (%d)", where, p.add); return SAR_ERR_INVALID; }
    return SAR_OK;
}

int check_volume_window(const VolumeState& v, uint32_t k0, uint32_t k1, const char* where) {
    if (!v.held) { set_error("%s: the runtime holds no volume (sar_runtime_volume first)", where); return SAR_ERR_INVALID; }
    if (!(k0 < k1 && k1 <= v.slabs)) {
        set_error("%s: the window must satisfy 0 <= k0 < k1 <= %u slabs (%u, %u)", where, v.slabs, k0, k1);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

float key_depth(uint32_t key) {  // sortable_f32 (sar_device.hpp) on the host
    const uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

// out: the caller's image. host_image: it is host memory — k_volume_march writes rt->rb.d_rgba and the caller reads it back
int march_launch(const sar_config* cfg, sar_runtime* rt, const sar_volume_march_params* params, sar_volume_march_stats* stats_out, void* out,
                 bool host_image, const char* where) {
    const sar_volume_march_params p = given_or_default(params, sar_volume_march_params_default);
    if (!std::isfinite(p.half_count) || p.half_count < 0.) {
        set_error("%s: half_count must be finite and not negative (%g)", where, p.half_count);
        return SAR_ERR_INVALID;
    }
    if (!(p.t_min >= 0. && p.t_min < 1.)) { set_error("%s: t_min must lie in [0, 1) (%g)", where, p.t_min); return SAR_ERR_INVALID; }
    if (!std::isfinite(p.pos_lo) || !std::isfinite(p.pos_hi)) {
        set_error("%s: pos_lo and pos_hi must be finite (%g, %g)", where, p.pos_lo, p.pos_hi);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(check_cfg_matches(cfg, rt));
    VolumeState& v = rt->volume;
    const uint32_t k1 = (v.held && p.k1 == 0) ? v.slabs : p.k1;  // (k1 == 0: every slab from k0 on)
    SAR_TRY(check_volume_window(v, p.k0, k1, where));
    if (!out) { set_error("%s: the output image is NULL", where); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    if (host_image) {
        HIP_TRY(rt->rb.d_rgba.grow(rt, static_cast<size_t>(rt->npix) * 8));
        SAR_TRY(rt->rb.wait_last_copy(rt->stream));
        out = rt->rb.d_rgba;
    }
    HIP_TRY(v.d_march.grow(nullptr, 1));

    VolumeMarchArgs a;
    std::memset(&a, 0, sizeof(a));
    a.vol = v.d_vol;
    a.out = static_cast<ushort4*>(out);
    a.sums = v.d_march;
    a.npix = rt->npix;
    a.slabs = v.slabs;
    a.k0 = p.k0;
    a.k1 = k1;
    a.transparent = cfg->transparent ? 1 : 0;
    a.half = p.half_count != 0. ? p.half_count : (v.stats.vmax ? static_cast<double>(v.stats.vmax) * 0.125 : 1.0);
    a.t_min = p.t_min;
    a.pos_lo = p.pos_lo;
    a.dpos = p.pos_hi - p.pos_lo;
    a.slabs_f = static_cast<double>(v.slabs);
    for (int c = 0; c < 3; ++c) a.bg[c] = static_cast<double>(p.background[c]) / 65535.0;
    a.pal = palette_params(cfg);

    HIP_TRY(hipMemsetAsync(v.d_march, 0, sizeof(VolumeMarchSums), rt->stream));
    rt->tm.single_begin(rt->tm.colorize_span, rt->stream);
    launch_volume_march(a, rt->stream);
    rt->tm.single_end(rt->tm.colorize_span, rt->tm.colorize_timed, rt->stream);
    HIP_TRY(hipGetLastError());
    if (stats_out) {
        static_assert(sizeof(sar_volume_march_stats) == sizeof(VolumeMarchSums), "the device's block is the record");
        HIP_TRY(hipMemcpyAsync(stats_out, v.d_march, sizeof(VolumeMarchSums), hipMemcpyDeviceToHost, rt->stream));
        if (!host_image) HIP_TRY(hipStreamSynchronize(rt->stream));
    }
    return SAR_OK;
}

}  // namespace

extern "C" {

int sar_volume_params_default(sar_volume_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->z_lo = -1.0;
    out->z_hi = 1.0;
    out->slabs = 64;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_volume_march_params_default(sar_volume_march_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));  // half_count 0: from vmax; t_min 0; the whole depth range; a black background
    out->pos_hi = 1.0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_volume_slab(const sar_volume_params* params, float zf, int32_t* k_out) try {
    const char* const where = "sar_volume_slab";
    if (!params || !k_out) { set_error("%s: the parameters or the output is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_volume_params(*params, where));
    const double dscale = static_cast<double>(params->slabs) / (params->z_hi - params->z_lo);
    *k_out = volume_slab(zf, params->z_lo, dscale, static_cast<double>(params->slabs));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_volume(const sar_config* cfg, sar_runtime* rt, const sar_volume_params* params, uint32_t n_jobs, uint64_t iters_per_job,
                       const double* starts_xyz_host, sar_volume_stats* stats_out) try {
    const char* const where = "sar_runtime_volume";
    const sar_volume_params p = given_or_default(params, sar_volume_params_default);
    SAR_TRY(check_volume_params(p, where));  // (no device needed to refuse the parameters)
    SAR_TRY(validate(cfg));
    const uint64_t voxels = static_cast<uint64_t>(cfg->width) * cfg->height * p.slabs;  // (below 2^31 * 2^10)
    if (voxels > kMaxVolumeVoxels) {
        set_error("%s: width * height * slabs must be at most 2^30 voxels (%llu)", where, static_cast<unsigned long long>(voxels));
        return SAR_ERR_INVALID;
    }
    if (!n_jobs || n_jobs > kMaxVolumeJobs) { set_error("%s: n_jobs must be 1 to 2^24 (%u)", where, n_jobs); return SAR_ERR_INVALID; }
    if (!iters_per_job || iters_per_job > kMaxVolumeIters) {
        set_error("%s: iters_per_job must be 1 to 2^40 (%llu)", where, static_cast<unsigned long long>(iters_per_job));
        return SAR_ERR_INVALID;
    }
    if (starts_xyz_host)
        for (size_t k = 0; k < static_cast<size_t>(n_jobs) * 3u; ++k)
            if (!std::isfinite(starts_xyz_host[k])) {
                set_error("%s: start point %zu is not finite", where, k / 3u);
                return SAR_ERR_INVALID;
            }
    if (!rt || !starts_xyz_host || !stats_out) {
        set_error("%s: the runtime, the start points or the statistics' output is NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(check_cfg_matches(cfg, rt));
    VolumeState& v = rt->volume;
    if (p.add && !(v.held && v.width == rt->W && v.height == rt->H && v.slabs == p.slabs && !std::memcmp(&v.z_lo, &p.z_lo, 8) &&
                   !std::memcmp(&v.z_hi, &p.z_hi, 8))) {
        set_error("%s: add needs a held volume of the same width, height, slabs, z_lo and z_hi", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_volume_warm, iterate_ms = k_volume_accumulate (sar_timing)

    const uint32_t chunk = std::min(rt->opt.volume_chunk ? rt->opt.volume_chunk : kDefaultVolumeChunk, n_jobs);
    const uint64_t steps = rt->opt.volume_steps ? rt->opt.volume_steps : kDefaultVolumeSteps;
    // (what can fail for want of room comes before the held volume is touched: a refusal leaves it as it was)
    HIP_TRY(v.d_state.grow(nullptr, static_cast<size_t>(chunk) * 3u));
    HIP_TRY(v.d_sums.grow(nullptr, 1));
    if (!p.add && voxels > v.d_vol.cap()) {
        DevBuf<uint32_t> fresh;
        HIP_TRY(fresh.grow(nullptr, voxels));
        HIP_TRY(hipStreamSynchronize(rt->stream));  // (a march of the volume that goes may still run)
        v.drop();
        v.d_vol = std::move(fresh);
    }
    const sar_volume_stats before = v.stats;
    const bool adding = p.add != 0;
    v.held = false;  // from here on a failure leaves no volume held
    if (!adding) HIP_TRY(hipMemsetAsync(v.d_vol, 0, voxels * sizeof(uint32_t), rt->stream));

    VolumeSums zero;
    std::memset(&zero, 0, sizeof(zero));
    zero.zmin_key = kVolumeNoMin;
    HIP_TRY(hipMemcpyAsync(v.d_sums, &zero, sizeof(zero), hipMemcpyHostToDevice, rt->stream));

    VolumeArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_map_params(*cfg, a.p);
    a.state = v.d_state;
    a.vol = v.d_vol;
    a.sums = v.d_sums;
    a.z_lo = p.z_lo;
    a.dscale = static_cast<double>(p.slabs) / (p.z_hi - p.z_lo);
    a.slabs_f = static_cast<double>(p.slabs);
    a.width = rt->W;
    a.npix = rt->npix;

    std::vector<double> soa(static_cast<size_t>(n_jobs) * 3u);  // every chunk's [3][m], alive until the stream has been waited for
    for (uint32_t first = 0; first < n_jobs; first += chunk) {
        const uint32_t m = std::min(chunk, n_jobs - first);
        double* const block = soa.data() + static_cast<size_t>(first) * 3u;
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t c = 0; c < 3u; ++c) block[static_cast<size_t>(c) * m + j] = starts_xyz_host[(static_cast<size_t>(first) + j) * 3u + c];
        HIP_TRY(hipMemcpyAsync(v.d_state, block, static_cast<size_t>(m) * 3u * sizeof(double), hipMemcpyHostToDevice, rt->stream));
        a.n_jobs = m;
        a.n_steps = 0;
        SAR_TRY(timed_launch(rt, rt->tm.warm, [&] { launch_volume_warm(a, rt->stream); }));
        for (uint64_t done = 0; done < iters_per_job; done += steps) {
            a.n_steps = static_cast<uint32_t>(std::min(steps, iters_per_job - done));
            SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_volume_accumulate(a, rt->stream); }));
        }
    }
    launch_volume_reduce(v.d_vol, voxels, v.d_sums, rt->stream);
    HIP_TRY(hipGetLastError());
    VolumeSums s;
    HIP_TRY(hipMemcpyAsync(&s, v.d_sums, sizeof(s), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->tm.last_iterations += static_cast<uint64_t>(n_jobs) * iters_per_job;

    sar_volume_stats st;
    std::memset(&st, 0, sizeof(st));
    st.visits = s.visits;
    st.below = s.below;
    st.above = s.above;
    st.nan = s.nan;
    st.stored = s.visits - s.below - s.above - s.nan;
    st.z_min = s.zmin_key == kVolumeNoMin ? std::numeric_limits<float>::infinity() : key_depth(s.zmin_key);
    st.z_max = s.zmax_key == 0u ? -std::numeric_limits<float>::infinity() : key_depth(s.zmax_key);
    if (adding) {  // the held volume's statistics plus this call's visit classes
        st.visits += before.visits;
        st.stored += before.stored;
        st.below += before.below;
        st.above += before.above;
        st.nan += before.nan;
        st.z_min = before.z_min < st.z_min ? before.z_min : st.z_min;
        st.z_max = before.z_max > st.z_max ? before.z_max : st.z_max;
    }
    st.nonempty = s.nonempty;
    st.vmax = s.vmax;
    v.stats = st;
    v.width = rt->W;
    v.height = rt->H;
    v.slabs = p.slabs;
    v.z_lo = p.z_lo;
    v.z_hi = p.z_hi;
    v.held = true;
    *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_volume_free(sar_runtime* rt) try {
    if (!rt) { set_error("sar_runtime_volume_free: the runtime is NULL"); return SAR_ERR_INVALID; }
    if (!rt->volume.d_vol) { rt->volume.held = false; return SAR_OK; }
    HIP_TRY(hipSetDevice(rt->device));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->volume.drop();
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_volume_section(sar_runtime* rt, uint32_t k0, uint32_t k1, uint32_t* count_out_host, int32_t* nearest_out_host) try {
    const char* const where = "sar_runtime_volume_section";
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    VolumeState& v = rt->volume;
    SAR_TRY(check_volume_window(v, k0, k1, where));
    if (!count_out_host && !nearest_out_host) return SAR_OK;
    HIP_TRY(hipSetDevice(rt->device));
    const size_t npix = static_cast<size_t>(v.width) * v.height;
    HIP_TRY(v.d_section.grow(nullptr, npix * 2u));
    VolumeSectionArgs a;
    std::memset(&a, 0, sizeof(a));
    a.vol = v.d_vol;
    a.count = count_out_host ? v.d_section.get() : nullptr;
    a.nearest = nearest_out_host ? reinterpret_cast<int32_t*>(v.d_section.get() + npix) : nullptr;
    a.npix = static_cast<uint32_t>(npix);
    a.k0 = k0;
    a.k1 = k1;
    rt->tm.single_begin(rt->tm.colorize_span, rt->stream);
    launch_volume_section(a, rt->stream);
    rt->tm.single_end(rt->tm.colorize_span, rt->tm.colorize_timed, rt->stream);
    HIP_TRY(hipGetLastError());
    if (count_out_host) HIP_TRY(hipMemcpyAsync(count_out_host, a.count, npix * 4u, hipMemcpyDeviceToHost, rt->stream));
    if (nearest_out_host) HIP_TRY(hipMemcpyAsync(nearest_out_host, a.nearest, npix * 4u, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_volume_read(sar_runtime* rt, uint32_t k0, uint32_t k1, uint32_t* out_host) try {
    const char* const where = "sar_runtime_volume_read";
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    VolumeState& v = rt->volume;
    SAR_TRY(check_volume_window(v, k0, k1, where));
    if (!out_host) { set_error("%s: the output is NULL", where); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    const size_t npix = static_cast<size_t>(v.width) * v.height;
    HIP_TRY(hipMemcpyAsync(out_host, v.d_vol.get() + npix * k0, npix * (k1 - k0) * 4u, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_volume_march_device(const sar_config* cfg, sar_runtime* rt, const sar_volume_march_params* params,
                                    sar_volume_march_stats* stats_out, void* rgba_out_dev) try {
    return march_launch(cfg, rt, params, stats_out, rgba_out_dev, false, "sar_runtime_volume_march_device");
} catch (...) { return sar::abi_caught(); }

int sar_runtime_volume_march(const sar_config* cfg, sar_runtime* rt, const sar_volume_march_params* params, sar_volume_march_stats* stats_out,
                             uint16_t* rgba_out_host) try {
    SAR_TRY(march_launch(cfg, rt, params, stats_out, rgba_out_host, true, "sar_runtime_volume_march"));
    HIP_TRY(hipMemcpyAsync(rgba_out_host, rt->rb.d_rgba, static_cast<size_t>(rt->npix) * 8, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
