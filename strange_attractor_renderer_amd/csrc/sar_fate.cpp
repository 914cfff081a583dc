// sar_fate.cpp — the host half of the basin probes (include/sar.h: sar_runtime_basin_fates, sar_runtime_basin_uncertainty): the
// checks, the lazy upload of the held picture's label table (sar_basin.cpp builds it), the launches of k_basin_fate and k_basin_ladder
// (sar_fate.hip) and the levels' records.
//
// Built with -ffp-contract=off like every file that shares an expression with a kernel.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_fate.hpp"

using namespace sar;

namespace {

int check_points(const char* where, uint32_t n, uint32_t most, const char* most_text, const double* points, const void* out) {
    if (!n || n > most) { set_error("%s: 1 to %s points (%u)", where, most_text, n); return SAR_ERR_INVALID; }
    if (!points || !out) { set_error("%s: the points or the output buffer is NULL", where); return SAR_ERR_INVALID; }
    for (size_t k = 0; k < static_cast<size_t>(n) * 3u; ++k)
        if (!std::isfinite(points[k])) {
            set_error("%s: the points must be finite (point %zu)", where, k / 3u);
            return SAR_ERR_INVALID;
        }
    return SAR_OK;
}

int check_ladder(const sar_basin_ladder_params& p, const char* where) {
    if (!std::isfinite(p.dir[0]) || !std::isfinite(p.dir[1]) || !std::isfinite(p.dir[2])) {
        set_error("%s: dir must be finite", where);
        return SAR_ERR_INVALID;
    }
    if (p.dir[0] == 0. && p.dir[1] == 0. && p.dir[2] == 0.) { set_error("%s: dir must not be all zero", where); return SAR_ERR_INVALID; }
    if (!std::isfinite(p.eps0) || !(p.eps0 > 0.)) { set_error("%s: eps0 must be positive and finite", where); return SAR_ERR_INVALID; }
    if (!p.levels || p.levels > kMaxLadderLevels) {
        set_error("%s: levels must be 1 to %u (%u)", where, kMaxLadderLevels, p.levels);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

// Behind an entry's refusals of its own arguments: the runtime, its held picture, the device, the timing spans, the label table on
// the device (uploaded by the first probe call after a basin call, so that the basin call itself stays as it was) and the argument
// block's share of the held picture.
int probe_begin(sar_runtime* rt, const char* where, FateArgs& a) {
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    BasinState& b = rt->basin;
    if (!b.held) { set_error("%s: the runtime holds no basin picture (a successful sar_runtime_basin first)", where); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));
    if (!b.label_uploaded) {
        HIP_TRY(b.d_node_label.grow(nullptr, b.h_node_label.size()));
        HIP_TRY(hipMemcpyAsync(b.d_node_label, b.h_node_label.data(), b.h_node_label.size() * sizeof(uint32_t), hipMemcpyHostToDevice, rt->stream));
        HIP_TRY(hipStreamSynchronize(rt->stream));
        b.label_uploaded = true;
    }
    std::memset(&a, 0, sizeof(a));
    a.map = b.held_map;
    for (int k = 0; k < 3; ++k) {
        a.box_lo[k] = b.held_box_lo[k];
        a.scale[k] = b.held_scale[k];
    }
    a.bound = b.held_bound;
    a.transient = b.held_transient;
    a.steps = b.held_steps;
    a.grid = b.held_grid;
    a.label = b.d_node_label;
    return SAR_OK;
}

}  // namespace

extern "C" {

int sar_basin_ladder_params_default(sar_basin_ladder_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->dir[0] = 1.;
    out->eps0 = 0.125;
    out->levels = 24;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_basin_fates(sar_runtime* rt, uint32_t n, const double* points_host, sar_basin_fate* fates_out_host,
                            sar_basin_fate_counts* counts_out) try {
    const char* where = "sar_runtime_basin_fates";
    SAR_TRY(check_points(where, n, kMaxFatePoints, "2^24", points_host, fates_out_host));  // (no device needed to refuse the arguments)
    FateArgs a;
    SAR_TRY(probe_begin(rt, where, a));
    const uint32_t slice = std::min(n, kFateChunk);
    HIP_TRY(rt->basin.d_probe.grow(nullptr, static_cast<size_t>(slice) * 3u));
    HIP_TRY(rt->basin.d_fates.grow(nullptr, slice));
    a.points = rt->basin.d_probe;
    a.fates = rt->basin.d_fates;
    for (uint32_t first = 0; first < n; first += slice) {
        a.n = std::min(slice, n - first);
        // (stream order: the last slice's kernel and read-back are done with both buffers before they are written again)
        HIP_TRY(hipMemcpyAsync(rt->basin.d_probe, points_host + static_cast<size_t>(first) * 3u, static_cast<size_t>(a.n) * 3u * sizeof(double),
                               hipMemcpyHostToDevice, rt->stream));
        SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_basin_fate(a, rt->stream); }));
        HIP_TRY(hipMemcpyAsync(fates_out_host + first, rt->basin.d_fates, static_cast<size_t>(a.n) * sizeof(sar_basin_fate), hipMemcpyDeviceToHost,
                               rt->stream));
    }
    HIP_TRY(hipStreamSynchronize(rt->stream));
    if (counts_out) {
        sar_basin_fate_counts c;
        std::memset(&c, 0, sizeof(c));
        c.points = n;
        for (uint32_t i = 0; i < n; ++i) {
            const sar_basin_fate& f = fates_out_host[i];
            ++(f.status != SAR_SEARCH_BOUNDED ? c.diverged : (f.label == kFateUnknown ? c.unknown : c.labelled));
        }
        *counts_out = c;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_basin_uncertainty(sar_runtime* rt, const sar_basin_ladder_params* params, uint32_t n, const double* base_host,
                                  sar_basin_uncertainty_level* levels_out_host, sar_basin_fate* fate0_out_host,
                                  sar_basin_ladder_mask* masks_out_host) try {
    const char* where = "sar_runtime_basin_uncertainty";
    const sar_basin_ladder_params p = given_or_default(params, sar_basin_ladder_params_default);
    SAR_TRY(check_ladder(p, where));  // (no device needed to refuse the arguments)
    SAR_TRY(check_points(where, n, kMaxLadderBases, "2^20", base_host, levels_out_host));
    FateArgs a;
    SAR_TRY(probe_begin(rt, where, a));
    const uint32_t K = p.levels, chunk = std::min(p.chunk ? p.chunk : kDefaultLadderChunk, n);
    for (int k = 0; k < 3; ++k) a.dir[k] = p.dir[k];
    for (uint32_t k = 0; k < K; ++k) a.eps[k] = std::ldexp(p.eps0, -static_cast<int>(k));  // exact (or exactly denormal / zero)
    a.levels = K;
    BasinState& b = rt->basin;
    HIP_TRY(b.d_probe.grow(nullptr, static_cast<size_t>(n) * 3u));
    HIP_TRY(b.d_fates.grow(nullptr, n));
    HIP_TRY(b.d_masks.grow(nullptr, n));
    HIP_TRY(b.d_levels.grow(nullptr, 2u * kMaxLadderLevels));
    HIP_TRY(hipMemcpyAsync(b.d_probe, base_host, static_cast<size_t>(n) * 3u * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemsetAsync(b.d_levels, 0, 2u * kMaxLadderLevels * sizeof(unsigned long long), rt->stream));
    a.counts = b.d_levels;
    for (uint32_t first = 0; first < n; first += chunk) {
        a.n = std::min(chunk, n - first);
        a.points = b.d_probe + static_cast<size_t>(first) * 3u;
        a.fates = b.d_fates + first;
        a.masks = b.d_masks + first;
        SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_basin_ladder(a, rt->stream); }));
    }
    unsigned long long counts[2u * kMaxLadderLevels];
    HIP_TRY(hipMemcpyAsync(counts, b.d_levels, sizeof(counts), hipMemcpyDeviceToHost, rt->stream));
    if (fate0_out_host)
        HIP_TRY(hipMemcpyAsync(fate0_out_host, b.d_fates, static_cast<size_t>(n) * sizeof(sar_basin_fate), hipMemcpyDeviceToHost, rt->stream));
    if (masks_out_host)
        HIP_TRY(hipMemcpyAsync(masks_out_host, b.d_masks, static_cast<size_t>(n) * sizeof(sar_basin_ladder_mask), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    for (uint32_t k = 0; k < K; ++k) {
        sar_basin_uncertainty_level& l = levels_out_host[k];
        if (counts[2u * k] > n || counts[2u * k + 1u] > n - counts[2u * k]) {
            set_error("%s: level %u counts %llu uncertain and %llu unknown of %u base points", where, k + 1u, counts[2u * k], counts[2u * k + 1u], n);
            return SAR_ERR_HIP;
        }
        l.eps = a.eps[k];
        l.uncertain = counts[2u * k];
        l.unknown = counts[2u * k + 1u];
        l.tested = n - l.unknown;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
