// sar_corr.cpp — the host half of the correlation dimension (include/sar.h: sar_pairs_*, sar_runtime_pairs, sar_corrdim_*,
// sar_runtime_corrdim): the checks, the groups of sets that share the device's point buffer, the chunked launches of k_corr_orbit and
// k_corr_pairs (sar_corr.hip), the read-back, and the host finish — the bin edges and the least-squares line of ln C on ln r. The
// orbit half (the checks of a shape and of the maps, the group's buffers, the launches of k_corr_orbit) is shared with
// sar_runtime_boxdim (sar_box.cpp) through sar_corr.hpp; the read-back of a group of maps is sar_analysis.hpp's.
//
// Built with -ffp-contract=off: the edges and the line are what a restatement in plain IEEE arithmetic gives.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_corr.hpp"
#include "sar_search.hpp"

using namespace sar;

namespace {

void pairs_defaults(sar_pairs_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->samples = 0;
    p->theiler = 0;
    p->sub_bits = 2;
    p->e_min = -64;
    p->e_max = 8;
}

int check_binning(uint32_t sub_bits, int32_t e_min, int32_t e_max, const char* where, CorrBinning* out) {
    if (sub_bits > kCorrMaxSubBits) { set_error("%s: sub_bits must be at most %u (%u)", where, kCorrMaxSubBits, sub_bits); return SAR_ERR_INVALID; }
    if (e_min < -1022 || e_max > 1023 || e_max <= e_min) {
        set_error("%s: the exponents must hold -1022 <= e_min < e_max <= 1023 (%d, %d)", where, e_min, e_max);
        return SAR_ERR_INVALID;
    }
    const uint32_t bins = (static_cast<uint32_t>(e_max - e_min) << sub_bits) + 2u;
    if (bins > kCorrMaxBins) { set_error("%s: at most %u bins (%u)", where, kCorrMaxBins, bins); return SAR_ERR_INVALID; }
    if (out) {
        out->base = static_cast<int32_t>(static_cast<uint32_t>(1023 + e_min) << sub_bits) - 1;
        out->top = static_cast<int32_t>(bins) - 1;
        out->shift = 20u - sub_bits;
        out->bins = bins;
    }
    return SAR_OK;
}

// r2_b, the upper edge of bin b < bins - 1: exact
double edge_r2(uint32_t b, uint32_t sub_bits, int32_t e_min) {
    const uint32_t e = b >> sub_bits, m = b & ((1u << sub_bits) - 1u);
    return std::ldexp(1. + static_cast<double>(m) / static_cast<double>(1u << sub_bits), e_min + static_cast<int>(e));
}

// pairs i < j of one trajectory with j - i <= theiler, over n / samples trajectories
uint64_t skipped_pairs(uint32_t n, uint32_t samples, uint32_t theiler) {
    const uint64_t s = samples, d = std::min<uint64_t>(theiler, s - 1u);
    return (n / samples) * (d * s - d * (d + 1u) / 2u);
}

void fit_line(const uint64_t* hist, uint32_t sub_bits, int32_t e_min, uint32_t bins, double c_lo, double r_hi, sar_corrdim_line* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    out->slope = out->intercept = out->rms = nan;
    out->first_bin = out->last_bin = out->used = 0;
    out->status = SAR_CORRDIM_NO_WINDOW;
    std::vector<double> x, y;
    uint64_t c = hist[0];
    uint32_t first = 0, last = 0;
    for (uint32_t b = 1; b + 1u < bins; ++b) {
        c += hist[b];
        const double r2 = edge_r2(b, sub_bits, e_min);
        if (!(static_cast<double>(c) >= c_lo) || !(std::sqrt(r2) <= r_hi)) continue;
        if (x.empty()) first = b;
        last = b;
        x.push_back(0.5 * std::log(r2));
        y.push_back(std::log(static_cast<double>(c)));
    }
    if (x.size() < 3) return;
    fit_least_squares(x.data(), y.data(), x.size(), &out->slope, &out->intercept, &out->rms);
    out->first_bin = first;
    out->last_bin = last;
    out->used = static_cast<uint32_t>(x.size());
    out->status = SAR_CORRDIM_FIT_OK;
}

int check_window(double c_lo, double r_hi, const char* where, const char* r_name) {
    if (!(c_lo >= 1.)) { set_error("%s: c_lo must be at least 1 pair", where); return SAR_ERR_INVALID; }
    if (!(r_hi > 0.)) { set_error("%s: %s must be positive", where, r_name); return SAR_ERR_INVALID; }
    return SAR_OK;
}

// The pair launches of one group of `sets` sets whose points lie in rt->corr.d_points: histograms zeroed, then every cell of the
// folded triangle for every set, at most `corr_chunk` workgroups per launch, then the read-back of the histograms into hist_out_host.
// Enqueues only.
int run_pairs(sar_runtime* rt, uint32_t sets, uint32_t n, uint32_t samples, uint32_t theiler, const CorrBinning& bin, bool with_state,
              uint64_t* hist_out_host) {
    HIP_TRY(hipMemsetAsync(rt->corr.d_hist, 0, static_cast<size_t>(sets) * bin.bins * sizeof(unsigned long long), rt->stream));
    CorrPairsArgs a;
    std::memset(&a, 0, sizeof(a));
    a.points = rt->corr.d_points;
    a.state = with_state ? rt->corr.d_state.get() : nullptr;
    a.hist = rt->corr.d_hist;
    a.nt = (n + kCorrTile - 1u) / kCorrTile;
    a.fold_m = corr_fold_m(a.nt);
    a.n = n;
    a.samples = samples;
    a.theiler = std::min(theiler, n);
    a.bin = bin;
    uint32_t rep = rt->opt.corr_replicas ? rt->opt.corr_replicas : kCorrMaxReplicas;  // the copies the LDS budget holds
    while (rep > 1u && (bin.bins + 1u) * rep * 4u > kCorrHistLdsBytes) rep >>= 1;  // (+ the spare row)
    while ((1u << a.rep_shift) < rep) ++a.rep_shift;
    const uint64_t cells = corr_fold_cells(a.nt);
    const uint64_t chunk = rt->opt.corr_chunk ? rt->opt.corr_chunk : kDefaultCorrChunk;
    auto launch = [&](uint32_t first_cell, uint32_t n_cells, uint32_t first_set, uint32_t n_sets) -> int {
        return timed_lds_launch(rt, rt->tm.iter, [&] { return launch_corr_pairs(a, first_cell, n_cells, first_set, n_sets, rt->stream); });
    };
    if (cells > chunk) {  // a set takes several launches
        for (uint32_t set = 0; set < sets; ++set)
            for (uint64_t first = 0; first < cells; first += chunk)
                SAR_TRY(launch(static_cast<uint32_t>(first), static_cast<uint32_t>(std::min<uint64_t>(chunk, cells - first)), set, 1u));
    } else {  // a launch takes several whole sets
        const uint32_t per = static_cast<uint32_t>(std::min<uint64_t>(chunk / cells, kCorrMaxGridY));
        for (uint32_t set = 0; set < sets; set += per) SAR_TRY(launch(0u, static_cast<uint32_t>(cells), set, std::min(per, sets - set)));
    }
    HIP_TRY(hipMemcpyAsync(hist_out_host, rt->corr.d_hist, static_cast<size_t>(sets) * bin.bins * sizeof(uint64_t), hipMemcpyDeviceToHost, rt->stream));
    return SAR_OK;
}

}  // namespace

namespace sar {

uint32_t corr_group_size(uint32_t n_sets, uint32_t n) {
    const uint64_t fit = std::max<uint64_t>(1u, kCorrPointBudget / n);
    return static_cast<uint32_t>(std::min<uint64_t>(n_sets, fit));
}

int corr_check_shape(const char* where, const CorrOrbitShape& s) {
    if (!s.jobs || s.jobs > kCorrMaxJobs) { set_error("%s: jobs must be 1 to 2^16 (%u)", where, s.jobs); return SAR_ERR_INVALID; }
    if (!s.samples || !s.stride) { set_error("%s: samples and stride must be at least 1", where); return SAR_ERR_INVALID; }
    if (static_cast<uint64_t>(s.jobs) * s.samples > kCorrMaxPoints) {
        set_error("%s: jobs * samples must be at most 2^20 points (%u, %u)", where, s.jobs, s.samples);
        return SAR_ERR_INVALID;
    }
    if (s.transient > kMaxSearchSteps || static_cast<uint64_t>(s.stride) * s.samples > kMaxSearchSteps) {
        set_error("%s: transient and stride * samples must be at most 2^31 (%u, %u * %u)", where, s.transient, s.stride, s.samples);
        return SAR_ERR_INVALID;
    }
    return check_bound(where, s.bound);
}

int corr_check_maps(const char* where, const CorrOrbitShape& s, uint32_t n_maps, const double* coeffs_host, const double* starts_xyz_host) {
    for (size_t k = 0; k < static_cast<size_t>(n_maps) * kSearchCoeffs; ++k)
        if (!std::isfinite(coeffs_host[k])) {
            set_error("%s: the coefficients must be finite (map %zu, entry %zu)", where, k / kSearchCoeffs, k % kSearchCoeffs);
            return SAR_ERR_INVALID;
        }
    if (starts_xyz_host)
        for (size_t k = 0; k < static_cast<size_t>(s.jobs) * 3u; ++k)
            if (!std::isfinite(starts_xyz_host[k])) { set_error("%s: the start points must be finite (job %zu)", where, k / 3u); return SAR_ERR_INVALID; }
    return SAR_OK;
}

int corr_orbits_begin(sar_runtime* rt, const CorrOrbitShape& s, const double* starts_xyz_host, uint32_t group) {
    const uint32_t jobs = s.jobs, n = jobs * s.samples;
    std::vector<double> drawn;
    SAR_TRY(starts_or_drawn(starts_xyz_host, s.seed, jobs, drawn));
    HIP_TRY(rt->corr.d_points.grow(nullptr, static_cast<size_t>(group) * n * 3u));
    HIP_TRY(rt->corr.d_state.grow(nullptr, group));
    HIP_TRY(rt->corr.d_coeffs.grow(nullptr, static_cast<size_t>(group) * kSearchCoeffs));
    HIP_TRY(rt->corr.d_starts.grow(nullptr, static_cast<size_t>(jobs) * 3u));
    HIP_TRY(hipMemcpyAsync(rt->corr.d_starts, starts_xyz_host, static_cast<size_t>(jobs) * 3u * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    if (!drawn.empty()) HIP_TRY(hipStreamSynchronize(rt->stream));  // (the drawn points leave with this call)
    return SAR_OK;
}

int corr_orbits_run(sar_runtime* rt, const CorrOrbitShape& s, const double* coeffs_host, uint32_t maps) {
    CorrOrbitArgs o;
    std::memset(&o, 0, sizeof(o));
    o.coeffs = rt->corr.d_coeffs;
    o.starts = rt->corr.d_starts;
    o.points = rt->corr.d_points;
    o.state = rt->corr.d_state;
    o.jobs = s.jobs;
    o.samples = s.samples;
    o.stride = s.stride;
    o.transient = s.transient;
    o.n = s.jobs * s.samples;
    o.bound = s.bound;
    const uint64_t chunk = rt->opt.corr_chunk ? rt->opt.corr_chunk : kDefaultCorrChunk;
    const uint32_t blocks = (s.jobs + 255u) / 256u;
    const uint32_t maps_per_launch = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(1u, chunk / blocks), kCorrMaxGridY));

    CorrMapState fresh;
    fresh.fail = kCorrNoFail;
    for (int k = 0; k < 3; ++k) { fresh.lo[k] = ~0ull; fresh.hi[k] = 0ull; }
    const std::vector<CorrMapState> state(maps, fresh);
    std::vector<double> coeffs(static_cast<size_t>(maps) * kSearchCoeffs);
    canonical_coeffs(coeffs_host, coeffs.size(), coeffs.data());
    HIP_TRY(hipMemcpyAsync(rt->corr.d_coeffs, coeffs.data(), coeffs.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(rt->corr.d_state, state.data(), maps * sizeof(CorrMapState), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (both vectors leave with this call)
    for (uint32_t m = 0; m < maps; m += maps_per_launch) {
        o.first_map = m;
        SAR_TRY(timed_launch(rt, rt->tm.warm, [&] { launch_corr_orbit(o, std::min(maps_per_launch, maps - m), rt->stream); }));
    }
    return SAR_OK;
}

}  // namespace sar

extern "C" {

int sar_pairs_params_default(sar_pairs_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    pairs_defaults(out);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_pairs_edges(const sar_pairs_params* p, uint32_t* bins_out, double* r_out) try {
    sar_pairs_params d;
    if (!p) { pairs_defaults(&d); p = &d; }
    CorrBinning bin;
    SAR_TRY(check_binning(p->sub_bits, p->e_min, p->e_max, "sar_pairs_edges", &bin));
    if (bins_out) *bins_out = bin.bins;
    if (r_out) {
        for (uint32_t b = 0; b + 1u < bin.bins; ++b) r_out[b] = std::sqrt(edge_r2(b, p->sub_bits, p->e_min));
        r_out[bin.bins - 1u] = std::numeric_limits<double>::infinity();
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_corrdim_fit(const uint64_t* hist, const sar_pairs_params* binning, double c_lo, double r_hi, sar_corrdim_line* out) try {
    sar_pairs_params d;
    if (!binning) { pairs_defaults(&d); binning = &d; }
    CorrBinning bin;
    SAR_TRY(check_binning(binning->sub_bits, binning->e_min, binning->e_max, "sar_corrdim_fit", &bin));
    SAR_TRY(check_window(c_lo, r_hi, "sar_corrdim_fit", "r_hi"));
    if (!hist || !out) { set_error("sar_corrdim_fit: the histogram or the result is NULL"); return SAR_ERR_INVALID; }
    fit_line(hist, binning->sub_bits, binning->e_min, bin.bins, c_lo, r_hi, out);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_pairs(sar_runtime* rt, const sar_pairs_params* p, uint32_t n_sets, uint32_t n, const double* points_host,
                      uint64_t* hist_out_host, sar_pairs_counts* counts_out_host) try {
    sar_pairs_params d;
    if (!p) { pairs_defaults(&d); p = &d; }
    CorrBinning bin;
    SAR_TRY(check_binning(p->sub_bits, p->e_min, p->e_max, "sar_runtime_pairs", &bin));  // (no device needed to refuse the parameters)
    const uint32_t samples = p->samples ? p->samples : n;
    SAR_TRY(check_set_points("sar_runtime_pairs", n));
    if (!samples || n % samples) { set_error("sar_runtime_pairs: samples must divide n (%u, %u)", samples, n); return SAR_ERR_INVALID; }
    if (!n_sets) return SAR_OK;
    if (!points_host || !hist_out_host) { set_error("sar_runtime_pairs: the points or the histogram buffer is NULL"); return SAR_ERR_INVALID; }
    SAR_TRY(check_points_not_nan("sar_runtime_pairs", n_sets, n, points_host));
    if (!rt) { set_error("sar_runtime_pairs: the runtime is NULL"); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_corr_orbit, iterate_ms = k_corr_pairs (sar_timing)
    const uint32_t group = corr_group_size(n_sets, n);
    HIP_TRY(rt->corr.d_points.grow(nullptr, static_cast<size_t>(group) * n * 3u));
    HIP_TRY(rt->corr.d_hist.grow(nullptr, static_cast<size_t>(group) * bin.bins));
    SAR_TRY(for_staged_sets(rt, n_sets, n, group, points_host, [&](uint32_t first, uint32_t sets) -> int {
        SAR_TRY(run_pairs(rt, sets, n, samples, p->theiler, bin, false, hist_out_host + static_cast<size_t>(first) * bin.bins));
        HIP_TRY(hipStreamSynchronize(rt->stream));
        return SAR_OK;
    }));
    if (counts_out_host)
        for (uint32_t s = 0; s < n_sets; ++s) {
            uint64_t c = 0;
            for (uint32_t b = 0; b < bin.bins; ++b) c += hist_out_host[static_cast<size_t>(s) * bin.bins + b];
            counts_out_host[s].counted = c;
            counts_out_host[s].skipped = skipped_pairs(n, samples, p->theiler);
        }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_corrdim_params_default(sar_corrdim_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->jobs = 256;
    out->samples = 128;
    out->stride = 4;
    out->transient = 1000;
    out->theiler = 0;
    out->sub_bits = 2;
    out->e_min = -64;
    out->e_max = 8;
    out->seed = 0;
    out->bound = 1e6;
    out->c_lo = 100.;
    out->r_hi_fraction = 0x1.0p-4;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_corrdim(sar_runtime* rt, const sar_corrdim_params* p, uint32_t n_maps, const double* coeffs_host, const double* starts_xyz_host,
                        uint64_t* hist_out_host, sar_corrdim_record* records_out_host, double* points_out_host) try {
    const char* where = "sar_runtime_corrdim";
    if (!p) { set_error("%s: the parameters are NULL", where); return SAR_ERR_INVALID; }
    CorrBinning bin;
    SAR_TRY(check_binning(p->sub_bits, p->e_min, p->e_max, where, &bin));  // (no device needed to refuse the parameters)
    const CorrOrbitShape shape = {p->jobs, p->samples, p->stride, p->transient, p->seed, p->bound};
    SAR_TRY(corr_check_shape(where, shape));
    SAR_TRY(check_window(p->c_lo, p->r_hi_fraction, where, "r_hi_fraction"));
    if (!n_maps) return SAR_OK;
    if (!coeffs_host || !hist_out_host || !records_out_host) {
        set_error("%s: the coefficients, the histogram buffer or the records are NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(corr_check_maps(where, shape, n_maps, coeffs_host, starts_xyz_host));
    const uint32_t samples = p->samples, n = p->jobs * samples;
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_corr_orbit, iterate_ms = k_corr_pairs (sar_timing)

    const uint32_t group = corr_group_size(n_maps, n);
    SAR_TRY(corr_orbits_begin(rt, shape, starts_xyz_host, group));
    HIP_TRY(rt->corr.d_hist.grow(nullptr, static_cast<size_t>(group) * bin.bins));

    MapGroupScratch scratch;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint32_t first = 0; first < n_maps; first += group) {
        const uint32_t maps = std::min(group, n_maps - first);
        SAR_TRY(corr_orbits_run(rt, shape, coeffs_host + static_cast<size_t>(first) * kSearchCoeffs, maps));
        SAR_TRY(run_pairs(rt, maps, n, samples, p->theiler, bin, true, hist_out_host + static_cast<size_t>(first) * bin.bins));
        SAR_TRY(read_map_group(rt, scratch, maps, n, records_out_host + first,
                               points_out_host ? points_out_host + static_cast<size_t>(first) * n * 3u : nullptr));
        for (uint32_t m = 0; m < maps; ++m) {
            sar_corrdim_record& r = records_out_host[first + m];
            const uint64_t* hist = hist_out_host + static_cast<size_t>(first + m) * bin.bins;
            if (r.status != SAR_SEARCH_BOUNDED) {
                r.r_hi = nan;
                r.line.slope = r.line.intercept = r.line.rms = nan;
                r.line.status = SAR_CORRDIM_NO_WINDOW;
                continue;
            }
            for (uint32_t b = 0; b < bin.bins; ++b) r.counted += hist[b];
            r.skipped = skipped_pairs(n, samples, p->theiler);
            const double dx = r.extent[1] - r.extent[0], dy = r.extent[3] - r.extent[2], dz = r.extent[5] - r.extent[4];
            r.r_hi = p->r_hi_fraction * std::sqrt((dx * dx + dy * dy) + dz * dz);
            fit_line(hist, p->sub_bits, p->e_min, bin.bins, p->c_lo, r.r_hi, &r.line);
        }
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
