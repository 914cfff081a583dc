// sar_rqa.cpp — the host half of the recurrence analysis (include/sar.h: sar_recurrence_*, sar_runtime_recurrence,
// sar_runtime_recurrence_plot, sar_rqa_*, sar_runtime_rqa): the checks, the groups of sets that share the device's point buffer, the
// chunked launches of k_rqa_diag and k_rqa_vert (sar_rqa.hip), the read-back, every map's own threshold from its extent, and the
// measures of sar_rqa_measures. The maps' points come from k_corr_orbit through sar_corr.cpp's orbit half, as sar_runtime_corrdim's do.
//
// Built with -ffp-contract=off: a map's eps2 and the measures are what a restatement in plain IEEE arithmetic gives.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_corr.hpp"
#include "sar_rqa.hpp"
#include "sar_search.hpp"

using namespace sar;

namespace {

int check_lines(const char* where, uint32_t line_bins, uint32_t chunk) {
    if (line_bins < kRqaMinBins || line_bins > kRqaMaxBins) {
        set_error("%s: line_bins must be %u to %u (%u)", where, kRqaMinBins, kRqaMaxBins, line_bins);
        return SAR_ERR_INVALID;
    }
    if (chunk > kMaxRqaChunk) { set_error("%s: chunk must be at most 2^30 workgroups (%u)", where, chunk); return SAR_ERR_INVALID; }
    return SAR_OK;
}

int check_eps2(const char* where, double eps2) {
    if (eps2 > 0. && std::isfinite(eps2)) return SAR_OK;
    set_error("%s: eps2 must be positive and finite", where);
    return SAR_ERR_INVALID;
}

// T of a set of n points, behind the checks of n and samples
int set_samples(const char* where, uint32_t samples, uint32_t n, uint32_t* out) {
    SAR_TRY(check_set_points(where, n));
    const uint32_t s = samples ? samples : n;
    if (n % s) { set_error("%s: samples must divide n (%u, %u)", where, s, n); return SAR_ERR_INVALID; }
    *out = s;
    return SAR_OK;
}

// the pairs i < j outside the Theiler window of `jobs` trajectories of `samples` points
uint64_t window_pairs(uint32_t jobs, uint32_t samples, uint32_t theiler) {
    const uint64_t d = rqa_diagonals(samples, theiler);
    return jobs * (d * (d + 1u) / 2u);
}

// The launches of one group of `sets` sets whose points lie in rt->corr.d_points, with the thresholds eps2[sets]: counts zeroed, then
// k_rqa_diag over sets * jobs * folded bands workgroups and k_rqa_vert over sets * jobs * column tiles, `chunk` per launch, then the
// read-back into `rows` ([sets][rqa_row]). Waits for the stream.
int run_lines(sar_runtime* rt, uint32_t sets, uint32_t jobs, uint32_t samples, uint32_t theiler, uint32_t line_bins, uint32_t chunk,
              const double* eps2, std::vector<unsigned long long>& rows) {
    const uint32_t row = rqa_row(line_bins);
    rows.resize(static_cast<size_t>(sets) * row);
    HIP_TRY(hipMemcpyAsync(rt->rqa.d_eps2, eps2, sets * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemsetAsync(rt->rqa.d_out, 0, rows.size() * sizeof(unsigned long long), rt->stream));
    RqaArgs a;
    std::memset(&a, 0, sizeof(a));
    a.points = rt->corr.d_points;
    a.eps2 = rt->rqa.d_eps2;
    a.out = rt->rqa.d_out;
    a.n = jobs * samples;
    a.jobs = jobs;
    a.samples = samples;
    a.theiler = std::min(theiler, samples);  // (the kernels add to it)
    a.line_bins = line_bins;
    a.rep_shift = rqa_rep_shift(line_bins);
    const uint32_t per = chunk ? chunk : kDefaultRqaChunk;
    if (rqa_diagonals(samples, theiler)) {  // (none: the matrix is all zero)
        a.per_job = rqa_folded_bands(samples, theiler);
        const uint32_t diag_total = sets * jobs * a.per_job;  // (sets * jobs * samples <= 2^24)
        for (uint32_t first = 0; first < diag_total; first += std::min(per, diag_total - first)) {
            const uint32_t count = std::min(per, diag_total - first);
            SAR_TRY(timed_lds_launch(rt, rt->tm.iter, [&] { return launch_rqa_diag(a, first, count, rt->stream); }));
        }
        a.per_job = (samples + kRqaBlock - 1u) / kRqaBlock;
        const uint32_t vert_total = sets * jobs * a.per_job;
        for (uint32_t first = 0; first < vert_total; first += std::min(per, vert_total - first)) {
            const uint32_t count = std::min(per, vert_total - first);
            SAR_TRY(timed_lds_launch(rt, rt->tm.fold, [&] { return launch_rqa_vert(a, first, count, rt->stream); }));
        }
    }
    HIP_TRY(hipMemcpyAsync(rows.data(), rt->rqa.d_out, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
}

// one set's row into the caller's histograms and (nullable) record
void row_out(const unsigned long long* row, uint32_t line_bins, uint64_t pairs, uint64_t* diag, uint64_t* vert, sar_recurrence_record* r) {
    const uint32_t b1 = line_bins + 1u;
    std::memcpy(diag, row, b1 * sizeof(uint64_t));
    std::memcpy(vert, row + b1, b1 * sizeof(uint64_t));
    if (!r) return;
    r->recurrences = row[2u * b1];
    r->pairs = pairs;
    r->diag_lines = r->vert_lines = 0;
    for (uint32_t l = 0; l < b1; ++l) { r->diag_lines += diag[l]; r->vert_lines += vert[l]; }
    r->diag_longest = row[2u * b1 + 1u];
    r->vert_longest = row[2u * b1 + 2u];
}

int grow_lines(sar_runtime* rt, uint32_t group, uint32_t line_bins) {
    HIP_TRY(rt->rqa.d_out.grow(nullptr, static_cast<size_t>(group) * rqa_row(line_bins)));
    HIP_TRY(rt->rqa.d_eps2.grow(nullptr, group));
    return SAR_OK;
}

double quotient(uint64_t num, uint64_t den) {
    return den ? static_cast<double>(num) / static_cast<double>(den) : std::numeric_limits<double>::quiet_NaN();
}

// (total - S) / total, (total - S) / N and the entropy of hist over l >= l_min
void line_measures(const uint64_t* hist, uint32_t line_bins, uint32_t l_min, uint64_t total, double* share, double* mean, double* entr) {
    uint64_t below = 0, lines = 0;
    for (uint32_t l = 1; l < l_min; ++l) below += l * hist[l];
    for (uint32_t l = l_min; l <= line_bins; ++l) lines += hist[l];
    *share = quotient(total - below, total);
    *mean = quotient(total - below, lines);
    if (!entr) return;
    double h = lines ? 0. : std::numeric_limits<double>::quiet_NaN();
    for (uint32_t l = l_min; l <= line_bins && lines; ++l) {
        if (!hist[l]) continue;
        const double p = static_cast<double>(hist[l]) / static_cast<double>(lines);
        h = h - p * std::log(p);
    }
    *entr = h;
}

}  // namespace

extern "C" {

int sar_recurrence_params_default(sar_recurrence_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->line_bins = 256;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_recurrence(sar_runtime* rt, const sar_recurrence_params* p, uint32_t n_sets, uint32_t n, const double* points_host,
                           uint64_t* diag_out_host, uint64_t* vert_out_host, sar_recurrence_record* records_out_host) try {
    const char* where = "sar_runtime_recurrence";
    const sar_recurrence_params d = given_or_default(p, sar_recurrence_params_default);
    SAR_TRY(check_lines(where, d.line_bins, d.chunk));  // (no device needed to refuse the parameters)
    SAR_TRY(check_eps2(where, d.eps2));
    uint32_t samples;
    SAR_TRY(set_samples(where, d.samples, n, &samples));
    if (!n_sets) return SAR_OK;
    if (!points_host || !diag_out_host || !vert_out_host) { set_error("%s: the points or a histogram buffer is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_points_not_nan(where, n_sets, n, points_host));
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_rqa_diag, resolve_ms = k_rqa_vert (sar_timing)
    const uint32_t group = corr_group_size(n_sets, n), jobs = n / samples, b1 = d.line_bins + 1u;
    HIP_TRY(rt->corr.d_points.grow(nullptr, static_cast<size_t>(group) * n * 3u));
    SAR_TRY(grow_lines(rt, group, d.line_bins));
    const std::vector<double> eps2(group, d.eps2);
    const uint64_t pairs = window_pairs(jobs, samples, d.theiler);
    std::vector<unsigned long long> rows;
    return for_staged_sets(rt, n_sets, n, group, points_host, [&](uint32_t first, uint32_t sets) -> int {
        SAR_TRY(run_lines(rt, sets, jobs, samples, d.theiler, d.line_bins, d.chunk, eps2.data(), rows));
        for (uint32_t s = 0; s < sets; ++s)
            row_out(rows.data() + static_cast<size_t>(s) * rqa_row(d.line_bins), d.line_bins, pairs, diag_out_host + static_cast<size_t>(first + s) * b1,
                    vert_out_host + static_cast<size_t>(first + s) * b1, records_out_host ? records_out_host + first + s : nullptr);
        return SAR_OK;
    });
} catch (...) { return sar::abi_caught(); }

int sar_runtime_recurrence_plot(sar_runtime* rt, const sar_recurrence_params* p, uint32_t n, const double* points_host, uint32_t job,
                                uint32_t i0, uint32_t j0, uint32_t height, uint32_t width, uint8_t* out_host) try {
    const char* where = "sar_runtime_recurrence_plot";
    const sar_recurrence_params d = given_or_default(p, sar_recurrence_params_default);
    SAR_TRY(check_lines(where, d.line_bins, d.chunk));
    SAR_TRY(check_eps2(where, d.eps2));
    uint32_t samples;
    SAR_TRY(set_samples(where, d.samples, n, &samples));
    if (job >= n / samples) { set_error("%s: the set has %u trajectories (job %u)", where, n / samples, job); return SAR_ERR_INVALID; }
    SAR_TRY(check_plane_size(where, width, height));
    if (static_cast<uint64_t>(i0) + height > samples || static_cast<uint64_t>(j0) + width > samples) {
        set_error("%s: the window leaves the trajectory of %u points (%u + %u, %u + %u)", where, samples, i0, height, j0, width);
        return SAR_ERR_INVALID;
    }
    if (!points_host || !out_host) { set_error("%s: the points or the picture is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_points_not_nan(where, 1u, n, points_host));
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));
    const size_t pixels = static_cast<size_t>(height) * width;
    HIP_TRY(rt->corr.d_points.grow(nullptr, static_cast<size_t>(samples) * 3u));
    HIP_TRY(rt->rqa.d_plot.grow(nullptr, pixels));
    std::vector<double> soa(static_cast<size_t>(samples) * 3u);
    for (uint32_t i = 0; i < samples; ++i)
        for (uint32_t k = 0; k < 3u; ++k) soa[static_cast<size_t>(k) * samples + i] = points_host[(static_cast<size_t>(job) * samples + i) * 3u + k];
    HIP_TRY(hipMemcpyAsync(rt->corr.d_points, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    RqaPlotArgs a;
    std::memset(&a, 0, sizeof(a));
    a.points = rt->corr.d_points;
    a.out = rt->rqa.d_plot;
    a.samples = samples;
    a.theiler = d.theiler;
    a.i0 = i0;
    a.j0 = j0;
    a.height = height;
    a.width = width;
    a.eps2 = d.eps2;
    SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_rqa_plot(a, rt->stream); }));
    HIP_TRY(hipMemcpyAsync(out_host, rt->rqa.d_plot, pixels, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (the staging leaves with this call)
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_rqa_params_default(sar_rqa_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->jobs = 16;
    out->samples = 1024;
    out->stride = 1;
    out->transient = 1000;
    out->seed = 0;
    out->bound = 1e6;
    out->theiler = 0;
    out->line_bins = 256;
    out->eps2 = 0.;
    out->eps_fraction = 0.05;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_rqa(sar_runtime* rt, const sar_rqa_params* p, uint32_t n_maps, const double* coeffs_host, const double* starts_xyz_host,
                    uint64_t* diag_out_host, uint64_t* vert_out_host, sar_rqa_record* records_out_host, double* points_out_host) try {
    const char* where = "sar_runtime_rqa";
    if (!p) { set_error("%s: the parameters are NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_lines(where, p->line_bins, p->chunk));  // (no device needed to refuse the parameters)
    if (!(p->eps2 >= 0.) || !std::isfinite(p->eps2)) { set_error("%s: eps2 must be 0 or positive and finite", where); return SAR_ERR_INVALID; }
    if (!(p->eps2 > 0.) && !(p->eps_fraction > 0. && std::isfinite(p->eps_fraction))) {
        set_error("%s: eps_fraction must be positive and finite where eps2 is 0", where);
        return SAR_ERR_INVALID;
    }
    const CorrOrbitShape shape = {p->jobs, p->samples, p->stride, p->transient, p->seed, p->bound};
    SAR_TRY(corr_check_shape(where, shape));
    if (!n_maps) return SAR_OK;
    if (!coeffs_host || !diag_out_host || !vert_out_host || !records_out_host) {
        set_error("%s: the coefficients, a histogram buffer or the records are NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(corr_check_maps(where, shape, n_maps, coeffs_host, starts_xyz_host));
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_corr_orbit, iterate_ms = k_rqa_diag, resolve_ms = k_rqa_vert
    const uint32_t samples = p->samples, n = p->jobs * samples, b1 = p->line_bins + 1u;
    const uint32_t group = corr_group_size(n_maps, n);
    SAR_TRY(corr_orbits_begin(rt, shape, starts_xyz_host, group));
    SAR_TRY(grow_lines(rt, group, p->line_bins));
    const uint64_t pairs = window_pairs(p->jobs, samples, p->theiler);
    MapGroupScratch scratch;
    std::vector<double> eps2;
    std::vector<unsigned long long> rows;
    for (uint32_t first = 0; first < n_maps; first += group) {
        const uint32_t maps = std::min(group, n_maps - first);
        SAR_TRY(corr_orbits_run(rt, shape, coeffs_host + static_cast<size_t>(first) * kSearchCoeffs, maps));
        SAR_TRY(read_map_group(rt, scratch, maps, n, records_out_host + first,
                               points_out_host ? points_out_host + static_cast<size_t>(first) * n * 3u : nullptr));
        eps2.assign(maps, 0.);
        for (uint32_t m = 0; m < maps; ++m) {
            sar_rqa_record& r = records_out_host[first + m];
            if (r.status != SAR_SEARCH_BOUNDED) continue;
            double e = p->eps2;
            if (!(e > 0.)) {
                const double dx = r.extent[1] - r.extent[0], dy = r.extent[3] - r.extent[2], dz = r.extent[5] - r.extent[4];
                e = (p->eps_fraction * p->eps_fraction) * ((dx * dx + dy * dy) + dz * dz);
            }
            r.eps2 = eps2[m] = (e > 0. && std::isfinite(e)) ? e : 0.;
        }
        SAR_TRY(run_lines(rt, maps, p->jobs, samples, p->theiler, p->line_bins, p->chunk, eps2.data(), rows));
        for (uint32_t m = 0; m < maps; ++m)
            row_out(rows.data() + static_cast<size_t>(m) * rqa_row(p->line_bins), p->line_bins, eps2[m] > 0. ? pairs : 0u,
                    diag_out_host + static_cast<size_t>(first + m) * b1, vert_out_host + static_cast<size_t>(first + m) * b1,
                    &records_out_host[first + m].counts);
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_rqa_measures(const uint64_t* diag, const uint64_t* vert, const sar_recurrence_record* record, uint32_t line_bins, uint32_t l_min,
                     uint32_t v_min, sar_rqa_measures_out* out) try {
    const char* where = "sar_rqa_measures";
    SAR_TRY(check_lines(where, line_bins, 0u));
    if (!l_min || l_min > line_bins || !v_min || v_min > line_bins) {
        set_error("%s: l_min and v_min must be 1 to line_bins (%u, %u, %u)", where, l_min, v_min, line_bins);
        return SAR_ERR_INVALID;
    }
    if (!diag || !vert || !record || !out) { set_error("%s: a histogram, the record or the result is NULL", where); return SAR_ERR_INVALID; }
    std::memset(out, 0, sizeof(*out));
    out->rr = quotient(record->recurrences, record->pairs);
    line_measures(diag, line_bins, l_min, record->recurrences, &out->det, &out->l_mean, &out->entr);
    out->l_max = record->diag_longest;
    out->div = quotient(1u, record->diag_longest);
    line_measures(vert, line_bins, v_min, 2u * record->recurrences, &out->lam, &out->tt, nullptr);
    out->v_max = record->vert_longest;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
