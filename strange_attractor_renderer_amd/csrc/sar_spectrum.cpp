// sar_spectrum.cpp — the host half of the power spectra (include/sar.h: sar_spectra_*, sar_runtime_spectra, sar_spectrum_*,
// sar_runtime_spectrum): the twiddle and window tables, the checks, the groups of sets that share the device's point buffer, the
// chunked launches of k_spectrum and the launch of k_spectrum_fold (sar_spectrum.hip), and the read-back. The maps' points come
// from k_corr_orbit through sar_corr.cpp's orbit half, as sar_runtime_corrdim's and sar_runtime_boxdim's do.
//
// Built with -ffp-contract=off: the tables are what a restatement in plain IEEE arithmetic over the same libm gives.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_corr.hpp"
#include "sar_search.hpp"
#include "sar_spectrum.hpp"

using namespace sar;

namespace {

// log2 of a power of two N in 8..4096, or 0
uint32_t transform_log2(uint32_t n) {
    for (uint32_t l = kSpectrumMinLog2; l <= kSpectrumMaxLog2; ++l)
        if (n == (1u << l)) return l;
    return 0u;
}

int check_transform(const char* where, uint32_t n, uint32_t hop, uint32_t window, const double proj[3], uint32_t chunk) {
    if (!transform_log2(n)) { set_error("%s: n must be a power of two from 8 to %u (%u)", where, kSpectrumMaxN, n); return SAR_ERR_INVALID; }
    if (!hop || hop > n) { set_error("%s: hop must be 1 to n (%u, n = %u)", where, hop, n); return SAR_ERR_INVALID; }
    if (window != SAR_WINDOW_RECT && window != SAR_WINDOW_HANN) {
        set_error("%s: the window must be SAR_WINDOW_RECT or SAR_WINDOW_HANN (%u)", where, window);
        return SAR_ERR_INVALID;
    }
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(proj[k])) { set_error("%s: proj must be finite", where); return SAR_ERR_INVALID; }
    if (chunk > kMaxSpectrumChunk) { set_error("%s: chunk must be at most 2^30 workgroups (%u)", where, chunk); return SAR_ERR_INVALID; }
    return SAR_OK;
}

void make_twiddles(uint32_t n, double* out) {
    for (uint32_t k = 0; k < n / 2u; ++k) {
        const double angle = 2.0 * M_PI * static_cast<double>(k) / static_cast<double>(n);
        out[2u * k] = std::cos(angle);
        out[2u * k + 1u] = -std::sin(angle);
    }
}

void make_window(uint32_t window, uint32_t n, double* out) {
    for (uint32_t t = 0; t < n; ++t)
        out[t] = window == SAR_WINDOW_RECT ? 1.0 : 0.5 - 0.5 * std::cos(2.0 * M_PI * static_cast<double>(t) / static_cast<double>(n));
}

// the trajectories and segments of a set of n_points points under checked transform parameters
int set_shape(const char* where, const sar_spectra_params* p, uint32_t n_points, uint32_t* samples, uint32_t* jobs, uint32_t* segments) {
    SAR_TRY(check_set_points(where, n_points));
    const uint32_t s = p->samples ? p->samples : n_points;
    if (n_points % s) { set_error("%s: samples must divide n_points (%u, %u)", where, s, n_points); return SAR_ERR_INVALID; }
    if (s < p->n) { set_error("%s: samples must be at least n: a trajectory holds no segment (%u, n = %u)", where, s, p->n); return SAR_ERR_INVALID; }
    *samples = s;
    *jobs = n_points / s;
    *segments = (s - p->n) / p->hop + 1u;
    return SAR_OK;
}

// The tables up and the argument block of one call's launches; the buffers for groups of `group` sets
int spectrum_begin(sar_runtime* rt, uint32_t n, uint32_t hop, uint32_t window, const double proj[3], uint32_t jobs, uint32_t samples,
                   uint32_t segments, uint32_t group, SpectrumArgs* out) {
    SpectrumArgs a;
    std::memset(&a, 0, sizeof(a));
    a.log2n = transform_log2(n);
    a.hop = hop;
    a.jobs = jobs;
    a.samples = samples;
    a.segments = segments;
    a.n_points = jobs * samples;
    a.row = n / 2u + 2u;
    a.inv_n = 1.0 / static_cast<double>(n);
    for (int k = 0; k < 3; ++k) a.proj[k] = proj[k];
    std::vector<double> tables(2u * static_cast<size_t>(n));  // the twiddles, then the window
    make_twiddles(n, tables.data());
    make_window(window, n, tables.data() + n);
    HIP_TRY(rt->spectrum.d_tables.grow(nullptr, tables.size()));
    HIP_TRY(rt->spectrum.d_scratch.grow(nullptr, static_cast<size_t>(group) * jobs * a.row));
    HIP_TRY(rt->spectrum.d_power.grow(nullptr, static_cast<size_t>(group) * a.row));
    HIP_TRY(hipMemcpyAsync(rt->spectrum.d_tables, tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (the tables leave with this call)
    a.twiddles = rt->spectrum.d_tables;
    a.window = rt->spectrum.d_tables + n;
    a.scratch = rt->spectrum.d_scratch;
    a.power = rt->spectrum.d_power;
    *out = a;
    return SAR_OK;
}

// One group of `sets` sets whose points lie in rt->corr.d_points: k_spectrum over its sets * jobs workgroups, `chunk` per launch,
// then k_spectrum_fold; the rows come back into `rows` ([sets][row]). Waits for the stream.
int run_spectra(sar_runtime* rt, SpectrumArgs a, uint32_t chunk, uint32_t sets, bool with_state, std::vector<double>& rows) {
    a.points = rt->corr.d_points;
    a.state = with_state ? rt->corr.d_state.get() : nullptr;
    const uint32_t total = sets * a.jobs, per = chunk ? chunk : kDefaultSpectrumChunk;  // (sets * jobs <= 2^24 / samples)
    for (uint32_t first = 0; first < total; first += std::min(per, total - first)) {
        const uint32_t count = std::min(per, total - first);
        SAR_TRY(timed_lds_launch(rt, rt->tm.iter, [&] { return launch_spectrum(a, first, count, rt->stream); }));
    }
    SAR_TRY(timed_launch(rt, rt->tm.fold, [&] { launch_spectrum_fold(a, sets, rt->stream); }));
    rows.resize(static_cast<size_t>(sets) * a.row);
    HIP_TRY(hipMemcpyAsync(rows.data(), rt->spectrum.d_power, rows.size() * sizeof(double), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
}

}  // namespace

extern "C" {

int sar_spectra_params_default(sar_spectra_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->n = 1024;
    out->hop = 512;
    out->window = SAR_WINDOW_HANN;
    out->proj[0] = 1.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_spectrum_twiddles(uint32_t n, double* out) try {
    if (!transform_log2(n)) { set_error("sar_spectrum_twiddles: n must be a power of two from 8 to %u (%u)", kSpectrumMaxN, n); return SAR_ERR_INVALID; }
    if (!out) { set_error("sar_spectrum_twiddles: the table is NULL"); return SAR_ERR_INVALID; }
    make_twiddles(n, out);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_spectrum_window(uint32_t window, uint32_t n, double* out) try {
    const double proj[3] = {1., 0., 0.};
    SAR_TRY(check_transform("sar_spectrum_window", n, 1u, window, proj, 0u));
    if (!out) { set_error("sar_spectrum_window: the table is NULL"); return SAR_ERR_INVALID; }
    make_window(window, n, out);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_spectra_segments(const sar_spectra_params* p, uint32_t n_points, uint32_t* jobs_out, uint32_t* segments_out) try {
    const char* where = "sar_spectra_segments";
    const sar_spectra_params d = given_or_default(p, sar_spectra_params_default);
    SAR_TRY(check_transform(where, d.n, d.hop, d.window, d.proj, d.chunk));
    uint32_t samples, jobs, segments;
    SAR_TRY(set_shape(where, &d, n_points, &samples, &jobs, &segments));
    if (jobs_out) *jobs_out = jobs;
    if (segments_out) *segments_out = segments;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_spectra(sar_runtime* rt, const sar_spectra_params* p, uint32_t n_sets, uint32_t n_points, const double* points_host,
                        double* power_out_host, sar_spectra_record* records_out_host) try {
    const char* where = "sar_runtime_spectra";
    const sar_spectra_params d = given_or_default(p, sar_spectra_params_default);
    SAR_TRY(check_transform(where, d.n, d.hop, d.window, d.proj, d.chunk));  // (no device needed to refuse the parameters)
    uint32_t samples, jobs, segments;
    SAR_TRY(set_shape(where, &d, n_points, &samples, &jobs, &segments));
    if (!n_sets) return SAR_OK;
    if (!points_host || !power_out_host) { set_error("%s: the points or the power buffer is NULL", where); return SAR_ERR_INVALID; }
    const size_t total = static_cast<size_t>(n_sets) * n_points * 3u;
    for (size_t k = 0; k < total; ++k)
        if (!std::isfinite(points_host[k])) {
            set_error("%s: coordinate %zu of point %zu of set %zu is not finite", where, k % 3u, k / 3u % n_points, k / 3u / n_points);
            return SAR_ERR_INVALID;
        }
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_spectrum, resolve_ms = k_spectrum_fold (sar_timing)
    const uint32_t group = corr_group_size(n_sets, n_points), bins = d.n / 2u + 1u;
    HIP_TRY(rt->corr.d_points.grow(nullptr, static_cast<size_t>(group) * n_points * 3u));
    SpectrumArgs a;
    SAR_TRY(spectrum_begin(rt, d.n, d.hop, d.window, d.proj, jobs, samples, segments, group, &a));
    std::vector<double> rows;
    return for_staged_sets(rt, n_sets, n_points, group, points_host, [&](uint32_t first, uint32_t sets) -> int {
        SAR_TRY(run_spectra(rt, a, d.chunk, sets, false, rows));
        for (uint32_t s = 0; s < sets; ++s) {
            const double* row = rows.data() + static_cast<size_t>(s) * a.row;
            std::memcpy(power_out_host + static_cast<size_t>(first + s) * bins, row, bins * sizeof(double));
            if (records_out_host) {
                sar_spectra_record& r = records_out_host[first + s];
                r.jobs = jobs;
                r.segments = segments;
                r.energy = row[bins];
            }
        }
        return SAR_OK;
    });
} catch (...) { return sar::abi_caught(); }

int sar_spectrum_params_default(sar_spectrum_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->jobs = 16;
    out->segments = 15;
    out->n = 1024;
    out->hop = 512;
    out->window = SAR_WINDOW_HANN;
    out->stride = 1;
    out->transient = 1000;
    out->seed = 0;
    out->bound = 1e6;
    out->proj[0] = 1.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_spectrum(sar_runtime* rt, const sar_spectrum_params* p, uint32_t n_maps, const double* coeffs_host, const double* starts_xyz_host,
                         double* power_out_host, sar_spectrum_record* records_out_host, double* points_out_host) try {
    const char* where = "sar_runtime_spectrum";
    if (!p) { set_error("%s: the parameters are NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_transform(where, p->n, p->hop, p->window, p->proj, p->chunk));  // (no device needed to refuse the parameters)
    if (!p->segments) { set_error("%s: segments must be at least 1", where); return SAR_ERR_INVALID; }
    // samples = (segments - 1) * hop + n; beyond 2^20 the shape's check refuses it with any jobs
    const uint64_t samples64 = static_cast<uint64_t>(p->segments - 1u) * p->hop + p->n;
    const uint32_t samples = static_cast<uint32_t>(std::min<uint64_t>(samples64, kCorrMaxPoints + 1u));
    const CorrOrbitShape shape = {p->jobs, samples, p->stride, p->transient, p->seed, p->bound};
    SAR_TRY(corr_check_shape(where, shape));
    if (!n_maps) return SAR_OK;
    if (!coeffs_host || !power_out_host || !records_out_host) {
        set_error("%s: the coefficients, the power buffer or the records are NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(corr_check_maps(where, shape, n_maps, coeffs_host, starts_xyz_host));
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_corr_orbit, iterate_ms = k_spectrum, resolve_ms = k_spectrum_fold
    const uint32_t n_points = p->jobs * samples, bins = p->n / 2u + 1u;
    const uint32_t group = corr_group_size(n_maps, n_points);
    SAR_TRY(corr_orbits_begin(rt, shape, starts_xyz_host, group));
    SpectrumArgs a;
    SAR_TRY(spectrum_begin(rt, p->n, p->hop, p->window, p->proj, p->jobs, samples, p->segments, group, &a));
    MapGroupScratch scratch;
    std::vector<double> rows;
    for (uint32_t first = 0; first < n_maps; first += group) {
        const uint32_t maps = std::min(group, n_maps - first);
        SAR_TRY(corr_orbits_run(rt, shape, coeffs_host + static_cast<size_t>(first) * kSearchCoeffs, maps));
        SAR_TRY(run_spectra(rt, a, p->chunk, maps, true, rows));
        SAR_TRY(read_map_group(rt, scratch, maps, n_points, records_out_host + first,
                               points_out_host ? points_out_host + static_cast<size_t>(first) * n_points * 3u : nullptr));
        for (uint32_t m = 0; m < maps; ++m) {
            sar_spectrum_record& r = records_out_host[first + m];
            const double* row = rows.data() + static_cast<size_t>(m) * a.row;
            std::memcpy(power_out_host + static_cast<size_t>(first + m) * bins, row, bins * sizeof(double));  // (DIVERGED: +0.0)
            const bool bounded = r.status == SAR_SEARCH_BOUNDED;
            r.segments = bounded ? p->segments : 0u;
            r.energy = bounded ? row[bins] : 0.;
        }
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
