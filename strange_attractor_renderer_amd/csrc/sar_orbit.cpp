// sar_orbit.cpp — the host half of the orbit diagrams (include/sar.h: sar_orbit_*, sar_runtime_orbit): the checks, every column's
// coefficient block, the chunked launches of k_orbit (sar_orbit.hip) and the read-back of the diagram, the statistics and the max.
//
// Built with -ffp-contract=off: sar_orbit_coeffs must produce the doubles the kernel steps with, and scale the host's quotient.
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_orbit.hpp"
#include "sar_search.hpp"

using namespace sar;

namespace {

int check_orbit(const sar_orbit_params* p, const char* where) {
    if (!p) { set_error("%s: the parameters are NULL", where); return SAR_ERR_INVALID; }
    if (!p->width || p->width > kMaxOrbitWidth || !p->height || p->height > kMaxOrbitHeight) {
        set_error("%s: the diagram must hold 1 to %u columns of 1 to %u bins (%u x %u)", where, kMaxOrbitWidth, kMaxOrbitHeight, p->width,
                  p->height);
        return SAR_ERR_INVALID;
    }
    if (!p->jobs || p->jobs > kMaxOrbitJobs) {
        set_error("%s: jobs must be 1 to %u (%u)", where, kMaxOrbitJobs, p->jobs);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(check_steps(where, p->transient, p->steps));
    if (static_cast<uint64_t>(p->jobs) * p->steps >= (1ull << 32)) {
        set_error("%s: jobs * steps must stay below 2^32, a bin is 32 bits (%u jobs, %u steps)", where, p->jobs, p->steps);
        return SAR_ERR_INVALID;
    }
    for (uint32_t k = 0; k < kSearchCoeffs; ++k)
        if (!std::isfinite(p->a[k]) || !std::isfinite(p->b[k])) {
            set_error("%s: a and b must be finite (entry %u)", where, k);
            return SAR_ERR_INVALID;
        }
    SAR_TRY(check_bound(where, p->bound));
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->proj[k])) {
            set_error("%s: proj must be finite", where);
            return SAR_ERR_INVALID;
        }
    if (!std::isfinite(p->v_lo) || !std::isfinite(p->v_hi) || !(p->v_lo < p->v_hi)) {
        set_error("%s: v_lo and v_hi must be finite with v_lo < v_hi", where);
        return SAR_ERR_INVALID;
    }
    if (!std::isfinite(static_cast<double>(p->height) / (p->v_hi - p->v_lo))) {
        set_error("%s: height / (v_hi - v_lo) is not finite", where);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

// column c's block: orbit_coeff over the 30 entries, span = b - a once per entry
void orbit_column(const sar_orbit_params* p, uint32_t c, double out30[30]) {
    for (uint32_t k = 0; k < kSearchCoeffs; ++k) out30[k] = orbit_coeff(p->a[k], p->b[k] - p->a[k], c, p->width);
}

}  // namespace

extern "C" {

int sar_orbit_params_default(sar_orbit_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->width = 1024;
    out->height = 512;
    out->jobs = 256;
    out->transient = 1000;
    out->steps = 4096;
    out->seed = 0;
    out->bound = 1e6;
    out->proj[0] = 1.;
    out->v_lo = -1.;
    out->v_hi = 1.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_orbit_coeffs(const sar_orbit_params* p, uint32_t column, double out30[30]) try {
    SAR_TRY(check_orbit(p, "sar_orbit_coeffs"));
    if (!out30 || column >= p->width) return SAR_ERR_INVALID;
    orbit_column(p, column, out30);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_orbit(sar_runtime* rt, const sar_orbit_params* p, const double* starts_xyz_host, uint32_t* count_out_host,
                      sar_orbit_column* stats_out_host, uint32_t* max_out) try {
    SAR_TRY(check_orbit(p, "sar_runtime_orbit"));  // (no device needed to refuse the parameters)
    if (!rt || !count_out_host) { set_error("sar_runtime_orbit: the runtime or the count buffer is NULL"); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_orbit (sar_timing)
    const uint32_t width = p->width, jobs = p->jobs;
    const size_t bins = static_cast<size_t>(p->height) * width;

    static_assert(sizeof(SearchCoeffs) == kSearchCoeffs * sizeof(double), "a column's block is its 30 coefficients, x, y, z rows");
    std::vector<SearchCoeffs> cols(width);
    for (uint32_t c = 0; c < width; ++c) {
        double k30[kSearchCoeffs];
        orbit_column(p, c, k30);
        std::memcpy(&cols[c], k30, sizeof(k30));  // the x, y, z rows of 10
    }
    std::vector<double> drawn;
    SAR_TRY(starts_or_drawn(starts_xyz_host, p->seed, jobs, drawn));

    HIP_TRY(rt->orbit.d_cols.grow(nullptr, width));
    HIP_TRY(rt->orbit.d_stats.grow(nullptr, width));
    HIP_TRY(rt->orbit.d_starts.grow(nullptr, static_cast<size_t>(jobs) * 3));
    HIP_TRY(rt->orbit.d_count.grow(nullptr, bins));
    HIP_TRY(rt->orbit.d_max.grow(nullptr, 1));
    HIP_TRY(hipMemcpyAsync(rt->orbit.d_cols, cols.data(), static_cast<size_t>(width) * sizeof(SearchCoeffs), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(rt->orbit.d_starts, starts_xyz_host, static_cast<size_t>(jobs) * 3 * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemsetAsync(rt->orbit.d_max, 0, sizeof(uint32_t), rt->stream));

    OrbitArgs a;
    std::memset(&a, 0, sizeof(a));
    a.cols = rt->orbit.d_cols;
    a.starts = rt->orbit.d_starts;
    a.count = rt->orbit.d_count;
    a.stats = rt->orbit.d_stats;
    a.max = rt->orbit.d_max;
    a.width = width;
    a.height = p->height;
    a.jobs = jobs;
    a.transient = p->transient;
    a.steps = p->steps;
    a.bound = p->bound;
    for (int k = 0; k < 3; ++k) a.proj[k] = p->proj[k];
    a.v_lo = p->v_lo;
    a.scale = static_cast<double>(p->height) / (p->v_hi - p->v_lo);
    const uint32_t chunk = rt->opt.orbit_chunk ? rt->opt.orbit_chunk : kDefaultOrbitChunk;
    for (uint32_t first = 0; first < width; first += chunk) {
        a.first_col = first;
        SAR_TRY(timed_lds_launch(rt, rt->tm.iter,
                             [&] { return launch_orbit(a, width - first < chunk ? width - first : chunk, rt->stream); }));
    }
    HIP_TRY(hipMemcpyAsync(count_out_host, rt->orbit.d_count, bins * sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
    if (stats_out_host)
        HIP_TRY(hipMemcpyAsync(stats_out_host, rt->orbit.d_stats, static_cast<size_t>(width) * sizeof(sar_orbit_column), hipMemcpyDeviceToHost, rt->stream));
    if (max_out) HIP_TRY(hipMemcpyAsync(max_out, rt->orbit.d_max, sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
