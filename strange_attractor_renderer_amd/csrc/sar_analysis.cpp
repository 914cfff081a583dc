// sar_analysis.cpp — the shared host code of the analysis families (sar_analysis.hpp).
//
// Built with -ffp-contract=off: sweep_args and fit_least_squares are what restatements in plain IEEE arithmetic give.
#include <cmath>
#include <limits>

#include "sar_analysis.hpp"

namespace sar {

int analysis_begin(sar_runtime* rt) {
    HIP_TRY(hipSetDevice(rt->device));
    rt->tm.restart_unless_accumulating();
    return SAR_OK;
}

int check_steps(const char* where, uint32_t transient, uint32_t steps) {
    if (transient <= kMaxSearchSteps && steps <= kMaxSearchSteps) return SAR_OK;
    set_error("%s: transient and steps must be at most 2^31 (%u, %u)", where, transient, steps);
    return SAR_ERR_INVALID;
}

int check_bound(const char* where, double bound) {
    if (bound > 0. && std::isfinite(bound)) return SAR_OK;
    set_error("%s: bound must be positive and finite", where);
    return SAR_ERR_INVALID;
}

int check_plane_size(const char* where, uint32_t width, uint32_t height) {
    static_assert(kMaxPlanePixels == 1u << 24 && kMaxBasinPixels == kMaxPlanePixels, "the text says 2^24");
    if (width && height && static_cast<uint64_t>(width) * height <= kMaxPlanePixels) return SAR_OK;
    set_error("%s: the plane must hold 1 to 2^24 pixels (%u x %u)", where, width, height);
    return SAR_ERR_INVALID;
}

int check_set_points(const char* where, uint32_t n) {
    static_assert(kCorrMaxPoints == 1u << 20 && kBoxMaxPoints == kCorrMaxPoints, "the text says 2^20");
    if (n && n <= kCorrMaxPoints) return SAR_OK;
    set_error("%s: a set must hold 1 to 2^20 points (%u)", where, n);
    return SAR_ERR_INVALID;
}

int check_sweep_axes(const char* where, const uint32_t axis[2]) {
    if (axis[0] <= 29 && axis[1] <= 29 && axis[0] != axis[1]) return SAR_OK;
    set_error("%s: the axes must be two distinct coefficients 0..29 (%u, %u)", where, axis[0], axis[1]);
    return SAR_ERR_INVALID;
}

int check_sweep_ranges(const char* where, const double lo[2], const double hi[2]) {
    if (std::isfinite(lo[0]) && std::isfinite(hi[0]) && std::isfinite(lo[1]) && std::isfinite(hi[1])) return SAR_OK;
    set_error("%s: lo and hi must be finite", where);
    return SAR_ERR_INVALID;
}

int check_points_not_nan(const char* where, uint32_t n_sets, uint32_t n, const double* points_host) {
    const size_t total = static_cast<size_t>(n_sets) * n * 3u;
    for (size_t k = 0; k < total; ++k)
        if (std::isnan(points_host[k])) {
            set_error("%s: coordinate %zu of point %zu of set %zu is NaN", where, k % 3u, k / 3u % n, k / 3u / n);
            return SAR_ERR_INVALID;
        }
    return SAR_OK;
}

PlaneArgs sweep_args(const double base[30], const uint32_t axis[2], const double lo[2], const double hi[2], uint32_t width, uint32_t height,
                     uint32_t transient, uint32_t steps, const double start[3], double bound) {
    PlaneArgs a;
    std::memset(&a, 0, sizeof(a));
    canonical_coeffs(base, kSearchCoeffs, a.base);
    for (int k = 0; k < 2; ++k) {
        a.lo[k] = lo[k];
        a.span[k] = hi[k] - lo[k];
        a.axis[k] = axis[k];
    }
    a.width = width;
    a.height = height;
    a.tiles_x = (width + kPlaneTile - 1) / kPlaneTile;
    a.transient = transient;
    a.steps = steps;
    for (int k = 0; k < 3; ++k) a.start[k] = start[k];
    a.bound = bound;
    return a;
}

int sweep_coeffs(const PlaneArgs& a, uint32_t x, uint32_t y, double out30[30]) {
    if (!out30 || x >= a.width || y >= a.height) return SAR_ERR_INVALID;
    for (uint32_t j = 0; j < kSearchCoeffs; ++j) out30[j] = plane_coeff(a, x, y, j);
    return SAR_OK;
}

int starts_or_drawn(const double*& starts_xyz_host, uint64_t seed, uint32_t jobs, std::vector<double>& drawn) {
    if (starts_xyz_host) return SAR_OK;
    drawn.resize(static_cast<size_t>(jobs) * 3u);
    SAR_TRY(sar_start_points(seed, 0, jobs, drawn.data()));
    starts_xyz_host = drawn.data();
    return SAR_OK;
}

int32_t decode_map_state(const CorrMapState& s, uint32_t& fail_job, uint64_t& fail_step, double extent[6]) {
    if (s.fail != kCorrNoFail) {
        const double inf = std::numeric_limits<double>::infinity();
        fail_job = static_cast<uint32_t>(s.fail >> 40);
        fail_step = s.fail & ((1ull << 40) - 1u);
        for (int k = 0; k < 3; ++k) { extent[2 * k] = inf; extent[2 * k + 1] = -inf; }
        return SAR_SEARCH_DIVERGED;
    }
    fail_job = 0, fail_step = 0;
    for (int k = 0; k < 3; ++k) {
        const unsigned long long lo = corr_unsortable(s.lo[k]), hi = corr_unsortable(s.hi[k]);
        std::memcpy(&extent[2 * k], &lo, 8);
        std::memcpy(&extent[2 * k + 1], &hi, 8);
    }
    return SAR_SEARCH_BOUNDED;
}

void map_points_out(int32_t status, const double* soa, uint32_t n, double* aos) {
    if (status != SAR_SEARCH_BOUNDED) {
        std::memset(aos, 0, static_cast<size_t>(n) * 3u * sizeof(double));
        return;
    }
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t k = 0; k < 3u; ++k) aos[static_cast<size_t>(i) * 3u + k] = soa[static_cast<size_t>(k) * n + i];
}

void fit_least_squares(const double* x, const double* y, size_t k, double* slope, double* intercept, double* rms) {
    double sx = 0., sy = 0.;
    for (size_t i = 0; i < k; ++i) { sx = sx + x[i]; sy = sy + y[i]; }
    const double mx = sx / static_cast<double>(k), my = sy / static_cast<double>(k);
    double sxx = 0., sxy = 0.;
    for (size_t i = 0; i < k; ++i) {
        sxx = sxx + (x[i] - mx) * (x[i] - mx);
        sxy = sxy + (x[i] - mx) * (y[i] - my);
    }
    const double m = *slope = sxy / sxx, c = *intercept = my - m * mx;
    double ss = 0.;
    for (size_t i = 0; i < k; ++i) {
        const double d = y[i] - (c + m * x[i]);
        ss = ss + d * d;
    }
    *rms = std::sqrt(ss / static_cast<double>(k));
}

}  // namespace sar
