// sar_analysis.hpp — what the entry points of the analysis families share on the host (sar_search.cpp, sar_plane.cpp, sar_gallery.cpp,
// sar_orbit.cpp, sar_corr.cpp, sar_box.cpp, sar_basin.cpp, sar_period.cpp, sar_density.cpp, sar_cycles.cpp, sar_manifold.cpp, sar_ftle.cpp, sar_spectrum.cpp, sar_rqa.cpp): the checks and refusal texts that more
// than one family makes, the launch loops, the staging of point sets, the read-back of recorded orbits and the least-squares line.
// Host only: no .hip file includes it. Not part of the ABI.
#pragma once

#include <algorithm>
#include <cstring>

#include "sar_runtime_impl.hpp"

namespace sar {

// Behind an entry's refusals: the runtime's device, and where the call does not accumulate timing its spans started afresh — which
// kernel a family books as warmup_ms and which as iterate_ms is include/sar.h's (sar_timing).
int analysis_begin(sar_runtime* rt);
// transient and steps at most 2^31 each: the kernels' step counters advance by kSearchCheck and must not wrap
int check_steps(const char* where, uint32_t transient, uint32_t steps);
// bound positive and finite. (Not the search's check: sar_runtime_search accepts an infinite bound and keeps its own text.)
int check_bound(const char* where, double bound);
// 1 to 2^24 pixels (the planes, the period planes, the basins); 1 to 2^20 points of a set (the pairs, the boxes)
int check_plane_size(const char* where, uint32_t width, uint32_t height);
int check_set_points(const char* where, uint32_t n);
// A sweep's axes, two distinct coefficients, and its ranges, finite. Two calls: the planes check their size between them.
int check_sweep_axes(const char* where, const uint32_t axis[2]);
int check_sweep_ranges(const char* where, const double lo[2], const double hi[2]);
// no coordinate of [n_sets][n][3] is NaN
int check_points_not_nan(const char* where, uint32_t n_sets, uint32_t n, const double* points_host);

// a caller's parameters or colours, or where it passed NULL what `defaults` (a sar_*_default of include/sar.h) fills in
template <typename T>
T given_or_default(const T* given, int (*defaults)(T*)) {
    T t;
    defaults(&t);
    return given ? *given : t;
}
// dst[k] = src[k] with -0.0 -> +0.0, as sar_render treats its coefficients
inline void canonical_coeffs(const double* src, size_t n, double* dst) {
    for (size_t k = 0; k < n; ++k) dst[k] = 0. + 1. * src[k];
}
// The kernels' view of a checked sweep (the planes, the sweep form of the period planes, which pass max_period as steps): base
// canonicalised, span = hi - lo once. plane_coeff gives the device's doubles from it.
PlaneArgs sweep_args(const double base[30], const uint32_t axis[2], const double lo[2], const double hi[2], uint32_t width, uint32_t height,
                     uint32_t transient, uint32_t steps, const double start[3], double bound);
// the tail of sar_plane_coeffs / sar_period_coeffs behind their checks: pixel (x, y)'s 30 coefficients
int sweep_coeffs(const PlaneArgs& a, uint32_t x, uint32_t y, double out30[30]);
// where the caller passed no start points: the first `jobs` points of the stream of `seed`, drawn into `drawn`, in their place
int starts_or_drawn(const double*& starts_xyz_host, uint64_t seed, uint32_t jobs, std::vector<double>& drawn);

// The 8 x 8 tiles of a width x height picture (the planes, the basins, the period planes), row-major, in bands of at most `per`:
// the whole tiles a launch of `chunk` pixels takes, at least one and no more than there are
struct TileBands { uint32_t tiles_x, tiles, per; };
inline TileBands tile_bands(uint32_t width, uint32_t height, uint32_t chunk) {
    const uint32_t tiles_x = (width + kPlaneTile - 1) / kPlaneTile, tiles = tiles_x * ((height + kPlaneTile - 1) / kPlaneTile);
    return {tiles_x, tiles, std::min(std::max(chunk / (kPlaneTile * kPlaneTile), 1u), tiles)};
}
// band(first_tile, n_tiles) for every band in turn; it returns a status
template <typename Band>
int for_tile_bands(const TileBands& b, Band&& band) {
    for (uint32_t first = 0; first < b.tiles; first += b.per) SAR_TRY(band(first, std::min(b.per, b.tiles - first)));
    return SAR_OK;
}

// One launch inside a span: span_begin, launch(), hipGetLastError, span_end
template <typename Launch>
int timed_launch(sar_runtime* rt, SpanList& spans, Launch&& launch) {
    rt->tm.span_begin(spans, rt->stream);
    launch();
    HIP_TRY(hipGetLastError());
    rt->tm.span_end(spans, rt->stream);
    return SAR_OK;
}
// The same for a launch wrapper that sets its kernel's dynamic-LDS attribute first (launch_orbit, launch_corr_pairs,
// launch_gallery): launch() returns 0, or the hipError_t of hipFuncSetAttribute
template <typename Launch>
int timed_lds_launch(sar_runtime* rt, SpanList& spans, Launch&& launch) {
    int attr = 0;
    const int status = timed_launch(rt, spans, [&] { attr = launch(); });
    if (attr != 0) { set_error("hipFuncSetAttribute(max dynamic LDS) failed: %d", attr); return SAR_ERR_HIP; }
    return status;
}

// The tail of sar_runtime_plane_colorize / sar_runtime_basin_colorize / sar_runtime_period_colorize, behind the checks of their own
// colours: the palette's length, the refusal where the runtime holds no `what` of width x height (`producer` makes one), the RGBA16
// image's buffer, launch(npix, rgba) and the read-back.
template <typename Launch>
int colorize_tail(const char* where, const char* what, const char* producer, const sar_config* cfg, sar_runtime* rt, uint32_t width,
                  uint32_t height, DevBuf<uint16_t>& rgba, uint16_t* rgba16_out_host, Launch&& launch) {
    if (cfg->palette_len < 1 || cfg->palette_len > SAR_PALETTE_MAX) {
        set_error("%s: the palette must hold 1 to %d entries (%u)", where, SAR_PALETTE_MAX, cfg->palette_len);
        return SAR_ERR_INVALID;
    }
    if (!width) { set_error("%s: the runtime has no %s (%s first)", where, what, producer); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    const uint32_t npix = width * height;
    HIP_TRY(rgba.grow(nullptr, static_cast<size_t>(npix) * 4));
    launch(npix, rgba.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(rgba16_out_host, rgba, static_cast<size_t>(npix) * 8, hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
}

// The caller's sets [n_sets][n][3] through rt->corr.d_points (grown for `group` sets) in groups: each group staged as [set][3][n]
// and uploaded, then run(first_set, sets), which returns a status and has waited for the stream when it does (the staging is reused).
template <typename Run>
int for_staged_sets(sar_runtime* rt, uint32_t n_sets, uint32_t n, uint32_t group, const double* points_host, Run&& run) {
    const size_t set = static_cast<size_t>(n) * 3u;
    std::vector<double> soa;
    for (uint32_t first = 0; first < n_sets; first += group) {
        const uint32_t sets = std::min(group, n_sets - first);
        soa.resize(sets * set);
        for (uint32_t s = 0; s < sets; ++s)
            for (uint32_t i = 0; i < n; ++i)
                for (uint32_t k = 0; k < 3u; ++k) soa[s * set + static_cast<size_t>(k) * n + i] = points_host[(first + s) * set + i * 3u + k];
        HIP_TRY(hipMemcpyAsync(rt->corr.d_points, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream));
        SAR_TRY(run(first, sets));
    }
    return SAR_OK;
}

// What read_map_group reads into, kept across the groups of a call
struct MapGroupScratch {
    std::vector<CorrMapState> state;
    std::vector<double> soa;
};
// a state read back: BOUNDED and the extent decoded, or DIVERGED, the failure and the extent (+inf, -inf) x 3; a map's points for
// the caller, [n][3] from the device's [3][n], zero for a DIVERGED map
int32_t decode_map_state(const CorrMapState& s, uint32_t& fail_job, uint64_t& fail_step, double extent[6]);
void map_points_out(int32_t status, const double* soa, uint32_t n, double* aos);
// One group of `maps` maps behind corr_orbits_run (sar_corr.hpp): the states and (points_out[maps][n][3], nullable) the points read
// back and waited for, then the header of every record — zeroed, then status, failure and extent — and its points. What a family
// adds to a record comes after.
template <typename Record>
int read_map_group(sar_runtime* rt, MapGroupScratch& h, uint32_t maps, uint32_t n, Record* records, double* points_out) {
    h.state.resize(maps);
    HIP_TRY(hipMemcpyAsync(h.state.data(), rt->corr.d_state, maps * sizeof(CorrMapState), hipMemcpyDeviceToHost, rt->stream));
    if (points_out) {
        h.soa.resize(static_cast<size_t>(maps) * n * 3u);
        HIP_TRY(hipMemcpyAsync(h.soa.data(), rt->corr.d_points, h.soa.size() * sizeof(double), hipMemcpyDeviceToHost, rt->stream));
    }
    HIP_TRY(hipStreamSynchronize(rt->stream));
    for (uint32_t m = 0; m < maps; ++m) {
        Record& r = records[m];
        std::memset(&r, 0, sizeof(r));
        r.status = decode_map_state(h.state[m], r.fail_job, r.fail_step, r.extent);
        const size_t at = static_cast<size_t>(m) * n * 3u;
        if (points_out) map_points_out(r.status, h.soa.data() + at, n, points_out + at);
    }
    return SAR_OK;
}

// The least-squares line y = intercept + slope x through k >= 1 points, and the rms of its residuals. The order of the operations
// is held bit for bit by restatements (sar_corrdim_fit, sar_boxdim_fit): sums, means, sxx / sxy, slope, intercept, rms.
void fit_least_squares(const double* x, const double* y, size_t k, double* slope, double* intercept, double* rms);

}  // namespace sar
