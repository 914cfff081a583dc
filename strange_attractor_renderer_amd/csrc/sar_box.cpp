// sar_box.cpp — the host half of box counting (include/sar.h: sar_box_*, sar_runtime_boxes, sar_boxdim_*, sar_runtime_boxdim): the
// checks, the groups of sets that share the device's buffers, the launches of k_box_insert and k_box_level (sar_box.hip), the
// read-back, and the host finish — level 0's row, a map's cube, and the three least-squares lines over the window of levels. The
// maps' points come from k_corr_orbit through sar_corr.cpp's orbit half, as sar_runtime_corrdim's do.
//
// Built with -ffp-contract=off: the lines are what a restatement in plain IEEE arithmetic gives.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_box.hpp"
#include "sar_corr.hpp"
#include "sar_search.hpp"

using namespace sar;

namespace {

void box_defaults(sar_box_params* p) {
    std::memset(p, 0, sizeof(*p));
    p->levels = kBoxMaxLevels;
    p->size = 1.;
}

int check_levels(const char* where, uint32_t levels) {
    if (!levels || levels > kBoxMaxLevels) { set_error("%s: levels must be 1 to %u (%u)", where, kBoxMaxLevels, levels); return SAR_ERR_INVALID; }
    return SAR_OK;
}

int check_occupancy(const char* where, double min_occupancy) {
    if (!(min_occupancy > 0.)) { set_error("%s: min_occupancy must be positive", where); return SAR_ERR_INVALID; }
    return SAR_OK;
}

// scale = 2^L / size, once, here
int make_cube(const char* where, const double origin[3], double size, uint32_t levels, BoxCube* out) {
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(origin[k])) { set_error("%s: the origin must be finite", where); return SAR_ERR_INVALID; }
    if (!std::isfinite(size) || !(size > 0.)) { set_error("%s: size must be finite and positive", where); return SAR_ERR_INVALID; }
    const double scale = static_cast<double>(1u << levels) / size;
    if (!std::isfinite(scale)) { set_error("%s: the scale 2^levels / size must be finite", where); return SAR_ERR_INVALID; }
    std::memset(out, 0, sizeof(*out));
    for (int k = 0; k < 3; ++k) out->origin[k] = origin[k];
    out->scale = scale;
    return SAR_OK;
}

// the slots of a set's tables: "box_slots", or the smallest power of two >= 2 n
int table_slots(const sar_runtime* rt, const char* where, uint32_t n, uint32_t* slots, uint32_t* bits) {
    uint32_t s = rt->opt.box_slots;
    if (!s) for (s = 2u; s < 2u * n; s <<= 1) {}
    if (s <= n) { set_error("%s: box_slots (%u) must be above the points of a set (%u)", where, s, n); return SAR_ERR_INVALID; }
    *slots = s;
    for (*bits = 0; (1u << *bits) < s; ++*bits) {}
    return SAR_OK;
}

// sets per group: what fits the device's point buffer and its tables
uint32_t group_size(uint32_t n_sets, uint32_t n, uint32_t slots) {
    const uint64_t fit = std::max<uint64_t>(1u, std::min(kBoxPointBudget / n, kBoxSlotBudget / slots));
    return static_cast<uint32_t>(std::min<uint64_t>(n_sets, fit));
}

int grow_tables(sar_runtime* rt, uint32_t group, uint32_t slots, uint32_t levels) {
    HIP_TRY(rt->box.d_cubes.grow(nullptr, group));
    HIP_TRY(rt->box.d_keys.grow(nullptr, 2u * static_cast<size_t>(group) * slots));
    HIP_TRY(rt->box.d_counts.grow(nullptr, 2u * static_cast<size_t>(group) * slots));
    HIP_TRY(rt->box.d_sums.grow(nullptr, static_cast<size_t>(group) * (levels + 1u) * 4u));
    HIP_TRY(rt->box.d_overflow.grow(nullptr, 1));
    return SAR_OK;
}

// The box launches of one group of `sets` sets whose points lie in rt->corr.d_points and whose cubes are `cubes`: table 0 emptied
// and the sums zeroed, then k_box_insert and k_box_level for L .. 1, "box_chunk" sets per launch; the rows come back into
// rows_out[sets][L + 1] with level 0's written here. Waits for the stream.
int run_boxes(sar_runtime* rt, const char* where, const BoxCube* cubes, uint32_t sets, uint32_t n, uint32_t levels, uint32_t slots,
              uint32_t slot_bits, sar_box_level* rows_out) {
    const size_t table = static_cast<size_t>(sets) * slots, rows = static_cast<size_t>(sets) * (levels + 1u);
    HIP_TRY(hipMemcpyAsync(rt->box.d_cubes, cubes, sets * sizeof(BoxCube), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemsetAsync(rt->box.d_keys, 0xff, table * sizeof(unsigned long long), rt->stream));  // kBoxEmpty
    HIP_TRY(hipMemsetAsync(rt->box.d_counts, 0, table * sizeof(uint32_t), rt->stream));
    HIP_TRY(hipMemsetAsync(rt->box.d_sums, 0, rows * sizeof(sar_box_level), rt->stream));
    HIP_TRY(hipMemsetAsync(rt->box.d_overflow, 0, sizeof(uint32_t), rt->stream));
    BoxArgs a;
    std::memset(&a, 0, sizeof(a));
    a.points = rt->corr.d_points;
    a.cubes = rt->box.d_cubes;
    a.keys = rt->box.d_keys;
    a.counts = rt->box.d_counts;
    a.table_stride = table;
    a.sums = rt->box.d_sums;
    a.overflow = rt->box.d_overflow;
    a.n = n;
    a.slots = slots;
    a.slot_bits = slot_bits;
    a.levels = levels;
    const uint32_t per = rt->opt.box_chunk ? rt->opt.box_chunk : kBoxMaxGridY;
    for (uint32_t set = 0; set < sets; set += per) {
        const uint32_t now = std::min(per, sets - set);
        a.first_set = set;
        SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_box_insert(a, now, rt->stream); }));
        for (uint32_t level = levels; level >= 1u; --level)
            SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_box_level(a, level, now, rt->stream); }));
    }
    uint32_t overflow = 0;
    static_assert(sizeof(sar_box_level) == 4 * sizeof(unsigned long long), "a row of the device's sums is a sar_box_level");
    HIP_TRY(hipMemcpyAsync(rows_out, rt->box.d_sums, rows * sizeof(sar_box_level), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipMemcpyAsync(&overflow, rt->box.d_overflow, sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    if (overflow) { set_error("%s: a hash table of %u slots overflowed with %u points (internal)", where, slots, n); return SAR_ERR_INTERNAL; }
    for (uint32_t s = 0; s < sets; ++s) {
        if (cubes[s].skip) continue;
        sar_box_level& r = rows_out[static_cast<size_t>(s) * (levels + 1u)];
        r.cells = 1;
        r.singles = n == 1u ? 1u : 0u;
        r.sum_sq = static_cast<uint64_t>(n) * n;
        r.n_log_n = static_cast<uint64_t>(n) * box_lg32(n);
    }
    return SAR_OK;
}

void no_window(sar_boxdim_lines* out) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::memset(out, 0, sizeof(*out));
    for (sar_boxdim_line* l : {&out->d0, &out->d1, &out->d2}) l->slope = l->intercept = l->rms = nan;
    out->status = SAR_BOXDIM_NO_WINDOW;
}

void fit_lines(const sar_box_level* levels, uint32_t L, uint32_t n, uint32_t l_min, double min_occupancy, sar_boxdim_lines* out) {
    no_window(out);
    const double ln2 = std::log(2.), dn = static_cast<double>(n), ln_n = std::log(dn);
    std::vector<double> x, y0, y1, y2;
    uint32_t first = 0, last = 0;
    for (uint32_t l = l_min; l <= L; ++l) {
        const sar_box_level& r = levels[l];
        if (!r.cells || !(dn >= min_occupancy * static_cast<double>(r.cells))) continue;
        if (x.empty()) first = l;
        last = l;
        x.push_back(static_cast<double>(l) * ln2);
        y0.push_back(std::log(static_cast<double>(r.cells)));
        y1.push_back(ln_n - (static_cast<double>(r.n_log_n) / 4294967296.) * ln2 / dn);
        y2.push_back(2. * ln_n - std::log(static_cast<double>(r.sum_sq)));
    }
    if (x.size() < 3) return;
    const auto fit = [&x](const std::vector<double>& y, sar_boxdim_line* l) {
        fit_least_squares(x.data(), y.data(), x.size(), &l->slope, &l->intercept, &l->rms);
    };
    fit(y0, &out->d0);
    fit(y1, &out->d1);
    fit(y2, &out->d2);
    out->first_level = first;
    out->last_level = last;
    out->used = static_cast<uint32_t>(x.size());
    out->status = SAR_BOXDIM_FIT_OK;
}

}  // namespace

extern "C" {

int sar_box_params_default(sar_box_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    box_defaults(out);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_box_log2_q32(uint32_t n, uint64_t* out) try {
    if (!n || !out) { set_error("sar_box_log2_q32: n must be at least 1 and the result not NULL"); return SAR_ERR_INVALID; }
    *out = box_lg32(n);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_boxdim_fit(const sar_box_level* levels, uint32_t L, uint32_t n, uint32_t l_min, double min_occupancy, sar_boxdim_lines* out) try {
    const char* where = "sar_boxdim_fit";
    SAR_TRY(check_levels(where, L));
    SAR_TRY(check_set_points(where, n));
    SAR_TRY(check_occupancy(where, min_occupancy));
    if (!levels || !out) { set_error("%s: the levels or the result is NULL", where); return SAR_ERR_INVALID; }
    fit_lines(levels, L, n, l_min, min_occupancy, out);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_boxes(sar_runtime* rt, const sar_box_params* p, uint32_t n_sets, uint32_t n, const double* points_host,
                      sar_box_level* levels_out_host) try {
    const char* where = "sar_runtime_boxes";
    sar_box_params d;
    if (!p) { box_defaults(&d); p = &d; }
    SAR_TRY(check_levels(where, p->levels));  // (no device needed to refuse the parameters)
    BoxCube cube;
    SAR_TRY(make_cube(where, p->origin, p->size, p->levels, &cube));
    SAR_TRY(check_set_points(where, n));
    if (!n_sets) return SAR_OK;
    if (!points_host || !levels_out_host) { set_error("%s: the points or the levels buffer is NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_points_not_nan(where, n_sets, n, points_host));
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    uint32_t slots, slot_bits;
    SAR_TRY(table_slots(rt, where, n, &slots, &slot_bits));
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = the box kernels (sar_timing)
    const uint32_t L = p->levels, group = group_size(n_sets, n, slots);
    HIP_TRY(rt->corr.d_points.grow(nullptr, static_cast<size_t>(group) * n * 3u));
    SAR_TRY(grow_tables(rt, group, slots, L));
    const std::vector<BoxCube> cubes(group, cube);
    return for_staged_sets(rt, n_sets, n, group, points_host, [&](uint32_t first, uint32_t sets) {
        return run_boxes(rt, where, cubes.data(), sets, n, L, slots, slot_bits, levels_out_host + static_cast<size_t>(first) * (L + 1u));
    });
} catch (...) { return sar::abi_caught(); }

int sar_boxdim_params_default(sar_boxdim_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->jobs = 256;
    out->samples = 128;
    out->stride = 4;
    out->transient = 1000;
    out->levels = kBoxMaxLevels;
    out->l_min = 3;
    out->seed = 0;
    out->bound = 1e6;
    out->min_occupancy = 16.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_boxdim(sar_runtime* rt, const sar_boxdim_params* p, uint32_t n_maps, const double* coeffs_host, const double* starts_xyz_host,
                       sar_box_level* levels_out_host, sar_boxdim_record* records_out_host, double* points_out_host) try {
    const char* where = "sar_runtime_boxdim";
    if (!p) { set_error("%s: the parameters are NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_levels(where, p->levels));  // (no device needed to refuse the parameters)
    const CorrOrbitShape shape = {p->jobs, p->samples, p->stride, p->transient, p->seed, p->bound};
    SAR_TRY(corr_check_shape(where, shape));
    SAR_TRY(check_occupancy(where, p->min_occupancy));
    if (!n_maps) return SAR_OK;
    if (!coeffs_host || !levels_out_host || !records_out_host) {
        set_error("%s: the coefficients, the levels buffer or the records are NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(corr_check_maps(where, shape, n_maps, coeffs_host, starts_xyz_host));
    if (!rt) { set_error("%s: the runtime is NULL", where); return SAR_ERR_INVALID; }
    const uint32_t n = p->jobs * p->samples, L = p->levels;
    uint32_t slots, slot_bits;
    SAR_TRY(table_slots(rt, where, n, &slots, &slot_bits));
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_corr_orbit, iterate_ms = the box kernels (sar_timing)

    const uint32_t group = group_size(n_maps, n, slots);
    SAR_TRY(corr_orbits_begin(rt, shape, starts_xyz_host, group));
    SAR_TRY(grow_tables(rt, group, slots, L));
    MapGroupScratch scratch;
    std::vector<BoxCube> cubes;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (uint32_t first = 0; first < n_maps; first += group) {
        const uint32_t maps = std::min(group, n_maps - first);
        SAR_TRY(corr_orbits_run(rt, shape, coeffs_host + static_cast<size_t>(first) * kSearchCoeffs, maps));
        SAR_TRY(read_map_group(rt, scratch, maps, n, records_out_host + first,  // (before the boxes: the cubes come from the extents)
                               points_out_host ? points_out_host + static_cast<size_t>(first) * n * 3u : nullptr));
        cubes.assign(maps, BoxCube{});
        for (uint32_t m = 0; m < maps; ++m) {
            sar_boxdim_record& r = records_out_host[first + m];
            if (r.status != SAR_SEARCH_BOUNDED) {
                r.origin[0] = r.origin[1] = r.origin[2] = r.size = nan;
                cubes[m].skip = 1u;
                continue;
            }
            double size = 0.;
            for (int k = 0; k < 3; ++k) {
                r.origin[k] = r.extent[2 * k];
                const double span = r.extent[2 * k + 1] - r.extent[2 * k];
                size = span > size ? span : size;
            }
            r.size = size > 0. ? size : 1.;
            SAR_TRY(make_cube(where, r.origin, r.size, L, &cubes[m]));
        }
        sar_box_level* rows = levels_out_host + static_cast<size_t>(first) * (L + 1u);
        SAR_TRY(run_boxes(rt, where, cubes.data(), maps, n, L, slots, slot_bits, rows));
        for (uint32_t m = 0; m < maps; ++m) {
            sar_boxdim_record& r = records_out_host[first + m];
            if (r.status == SAR_SEARCH_BOUNDED) fit_lines(rows + static_cast<size_t>(m) * (L + 1u), L, n, p->l_min, p->min_occupancy, &r.lines);
            else no_window(&r.lines);
        }
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
