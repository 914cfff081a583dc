// sar_cycles.cpp — the host half of the cycles family (include/sar.h: sar_cycles_*, sar_cycle_charpoly, sar_runtime_cycles): the
// checks, the lattice of starts, the characteristic polynomial, and the chunked launches of k_cycles_newton and k_cycles_merge
// (sar_cycles.hip) with the read-back of the records and the orbit slots.
//
// Built with -ffp-contract=off: sar_cycles_starts must produce the doubles the device starts from, and sar_cycle_charpoly what a
// restatement in plain IEEE arithmetic gives.
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_cycles.hpp"

using namespace sar;

namespace {

bool positive_finite(double v) { return v > 0. && std::isfinite(v); }

// what both forms of the starts need
int check_cycles(const sar_cycles_params& p, const char* where) {
    if (!p.period || p.period > kMaxCyclePeriod) {
        set_error("%s: period must be 1 to %u (%u)", where, kMaxCyclePeriod, p.period);
        return SAR_ERR_INVALID;
    }
    if (p.max_newton > kMaxCycleNewton) {
        set_error("%s: max_newton must be at most %u (%u)", where, kMaxCycleNewton, p.max_newton);
        return SAR_ERR_INVALID;
    }
    if (!p.cap || p.cap > kMaxCycleCap) {
        set_error("%s: cap must be 1 to %u orbits per map (%u)", where, kMaxCycleCap, p.cap);
        return SAR_ERR_INVALID;
    }
    if (!positive_finite(p.tol) || !positive_finite(p.same)) {
        set_error("%s: tol and same must be positive and finite", where);
        return SAR_ERR_INVALID;
    }
    if (!(p.merge >= 0.) || !std::isfinite(p.merge)) {
        set_error("%s: merge must be finite and not negative", where);
        return SAR_ERR_INVALID;
    }
    return check_bound(where, p.bound);
}

// the lattice form: grid and box
int check_cycles_lattice(const sar_cycles_params& p, const char* where) {
    // (grid <= 4096 first: the cube then stays below 2^64)
    if (!p.grid || p.grid > kMaxCycleJobs || static_cast<uint64_t>(p.grid) * p.grid * p.grid > kMaxCycleJobs) {
        set_error("%s: grid^3 must be 1 to %u starts (grid %u)", where, kMaxCycleJobs, p.grid);
        return SAR_ERR_INVALID;
    }
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(p.box_lo[k]) || !std::isfinite(p.box_hi[k])) {
            set_error("%s: box_lo and box_hi must be finite", where);
            return SAR_ERR_INVALID;
        }
        if (!(p.box_lo[k] < p.box_hi[k])) {
            set_error("%s: box_lo must be below box_hi on every axis (axis %d)", where, k);
            return SAR_ERR_INVALID;
        }
    }
    return SAR_OK;
}

// start j = (ix grid + iy) grid + iz at lo + ((double)i + 0.5) * step per axis, step = (hi - lo) / (double)grid once
void cycles_lattice(const sar_cycles_params& p, double* out) {
    const uint32_t g = p.grid;
    double step[3];
    for (int k = 0; k < 3; ++k) step[k] = (p.box_hi[k] - p.box_lo[k]) / static_cast<double>(g);
    for (uint32_t ix = 0; ix < g; ++ix)
        for (uint32_t iy = 0; iy < g; ++iy)
            for (uint32_t iz = 0; iz < g; ++iz) {
                double* o = out + (static_cast<size_t>(ix * g + iy) * g + iz) * 3u;
                o[0] = p.box_lo[0] + (static_cast<double>(ix) + 0.5) * step[0];
                o[1] = p.box_lo[1] + (static_cast<double>(iy) + 0.5) * step[1];
                o[2] = p.box_lo[2] + (static_cast<double>(iz) + 0.5) * step[2];
            }
}

}  // namespace

extern "C" {

int sar_cycles_params_default(sar_cycles_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->period = 1;
    out->jobs = 512;
    out->grid = 8;
    out->max_newton = 64;
    out->cap = 64;
    for (int k = 0; k < 3; ++k) {
        out->box_lo[k] = -2.;
        out->box_hi[k] = 2.;
    }
    out->tol = 1e-12;
    out->bound = 1e6;
    out->merge = 1e-6;
    out->same = 1e-9;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_cycles_starts(const sar_cycles_params* params, double* out_xyz_host) try {
    const sar_cycles_params p = given_or_default(params, sar_cycles_params_default);
    SAR_TRY(check_cycles_lattice(p, "sar_cycles_starts"));
    if (!out_xyz_host) return SAR_ERR_INVALID;
    cycles_lattice(p, out_xyz_host);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_cycle_charpoly(const double M[9], double out3[3]) try {
    if (!M || !out3) return SAR_ERR_INVALID;
    const double c00 = M[4] * M[8] - M[5] * M[7], c01 = M[5] * M[6] - M[3] * M[8], c02 = M[3] * M[7] - M[4] * M[6];
    out3[0] = (M[0] + M[4]) + M[8];
    out3[1] = ((M[0] * M[4] - M[1] * M[3]) + (M[0] * M[8] - M[2] * M[6])) + c00;
    out3[2] = (M[0] * c00 + M[1] * c01) + M[2] * c02;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_cycles(sar_runtime* rt, const sar_cycles_params* params, uint32_t n_maps, const double* coeffs_host,
                       const double* starts_xyz_host, sar_cycles_record* records_out_host, sar_cycle_orbit* orbits_out_host) try {
    const char* const where = "sar_runtime_cycles";
    const sar_cycles_params p = given_or_default(params, sar_cycles_params_default);
    SAR_TRY(check_cycles(p, where));  // (no device needed to refuse the parameters)
    if (starts_xyz_host) {
        if (!p.jobs || p.jobs > kMaxCycleJobs) {
            set_error("%s: jobs must be 1 to %u (%u)", where, kMaxCycleJobs, p.jobs);
            return SAR_ERR_INVALID;
        }
        SAR_TRY(check_points_not_nan(where, 1, p.jobs, starts_xyz_host));
    } else {
        SAR_TRY(check_cycles_lattice(p, where));
    }
    if (n_maps > kMaxCycleMaps) {
        set_error("%s: a call takes at most 2^20 maps (%u)", where, n_maps);
        return SAR_ERR_INVALID;
    }
    if (!n_maps) return SAR_OK;
    if (!rt || !coeffs_host || !records_out_host || !orbits_out_host) {
        set_error("%s: the runtime, the coefficients or an output buffer is NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_cycles_newton, resolve_ms = k_cycles_merge (sar_timing)

    const uint32_t jobs = starts_xyz_host ? p.jobs : p.grid * p.grid * p.grid, cap = p.cap;
    std::vector<double> lattice;
    if (!starts_xyz_host) {
        lattice.resize(static_cast<size_t>(jobs) * 3u);
        cycles_lattice(p, lattice.data());
        starts_xyz_host = lattice.data();
    }
    static_assert(sizeof(SearchCoeffs) == kSearchCoeffs * sizeof(double), "a map's block is its 30 coefficients, x, y, z rows");
    std::vector<SearchCoeffs> maps(n_maps);
    canonical_coeffs(coeffs_host, static_cast<size_t>(n_maps) * kSearchCoeffs, reinterpret_cast<double*>(maps.data()));

    // whole maps per launch: `chunk` lanes, and as many orbit slots at most
    const uint32_t chunk = rt->opt.cycles_chunk ? rt->opt.cycles_chunk : kDefaultCyclesChunk;
    const uint32_t per = std::min(std::max(chunk / std::max(jobs, cap), 1u), n_maps);
    HIP_TRY(rt->cycles.d_coeffs.grow(nullptr, n_maps));
    HIP_TRY(rt->cycles.d_starts.grow(nullptr, static_cast<size_t>(jobs) * 3u));
    HIP_TRY(rt->cycles.d_finds.grow(nullptr, static_cast<size_t>(per) * jobs));
    HIP_TRY(rt->cycles.d_rec.grow(nullptr, per));
    HIP_TRY(rt->cycles.d_orbits.grow(nullptr, static_cast<size_t>(per) * cap));
    HIP_TRY(hipMemcpyAsync(rt->cycles.d_coeffs, maps.data(), static_cast<size_t>(n_maps) * sizeof(SearchCoeffs), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(rt->cycles.d_starts, starts_xyz_host, static_cast<size_t>(jobs) * 3u * sizeof(double), hipMemcpyHostToDevice, rt->stream));

    CyclesArgs a;
    std::memset(&a, 0, sizeof(a));
    a.starts = rt->cycles.d_starts;
    a.finds = rt->cycles.d_finds;
    a.records = rt->cycles.d_rec;
    a.orbits = rt->cycles.d_orbits;
    a.jobs = jobs;
    a.period = p.period;
    a.max_newton = p.max_newton;
    a.cap = cap;
    a.tol = p.tol;
    a.bound = p.bound;
    a.merge = p.merge;
    a.same = p.same;
    for (uint32_t first = 0; first < n_maps; first += per) {
        const uint32_t n = std::min(per, n_maps - first);
        a.coeffs = rt->cycles.d_coeffs + first;
        a.n_maps = n;
        SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_cycles_newton(a, rt->stream); }));
        SAR_TRY(timed_lds_launch(rt, rt->tm.fold, [&] { return launch_cycles_merge(a, rt->stream); }));
        HIP_TRY(hipMemcpyAsync(records_out_host + first, rt->cycles.d_rec, n * sizeof(sar_cycles_record), hipMemcpyDeviceToHost, rt->stream));
        HIP_TRY(hipMemcpyAsync(orbits_out_host + static_cast<size_t>(first) * cap, rt->cycles.d_orbits,
                               static_cast<size_t>(n) * cap * sizeof(sar_cycle_orbit), hipMemcpyDeviceToHost, rt->stream));
    }
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (the host's maps and starts have been read, too)
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
