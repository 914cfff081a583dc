// sar_section.cpp — the host half of the Poincare sections of flows (include/sar.h: sar_section_*, sar_runtime_section): the checks
// with the family's own refusal texts, one counted step on the host, and the launches — per chunk of chunk_jobs jobs the transient
// (sar_flow.hip's k_flow_transient), the counted steps in launches of chunk_steps (k_flow_section), the plot (k_section_plot), then
// the chunk's crossings, return times and records copied out; behind the last chunk flows' resolve into the runtime's frame.
//
// Built with -ffp-contract=off: sar_section_step must give what the kernel's lanes compute.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_section.hpp"

using namespace sar;

namespace {

int check_section_params(const sar_section_params& p, const char* where) {
    bool any = false;
    for (int k = 0; k < 10; ++k) {
        if (!std::isfinite(p.surface[k])) { set_error("%s: surface[%d] is not finite (%g)", where, k, p.surface[k]); return SAR_ERR_INVALID; }
        any = any || (k > 0 && p.surface[k] != 0.);
    }
    if (!any) { set_error("%s: the surface is a constant: surface[1] .. surface[9] are all zero", where); return SAR_ERR_INVALID; }
    if (!std::isfinite(p.dt) || !(p.dt > 0.)) { set_error("%s: dt must be finite and positive (%g)", where, p.dt); return SAR_ERR_INVALID; }
    if (!std::isfinite(p.bound) || !(p.bound > 0.)) { set_error("%s: bound must be finite and positive (%g)", where, p.bound); return SAR_ERR_INVALID; }
    if (p.direction < -1 || p.direction > 1) { set_error("%s: direction must be +1, -1 or 0 (%d)", where, p.direction); return SAR_ERR_INVALID; }
    return SAR_OK;
}

int check_section_run(const sar_section_params& p, const char* where) {
    if (p.plot != 0 && p.plot != 1) { set_error("%s: plot must be 0 or 1 (%d)", where, p.plot); return SAR_ERR_INVALID; }
    if (p.samples == 0 || p.samples > kMaxSectionSamples) {
        set_error("%s: samples must be 1 to 2^20 (%u)", where, p.samples);
        return SAR_ERR_INVALID;
    }
    if (p.max_steps == 0) { set_error("%s: max_steps must be at least 1", where); return SAR_ERR_INVALID; }
    if (p.chunk_jobs > kMaxFlowChunk || p.chunk_steps > kMaxFlowChunk) {
        set_error("%s: chunk_jobs and chunk_steps must be at most 2^24 (%u, %u)", where, p.chunk_jobs, p.chunk_steps);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

// next_point (sar_device.hpp) on the host: the ten terms of each sum, left to right
struct HostField {
    const MapParams& p;
    void operator()(double& x, double& y, double& z) const {
        const double t[9] = {x, x * x, x * y, x * z, y, y * y, y * z, z, z * z};
        double sx = p.cx[0], sy = p.cy[0], sz = p.cz[0];
        for (int k = 0; k < 9; ++k) {
            sx = sx + t[k] * p.cx[k + 1];
            sy = sy + t[k] * p.cy[k + 1];
            sz = sz + t[k] * p.cz[k + 1];
        }
        x = sx, y = sy, z = sz;
    }
};

SectionSurface surface_of(const sar_section_params& p) {
    SectionSurface f;
    for (int k = 0; k < 10; ++k) f.s[k] = p.surface[k];
    f.d2 = 2.0 * p.surface[2];
    f.d6 = 2.0 * p.surface[6];
    f.d9 = 2.0 * p.surface[9];
    return f;
}

double key_coordinate(unsigned long long key) {  // sortable_f64 (sar_device.hpp) on the host
    const unsigned long long b = corr_unsortable(key);
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

}  // namespace

extern "C" {

int sar_section_params_default(sar_section_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));  // the surface zero (the caller's to set), plot 0, chunk_jobs 0, chunk_steps 0: the defaults
    out->dt = 0.01;
    out->bound = 1e6;
    out->transient = 1000;
    out->direction = 1;
    out->samples = 1024;
    out->max_steps = 1u << 20;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_section_step(const sar_config* cfg, const sar_section_params* params, double xyz[3], double crossing[3], double* dt_out,
                     int32_t* kind_out) try {
    const char* const where = "sar_section_step";
    if (!cfg || !params || !xyz) { set_error("%s: the config, the parameters or the point is NULL", where); return SAR_ERR_INVALID; }
    const sar_section_params p = *params;
    SAR_TRY(check_section_params(p, where));
    SAR_TRY(validate(cfg));
    MapParams mp;
    std::memset(&mp, 0, sizeof(mp));
    fill_map_params(*cfg, mp);
    const SectionSurface f = surface_of(p);
    const double g0 = section_g(f, xyz[0], xyz[1], xyz[2]);
    double g1 = 0., q[3] = {0., 0., 0.}, dt = 0.;
    const int kind = section_step(HostField{mp}, f, p.dt, p.dt * 0.5, p.dt / 6.0, p.bound, p.direction, g0, xyz[0], xyz[1], xyz[2], g1, q[0],
                                  q[1], q[2], dt);
    if (kind > 0) {
        if (crossing) std::memcpy(crossing, q, sizeof(q));
        if (dt_out) *dt_out = dt;
    }
    if (kind_out) *kind_out = kind;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_section(const sar_config* cfg, sar_runtime* rt, const sar_section_params* params, uint32_t n_jobs,
                        const double* starts_xyz_host, double* points_out, double* ret_out, sar_section_record* records_out,
                        sar_section_stats* stats_out) try {
    const char* const where = "sar_runtime_section";
    if (!params) { set_error("%s: the parameters are NULL (there is no default surface)", where); return SAR_ERR_INVALID; }
    const sar_section_params p = *params;
    SAR_TRY(check_section_params(p, where));  // (no device needed to refuse the parameters)
    SAR_TRY(check_section_run(p, where));
    SAR_TRY(validate(cfg));
    if (!n_jobs) { set_error("%s: n_jobs must be at least 1", where); return SAR_ERR_INVALID; }
    if (static_cast<uint64_t>(n_jobs) * p.samples > kMaxSectionCrossings) {
        set_error("%s: n_jobs * samples must be at most 2^24 (%u * %u)", where, n_jobs, p.samples);
        return SAR_ERR_INVALID;
    }
    if (starts_xyz_host)
        for (size_t k = 0; k < static_cast<size_t>(n_jobs) * 3u; ++k)
            if (!std::isfinite(starts_xyz_host[k])) {
                set_error("%s: start point %zu is not finite", where, k / 3u);
                return SAR_ERR_INVALID;
            }
    if (!rt || !starts_xyz_host || !points_out || !ret_out || !records_out || !stats_out) {
        set_error("%s: the runtime, the start points or an output is NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(check_cfg_matches(cfg, rt));
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_flow_transient, iterate_ms = k_flow_section, colorize_ms = k_flow_resolve

    const bool plot = p.plot != 0;
    const uint32_t chunk = std::min(p.chunk_jobs ? p.chunk_jobs : kDefaultFlowChunkJobs, n_jobs);
    const uint64_t csteps = p.chunk_steps ? p.chunk_steps : kDefaultFlowChunkSteps;
    const uint32_t samples = p.samples;
    FlowState& f = rt->flow;
    SectionState& s = rt->section;
    // (what can fail for want of room comes before the frame is touched: a refusal leaves it as it was)
    HIP_TRY(f.d_state.grow(nullptr, static_cast<size_t>(chunk) * 3u));
    HIP_TRY(f.d_sums.grow(nullptr, 1));
    if (plot) HIP_TRY(f.d_keys.grow(nullptr, rt->npix));
    HIP_TRY(s.d_rows.grow(nullptr, static_cast<size_t>(chunk) * kSectionRows));
    HIP_TRY(s.d_dt_prev.grow(nullptr, chunk));
    HIP_TRY(s.d_cross.grow(nullptr, static_cast<size_t>(chunk) * samples * 4u));
    HIP_TRY(s.d_sums.grow(nullptr, 1));
    std::vector<double> soa(static_cast<size_t>(chunk) * 3u), zeros(chunk, 0.), cross(static_cast<size_t>(chunk) * samples * 4u);
    std::vector<uint32_t> rows(static_cast<size_t>(chunk) * kSectionRows), rows_back(rows.size());

    if (plot) HIP_TRY(hipMemsetAsync(f.d_keys, 0, static_cast<size_t>(rt->npix) * sizeof(unsigned long long), rt->stream));
    FlowSums fzero;  // k_flow_transient adds its escapes here; k_flow_section counts them itself, from the marks
    std::memset(&fzero, 0, sizeof(fzero));
    HIP_TRY(hipMemcpyAsync(f.d_sums, &fzero, sizeof(fzero), hipMemcpyHostToDevice, rt->stream));
    SectionSums zero;
    std::memset(&zero, 0, sizeof(zero));
    for (int c = 0; c < 3; ++c) zero.lo[c] = kFlowNoMin;
    zero.ret_lo = kFlowNoMin;
    HIP_TRY(hipMemcpyAsync(s.d_sums, &zero, sizeof(zero), hipMemcpyHostToDevice, rt->stream));

    FlowArgs t;  // the transient's
    std::memset(&t, 0, sizeof(t));
    fill_map_params(*cfg, t.p);
    fill_ct_params(*cfg, t.ct);
    t.state = f.d_state;
    t.sums = f.d_sums;
    t.h = p.dt;
    t.h2 = p.dt * 0.5;
    t.h6 = p.dt / 6.0;
    t.bound = p.bound;
    t.width = rt->W;
    t.stride = 1;

    SectionArgs a;
    std::memset(&a, 0, sizeof(a));
    a.p = t.p;
    a.f = surface_of(p);
    a.state = f.d_state;
    a.dt_prev = s.d_dt_prev;
    a.rows = s.d_rows;
    a.cross = s.d_cross;
    a.sums = s.d_sums;
    a.h = t.h;
    a.h2 = t.h2;
    a.h6 = t.h6;
    a.bound = p.bound;
    a.samples = samples;
    a.direction = p.direction;

    SectionPlotArgs q;
    std::memset(&q, 0, sizeof(q));
    q.p = t.p;
    q.cross = s.d_cross;
    q.count = rt->d_count;
    q.keys = f.d_keys;
    q.sums = s.d_sums;
    q.samples = samples;
    q.width = rt->W;

    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::fill(points_out, points_out + static_cast<size_t>(n_jobs) * samples * 3u, nan);
    std::fill(ret_out, ret_out + static_cast<size_t>(n_jobs) * samples, nan);
    for (uint32_t first = 0; first < n_jobs; first += chunk) {
        const uint32_t m = std::min(chunk, n_jobs - first);
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t c = 0; c < 3u; ++c) soa[static_cast<size_t>(c) * m + j] = starts_xyz_host[(static_cast<size_t>(first) + j) * 3u + c];
        for (uint32_t j = 0; j < m; ++j) {  // the rows of a job before its first step: status, found, rough, steps, clock_step, t_prev
            rows[j] = SAR_SECTION_SHORT;
            rows[m + j] = rows[2u * m + j] = rows[3u * m + j] = rows[5u * m + j] = 0u;
            rows[4u * m + j] = kSectionNone;
        }
        HIP_TRY(hipMemcpyAsync(f.d_state, soa.data(), static_cast<size_t>(m) * 3u * sizeof(double), hipMemcpyHostToDevice, rt->stream));
        HIP_TRY(hipMemcpyAsync(s.d_rows, rows.data(), static_cast<size_t>(m) * kSectionRows * sizeof(uint32_t), hipMemcpyHostToDevice, rt->stream));
        HIP_TRY(hipMemcpyAsync(s.d_dt_prev, zeros.data(), static_cast<size_t>(m) * sizeof(double), hipMemcpyHostToDevice, rt->stream));
        t.n_jobs = a.n_jobs = q.n_jobs = m;
        q.found = s.d_rows.get() + m;
        for (uint64_t done = 0; done < p.transient; done += csteps) {
            t.n_steps = static_cast<uint32_t>(std::min<uint64_t>(csteps, p.transient - done));
            SAR_TRY(timed_launch(rt, rt->tm.warm, [&] { launch_flow_transient(t, rt->stream); }));
        }
        for (uint64_t done = 0; done < p.max_steps; done += csteps) {  // (max_steps alone ends them: nothing is read back in between)
            a.n_steps = static_cast<uint32_t>(std::min<uint64_t>(csteps, p.max_steps - done));
            a.t0 = static_cast<uint32_t>(done);
            SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_flow_section(a, rt->stream); }));
        }
        if (plot) {
            launch_section_plot(q, rt->stream);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(rows_back.data(), s.d_rows, static_cast<size_t>(m) * kSectionRows * sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
        HIP_TRY(hipMemcpyAsync(cross.data(), s.d_cross, static_cast<size_t>(m) * samples * 4u * sizeof(double), hipMemcpyDeviceToHost, rt->stream));
        HIP_TRY(hipStreamSynchronize(rt->stream));  // (the staging is reused by the next chunk)
        for (uint32_t j = 0; j < m; ++j) {
            sar_section_record& rec = records_out[first + j];
            rec.status = rows_back[j];
            rec.found = rows_back[m + j];
            rec.rough = rows_back[2u * m + j];
            rec.steps = rows_back[3u * m + j];
            rec.clock_step = rows_back[4u * m + j];
            rec._pad = 0;
            const double* const src = cross.data() + static_cast<size_t>(j) * samples * 4u;
            double* const pts = points_out + (static_cast<size_t>(first) + j) * samples * 3u;
            double* const ret = ret_out + (static_cast<size_t>(first) + j) * samples;
            for (uint32_t k = 0; k < rec.found && k < samples; ++k) {
                std::memcpy(pts + static_cast<size_t>(k) * 3u, src + static_cast<size_t>(k) * 4u, 3u * sizeof(double));
                ret[k] = src[static_cast<size_t>(k) * 4u + 3u];
            }
        }
    }
    if (plot) {
        FlowResolveArgs r;
        std::memset(&r, 0, sizeof(r));
        r.keys = f.d_keys;
        r.count = rt->d_count;
        r.zkey = rt->d_key;
        r.steps = rt->d_steps;
        r.scalars = rt->d_scalars;
        r.npix = rt->npix;
        rt->tm.single_begin(rt->tm.colorize_span, rt->stream);
        launch_flow_resolve(r, rt->stream);
        rt->tm.single_end(rt->tm.colorize_span, rt->tm.colorize_timed, rt->stream);
        HIP_TRY(hipGetLastError());
        SAR_TRY(rt->hints.clear(rt->npix, rt->stream));  // what sar_runtime_load does for the depth hints: the next render learns them anew
    }
    SectionSums sums;
    uint32_t sc[SC_COUNT];
    HIP_TRY(hipMemcpyAsync(&sums, s.d_sums, sizeof(sums), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipMemcpyAsync(sc, rt->d_scalars, sizeof(sc), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->tm.last_iterations += sums.steps;

    sar_section_stats st;
    std::memset(&st, 0, sizeof(st));
    st.steps = sums.steps;
    st.crossings = sums.crossings;
    st.rough = sums.rough;
    st.clocked = sums.clocked;
    st.full = sums.full;
    st.escaped = sums.escaped;
    st.escaped_transient = sums.escaped_transient;
    st.short_jobs = n_jobs - sums.full - sums.escaped - sums.escaped_transient;
    st.visits = sums.visits;
    st.outside = sums.outside;
    const double inf = std::numeric_limits<double>::infinity();
    for (int c = 0; c < 3; ++c) {
        st.extent[2 * c] = sums.lo[c] == kFlowNoMin ? inf : key_coordinate(sums.lo[c]);
        st.extent[2 * c + 1] = sums.hi[c] == 0ull ? -inf : key_coordinate(sums.hi[c]);
    }
    st.ret_min = sums.ret_lo == kFlowNoMin ? inf : key_coordinate(sums.ret_lo);
    st.ret_max = sums.ret_hi == 0ull ? -inf : key_coordinate(sums.ret_hi);
    st.residual_max = sums.residual == 0ull ? 0. : key_coordinate(sums.residual);
    st.max = sc[SC_WRAP] ? 0xFFFFFFFFu : sc[SC_MAX];
    *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
