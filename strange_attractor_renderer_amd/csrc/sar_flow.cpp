// sar_flow.cpp — the host half of flow rendering (include/sar.h: sar_flow_*, sar_runtime_render_flow): the checks with the family's
// own refusal texts, one RK4 step on the host, and the launches of sar_flow.hip's kernels — the transient, then the counted steps in
// launches of chunk_jobs jobs by chunk_steps steps, then the resolve into the runtime's frame.
//
// Built with -ffp-contract=off: h * 0.5 and h / 6.0 are one IEEE operation each, and sar_flow_step must give what the kernels' lanes
// compute.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_flow.hpp"

using namespace sar;

namespace {

int check_flow_params(const sar_flow_params& p, const char* where) {
    if (!std::isfinite(p.dt) || !(p.dt > 0.)) { set_error("%s: dt must be finite and positive (%g)", where, p.dt); return SAR_ERR_INVALID; }
    if (!std::isfinite(p.bound) || !(p.bound > 0.)) { set_error("%s: bound must be finite and positive (%g)", where, p.bound); return SAR_ERR_INVALID; }
    if (p.stride == 0) { set_error("%s: stride must be at least 1", where); return SAR_ERR_INVALID; }
    if (p.plot != 0 && p.plot != 1) { set_error("%s: plot must be 0 or 1 (%d)", where, p.plot); return SAR_ERR_INVALID; }
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

double key_coordinate(unsigned long long key) {  // sortable_f64 (sar_device.hpp) on the host
    const unsigned long long b = corr_unsortable(key);
    double v;
    std::memcpy(&v, &b, 8);
    return v;
}

}  // namespace

extern "C" {

int sar_flow_params_default(sar_flow_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));  // chunk_jobs 0, chunk_steps 0: the defaults
    out->dt = 0.01;
    out->bound = 1e6;
    out->transient = 1000;
    out->stride = 1;
    out->plot = 1;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_flow_step(const sar_config* cfg, const sar_flow_params* params, double xyz[3], int32_t* within_out) try {
    const char* const where = "sar_flow_step";
    if (!cfg || !xyz) { set_error("%s: the config or the point is NULL", where); return SAR_ERR_INVALID; }
    const sar_flow_params p = given_or_default(params, sar_flow_params_default);
    SAR_TRY(check_flow_params(p, where));
    SAR_TRY(validate(cfg));
    MapParams mp;
    std::memset(&mp, 0, sizeof(mp));
    fill_map_params(*cfg, mp);
    const bool within = flow_step(HostField{mp}, p.dt, p.dt * 0.5, p.dt / 6.0, p.bound, xyz[0], xyz[1], xyz[2]);
    if (within_out) *within_out = within ? 1 : 0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_render_flow(const sar_config* cfg, sar_runtime* rt, const sar_flow_params* params, uint32_t n_jobs, uint64_t steps_per_job,
                            const double* starts_xyz_host, sar_flow_stats* stats_out) try {
    const char* const where = "sar_runtime_render_flow";
    const sar_flow_params p = given_or_default(params, sar_flow_params_default);
    SAR_TRY(check_flow_params(p, where));  // (no device needed to refuse the parameters)
    SAR_TRY(validate(cfg));
    if (!n_jobs) { set_error("%s: n_jobs must be at least 1", where); return SAR_ERR_INVALID; }
    if (steps_per_job / p.stride > kMaxFlowPlots) {
        set_error("%s: steps_per_job / stride must be at most 2^32 - 1, what one job may add to a pixel (%llu / %u)", where,
                  static_cast<unsigned long long>(steps_per_job), p.stride);
        return SAR_ERR_INVALID;
    }
    if (starts_xyz_host)
        for (size_t k = 0; k < static_cast<size_t>(n_jobs) * 3u; ++k)
            if (!std::isfinite(starts_xyz_host[k])) {
                set_error("%s: start point %zu is not finite", where, k / 3u);
                return SAR_ERR_INVALID;
            }
    if (!rt || !starts_xyz_host || !stats_out) {
        set_error("%s: the runtime, the start points or the statistics' output is NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(check_cfg_matches(cfg, rt));
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_flow_transient, iterate_ms = k_flow_render, colorize_ms = k_flow_resolve

    const bool plot = p.plot != 0;
    const uint32_t chunk = std::min(p.chunk_jobs ? p.chunk_jobs : kDefaultFlowChunkJobs, n_jobs);
    const uint64_t csteps = p.chunk_steps ? p.chunk_steps : kDefaultFlowChunkSteps;
    FlowState& f = rt->flow;
    // (what can fail for want of room comes before the frame is touched: a refusal leaves it as it was)
    HIP_TRY(f.d_state.grow(nullptr, static_cast<size_t>(chunk) * 3u));
    HIP_TRY(f.d_sums.grow(nullptr, 1));
    if (plot) HIP_TRY(f.d_keys.grow(nullptr, rt->npix));

    // The frame needs no folding first: a render call leaves count, the depth keys (low word 0xFFFFFFFF) and steps final behind what it
    // enqueued on the launch stream, which is the state sar_runtime_load writes, and these launches follow on the same stream.
    if (plot) HIP_TRY(hipMemsetAsync(f.d_keys, 0, static_cast<size_t>(rt->npix) * sizeof(unsigned long long), rt->stream));
    FlowSums zero;
    std::memset(&zero, 0, sizeof(zero));
    for (int c = 0; c < 3; ++c) zero.lo[c] = kFlowNoMin;
    HIP_TRY(hipMemcpyAsync(f.d_sums, &zero, sizeof(zero), hipMemcpyHostToDevice, rt->stream));

    FlowArgs a;
    std::memset(&a, 0, sizeof(a));
    fill_map_params(*cfg, a.p);
    fill_ct_params(*cfg, a.ct);
    a.state = f.d_state;
    a.count = plot ? rt->d_count.get() : nullptr;
    a.keys = plot ? f.d_keys.get() : nullptr;
    a.sums = f.d_sums;
    a.h = p.dt;
    a.h2 = p.dt * 0.5;
    a.h6 = p.dt / 6.0;
    a.bound = p.bound;
    a.width = rt->W;
    a.stride = p.stride;
    a.plot = plot ? 1 : 0;

    std::vector<double> soa(static_cast<size_t>(n_jobs) * 3u);  // every chunk's [3][m], alive until the stream has been waited for
    for (uint32_t first = 0; first < n_jobs; first += chunk) {
        const uint32_t m = std::min(chunk, n_jobs - first);
        double* const block = soa.data() + static_cast<size_t>(first) * 3u;
        for (uint32_t j = 0; j < m; ++j)
            for (uint32_t c = 0; c < 3u; ++c) block[static_cast<size_t>(c) * m + j] = starts_xyz_host[(static_cast<size_t>(first) + j) * 3u + c];
        HIP_TRY(hipMemcpyAsync(f.d_state, block, static_cast<size_t>(m) * 3u * sizeof(double), hipMemcpyHostToDevice, rt->stream));
        a.n_jobs = m;
        for (uint64_t done = 0; done < p.transient; done += csteps) {
            a.n_steps = static_cast<uint32_t>(std::min<uint64_t>(csteps, p.transient - done));
            SAR_TRY(timed_launch(rt, rt->tm.warm, [&] { launch_flow_transient(a, rt->stream); }));
        }
        for (uint64_t done = 0; done < steps_per_job; done += csteps) {
            a.n_steps = static_cast<uint32_t>(std::min(csteps, steps_per_job - done));
            a.phase = static_cast<uint32_t>(done % p.stride);
            SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_flow_render(a, rt->stream); }));
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
    FlowSums s;
    uint32_t sc[SC_COUNT];
    HIP_TRY(hipMemcpyAsync(&s, f.d_sums, sizeof(s), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipMemcpyAsync(sc, rt->d_scalars, sizeof(sc), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->tm.last_iterations += static_cast<uint64_t>(n_jobs) * steps_per_job;

    sar_flow_stats st;
    std::memset(&st, 0, sizeof(st));
    st.steps = s.steps;
    st.visits = s.visits;
    st.outside = s.outside;
    st.escaped_transient = s.escaped_transient;
    st.escaped = s.escaped;
    st.alive = n_jobs - s.escaped_transient - s.escaped;
    st.count_atomics = s.count_atomics;
    st.key_atomics = s.key_atomics;
    for (int c = 0; c < 3; ++c) {
        st.extent[2 * c] = s.lo[c] == kFlowNoMin ? std::numeric_limits<double>::infinity() : key_coordinate(s.lo[c]);
        st.extent[2 * c + 1] = s.hi[c] == 0ull ? -std::numeric_limits<double>::infinity() : key_coordinate(s.hi[c]);
    }
    st.max = sc[SC_WRAP] ? 0xFFFFFFFFu : sc[SC_MAX];
    *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
