// sar_density.cpp — the host half of density estimation (include/sar.h: sar_density_*, sar_runtime_density): the weight tables of
// the contract, the packed plan the kernel keeps in LDS, the checks, the snapshot and the scratch, the launch of k_density
// (sar_density.hip) and the statistics.
//
// Built with -ffp-contract=off: t, u and q of a weight are one IEEE operation each.
#include <cmath>
#include <cstring>

#include "sar_analysis.hpp"
#include "sar_density.hpp"

using namespace sar;

void sar::density_row(uint32_t S, uint32_t c, uint32_t* out) {
    std::memset(out, 0, S * sizeof(uint32_t));
    if (c >= S) {  // the identity
        out[0] = 65536u;
        return;
    }
    const int R = static_cast<int>(density_radius(S));
    std::vector<int64_t> q(S, 0);
    for (uint32_t d2 = 0; d2 < S && d2 * c < S; ++d2) {
        const double t = static_cast<double>(d2 * c) / static_cast<double>(S);
        const double u = 1.0 - t;
        const double uu = u * u;
        q[d2] = static_cast<int64_t>(std::floor(uu * 1048576.0));
    }
    auto live = [&](int dx, int dy) { return static_cast<uint32_t>(dx * dx + dy * dy) * c < S; };
    int64_t n = 0;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx)
            if (live(dx, dy)) n += q[dx * dx + dy * dy];
    for (uint32_t d2 = 1; d2 < S && d2 * c < S; ++d2) out[d2] = static_cast<uint32_t>((q[d2] << 16) / n);
    uint32_t rest = 0;
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx)
            if ((dx || dy) && live(dx, dy)) rest += out[dx * dx + dy * dy];
    out[0] = 65536u - rest;
}

std::vector<uint32_t> sar::density_plan(uint32_t S) {
    std::vector<uint32_t> rows(static_cast<size_t>(S) * S, 0u);  // [c][d2]; row 0 unused
    for (uint32_t c = 1; c < S; ++c) density_row(S, c, &rows[static_cast<size_t>(c) * S]);
    std::vector<uint32_t> plan(S, 0u);
    for (uint32_t d2 = 0; d2 < S; ++d2) {
        plan[d2] = static_cast<uint32_t>(plan.size());
        const uint32_t classes = d2 ? (S - 1u) / d2 : S - 1u;
        for (uint32_t c = 1; c <= classes; ++c) plan.push_back(rows[static_cast<size_t>(c) * S + d2]);
    }
    return plan;
}

namespace {

int check_density(const sar_density_params* p, const char* where) {
    if (p->samples < kDensityMinSamples || p->samples > kDensityMaxSamples) {
        set_error("%s: samples must be %u to %u (%u)", where, kDensityMinSamples, kDensityMaxSamples, p->samples);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

}  // namespace

extern "C" {

int sar_density_params_default(sar_density_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->samples = kDensityDefaultSamples;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_density_radius(const sar_density_params* params, uint32_t* out_radius) try {
    const sar_density_params p = given_or_default(params, sar_density_params_default);
    SAR_TRY(check_density(&p, "sar_density_radius"));
    if (!out_radius) return SAR_ERR_INVALID;
    *out_radius = density_radius(p.samples);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_density_weights(const sar_density_params* params, uint32_t c, uint32_t* out) try {
    const sar_density_params p = given_or_default(params, sar_density_params_default);
    SAR_TRY(check_density(&p, "sar_density_weights"));
    if (!c) { set_error("sar_density_weights: class 0 has no table (an empty pixel spreads nothing)"); return SAR_ERR_INVALID; }
    if (!out) return SAR_ERR_INVALID;
    density_row(p.samples, c, out);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_density(sar_runtime* rt, const sar_density_params* params, sar_density_stats* stats_out) try {
    const sar_density_params p = given_or_default(params, sar_density_params_default);
    SAR_TRY(check_density(&p, "sar_runtime_density"));  // (no device needed to refuse the parameters)
    if (!rt) { set_error("sar_runtime_density: the runtime is NULL"); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_density (sar_timing)
    const size_t npix = rt->npix;
    // the snapshot (steps first: 8-byte aligned whatever npix), the reduction block and the plan: plain allocations (not the group
    // slab), kept for the next call and freed with the runtime
    HIP_TRY(rt->density.d_snap.grow(nullptr, npix * 12u));
    HIP_TRY(rt->density.d_stats.grow(nullptr, 1));
    std::vector<uint32_t>& plan = rt->density.h_plans[p.samples];
    if (plan.empty()) plan = density_plan(p.samples);
    if (plan.size() > kDensityPlanMaxWords) { set_error("sar_runtime_density: the plan outgrew its buffer"); return SAR_ERR_INTERNAL; }
    if (rt->density.plan_samples != p.samples) {
        rt->density.plan_samples = 0;
        HIP_TRY(rt->density.d_plan.grow(nullptr, kDensityPlanMaxWords));
        // behind the last call's kernel, which may still read the old plan
        HIP_TRY(hipMemcpyAsync(rt->density.d_plan, plan.data(), plan.size() * sizeof(uint32_t), hipMemcpyHostToDevice, rt->stream));
        rt->density.plan_samples = p.samples;
    }
    double* snap_steps = reinterpret_cast<double*>(rt->density.d_snap.get());
    uint32_t* snap_count = reinterpret_cast<uint32_t*>(rt->density.d_snap.get() + npix * 8u);
    HIP_TRY(hipMemcpyAsync(snap_steps, rt->d_steps, npix * 8u, hipMemcpyDeviceToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(snap_count, rt->d_count, npix * 4u, hipMemcpyDeviceToDevice, rt->stream));
    HIP_TRY(hipMemsetAsync(rt->density.d_stats, 0, sizeof(DensityDeviceStats), rt->stream));
    HIP_TRY(hipMemsetAsync(rt->d_scalars + SC_MAX, 0, sizeof(uint32_t), rt->stream));  // max is recomputed; the wrap flag stays
    DensityArgs a;
    std::memset(&a, 0, sizeof(a));
    a.snap_steps = snap_steps;
    a.snap_count = snap_count;
    a.steps = rt->d_steps;
    a.count = rt->d_count;
    a.scalars = rt->d_scalars;
    a.stats = rt->density.d_stats;
    a.plan = rt->density.d_plan;
    a.width = rt->W;
    a.height = rt->H;
    a.S = p.samples;
    a.R = density_radius(p.samples);
    a.tile_h = rt->opt.density_tile ? rt->opt.density_tile : kDensityDefaultTileH;
    a.tiles_x = (rt->W + kDensityTileW - 1u) / kDensityTileW;
    a.plan_words = static_cast<uint32_t>(plan.size());
    const uint32_t tiles = a.tiles_x * ((rt->H + a.tile_h - 1u) / a.tile_h);
    SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_density(a, tiles, rt->stream); }));
    if (stats_out) {
        DensityDeviceStats st;
        HIP_TRY(hipMemcpyAsync(&st, rt->density.d_stats, sizeof(st), hipMemcpyDeviceToHost, rt->stream));
        HIP_TRY(hipStreamSynchronize(rt->stream));
        *stats_out = st.s;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_density_tiles(sar_runtime* rt, uint32_t* tiles_out, uint32_t* copied_out) try {
    if (!rt || !tiles_out || !copied_out) return SAR_ERR_INVALID;
    if (!rt->density.d_stats) { set_error("sar_runtime_density_tiles: the runtime has not filtered yet (sar_runtime_density first)"); return SAR_ERR_INVALID; }
    HIP_TRY(hipSetDevice(rt->device));
    DensityDeviceStats st;
    HIP_TRY(hipMemcpyAsync(&st, rt->density.d_stats, sizeof(st), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    *tiles_out = st.tiles;
    *copied_out = st.tiles_copied;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
