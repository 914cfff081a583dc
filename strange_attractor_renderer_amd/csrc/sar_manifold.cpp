// sar_manifold.cpp — the host half of the unstable-manifold family (include/sar.h: sar_manifold_*, sar_runtime_manifold): the checks
// with the family's own refusal texts, the fundamental domain of every branch, the launch of k_manifold (sar_manifold.hip) behind
// the cleared images, and the read-back of the images and the records.
//
// Built with -ffp-contract=off: the fundamental domains' ends a, b and d = b - a are the doubles the device's samples are made
// from, and sar_manifold_pixel must give what k_manifold's lanes compute.
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_manifold.hpp"

using namespace sar;

namespace {

int check_manifold_params(const sar_manifold_params& p, const char* where) {
    if (p.samples < kMinManifoldSamples || p.samples > kMaxManifoldSamples) {
        set_error("%s: samples must be 2 to 2^20 points of a fundamental domain (%u)", where, p.samples);
        return SAR_ERR_INVALID;
    }
    if (p.steps > kMaxManifoldSteps) {
        set_error("%s: steps must be at most %u for a manifold (%u)", where, kMaxManifoldSteps, p.steps);
        return SAR_ERR_INVALID;
    }
    if (!p.max_span || p.max_span > kMaxManifoldSpan) {
        set_error("%s: max_span must be 1 to %u pixels (%u)", where, kMaxManifoldSpan, p.max_span);
        return SAR_ERR_INVALID;
    }
    return check_bound(where, p.bound);
}

int check_manifold_totals(const sar_manifold_params& p, uint32_t n_branches, const char* where) {
    if (n_branches > kMaxManifoldBranches) {
        set_error("%s: a call takes at most %u branches (%u)", where, kMaxManifoldBranches, n_branches);
        return SAR_ERR_INVALID;
    }
    // (4096 * 2^20 * 2^16 = 2^48: no overflow)
    const uint64_t segments = static_cast<uint64_t>(n_branches) * (p.samples - 1u) * (static_cast<uint64_t>(p.steps) + 1u);
    if (segments >= (1ull << 32)) {
        set_error("%s: branches * (samples - 1) * (steps + 1) must stay below 2^32 segments (%llu)", where,
                  static_cast<unsigned long long>(segments));
        return SAR_ERR_INVALID;
    }
    const uint64_t lanes = static_cast<uint64_t>(n_branches) * manifold_waves_per_branch(p.samples) * 64u;
    if (lanes > kMaxManifoldLanes) {
        set_error("%s: a call takes at most 2^26 lanes, 64 per 63 segments of a branch (%llu)", where, static_cast<unsigned long long>(lanes));
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

int check_manifold_branch(const sar_manifold_branch& b, uint32_t index, const char* where) {
    bool finite = std::isfinite(b.delta), any = false;
    for (int k = 0; k < 3; ++k) {
        finite = finite && std::isfinite(b.base[k]) && std::isfinite(b.dir[k]);
        any = any || b.dir[k] != 0.;
    }
    if (!finite) {
        set_error("%s: branch %u: base, dir and delta must be finite", where, index);
        return SAR_ERR_INVALID;
    }
    if (b.delta == 0. || !any) {
        set_error("%s: branch %u: delta and dir must not be zero", where, index);
        return SAR_ERR_INVALID;
    }
    if (!b.period || b.period > kMaxManifoldPeriod) {
        set_error("%s: branch %u: period must be 1 to %u map steps per return (%u)", where, index, kMaxManifoldPeriod, b.period);
        return SAR_ERR_INVALID;
    }
    return SAR_OK;
}

// cfg's hoisted constants with ALL 30 coefficients through `0. + 1. * c` (fill_map_params does it for the constant terms)
void manifold_map_params(const sar_config& cfg, MapParams& p) {
    fill_map_params(cfg, p);
    canonical_coeffs(p.cx, 10, p.cx);
    canonical_coeffs(p.cy, 10, p.cy);
    canonical_coeffs(p.cz, 10, p.cz);
}

bool within_bound(const double v[3], double bound) { return std::fabs(v[0]) <= bound && std::fabs(v[1]) <= bound && std::fabs(v[2]) <= bound; }

// next_point (sar_device.hpp) on the host: the ten terms of each sum, left to right
void host_next_point(const MapParams& p, double v[3]) {
    const double x = v[0], y = v[1], z = v[2];
    const double t[9] = {x, x * x, x * y, x * z, y, y * y, y * z, z, z * z};
    double sx = p.cx[0], sy = p.cy[0], sz = p.cz[0];
    for (int k = 0; k < 9; ++k) {
        sx = sx + t[k] * p.cx[k + 1];
        sy = sy + t[k] * p.cy[k + 1];
        sz = sz + t[k] * p.cz[k + 1];
    }
    v[0] = sx;
    v[1] = sy;
    v[2] = sz;
}

// a and b of one branch into the record, and the device's block; false where a point on the way fails the bound test
bool fundamental_domain(const MapParams& p, const sar_manifold_branch& br, double bound, sar_manifold_record& rec, ManifoldBranch& dev) {
    double v[3];
    for (int k = 0; k < 3; ++k) rec.a[k] = v[k] = br.base[k] + br.delta * br.dir[k];
    bool ok = within_bound(v, bound);
    for (uint32_t s = 0; s < br.period; ++s) {
        host_next_point(p, v);
        ok = ok && within_bound(v, bound);
    }
    for (int k = 0; k < 3; ++k) {
        rec.b[k] = v[k];
        dev.a[k] = rec.a[k];
        dev.d[k] = rec.b[k] - rec.a[k];
    }
    dev.live = ok ? 1u : 0u;
    dev._pad = 0u;
    return ok;
}

}  // namespace

extern "C" {

int sar_manifold_params_default(sar_manifold_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->samples = 4096;
    out->steps = 32;
    out->max_span = 16;
    out->bound = 1e6;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_manifold_pixel(const sar_config* cfg, const double xyz[3], double out_fi_fj[2]) try {
    SAR_TRY(validate(cfg));
    if (!xyz || !out_fi_fj) return SAR_ERR_INVALID;
    MapParams p;
    manifold_map_params(*cfg, p);
    manifold_project(p, xyz[0], xyz[1], xyz[2], out_fi_fj[0], out_fi_fj[1]);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_manifold(sar_runtime* rt, const sar_config* cfg, const sar_manifold_params* params, uint32_t n_branches,
                         const sar_manifold_branch* branches_host, uint32_t* count_out_host, uint32_t* first_out_host,
                         sar_manifold_record* records_out_host) try {
    const char* const where = "sar_runtime_manifold";
    const sar_manifold_params p = given_or_default(params, sar_manifold_params_default);
    SAR_TRY(validate(cfg));  // (no device needed to refuse the parameters)
    SAR_TRY(check_plane_size(where, cfg->width, cfg->height));
    SAR_TRY(check_manifold_params(p, where));
    SAR_TRY(check_manifold_totals(p, n_branches, where));
    if (!n_branches) return SAR_OK;
    // (the branches are refused before a missing runtime is: no device is needed to see what is wrong with them)
    if (branches_host)
        for (uint32_t k = 0; k < n_branches; ++k) SAR_TRY(check_manifold_branch(branches_host[k], k, where));
    if (!rt || !branches_host || !count_out_host || !first_out_host || !records_out_host) {
        set_error("%s: the runtime, the branches or an output buffer of the manifold is NULL", where);
        return SAR_ERR_INVALID;
    }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_manifold (sar_timing)

    ManifoldArgs a;
    std::memset(&a, 0, sizeof(a));
    manifold_map_params(*cfg, a.p);
    std::vector<ManifoldBranch> blocks(n_branches);
    std::vector<ManifoldSums> sums(n_branches);
    std::memset(sums.data(), 0, sums.size() * sizeof(ManifoldSums));
    for (uint32_t k = 0; k < n_branches; ++k) {
        sar_manifold_record& r = records_out_host[k];
        std::memset(&r, 0, sizeof(r));
        r.status = fundamental_domain(a.p, branches_host[k], p.bound, r, blocks[k]) ? SAR_MANIFOLD_OK : SAR_MANIFOLD_DOMAIN_ESCAPED;
        sums[k].first_long_step = kManifoldNone;
    }

    const size_t npix = static_cast<size_t>(cfg->width) * cfg->height;
    ManifoldState& m = rt->manifold;
    HIP_TRY(m.d_branches.grow(nullptr, n_branches));
    HIP_TRY(m.d_sums.grow(nullptr, n_branches));
    HIP_TRY(m.d_count.grow(nullptr, npix));
    HIP_TRY(m.d_first.grow(nullptr, npix));
    HIP_TRY(hipMemcpyAsync(m.d_branches, blocks.data(), n_branches * sizeof(ManifoldBranch), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(m.d_sums, sums.data(), n_branches * sizeof(ManifoldSums), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemsetAsync(m.d_count, 0, npix * sizeof(uint32_t), rt->stream));
    HIP_TRY(hipMemsetAsync(m.d_first, 0xFF, npix * sizeof(uint32_t), rt->stream));

    a.branches = m.d_branches;
    a.sums = m.d_sums;
    a.count = m.d_count;
    a.first = m.d_first;
    a.n_branches = n_branches;
    a.samples = p.samples;
    a.steps = p.steps;
    a.max_span = p.max_span;
    a.waves_per_branch = manifold_waves_per_branch(p.samples);
    a.width = cfg->width;
    a.height = cfg->height;
    a.bound = p.bound;
    SAR_TRY(timed_launch(rt, rt->tm.iter, [&] { launch_manifold(a, rt->stream); }));

    HIP_TRY(hipMemcpyAsync(count_out_host, m.d_count, npix * sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipMemcpyAsync(first_out_host, m.d_first, npix * sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipMemcpyAsync(sums.data(), m.d_sums, n_branches * sizeof(ManifoldSums), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));  // (the host's blocks and sums have been read, too)
    for (uint32_t k = 0; k < n_branches; ++k) {
        sar_manifold_record& r = records_out_host[k];
        const ManifoldSums& s = sums[k];
        r.first_long_step = s.first_long_step;
        r.alive_end = s.alive_end;
        r.n_drawn = s.drawn;
        r.n_dead = s.dead;
        r.n_far = s.far;
        r.n_long = s.longs;
        r.pixels = s.pixels;
        r.length_px = s.length_px;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
