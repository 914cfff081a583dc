// sar_basin.cpp — the host half of the basins of attraction (include/sar.h: sar_basin_*, sar_runtime_basin,
// sar_runtime_basin_colorize): the checks, the plane's two parameter tables, the chunked launches of k_basin_screen and k_basin_mark
// (sar_basin.hip), k_basin_finish, and — one loop over the pixels and one over the cells — the table of attractors, the labels and
// the statistics.
//
// Built with -ffp-contract=off: sar_basin_start must produce the doubles the kernels start from, and scale the host's quotient.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_basin.hpp"

using namespace sar;

namespace {

int check_basin(const sar_basin_params* p, const char* where) {
    if (!p) { set_error("%s: the parameters are NULL", where); return SAR_ERR_INVALID; }
    SAR_TRY(check_plane_size(where, p->width, p->height));
    SAR_TRY(check_steps(where, p->transient, p->steps));
    if (static_cast<uint64_t>(p->transient) + p->steps >= (1ull << 32)) {
        set_error("%s: transient + steps must stay below 2^32, escape_step is 32 bits (%u, %u)", where, p->transient, p->steps);
        return SAR_ERR_INVALID;
    }
    if (!p->grid || p->grid > kMaxBasinGrid) {
        set_error("%s: grid must be 1 to %u (%u)", where, kMaxBasinGrid, p->grid);
        return SAR_ERR_INVALID;
    }
    for (uint32_t k = 0; k < kSearchCoeffs; ++k)
        if (!std::isfinite(p->coeffs[k])) {
            set_error("%s: the coefficients must be finite (entry %u)", where, k);
            return SAR_ERR_INVALID;
        }
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(p->origin[k]) || !std::isfinite(p->du[k]) || !std::isfinite(p->dv[k])) {
            set_error("%s: origin, du and dv must be finite", where);
            return SAR_ERR_INVALID;
        }
    SAR_TRY(check_bound(where, p->bound));
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(p->box_lo[k]) || !std::isfinite(p->box_hi[k]) || !(p->box_lo[k] < p->box_hi[k])) {
            set_error("%s: box_lo and box_hi must be finite with box_lo < box_hi", where);
            return SAR_ERR_INVALID;
        }
        if (!std::isfinite(static_cast<double>(p->grid) / (p->box_hi[k] - p->box_lo[k]))) {
            set_error("%s: grid / (box_hi - box_lo) is not finite", where);
            return SAR_ERR_INVALID;
        }
    }
    return SAR_OK;
}

struct Component {
    uint32_t pixels = 0, cells = 0, first_pixel = kBasinEmpty;
    uint32_t lo[3] = {kBasinEmpty, kBasinEmpty, kBasinEmpty}, hi[3] = {0, 0, 0};
};

}  // namespace

extern "C" {

int sar_basin_params_default(sar_basin_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->origin[0] = out->origin[1] = -1.;
    out->du[0] = 2.;
    out->dv[1] = 2.;
    out->width = out->height = 256;
    out->transient = 1000;
    out->steps = 256;
    out->bound = 1e6;
    out->grid = 32;
    for (int k = 0; k < 3; ++k) {
        out->box_lo[k] = -1.;
        out->box_hi[k] = 1.;
    }
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_basin_start(const sar_basin_params* p, uint32_t x, uint32_t y, double out3[3]) try {
    SAR_TRY(check_basin(p, "sar_basin_start"));
    if (!out3 || x >= p->width || y >= p->height) return SAR_ERR_INVALID;
    const double tu = basin_param(x, p->width), tv = basin_param(p->height - 1u - y, p->height);
    for (int k = 0; k < 3; ++k) out3[k] = basin_start(p->origin[k], p->du[k], p->dv[k], tu, tv);
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_basin(sar_runtime* rt, const sar_basin_params* p, sar_basin_pixel* pixels_out_host, sar_basin_attractor* attractors_out_host,
                      uint32_t cap, uint32_t* n_out, sar_basin_stats* stats_out) try {
    if (rt) rt->basin.held = false;  // the probes (sar_fate.cpp) hold the LAST call's picture, and only if it succeeds
    SAR_TRY(check_basin(p, "sar_runtime_basin"));  // (no device needed to refuse the parameters)
    if (!rt || !pixels_out_host) { set_error("sar_runtime_basin: the runtime or the pixel buffer is NULL"); return SAR_ERR_INVALID; }
    if (cap && !attractors_out_host) { set_error("sar_runtime_basin: cap is %u and the attractor buffer NULL", cap); return SAR_ERR_INVALID; }
    SAR_TRY(analysis_begin(rt));  // with timing on: warmup_ms = k_basin_screen, iterate_ms = k_basin_mark (sar_timing)
    rt->basin.width = rt->basin.height = 0;  // no basin picture until this one is whole
    const uint32_t width = p->width, height = p->height, npix = width * height, G = p->grid, nodes = G * G * G;
    const TileBands bands = tile_bands(width, height, rt->opt.basin_chunk ? rt->opt.basin_chunk : kDefaultBasinChunk);
    const size_t slots = static_cast<size_t>(bands.per) * kPlaneTile * kPlaneTile;

    // the plane's parameters, one division per column and per row (basin_param), and the sortable extent's neutral elements
    std::vector<double> t(static_cast<size_t>(width) + height);
    for (uint32_t x = 0; x < width; ++x) t[x] = basin_param(x, width);
    for (uint32_t y = 0; y < height; ++y) t[width + y] = basin_param(height - 1u - y, height);
    unsigned long long ext[6];
    for (int k = 0; k < 3; ++k) {
        ext[2 * k] = ~0ull;
        ext[2 * k + 1] = 0ull;
    }

    HIP_TRY(rt->basin.d_t.grow(nullptr, t.size()));
    HIP_TRY(rt->basin.d_pix.grow(nullptr, npix));
    HIP_TRY(rt->basin.d_label.grow(nullptr, npix));
    HIP_TRY(rt->basin.d_last.grow(nullptr, npix));
    HIP_TRY(rt->basin.d_counter.grow(nullptr, 1));
    HIP_TRY(rt->basin.d_surv_pix.grow(nullptr, slots));
    HIP_TRY(rt->basin.d_surv_xyz.grow(nullptr, slots * 3));
    HIP_TRY(rt->basin.d_parent.grow(nullptr, nodes));
    HIP_TRY(rt->basin.d_node_root.grow(nullptr, nodes));
    HIP_TRY(rt->basin.d_extent.grow(nullptr, 6));
    HIP_TRY(hipMemcpyAsync(rt->basin.d_t, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(rt->basin.d_extent, ext, sizeof(ext), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemsetAsync(rt->basin.d_parent, 0xFF, static_cast<size_t>(nodes) * sizeof(uint32_t), rt->stream));  // kBasinEmpty

    BasinArgs a;
    std::memset(&a, 0, sizeof(a));
    canonical_coeffs(p->coeffs, 10, a.map.cx);
    canonical_coeffs(p->coeffs + 10, 10, a.map.cy);
    canonical_coeffs(p->coeffs + 20, 10, a.map.cz);
    for (int k = 0; k < 3; ++k) {
        a.origin[k] = p->origin[k];
        a.du[k] = p->du[k];
        a.dv[k] = p->dv[k];
        a.box_lo[k] = p->box_lo[k];
        a.scale[k] = static_cast<double>(G) / (p->box_hi[k] - p->box_lo[k]);
    }
    a.bound = p->bound;
    a.tu = rt->basin.d_t;
    a.tv = rt->basin.d_t + width;
    a.pixels = rt->basin.d_pix;
    a.counter = rt->basin.d_counter;
    a.surv_pix = rt->basin.d_surv_pix;
    a.surv_xyz = rt->basin.d_surv_xyz;
    a.parent = rt->basin.d_parent;
    a.last_node = rt->basin.d_last;
    a.node_root = rt->basin.d_node_root;
    a.extent = rt->basin.d_extent;
    a.width = width;
    a.height = height;
    a.tiles_x = bands.tiles_x;
    a.transient = p->transient;
    a.steps = p->steps;
    a.grid = G;
    a.nodes = nodes;
    SAR_TRY(for_tile_bands(bands, [&](uint32_t first, uint32_t n) -> int {
        a.first_tile = first;
        a.n_tiles = n;
        a.slots = n * kPlaneTile * kPlaneTile;
        // (stream order: the last launch's k_basin_mark has read its count and its survivors before they are written again)
        HIP_TRY(hipMemsetAsync(rt->basin.d_counter, 0, sizeof(uint32_t), rt->stream));
        SAR_TRY(timed_launch(rt, rt->tm.warm, [&] { launch_basin_screen(a, rt->stream); }));
        return timed_launch(rt, rt->tm.iter, [&] { launch_basin_mark(a, rt->stream); });
    }));
    launch_basin_finish(a, rt->stream);
    HIP_TRY(hipGetLastError());
    std::vector<uint32_t> node_root(nodes);
    HIP_TRY(hipMemcpyAsync(pixels_out_host, rt->basin.d_pix, static_cast<size_t>(npix) * sizeof(sar_basin_pixel), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipMemcpyAsync(node_root.data(), rt->basin.d_node_root, static_cast<size_t>(nodes) * sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipMemcpyAsync(ext, rt->basin.d_extent, sizeof(ext), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));

    // the table: a component per root (a root is a node: direct-indexed), its basin from the pixels, its cells from the grid
    sar_basin_stats st;
    std::memset(&st, 0, sizeof(st));
    st.pixels = npix;
    std::vector<uint32_t> slot_of(nodes, kBasinEmpty);
    std::vector<Component> comps;
    std::vector<uint32_t> roots;
    auto component = [&](uint32_t root) -> Component& {
        if (slot_of[root] == kBasinEmpty) {
            slot_of[root] = static_cast<uint32_t>(comps.size());
            comps.emplace_back();
            roots.push_back(root);
        }
        return comps[slot_of[root]];
    };
    for (uint32_t i = 0; i < npix; ++i) {
        const sar_basin_pixel& r = pixels_out_host[i];
        if (r.status != SAR_SEARCH_BOUNDED) {
            ++(r.escape_step <= p->transient ? st.escaped_transient : st.escaped_tail);
            continue;
        }
        ++st.bounded;
        if (r.root >= nodes) { set_error("sar_runtime_basin: pixel %u has root %u outside the grid", i, r.root); return SAR_ERR_HIP; }
        Component& c = component(r.root);
        if (!c.pixels++) c.first_pixel = i;  // (ascending i: the lowest pixel index)
    }
    for (uint32_t v = 0; v < nodes; ++v) {
        const uint32_t root = node_root[v];
        if (root == kBasinEmpty) continue;
        if (root >= nodes) { set_error("sar_runtime_basin: cell %u has root %u outside the grid", v, root); return SAR_ERR_HIP; }
        Component& c = component(root);
        ++c.cells;
        ++st.cells;
        const uint32_t cell[3] = {v % G, v / G % G, v / G / G};
        for (int k = 0; k < 3; ++k) {
            c.lo[k] = std::min(c.lo[k], cell[k]);
            c.hi[k] = std::max(c.hi[k], cell[k]);
        }
    }
    std::vector<uint32_t> order(comps.size());
    for (uint32_t k = 0; k < order.size(); ++k) order[k] = k;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        return comps[x].pixels != comps[y].pixels ? comps[x].pixels > comps[y].pixels : roots[x] < roots[y];
    });
    std::vector<uint32_t> label_of(comps.size());
    for (uint32_t k = 0; k < order.size(); ++k) {
        label_of[order[k]] = k;
        if (k >= cap) continue;
        const Component& c = comps[order[k]];
        sar_basin_attractor& o = attractors_out_host[k];
        o.root = roots[order[k]];
        o.pixels = c.pixels;
        o.cells = c.cells;
        o.first_pixel = c.first_pixel;
        for (int j = 0; j < 3; ++j) {
            o.cell_lo[j] = c.lo[j];
            o.cell_hi[j] = c.hi[j];
        }
    }
    st.attractors = comps.size();
    // the probes' table: every visited cell's label (the device gets it with the first probe call)
    rt->basin.h_node_label.assign(nodes, kBasinEmpty);
    for (uint32_t v = 0; v < nodes; ++v)
        if (node_root[v] != kBasinEmpty) rt->basin.h_node_label[v] = label_of[slot_of[node_root[v]]];
    std::vector<uint32_t> labels(npix, kBasinEmpty);
    for (uint32_t i = 0; i < npix; ++i) {
        sar_basin_pixel& r = pixels_out_host[i];
        if (r.status == SAR_SEARCH_BOUNDED) labels[i] = r.label = label_of[slot_of[r.root]];
    }
    for (int k = 0; k < 6; ++k) {
        const unsigned long long bits = corr_unsortable(ext[k]);
        std::memcpy(&st.extent[k], &bits, sizeof(bits));
    }
    if (!st.bounded)
        for (int k = 0; k < 3; ++k) {
            st.extent[2 * k] = HUGE_VAL;
            st.extent[2 * k + 1] = -HUGE_VAL;
        }
    // the labels go back for the colorize
    HIP_TRY(hipMemcpyAsync(rt->basin.d_label, labels.data(), static_cast<size_t>(npix) * sizeof(uint32_t), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    rt->basin.width = width;
    rt->basin.height = height;
    rt->basin.attractors = static_cast<uint32_t>(comps.size());
    rt->basin.held_map = a.map;
    for (int k = 0; k < 3; ++k) {
        rt->basin.held_box_lo[k] = a.box_lo[k];
        rt->basin.held_scale[k] = a.scale[k];
    }
    rt->basin.held_bound = a.bound;
    rt->basin.held_transient = a.transient;
    rt->basin.held_steps = a.steps;
    rt->basin.held_grid = G;
    rt->basin.label_uploaded = false;
    rt->basin.held = true;
    if (n_out) *n_out = static_cast<uint32_t>(comps.size());
    if (stats_out) *stats_out = st;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_basin_colors_default(sar_basin_colors* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->fade = 32.;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_basin_colorize(const sar_config* cfg, sar_runtime* rt, const sar_basin_colors* colors, uint16_t* rgba16_out_host) try {
    if (!cfg || !rt || !rgba16_out_host) return SAR_ERR_INVALID;
    const sar_basin_colors c = given_or_default(colors, sar_basin_colors_default);
    if (!(c.fade > 0.) || !std::isfinite(c.fade)) {
        set_error("sar_runtime_basin_colorize: fade must be positive and finite");
        return SAR_ERR_INVALID;
    }
    return colorize_tail("sar_runtime_basin_colorize", "basin picture", "sar_runtime_basin", cfg, rt, rt->basin.width, rt->basin.height,
                         rt->basin.d_rgba, rgba16_out_host, [&](uint32_t npix, uint16_t* rgba) {
                             launch_basin_colorize(rt->basin.d_pix, rt->basin.d_label, npix, palette_params(cfg), rt->basin.attractors, c.fade, rgba,
                                                   rt->stream);
                         });
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
