// sar_gallery.cpp — the host half of the gallery (include/sar.h: sar_gallery_*, sar_runtime_gallery, sar_frame_view_box): the
// checks, every tile's argument block, the chunked launches of k_gallery (sar_gallery.hip) and the read-back of the atlas, the raw
// tiles and the statistics.
//
// Built with -ffp-contract=off like the rest: sar_frame_view_box applies the rotation as the kernels do (Matrix3x3::mul_right).
#include <cmath>
#include <cstring>
#include <vector>

#include "sar_analysis.hpp"
#include "sar_gallery.hpp"

using namespace sar;

namespace {

int check_gallery(const sar_config* base, const sar_gallery_params* p) {
    if (!p) { set_error("sar_runtime_gallery: the parameters are NULL"); return SAR_ERR_INVALID; }
    if (!p->tile_width || !p->tile_height) {
        set_error("sar_runtime_gallery: a tile side is 0 (%u x %u)", p->tile_width, p->tile_height);
        return SAR_ERR_INVALID;
    }
    if (static_cast<uint64_t>(p->tile_width) * p->tile_height > kMaxGalleryTilePixels) {
        set_error("sar_runtime_gallery: a tile holds at most %u pixels (%u x %u)", kMaxGalleryTilePixels, p->tile_width, p->tile_height);
        return SAR_ERR_INVALID;
    }
    if (!p->cols) { set_error("sar_runtime_gallery: cols is 0"); return SAR_ERR_INVALID; }
    if (!p->jobs) { set_error("sar_runtime_gallery: jobs is 0"); return SAR_ERR_INVALID; }
    const uint64_t per_job = p->iterations / p->jobs;  // :1058
    // (per_job >= 2^32 alone is too many: the product below cannot overflow once it is not)
    if (per_job >= (1ull << 32) || static_cast<uint64_t>(p->jobs) * per_job >= (1ull << 32)) {
        set_error("sar_runtime_gallery: jobs * (iterations / jobs) must stay below 2^32, the visit ordinal is 32 bits (%u jobs, %llu iterations)",
                  p->jobs, static_cast<unsigned long long>(p->iterations));
        return SAR_ERR_INVALID;
    }
    if (!base) { set_error("sar_runtime_gallery: base is NULL"); return SAR_ERR_INVALID; }
    sar_config c = *base;  // what every cfg_i shares with base, at the tile's size
    c.width = p->tile_width;
    c.height = p->tile_height;
    if (validate(&c) != SAR_OK) return SAR_ERR_INVALID;  // (validate left the text)
    return SAR_OK;
}

}  // namespace

extern "C" {

int sar_gallery_params_default(sar_gallery_params* out) try {
    if (!out) return SAR_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    out->tile_width = out->tile_height = 128;
    out->cols = 8;
    out->jobs = 1024;
    out->iterations = 1ull << 20;
    out->seed = 0;
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_runtime_gallery(sar_runtime* rt, const sar_config* base, const sar_gallery_params* p, uint32_t n, const sar_gallery_item* items_host,
                        const double* starts_xyz_host, uint16_t* atlas_rgba16_out_host, uint32_t* count_out_host, float* zbuf_out_host,
                        double* steps_out_host, sar_gallery_stats* stats_out_host) try {
    SAR_TRY(check_gallery(base, p));  // (no device needed to refuse the parameters)
    if (n && !items_host) { set_error("sar_runtime_gallery: items_host is NULL"); return SAR_ERR_INVALID; }
    if (n == 0) return SAR_OK;
    if (!rt || !atlas_rgba16_out_host) { set_error("sar_runtime_gallery: the runtime or the atlas is NULL"); return SAR_ERR_INVALID; }
    const uint32_t npix = p->tile_width * p->tile_height, jobs = p->jobs;
    const uint32_t rows = (n - 1u) / p->cols + 1u;
    const uint64_t atlas_width = static_cast<uint64_t>(p->cols) * p->tile_width, atlas_px = atlas_width * rows * p->tile_height;
    if (atlas_width > 0xFFFFFFFFull) { set_error("sar_runtime_gallery: the atlas is wider than 2^32-1 pixels"); return SAR_ERR_RANGE; }
    SAR_TRY(analysis_begin(rt));  // with timing on: iterate_ms = k_gallery (sar_timing)

    // cfg_i = *base with item i's map and view at the tile's size: its hoisted constants, as sar_render_jobs would form them
    std::vector<GalleryTile> tiles(n);
    sar_config c = *base;
    c.width = p->tile_width;
    c.height = p->tile_height;
    c.iterations = p->iterations;
    c.jobs_total = jobs;
    for (uint32_t i = 0; i < n; ++i) {
        const sar_gallery_item& it = items_host[i];
        for (int k = 0; k < 10; ++k) {
            c.coeff_x[k] = it.coeff[k];
            c.coeff_y[k] = it.coeff[10 + k];
            c.coeff_z[k] = it.coeff[20 + k];
        }
        for (int k = 0; k < 3; ++k) c.center_camera[k] = it.center_camera[k];
        c.scale = it.scale;
        fill_map_params(c, tiles[i].p);
        fill_ct_params(c, tiles[i].ct);
    }
    std::vector<double> drawn;
    SAR_TRY(starts_or_drawn(starts_xyz_host, p->seed, jobs, drawn));

    uint32_t chunk = rt->opt.gallery_chunk ? rt->opt.gallery_chunk : kDefaultGalleryChunk;
    if (chunk > n) chunk = n;
    HIP_TRY(rt->gallery.d_tiles.grow(nullptr, n));
    HIP_TRY(rt->gallery.d_stats.grow(nullptr, n));
    HIP_TRY(rt->gallery.d_starts.grow(nullptr, static_cast<size_t>(jobs) * 3));
    HIP_TRY(rt->gallery.d_warm.grow(nullptr, static_cast<size_t>(chunk) * jobs * 3));
    HIP_TRY(rt->gallery.d_count.grow(nullptr, static_cast<size_t>(chunk) * npix));
    HIP_TRY(rt->gallery.d_zbuf.grow(nullptr, static_cast<size_t>(chunk) * npix));
    HIP_TRY(rt->gallery.d_steps.grow(nullptr, static_cast<size_t>(chunk) * npix));
    HIP_TRY(rt->gallery.d_atlas.grow(nullptr, atlas_px * 4));
    HIP_TRY(hipMemcpyAsync(rt->gallery.d_tiles, tiles.data(), static_cast<size_t>(n) * sizeof(GalleryTile), hipMemcpyHostToDevice, rt->stream));
    HIP_TRY(hipMemcpyAsync(rt->gallery.d_starts, starts_xyz_host, static_cast<size_t>(jobs) * 3 * sizeof(double), hipMemcpyHostToDevice, rt->stream));
    if (n % p->cols) {  // the cells of the last row that hold no tile: that row of tiles is one contiguous piece of the atlas
        const size_t row_px = static_cast<size_t>(atlas_width) * p->tile_height;
        HIP_TRY(hipMemsetAsync(rt->gallery.d_atlas + (rows - 1u) * row_px * 4, 0, row_px * 8, rt->stream));
    }

    GalleryArgs a;
    std::memset(&a, 0, sizeof(a));
    a.tiles = rt->gallery.d_tiles;
    a.starts = rt->gallery.d_starts;
    a.warm = rt->gallery.d_warm;
    a.count = rt->gallery.d_count;
    a.zbuf = rt->gallery.d_zbuf;
    a.steps = rt->gallery.d_steps;
    a.atlas = rt->gallery.d_atlas;
    a.stats = rt->gallery.d_stats;
    a.lut = rt->d_lnlut;
    a.lut_len = kLnLutEntries;
    a.tile_width = p->tile_width;
    a.tile_height = p->tile_height;
    a.npix = npix;
    a.cols = p->cols;
    a.atlas_width = static_cast<uint32_t>(atlas_width);
    a.jobs = jobs;
    a.iters = static_cast<uint32_t>(p->iterations / jobs);
    a.render_kind = base->render_kind;
    a.transparent = base->transparent;
    a.b_offset = base->brightness_offset;
    a.b_factor = base->brightness_factor;
    a.pal = palette_params(base);
    for (uint32_t first = 0; first < n; first += chunk) {
        const uint32_t m = n - first < chunk ? n - first : chunk;
        a.first_tile = first;
        SAR_TRY(timed_lds_launch(rt, rt->tm.iter, [&] { return launch_gallery(a, m, rt->stream); }));
        // the launch's raw tiles, before the next launch writes the scratch again (stream order)
        const size_t at = static_cast<size_t>(first) * npix, cnt = static_cast<size_t>(m) * npix;
        if (count_out_host) HIP_TRY(hipMemcpyAsync(count_out_host + at, rt->gallery.d_count, cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, rt->stream));
        if (zbuf_out_host) HIP_TRY(hipMemcpyAsync(zbuf_out_host + at, rt->gallery.d_zbuf, cnt * sizeof(float), hipMemcpyDeviceToHost, rt->stream));
        if (steps_out_host) HIP_TRY(hipMemcpyAsync(steps_out_host + at, rt->gallery.d_steps, cnt * sizeof(double), hipMemcpyDeviceToHost, rt->stream));
    }
    rt->tm.last_iterations += static_cast<uint64_t>(n) * jobs * a.iters;
    HIP_TRY(hipMemcpyAsync(atlas_rgba16_out_host, rt->gallery.d_atlas, atlas_px * 8, hipMemcpyDeviceToHost, rt->stream));
    if (stats_out_host)
        HIP_TRY(hipMemcpyAsync(stats_out_host, rt->gallery.d_stats, static_cast<size_t>(n) * sizeof(sar_gallery_stats), hipMemcpyDeviceToHost, rt->stream));
    HIP_TRY(hipStreamSynchronize(rt->stream));
    return SAR_OK;
} catch (...) { return sar::abi_caught(); }

int sar_frame_view_box(sar_config* cfg, const double raw_extent6[6], double margin, int sweep) try {
    if (!cfg || !raw_extent6) return SAR_ERR_INVALID;
    for (int k = 0; k < 6; ++k)
        if (!std::isfinite(raw_extent6[k])) {
            set_error("sar_frame_view_box: extent[%d] is not finite (a trajectory diverged?)", k);
            return SAR_ERR_INVALID;
        }
    double m[9];
    rotation_matrix(*cfg, m);
    double ext[6] = {HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL, HUGE_VAL, -HUGE_VAL};
    for (int corner = 0; corner < 8; ++corner) {
        const double x = raw_extent6[corner & 1], y = raw_extent6[2 + ((corner >> 1) & 1)], z = raw_extent6[4 + ((corner >> 2) & 1)];
        // Matrix3x3::mul_right (src/lib.rs:205-216), as sar_runtime_extent's kernel forms its screen-space points
        const double s[3] = {m[0] * x + m[1] * y + m[2] * z, m[3] * x + m[4] * y + m[5] * z, m[6] * x + m[7] * y + m[8] * z};
        for (int k = 0; k < 3; ++k) {
            if (s[k] < ext[2 * k]) ext[2 * k] = s[k];
            if (s[k] > ext[2 * k + 1]) ext[2 * k + 1] = s[k];
        }
    }
    return sar_frame_view(cfg, ext, margin, sweep);
} catch (...) { return sar::abi_caught(); }

}  // extern "C"
