// sar.hpp — header-only C++17 mirror of the reference crate's surface over the C ABI (sar.h).
//
// Names follow Icelk/strange-attractor-renderer (src/lib.rs): Config (:265), Runtime (:631), render (:747),
// colorize (:841), ParallelRenderer (:908), render_parallel (:1051). Errors become exceptions here (the
// reference panics); nothing throws across the C boundary itself.
#pragma once

#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "sar.h"

namespace sar {

struct Error : std::runtime_error {
    int status;
    Error(int s, const char* where)
        : std::runtime_error(std::string(where) + ": " + sar_status_string(s) + " — " + sar_last_error()), status(s) {}
};
inline void check(int status, const char* where) {
    if (status != SAR_OK) throw Error(status, where);
}

enum class RenderKind : int32_t { Gas = SAR_RENDER_GAS, Depth = SAR_RENDER_DEPTH };  // :233-239

// 16-bit RGBA image, row-major (FinalImage, :625)
struct FinalImage {
    uint32_t width = 0, height = 0;
    std::vector<uint16_t> rgba;
};

struct Config : sar_config {
    static Config poisson_saturne() {  // :310
        Config c;
        check(sar_config_poisson_saturne(&c), "Config::poisson_saturne");
        return c;
    }
    static Config solar_sail() {  // :355
        Config c;
        check(sar_config_solar_sail(&c), "Config::solar_sail");
        return c;
    }
    void validate() const { check(sar_config_validate(this), "Config::validate"); }
};

class Runtime {  // :631
public:
    explicit Runtime(const Config& config, int device = 0) { check(sar_runtime_new(&config, device, &rt_), "Runtime::new"); }
    ~Runtime() { sar_runtime_free(rt_); }
    Runtime(const Runtime&) = delete;
    Runtime& operator=(const Runtime&) = delete;
    Runtime(Runtime&& o) noexcept : rt_(std::exchange(o.rt_, nullptr)) {}

    void reset() { check(sar_runtime_reset(rt_), "Runtime::reset"); }                      // :682
    void merge(const Runtime& other) { check(sar_runtime_merge(rt_, other.rt_), "Runtime::merge"); }  // :708
    void seed(uint64_t s) { check(sar_runtime_seed(rt_, s), "Runtime::seed"); }
    uint32_t max() { uint32_t m = 0; check(sar_runtime_max(rt_, &m), "Runtime::max"); return m; }
    std::vector<uint32_t> count() {
        uint32_t w = 0, h = 0;
        check(sar_runtime_dims(rt_, &w, &h), "Runtime::dims");
        std::vector<uint32_t> out(static_cast<size_t>(w) * h);
        check(sar_runtime_count(rt_, out.data()), "Runtime::count");
        return out;
    }
    sar_runtime* handle() const { return rt_; }

private:
    sar_runtime* rt_ = nullptr;
};

// render(&config, &mut runtime): one trajectory of config.iterations (:747)
inline void render(const Config& config, Runtime& runtime) { check(sar_render(&config, runtime.handle()), "render"); }
// config.jobs_total trajectories with the sequential semantics of calling render that many times
inline void render_jobs(const Config& config, Runtime& runtime, const double* starts_xyz = nullptr) {
    check(sar_render_jobs(&config, runtime.handle(), starts_xyz), "render_jobs");
}
// F frames of a sweep (the CLI's frame loop, src/bin/main.rs:493-517) through ONE set of launches: frame i is
// render_jobs(configs[i], *runtimes[i], starts[i]) — bit for bit; the frames share the chip instead of following each other
inline void render_jobs_batch(const std::vector<const Config*>& configs, const std::vector<Runtime*>& runtimes,
                              const std::vector<const double*>& starts_xyz = {}) {
    if (configs.size() != runtimes.size() || (!starts_xyz.empty() && starts_xyz.size() != configs.size()))
        throw Error(SAR_ERR_INVALID, "render_jobs_batch: configs, runtimes and starts must have the same length");
    std::vector<const sar_config*> c(configs.begin(), configs.end());
    std::vector<sar_runtime*> r;
    for (Runtime* rt : runtimes) r.push_back(rt->handle());
    check(sar_render_jobs_batch(static_cast<uint32_t>(c.size()), c.data(), r.data(), starts_xyz.empty() ? nullptr : starts_xyz.data()),
          "render_jobs_batch");
}
// colorize(&config, &runtime) -> FinalImage (:841)
inline FinalImage colorize(const Config& config, Runtime& runtime) {
    FinalImage img;
    img.width = config.width;
    img.height = config.height;
    img.rgba.resize(static_cast<size_t>(config.width) * config.height * 4);
    check(sar_colorize(&config, runtime.handle(), img.rgba.data()), "colorize");
    return img;
}

// write_image_matches (src/bin/main.rs:40-100): colorize, convert by (transparent, 8bit) on the device, encode by
// (pam, bmp) — both need 8bit (:256-258) — and replace the extension of `name`. Returns the path written.
inline std::string write_image_matches(const Config& config, Runtime& runtime, const std::string& name, bool eight_bit = false,
                                       bool pam = false, bool bmp = false) {
    if ((pam || bmp) && !eight_bit) throw Error(SAR_ERR_INVALID, "write_image_matches: --pam/--bmp require --8bit");
    const int format = sar_image_format(config.transparent, eight_bit ? 1 : 0);
    std::vector<unsigned char> pixels(sar_image_bytes(format, config.width, config.height));
    check(sar_colorize_format(&config, runtime.handle(), format, pixels.data()), "colorize_format");
    const size_t dot = name.find_last_of('.'), slash = name.find_last_of('/');
    const std::string stem = (dot != std::string::npos && (slash == std::string::npos || dot > slash)) ? name.substr(0, dot) : name;
    const std::string path = stem + (pam ? ".pam" : (bmp ? ".bmp" : ".png"));
    check((pam ? sar_write_pam : (bmp ? sar_write_bmp : sar_write_png))(path.c_str(), format, config.width, config.height, pixels.data()),
          "write_image");
    return path;
}

// Sprott's search for chaotic maps (sar_runtime_search): candidates [first, first + n), generated from params.seed or the
// caller's coefficient sets (n x 30); the accepted records (all phase-2 records with keep_rejected) sorted by candidate.
struct SearchParams : sar_search_params {
    SearchParams() { check(sar_search_params_default(this), "SearchParams"); }
};
// At most `cap` records are returned (the first by candidate); `total` says how many there were.
struct SearchResult {
    std::vector<sar_search_record> records;
    uint32_t total = 0;
    sar_search_stats stats{};
};
inline SearchResult search_attractors(Runtime& runtime, const SearchParams& params, uint32_t n, uint64_t first = 0,
                                      const double* coeffs = nullptr, uint32_t cap = 65536) {
    SearchResult r;
    r.records.resize(n < cap ? n : cap);
    check(sar_runtime_search(runtime.handle(), &params, first, n, coeffs, r.records.data(), static_cast<uint32_t>(r.records.size()),
                             &r.total, &r.stats), "search_attractors");
    if (r.total < r.records.size()) r.records.resize(r.total);
    return r;
}
// candidate `index` of the stream `seed`: coeff_x, coeff_y, coeff_z
inline std::vector<double> search_candidate(uint64_t seed, uint64_t index, double lo = -1.2, double hi = 1.2) {
    std::vector<double> c(30);
    check(sar_search_candidate(seed, lo, hi, index, c.data()), "search_candidate");
    return c;
}
// config's view framed on the attractor: the screen-space extent, then center_camera and scale (sar_frame_view)
inline Config frame_view(const Config& config, Runtime& runtime, uint32_t n_jobs, uint64_t iters_per_job, double margin = 0.05,
                         bool sweep = false) {
    double ext[12];
    check(sar_runtime_extent(&config, runtime.handle(), n_jobs, iters_per_job, nullptr, ext), "frame_view: extent");
    Config out = config;
    check(sar_frame_view(&out, ext, margin, sweep ? 1 : 0), "frame_view");
    return out;
}

// Auto exposure: the levels stretch of the Gas tone curve from two quantiles of the covered counts (include/sar.h)
struct ExposureParams : sar_exposure_params {
    ExposureParams() { check(sar_exposure_params_default(this), "ExposureParams"); }
};
// the exposure of the runtime's current frame (waits for it)
inline sar_exposure exposure(const Config& config, Runtime& runtime, const ExposureParams& params = ExposureParams()) {
    sar_exposure e{};
    check(sar_runtime_exposure(&config, runtime.handle(), &params, &e), "exposure");
    return e;
}
// config with the brightness constants of that exposure: hold it over a sweep
inline Config auto_exposure(const Config& config, Runtime& runtime, const ExposureParams& params = ExposureParams()) {
    const sar_exposure e = exposure(config, runtime, params);
    Config out = config;
    out.brightness_offset = e.offset;
    out.brightness_factor = e.factor;
    return out;
}
// the mode: every whole-image Gas colorize of the runtime exposes its frame on its own; nullptr turns it off
inline void set_exposure(Runtime& runtime, const ExposureParams* params) {
    check(sar_runtime_set_exposure(runtime.handle(), params), "set_exposure");
}

// Auto colour range: the palette window of a Gas frame from two quantiles of the covered steps (include/sar.h)
struct ColorRangeParams : sar_color_range_params {
    ColorRangeParams() { check(sar_color_range_params_default(this), "ColorRangeParams"); }
};
// the colour range of the runtime's current frame (waits for it)
inline sar_color_range color_range(const Config& config, Runtime& runtime, const ColorRangeParams& params = ColorRangeParams()) {
    sar_color_range c{};
    check(sar_runtime_color_range(&config, runtime.handle(), &params, &c), "color_range");
    return c;
}
// config whose AdjustedVelocity constants carry that window in its steps
inline Config auto_color(const Config& config, Runtime& runtime, const ColorRangeParams& params = ColorRangeParams()) {
    const sar_color_range c = color_range(config, runtime, params);
    Config out = config;
    check(sar_color_range_to_velocity(&config, &c, &out), "auto_color");
    return out;
}
// the mode: every whole-image Gas colorize of the runtime picks its own window; nullptr turns it off
inline void set_color_range(Runtime& runtime, const ColorRangeParams* params) {
    check(sar_runtime_set_color_range(runtime.handle(), params), "set_color_range");
}
// the hold: one window for every whole-image Gas colorize of the runtime; nullptr turns it off
inline void hold_color_range(Runtime& runtime, const sar_color_range* range) {
    check(sar_runtime_hold_color_range(runtime.handle(), range), "hold_color_range");
}

// Orbit diagrams: where a line of maps settles, column by column (include/sar.h: sar_runtime_orbit)
struct OrbitParams : sar_orbit_params {
    OrbitParams() { check(sar_orbit_params_default(this), "OrbitParams"); }
};
struct OrbitDiagram {
    uint32_t width = 0, height = 0, max = 0;
    std::vector<uint32_t> count;           // [height][width], row 0 at the high end of the plotted range
    std::vector<sar_orbit_column> stats;   // [width]
};
// starts: jobs * 3 doubles, or nullptr for the stream of params.seed
inline OrbitDiagram orbit_diagram(Runtime& runtime, const OrbitParams& params, const double* starts = nullptr) {
    OrbitDiagram d;
    d.width = params.width;
    d.height = params.height;
    d.count.resize(static_cast<size_t>(params.width) * params.height);
    d.stats.resize(params.width);
    check(sar_runtime_orbit(runtime.handle(), &params, starts, d.count.data(), d.stats.data(), &d.max), "orbit_diagram");
    return d;
}
// column `column`'s map: coeff_x, coeff_y, coeff_z
inline std::vector<double> orbit_coeffs(const OrbitParams& params, uint32_t column) {
    std::vector<double> c(30);
    check(sar_orbit_coeffs(&params, column, c.data()), "orbit_coeffs");
    return c;
}

// Cycles: fixed points and periodic orbits of maps with M = D F^q, by Newton's method on the GPU (include/sar.h: sar_runtime_cycles)
struct CyclesParams : sar_cycles_params {
    CyclesParams() { check(sar_cycles_params_default(this), "CyclesParams"); }
};
struct Cycles {
    uint32_t n_maps = 0, cap = 0;
    std::vector<sar_cycles_record> records;   // [n_maps]
    std::vector<sar_cycle_orbit> orbits;      // [n_maps][cap]; map m's first records[m].n_orbits are in use
};
// coeffs: n_maps * 30 doubles; starts: params.jobs * 3 doubles, or nullptr for the lattice of params.grid^3 points over the box
inline Cycles cycles(Runtime& runtime, const CyclesParams& params, uint32_t n_maps, const double* coeffs, const double* starts = nullptr) {
    Cycles c;
    c.n_maps = n_maps;
    c.cap = params.cap;
    c.records.resize(n_maps);
    c.orbits.resize(static_cast<size_t>(n_maps) * params.cap);
    check(sar_runtime_cycles(runtime.handle(), &params, n_maps, coeffs, starts, c.records.data(), c.orbits.data()), "cycles");
    return c;
}
// the lattice's starts, grid^3 * 3 doubles
inline std::vector<double> cycles_starts(const CyclesParams& params) {
    std::vector<double> s(static_cast<size_t>(params.grid) * params.grid * params.grid * 3);
    check(sar_cycles_starts(&params, s.data()), "cycles_starts");
    return s;
}
// trace, sum of the principal 2 x 2 minors and determinant of an orbit's M: the coefficients its multipliers are the roots of
inline std::array<double, 3> cycle_charpoly(const double M[9]) {
    std::array<double, 3> c{};
    check(sar_cycle_charpoly(M, c.data()), "cycle_charpoly");
    return c;
}

// Unstable manifolds: the W^u of saddle cycles drawn as connected curves into a view (include/sar.h: sar_runtime_manifold)
struct ManifoldParams : sar_manifold_params {
    ManifoldParams() { check(sar_manifold_params_default(this), "ManifoldParams"); }
};
struct Manifolds {
    uint32_t width = 0, height = 0;
    std::vector<uint32_t> count, first;          // [height][width]; first: step * 4096 + branch, 0xFFFFFFFF where nothing was plotted
    std::vector<sar_manifold_record> records;    // [branches]
};
// cfg: the map, the view and the image's size (not necessarily the runtime's)
inline Manifolds manifolds(Runtime& runtime, const sar_config& cfg, const ManifoldParams& params, const std::vector<sar_manifold_branch>& branches) {
    Manifolds m;
    m.width = cfg.width;
    m.height = cfg.height;
    m.count.resize(static_cast<size_t>(cfg.width) * cfg.height);
    m.first.resize(m.count.size(), 0xFFFFFFFFu);
    m.records.resize(branches.size());
    check(sar_runtime_manifold(runtime.handle(), &cfg, &params, static_cast<uint32_t>(branches.size()), branches.data(), m.count.data(),
                               m.first.data(), m.records.data()), "manifolds");
    return m;
}
// fi, fj of a point in cfg's view: inside the image, (floor(fi), floor(fj)) is the pixel render gives it
inline std::array<double, 2> manifold_pixel(const sar_config& cfg, const double xyz[3]) {
    std::array<double, 2> f{};
    check(sar_manifold_pixel(&cfg, xyz, f.data()), "manifold_pixel");
    return f;
}

// Flows: the 30 coefficients as the vector field p' = P(p), RK4 with a fixed step, plotted into the runtime's frame (include/sar.h:
// sar_runtime_render_flow)
struct FlowParams : sar_flow_params {
    FlowParams() { check(sar_flow_params_default(this), "FlowParams"); }
};
// one RK4 step on the host, in place; returns whether the new point stayed within params.bound
inline bool flow_step(const sar_config& cfg, const FlowParams& params, std::array<double, 3>& xyz) {
    int32_t within = 0;
    check(sar_flow_step(&cfg, &params, xyz.data(), &within), "flow_step");
    return within != 0;
}
// starts: [jobs][3]; accumulates onto the runtime's frame
inline sar_flow_stats render_flow(const sar_config& cfg, Runtime& runtime, const FlowParams& params, const std::vector<double>& starts,
                                  uint64_t steps_per_job) {
    sar_flow_stats st{};
    check(sar_runtime_render_flow(&cfg, runtime.handle(), &params, static_cast<uint32_t>(starts.size() / 3), steps_per_job, starts.data(), &st),
          "render_flow");
    return st;
}

// Poincare sections of flows: the crossings of the trajectories with a quadric surface, refined by Henon's step, with their return
// times (include/sar.h: sar_runtime_section). The surface is the caller's to set: SectionParams().surface is all zero.
struct SectionParams : sar_section_params {
    SectionParams() { check(sar_section_params_default(this), "SectionParams"); }
};
// one counted step on the host: xyz p0 in, p1 out; the kind (0 none, 1 Henon, 2 rough, -1 escaped), on 1 and 2 the crossing and dt
inline int32_t section_step(const sar_config& cfg, const SectionParams& params, std::array<double, 3>& xyz, std::array<double, 3>& crossing,
                            double& dt) {
    int32_t kind = 0;
    check(sar_section_step(&cfg, &params, xyz.data(), crossing.data(), &dt, &kind), "section_step");
    return kind;
}
struct Section {
    std::vector<double> points;   // [jobs][samples][3], NaN where unfilled
    std::vector<double> ret;      // [jobs][samples]
    std::vector<sar_section_record> records;
    sar_section_stats stats{};
};
// starts: [jobs][3]; with params.plot = 1 the crossings accumulate onto the runtime's frame
inline Section section(const sar_config& cfg, Runtime& runtime, const SectionParams& params, const std::vector<double>& starts) {
    const size_t jobs = starts.size() / 3;
    Section s;
    s.points.resize(jobs * params.samples * 3);
    s.ret.resize(jobs * params.samples);
    s.records.resize(jobs);
    check(sar_runtime_section(&cfg, runtime.handle(), &params, static_cast<uint32_t>(jobs), starts.data(), s.points.data(), s.ret.data(),
                              s.records.data(), &s.stats),
          "section");
    return s;
}

// Volume rendering: the hit histogram resolved along the view ray, held by the runtime (include/sar.h: sar_runtime_volume*)
struct VolumeParams : sar_volume_params {
    VolumeParams() { check(sar_volume_params_default(this), "VolumeParams"); }
};
struct VolumeMarchParams : sar_volume_march_params {
    VolumeMarchParams() { check(sar_volume_march_params_default(this), "VolumeMarchParams"); }
};
// starts: [jobs][3]; the volume stays with the runtime for volume_section / volume_march
inline sar_volume_stats volume(const sar_config& cfg, Runtime& runtime, const VolumeParams& params, const std::vector<double>& starts,
                               uint64_t iters_per_job) {
    sar_volume_stats st{};
    check(sar_runtime_volume(&cfg, runtime.handle(), &params, static_cast<uint32_t>(starts.size() / 3), iters_per_job, starts.data(), &st), "volume");
    return st;
}
struct VolumeSection {
    std::vector<uint32_t> count;     // [height][width]: the sum of the slabs k0 <= k < k1
    std::vector<int32_t> nearest;    // [height][width]: the largest non-empty k of them, or -1
};
inline VolumeSection volume_section(Runtime& runtime, uint32_t k0, uint32_t k1) {
    uint32_t w = 0, h = 0;
    check(sar_runtime_dims(runtime.handle(), &w, &h), "volume_section");
    VolumeSection s;
    s.count.resize(static_cast<size_t>(w) * h);
    s.nearest.resize(s.count.size());
    check(sar_runtime_volume_section(runtime.handle(), k0, k1, s.count.data(), s.nearest.data()), "volume_section");
    return s;
}
// RGBA16, [height][width][4]
inline std::vector<uint16_t> volume_march(const sar_config& cfg, Runtime& runtime, const VolumeMarchParams& params,
                                          sar_volume_march_stats* stats = nullptr) {
    std::vector<uint16_t> rgba(static_cast<size_t>(cfg.width) * cfg.height * 4);
    check(sar_runtime_volume_march(&cfg, runtime.handle(), &params, stats, rgba.data()), "volume_march");
    return rgba;
}

// Correlation dimension: exact pair-distance histograms of point sets and of maps (include/sar.h: sar_runtime_pairs, sar_runtime_corrdim)
struct PairsParams : sar_pairs_params {
    PairsParams() { check(sar_pairs_params_default(this), "PairsParams"); }
};
struct CorrdimParams : sar_corrdim_params {
    CorrdimParams() { check(sar_corrdim_params_default(this), "CorrdimParams"); }
};
// r_b, the upper edge of every bin (the overflow bin's is +inf)
inline std::vector<double> pair_edges(const sar_pairs_params& binning) {
    uint32_t bins = 0;
    check(sar_pairs_edges(&binning, &bins, nullptr), "pair_edges");
    std::vector<double> r(bins);
    check(sar_pairs_edges(&binning, nullptr, r.data()), "pair_edges");
    return r;
}
// points: [n_sets][n][3]; returns hist[n_sets][bins]; counts ([n_sets]) may be nullptr
inline std::vector<uint64_t> pair_histogram(Runtime& runtime, const PairsParams& params, uint32_t n_sets, uint32_t n, const double* points,
                                            sar_pairs_counts* counts = nullptr) {
    std::vector<uint64_t> hist(static_cast<size_t>(n_sets) * pair_edges(params).size());
    check(sar_runtime_pairs(runtime.handle(), &params, n_sets, n, points, hist.data(), counts), "pair_histogram");
    return hist;
}
struct CorrelationDimension {
    std::vector<uint64_t> hist;                // [n_maps][bins]
    std::vector<sar_corrdim_record> records;   // [n_maps]; records[k].line.slope is D2
};
// coeffs: [n_maps][30]; starts: jobs * 3 doubles, or nullptr for the stream of params.seed
inline CorrelationDimension correlation_dimension(Runtime& runtime, const CorrdimParams& params, uint32_t n_maps, const double* coeffs,
                                                  const double* starts = nullptr) {
    PairsParams binning;
    binning.sub_bits = params.sub_bits;
    binning.e_min = params.e_min;
    binning.e_max = params.e_max;
    CorrelationDimension d;
    d.hist.resize(static_cast<size_t>(n_maps) * pair_edges(binning).size());
    d.records.resize(n_maps);
    check(sar_runtime_corrdim(runtime.handle(), &params, n_maps, coeffs, starts, d.hist.data(), d.records.data(), nullptr), "correlation_dimension");
    return d;
}
inline sar_corrdim_line corrdim_fit(const uint64_t* hist, const sar_pairs_params& binning, double c_lo, double r_hi) {
    sar_corrdim_line line;
    check(sar_corrdim_fit(hist, &binning, c_lo, r_hi, &line), "corrdim_fit");
    return line;
}

// Basins of attraction: the fate and the attractor of every start point of a plane (include/sar.h: sar_runtime_basin)
struct BasinParams : sar_basin_params {
    BasinParams() { check(sar_basin_params_default(this), "BasinParams"); }
};
struct BasinColors : sar_basin_colors {
    BasinColors() { check(sar_basin_colors_default(this), "BasinColors"); }
};
struct BasinMap {
    uint32_t width = 0, height = 0;
    uint32_t n_attractors = 0;                   // all of them; `attractors` holds the first `cap`
    std::vector<sar_basin_pixel> pixels;         // [height][width], row 0 at the high end of dv
    std::vector<sar_basin_attractor> attractors; // sorted by basin size
    sar_basin_stats stats{};
};
inline BasinMap basin_map(Runtime& runtime, const BasinParams& params, uint32_t cap = 64) {
    BasinMap b;
    b.width = params.width;
    b.height = params.height;
    b.pixels.resize(static_cast<size_t>(params.width) * params.height);
    b.attractors.resize(cap);
    check(sar_runtime_basin(runtime.handle(), &params, b.pixels.data(), cap ? b.attractors.data() : nullptr, cap, &b.n_attractors, &b.stats),
          "basin_map");
    b.attractors.resize(b.n_attractors < cap ? b.n_attractors : cap);
    return b;
}
// pixel (x, y)'s start point
inline std::vector<double> basin_start(const BasinParams& params, uint32_t x, uint32_t y) {
    std::vector<double> p(3);
    check(sar_basin_start(&params, x, y, p.data()), "basin_start");
    return p;
}
// RGBA16 of the runtime's last basin picture
inline FinalImage basin_colorize(const Config& config, Runtime& runtime, const BasinMap& basin, const BasinColors& colors = BasinColors()) {
    FinalImage img;
    img.width = basin.width;
    img.height = basin.height;
    img.rgba.resize(static_cast<size_t>(basin.width) * basin.height * 4);
    check(sar_runtime_basin_colorize(&config, runtime.handle(), &colors, img.rgba.data()), "basin_colorize");
    return img;
}
// Basin probes: the fates of any start points in the runtime's held basin picture, and the uncertainty ladder of its boundary
// (include/sar.h: sar_runtime_basin_fates, sar_runtime_basin_uncertainty)
struct BasinLadderParams : sar_basin_ladder_params {
    BasinLadderParams() { check(sar_basin_ladder_params_default(this), "BasinLadderParams"); }
};
// points: [n][3]
inline std::vector<sar_basin_fate> basin_fates(Runtime& runtime, const std::vector<double>& points, sar_basin_fate_counts* counts = nullptr) {
    std::vector<sar_basin_fate> fates(points.size() / 3);
    check(sar_runtime_basin_fates(runtime.handle(), static_cast<uint32_t>(fates.size()), points.data(), fates.data(), counts), "basin_fates");
    return fates;
}
struct BasinUncertainty {
    std::vector<sar_basin_uncertainty_level> levels;  // [params.levels]
    std::vector<sar_basin_fate> fate0;                // [n]: the base points' own fates
    std::vector<sar_basin_ladder_mask> masks;         // [n]
};
// base: [n][3]
inline BasinUncertainty basin_uncertainty(Runtime& runtime, const std::vector<double>& base, const BasinLadderParams& params = BasinLadderParams()) {
    BasinUncertainty u;
    const size_t n = base.size() / 3;
    u.levels.resize(params.levels);
    u.fate0.resize(n);
    u.masks.resize(n);
    check(sar_runtime_basin_uncertainty(runtime.handle(), &params, static_cast<uint32_t>(n), base.data(), u.levels.data(), u.fate0.data(),
                                        u.masks.data()), "basin_uncertainty");
    return u;
}

// Power spectra: Welch periodograms of point sets and of maps' orbits (include/sar.h: sar_runtime_spectra, sar_runtime_spectrum)
struct SpectraParams : sar_spectra_params {
    SpectraParams() { check(sar_spectra_params_default(this), "SpectraParams"); }
};
struct SpectrumParams : sar_spectrum_params {
    SpectrumParams() { check(sar_spectrum_params_default(this), "SpectrumParams"); }
};
// points: [n_sets][n_points][3]; returns power[n_sets][n / 2 + 1], raw sums; records ([n_sets]) may be nullptr
inline std::vector<double> power_spectra(Runtime& runtime, const SpectraParams& params, uint32_t n_sets, uint32_t n_points, const double* points,
                                         sar_spectra_record* records = nullptr) {
    std::vector<double> power(static_cast<size_t>(n_sets) * (params.n / 2 + 1));
    check(sar_runtime_spectra(runtime.handle(), &params, n_sets, n_points, points, power.data(), records), "power_spectra");
    return power;
}
struct Spectrum {
    std::vector<double> power;                   // [n_maps][n / 2 + 1]; bin k is k / (n * stride) cycles per step
    std::vector<sar_spectrum_record> records;    // [n_maps]
};
// coeffs: [n_maps][30]; starts: jobs * 3 doubles, or nullptr for the stream of params.seed
inline Spectrum power_spectrum(Runtime& runtime, const SpectrumParams& params, uint32_t n_maps, const double* coeffs,
                               const double* starts = nullptr) {
    Spectrum s;
    s.power.resize(static_cast<size_t>(n_maps) * (params.n / 2 + 1));
    s.records.resize(n_maps);
    check(sar_runtime_spectrum(runtime.handle(), &params, n_maps, coeffs, starts, s.power.data(), s.records.data(), nullptr), "power_spectrum");
    return s;
}

// Recurrence analysis: exact line-length histograms of recurrence plots (include/sar.h: sar_runtime_recurrence, sar_runtime_rqa)
struct RecurrenceParams : sar_recurrence_params {
    RecurrenceParams() { check(sar_recurrence_params_default(this), "RecurrenceParams"); }
};
struct RqaParams : sar_rqa_params {
    RqaParams() { check(sar_rqa_params_default(this), "RqaParams"); }
};
struct RecurrenceLines {
    std::vector<uint64_t> diag, vert;                // [n_sets][line_bins + 1] each
    std::vector<sar_recurrence_record> records;      // [n_sets]
};
// points: [n_sets][n][3]; params.eps2 must be set
inline RecurrenceLines recurrence_lines(Runtime& runtime, const RecurrenceParams& params, uint32_t n_sets, uint32_t n, const double* points) {
    RecurrenceLines r;
    r.diag.resize(static_cast<size_t>(n_sets) * (params.line_bins + 1));
    r.vert.resize(r.diag.size());
    r.records.resize(n_sets);
    check(sar_runtime_recurrence(runtime.handle(), &params, n_sets, n, points, r.diag.data(), r.vert.data(), r.records.data()), "recurrence_lines");
    return r;
}
// points: [n][3]; returns [height][width] bytes, 1 where R(i0 + y, j0 + x)
inline std::vector<uint8_t> recurrence_plot(Runtime& runtime, const RecurrenceParams& params, uint32_t n, const double* points, uint32_t job,
                                            uint32_t i0, uint32_t j0, uint32_t height, uint32_t width) {
    std::vector<uint8_t> out(static_cast<size_t>(height) * width);
    check(sar_runtime_recurrence_plot(runtime.handle(), &params, n, points, job, i0, j0, height, width, out.data()), "recurrence_plot");
    return out;
}
struct Recurrence {
    std::vector<uint64_t> diag, vert;                // [n_maps][line_bins + 1] each
    std::vector<sar_rqa_record> records;             // [n_maps]
};
// coeffs: [n_maps][30]; starts: jobs * 3 doubles, or nullptr for the stream of params.seed
inline Recurrence recurrence_analysis(Runtime& runtime, const RqaParams& params, uint32_t n_maps, const double* coeffs,
                                      const double* starts = nullptr) {
    Recurrence r;
    r.diag.resize(static_cast<size_t>(n_maps) * (params.line_bins + 1));
    r.vert.resize(r.diag.size());
    r.records.resize(n_maps);
    check(sar_runtime_rqa(runtime.handle(), &params, n_maps, coeffs, starts, r.diag.data(), r.vert.data(), r.records.data(), nullptr),
          "recurrence_analysis");
    return r;
}
inline sar_rqa_measures_out rqa_measures(const uint64_t* diag, const uint64_t* vert, const sar_recurrence_record& record, uint32_t line_bins,
                                         uint32_t l_min = 2, uint32_t v_min = 2) {
    sar_rqa_measures_out out;
    check(sar_rqa_measures(diag, vert, &record, line_bins, l_min, v_min, &out), "rqa_measures");
    return out;
}

// FTLE maps: the finite-time stretching of the flow map over a plane of start points (include/sar.h: sar_runtime_ftle)
struct FtleParams : sar_ftle_params {
    FtleParams() { check(sar_ftle_params_default(this), "FtleParams"); }
};
struct FtleColors : sar_ftle_colors {
    FtleColors() { check(sar_ftle_colors_default(this), "FtleColors"); }
};
struct FtleMap {
    uint32_t width = 0, height = 0;
    std::vector<sar_ftle_pixel> pixels;          // [height][width], row 0 at the high end of dv
    sar_ftle_stats stats{};
};
inline FtleMap ftle_map(Runtime& runtime, const FtleParams& params) {
    FtleMap m;
    m.width = params.width;
    m.height = params.height;
    m.pixels.resize(static_cast<size_t>(params.width) * params.height);
    check(sar_runtime_ftle(runtime.handle(), &params, m.pixels.data(), &m.stats), "ftle_map");
    return m;
}
// pixel (x, y)'s start point
inline std::vector<double> ftle_start(const FtleParams& params, uint32_t x, uint32_t y) {
    std::vector<double> p(3);
    check(sar_ftle_start(&params, x, y, p.data()), "ftle_start");
    return p;
}
// RGBA16 of the runtime's last FTLE map; colors.lo / colors.hi are the palette's window of ftle
inline FinalImage ftle_colorize(const Config& config, Runtime& runtime, const FtleMap& map, const FtleColors& colors = FtleColors()) {
    FinalImage img;
    img.width = map.width;
    img.height = map.height;
    img.rgba.resize(static_cast<size_t>(map.width) * map.height * 4);
    check(sar_runtime_ftle_colorize(&config, runtime.handle(), &colors, img.rgba.data()), "ftle_colorize");
    return img;
}

class ParallelRenderer {  // :908
public:
    explicit ParallelRenderer(int device = 0, uint32_t units = 0, uint64_t seed = 0) {
        check(sar_renderer_new(device, units, seed, &r_), "ParallelRenderer::new");
    }
    // every GPU of the node behind one renderer (jobs sharded over the devices, partial buffers merged over xGMI)
    explicit ParallelRenderer(const std::vector<int>& devices, uint32_t units = 0, uint64_t seed = 0) {
        check(sar_renderer_new_multi(devices.data(), static_cast<uint32_t>(devices.size()), units, seed, &r_), "ParallelRenderer::new_multi");
    }
    uint32_t num_devices() const { uint32_t n = 0; check(sar_renderer_num_devices(r_, &n), "num_devices"); return n; }
    ~ParallelRenderer() { shutdown(); }
    ParallelRenderer(const ParallelRenderer&) = delete;
    ParallelRenderer& operator=(const ParallelRenderer&) = delete;
    uint32_t num_threads() const { uint32_t n = 0; check(sar_renderer_num_units(r_, &n), "num_threads"); return n; }
    void shutdown() { sar_renderer_shutdown(r_); r_ = nullptr; }  // :1020
    // auto exposure of render_parallel's colorize (one device only); nullptr turns it off
    void set_exposure(const ExposureParams* params) { check(sar_renderer_set_exposure(r_, params), "ParallelRenderer::set_exposure"); }
    // auto colour range of render_parallel's colorize (one device only); nullptr turns it off
    void set_color_range(const ColorRangeParams* params) { check(sar_renderer_set_color_range(r_, params), "ParallelRenderer::set_color_range"); }
    sar_renderer* handle() const { return r_; }

private:
    sar_renderer* r_ = nullptr;
};

// render_parallel(&mut renderer, config, jobs_per_thread) -> FinalImage (:1051)
inline FinalImage render_parallel(ParallelRenderer& renderer, const Config& config, uint32_t jobs_per_thread) {
    FinalImage img;
    img.width = config.width;
    img.height = config.height;
    img.rgba.resize(static_cast<size_t>(config.width) * config.height * 4);
    check(sar_render_parallel(renderer.handle(), &config, jobs_per_thread, img.rgba.data()), "render_parallel");
    return img;
}

}  // namespace sar
