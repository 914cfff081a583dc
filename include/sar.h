/*
 * sar.h — C ABI of the MI355X-native strange-attractor iterate/accumulate path.
 *
 * This is the drop-in boundary for ONE hot path of Icelk/strange-attractor-renderer:
 *   iterate the polynomial-Sprott map -> scatter-accumulate count / depth / colour index
 *   -> merge partial buffers -> tone-map (colorize).
 *
 * The reference has no FFI: its boundary is the Rust crate surface
 *   Config / View / Colors / RenderKind          (reference src/lib.rs:228-492)
 *   Runtime::{new, reset, merge}                 (src/lib.rs:631-739)
 *   render(&Config, &mut Runtime)                (src/lib.rs:747-838)
 *   colorize(&Config, &Runtime) -> FinalImage    (src/lib.rs:841-904)
 *   ParallelRenderer::{new, shutdown}            (src/lib.rs:908-1031)
 *   render_parallel(&mut ParallelRenderer, Config, jobs_per_thread) (src/lib.rs:1051-1082)
 * Each entry point below names the reference item it replaces. A Rust `extern "C"` block a
 * maintainer would add to bind these is shown in INTEGRATION.md.
 *
 * Conventions
 *   - every function returns an int status (SAR_OK == 0); nothing unwinds across this boundary
 *     (the reference panics instead: src/lib.rs:709-710, 990, 1024);
 *   - plain pointers and sizes only; no C++/torch types;
 *   - a sar_runtime is bound to one HIP device + one HIP stream and is NOT thread-safe
 *     (same contract as `&mut Runtime`);
 *   - pointers named *_host are host memory, *_dev are device memory on the runtime's device;
 *   - image buffers are row-major, index = y*width + x (image::ImageBuffer Luma layout,
 *     src/lib.rs:808).
 */
#ifndef SAR_H
#define SAR_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SAR_ABI_VERSION 12  /* 12 (additions only, no layout or meaning of an earlier item changed, so the number stays): sar_section_* / sar_runtime_section (Poincare sections of flows); 12 (likewise): sar_flow_* / sar_runtime_render_flow (flows); 12 (likewise): sar_volume_* / sar_runtime_volume* (volume rendering); 12 (likewise):sar_recurrence_* / sar_runtime_recurrence / sar_runtime_recurrence_plot / sar_rqa_* / sar_runtime_rqa (recurrence analysis); 12 (likewise): sar_spectra_* / sar_runtime_spectra / sar_spectrum_* / sar_runtime_spectrum (power spectra); 12 (likewise): sar_ftle_* / sar_runtime_ftle / sar_runtime_ftle_colorize (FTLE maps); 12 (likewise): sar_manifold_* / sar_runtime_manifold (unstable manifolds); 12 (likewise): sar_cycles_* / sar_cycle_charpoly / sar_runtime_cycles (cycles); 12 (likewise): sar_shade_* (shaded rendering); 12 (likewise): sar_density_* / sar_runtime_density / sar_runtime_density_tiles (density estimation); 12 (likewise): sar_box_* / sar_runtime_boxes / sar_boxdim_* / sar_runtime_boxdim and SAR_ERR_INTERNAL (box counting); 12 (likewise): sar_period_* / sar_runtime_period / sar_runtime_period_colorize (period planes); 12 (likewise): sar_basin_* / sar_runtime_basin / sar_runtime_basin_colorize (basins of attraction); 12 (likewise): sar_pairs_* / sar_runtime_pairs / sar_corrdim_* / sar_runtime_corrdim (correlation dimension); 12: sar_orbit_* / sar_runtime_orbit (orbit diagrams); 11: sar_gallery_* / sar_runtime_gallery / sar_frame_view_box (the gallery); 10: sar_color_range_* / sar_runtime_color_range / sar_runtime_set_color_range / sar_runtime_hold_color_range / sar_renderer_set_color_range (auto colour range); 9: sar_plane_* / sar_runtime_plane / sar_runtime_plane_colorize (Lyapunov planes); 8: sar_exposure_* / sar_runtime_exposure / sar_runtime_set_exposure / sar_renderer_set_exposure (auto exposure); 7: sar_search_* / sar_runtime_search / sar_frame_view (the chaotic-map search); 6: sar_runtime_new_group, sar_exchange_* */

/* ---- status codes ------------------------------------------------------------------------
 * Every function that can fail returns one of these (the reference panics instead: assert_eq! / unwrap / expect); the text is
 * in sar_last_error(). No C++ exception leaves the library: one thrown inside an entry point comes back as SAR_ERR_OOM
 * (std::bad_alloc) or SAR_ERR_INVALID (anything else). */
enum {
    SAR_OK = 0,
    SAR_ERR_INVALID = 1,      /* NULL pointer / bad enum / empty palette (ref: Palette::new panics, :413-418) */
    SAR_ERR_DIM_MISMATCH = 2, /* merge of runtimes with different sizes (ref: assert_eq!, :709-710) */
    SAR_ERR_NO_DEVICE = 3,    /* no HIP device / HIP runtime unavailable */
    SAR_ERR_HIP = 4,          /* a HIP call failed; see sar_last_error() */
    SAR_ERR_OOM = 5,          /* device or host memory exhausted */
    SAR_ERR_RANGE = 6,        /* a size is out of range: width*height > 2^31-1, units*jobs_per_unit > 2^32-1 */
    SAR_ERR_IO = 7,           /* an image file could not be created or written (ref: File::create(..).unwrap(), main.rs:103) */
    SAR_ERR_INTERNAL = 8      /* the device reported a state the host's checks rule out (a full hash table of the box kernels) */
};

/* ---- closed enums (Rust generics / closures cannot cross a C ABI) ------------------------- */
enum { SAR_RENDER_GAS = 0, SAR_RENDER_DEPTH = 1 };            /* RenderKind, src/lib.rs:233-239 */
enum { SAR_ATTRACTOR_SPROTT2 = 0 };                           /* PolynomialSprott2Degree, :575-580 */
enum { SAR_CT_POISSON_SATURNE = 0, SAR_CT_ADJUSTED_VELOCITY = 1 }; /* color_transforms, :498-559 */

#define SAR_PALETTE_MAX 15   /* user entries; the duplicated last entry (:416-418) is added internally */

/*
 * POD mirror of Config<A,T> + View + Colors (src/lib.rs:253-308, 389-492), plus the two things
 * the reference hides: `seed` (it seeds SmallRng from OS entropy, :656) and `jobs_total`
 * (it derives T*J from the thread pool, :1058-1062).
 */
typedef struct sar_config {
    uint64_t iterations;          /* Config::iterations (:267) */
    uint32_t width;               /* :269 */
    uint32_t height;              /* :271 */
    int32_t  render_kind;         /* SAR_RENDER_*  (:273) */
    int32_t  transparent;         /* bool (:275) */
    double   angle;               /* radians (:277) */
    int32_t  silent;              /* bool (:280); this library never prints */
    int32_t  attractor_kind;      /* SAR_ATTRACTOR_* */
    double   coeff_x[10];         /* PolynomialSprott2Degree::x (:577) */
    double   coeff_y[10];         /* :578 */
    double   coeff_z[10];         /* :579 */
    uint32_t palette_len;         /* number of entries in palette_rgb, 1..SAR_PALETTE_MAX */
    uint32_t _pad0;
    double   palette_rgb[SAR_PALETTE_MAX][3]; /* Palette list (:409), linear r,g,b */
    double   brightness_offset;   /* BrighnessConstants::offset (:394) */
    double   brightness_factor;   /* BrighnessConstants::factor (:395) */
    double   center_camera[3];    /* View::center_camera (:257) */
    double   rotation_axis[3];    /* EulerAxisRotation::axis (:172) — NOT normalised (release build, :181-183) */
    double   rotation_angle;      /* EulerAxisRotation::rotation (:174) */
    double   scale;               /* View::scale (:260) */
    int32_t  color_transform;     /* SAR_CT_* */
    int32_t  _pad1;
    double   ct_offset;           /* AdjustedVelocity::offset (:508) */
    double   ct_factor;           /* AdjustedVelocity::factor (:509) */
    uint64_t seed;                /* seed of the runtime's start-point stream (see sar_start_points) */
    uint32_t jobs_total;          /* number of independent trajectories ("jobs", :1062) sar_render_jobs runs */
    uint32_t _pad2;
} sar_config;

typedef struct sar_runtime sar_runtime;     /* opaque; Runtime, src/lib.rs:631-646 */
typedef struct sar_renderer sar_renderer;   /* opaque; ParallelRenderer, src/lib.rs:908-915 */

/* Per-call device timings (HIP events on the runtime's stream), filled when timing is enabled. */
typedef struct sar_timing {
    float    iterate_ms;    /* sum over launch chunks of the iterate kernel (k_iterate_split / k_iterate_lean) alone */
    float    resolve_ms;    /* depth-winner payload resolve + max reduction */
    float    colorize_ms;   /* last colorize */
    float    merge_ms;      /* last merge */
    uint32_t iterate_launches;
    float    warmup_ms;     /* sum over launch chunks of the warm-up + packing kernel (was padding before ABI 2) */
    uint64_t iterations_counted; /* jobs * iterations-per-job executed by the last render call */
    uint64_t depth_atomics;      /* binned path: global depth atomics issued since the last query (statistic) */
    uint64_t depth_candidates;   /* binned path: visits that passed the depth-hint filter (one chip-wide key load each) since the last query */
} sar_timing;

/* ---- misc ---------------------------------------------------------------------------------- */
int         sar_abi_version(void);
/* Which sources this binary was built from: the first 16 hex digits of the SHA-256 over the files under csrc, this header and the compiler
 * flags (strange_attractor_renderer_amd/build.py: source_id). The Python loader recomputes it from the tree and refuses a
 * library that was built from other sources. */
const char* sar_build_id(void);
const char* sar_status_string(int status);
const char* sar_last_error(void);           /* thread-local, human readable */
int         sar_device_count(int* out_count);
/* "0000:c5:00.0" of a HIP device ordinal (cap >= 16): which physical GPU a rank really runs on, for run records. */
int         sar_device_pci_bus_id(int device, char* out, size_t cap);
/* FNV-1a (64 bit) over a host buffer: the checksum tests/golden/fullsize_checksums.json freezes the full-size frames with,
 * so that a run record can say "this frame's count / zbuf / steps / RGBA16 are the committed ones" without shipping them. */
int         sar_checksum_fnv1a64(const void* data_host, size_t nbytes, uint64_t* out);

/* ---- Config presets (data only) -------------------------------------------------------------- */
/* Config::new defaults (:289-307) + poisson_saturne() values (:310-352). */
int sar_config_poisson_saturne(sar_config* out);
/* Config::new defaults + solar_sail() values (:354-387) (library scale 1.7; the CLI overrides to 1). */
int sar_config_solar_sail(sar_config* out);
/* Checks enums, palette_len, non-zero dimensions. */
int sar_config_validate(const sar_config* cfg);

/* ---- host-side setup math (no device needed) -------------------------------------------------- */
/* EulerAxisRotation::to_rotation_matrix, release semantics (:176-196). m is row-major 3x3. */
int sar_rotation_matrix(const sar_config* cfg, double m_out[9]);
/*
 * The start-point stream the reference leaves to OS entropy (:656, :748). SplitMix64(seed) seeds xoshiro256++ (four outputs
 * = the state: what rand 0.9 documents for SmallRng::seed_from_u64 on 64-bit targets); every f64 is (next_u64 >> 11) * 2^-53,
 * multiplied by 0.1 (`rng.random::<Vec3>() * 0.1`). Jobs come in BLOCKS of 4096: block b draws from the generator after b
 * applications of xoshiro256's published jump() (2^128 steps each), and job k takes draws 3i..3i+2 of block k / 4096 as
 * x, y, z, with i = k % 4096 — so the first 4096 jobs are the plain stream, and any job's point is found without drawing
 * its predecessors' (a multi-device render_parallel draws every device's job slice on its own host thread). Writes n_jobs*3
 * doubles for jobs [first_job, first_job+n_jobs) (first_job <= 2^36: reaching a job costs first_job / 4096 jumps of about a
 * microsecond each). The published vectors of both generators and the jump polynomial are held by tests/test_oracle_kat.py.
 */
int sar_start_points(uint64_t seed, uint64_t first_job, uint32_t n_jobs, double* xyz_out_host);

/* ---- Runtime (src/lib.rs:631-739) -------------------------------------------------------------- */
/* Runtime::new (:660-665): allocates count/steps/zbuf for cfg->width x cfg->height on `device`,
 * resets them, seeds the start-point stream with cfg->seed. */
int sar_runtime_new(const sar_config* cfg, int device, sar_runtime** out);
int sar_runtime_free(sar_runtime* rt);
/* n runtimes (1..32) for the frames of ONE batch (sar_render_jobs_batch; the `sequence` loop, src/bin/main.rs:493-517, keeps one
 * renderer for all its frames): one stream, one read-back stream, every runtime's buffers — sized for frames like cfg in batches
 * of n — carved from ONE device allocation instead of some twenty. Each out[i] is an ordinary runtime, freed in any order. */
int sar_runtime_new_group(const sar_config* cfg, int device, uint32_t n, sar_runtime** out /* [n] */);
/* Runtime::reset (:682-699): count<-0, steps<-0.0, zbuf<--1.0, max<-0. The RNG stream is NOT reseeded. */
int sar_runtime_reset(sar_runtime* rt);
/* n resets at once — the frames of a batch of a sweep (:950-951 per frame): ONE launch for the runtimes that share a stream. */
int sar_runtime_reset_batch(uint32_t n, sar_runtime* const* rts);
/* Runtime::set_width_height (:667-675): reallocates + resets only when the size changes. */
int sar_runtime_set_width_height(sar_runtime* rt, uint32_t width, uint32_t height);
/* Reseed the start-point stream (the reference has no equivalent; needed for reproducibility). */
int sar_runtime_seed(sar_runtime* rt, uint64_t seed);
/* Runtime::merge (:708-738): dst.count += src.count (wrapping); dst.max = max(dst.max, merged counts);
 * where src.zbuf > dst.zbuf (strict; dst wins ties) take src's steps and zbuf. Same device required. */
int sar_runtime_merge(sar_runtime* dst, const sar_runtime* src);
int sar_runtime_synchronize(sar_runtime* rt);
int sar_runtime_dims(const sar_runtime* rt, uint32_t* width, uint32_t* height);
/* Use an existing hipStream_t (passed as void*) instead of the runtime's own stream. */
int sar_runtime_set_stream(sar_runtime* rt, void* hip_stream);
int sar_runtime_get_stream(const sar_runtime* rt, void** hip_stream_out);
/* The stream the read-backs of sar_colorize_format_async run on (made on first use). Runtimes that share a launch stream —
 * the frames of a batch — should share this one too (set it on the others; whoever made it must outlive them): a process
 * has few hardware queues, and every further stream shares one with somebody's kernels. */
int sar_runtime_get_copy_stream(sar_runtime* rt, void** hip_stream_out);
int sar_runtime_set_copy_stream(sar_runtime* rt, void* hip_stream);

/* ---- render (src/lib.rs:747-838) ------------------------------------------------------------------ */
/* Exactly `render`: ONE trajectory of cfg->iterations counted iterations after a start point drawn
 * from the runtime's stream and 1000 uncounted warm-up iterations. Accumulates into rt (no reset). */
int sar_render(const sar_config* cfg, sar_runtime* rt);
/*
 * The data-parallel form: equivalent to calling `render` cfg->jobs_total times on this un-reset
 * runtime (what one reference worker does, :956-988) with iterations = cfg->iterations / jobs_total
 * (floor; the job split of :1056-1058). Results are defined as the SEQUENTIAL result in job order
 * (job-major, iteration-minor ties). starts_xyz_host: jobs_total*3 doubles (pre-warm-up start points,
 * already scaled) or NULL to draw them from the runtime's stream.
 */
int sar_render_jobs(const sar_config* cfg, sar_runtime* rt, const double* starts_xyz_host);
/* Shard form: run only jobs [first_job, first_job+n_jobs) of the split above, each with
 * iters_per_job counted iterations. starts_xyz_host holds n_jobs*3 doubles for THIS slice (required). */
int sar_render_job_range(const sar_config* cfg, sar_runtime* rt, uint32_t n_jobs,
                         uint64_t iters_per_job, const double* starts_xyz_host);

/* The same with the start points already in device memory (n_jobs*3 doubles, same [job][xyz] layout, on the
 * runtime's device; read in stream order): nothing crosses PCIe, the call only enqueues. */
int sar_render_job_range_device(const sar_config* cfg, sar_runtime* rt, uint32_t n_jobs,
                                uint64_t iters_per_job, const double* starts_xyz_dev);

/* F frames of a sweep in ONE set of launches — F iterations of the CLI's frame loop (src/bin/main.rs:493-517: every frame a reset,
 * src/lib.rs:950-951, and a render_parallel of fresh jobs) at a time. Frame i is sar_render_jobs(cfgs[i], rts[i],
 * starts_xyz_host[i]), bit for bit; what changes is how the chip is filled: a frame of 65 536 jobs occupies a third of an MI355X,
 * so the frames' workgroups share ONE launch of each kernel (workgroup -> frame -> its argument block and buffers), the frames
 * dealt to the XCDs. It applies to distinct runtimes on one device with one image size (make them with sar_runtime_new_group) and
 * configs with the same jobs_total, iterations per job and scale whose jobs are resident at once (one launch chunk, at most
 * 4 Mpx); anything else — and n_frames == 1 — runs frame after frame, same result. The work is enqueued on rts[0]'s stream (a
 * runtime on another stream is ordered with it through events); the launch options (sar_runtime_set_option) are rts[0]'s.
 * starts_xyz_host[i] == NULL (or starts_xyz_host == NULL) draws frame i's points from rts[i]'s own stream. */
int sar_render_jobs_batch(uint32_t n_frames, const sar_config* const* cfgs, sar_runtime* const* rts,
                          const double* const* starts_xyz_host);
/* How many frames like cfg to render per batch: 1 when frames of this shape cannot share launches (the test sar_render_jobs_batch
 * makes — a caller then builds ONE runtime per lane, not a batch of them); otherwise a multiple of eight, 8..32, the smallest
 * whose last round of equally long wave pairs fills an XCD (eight pairs per CU; a frame takes one per 64 jobs that survive the
 * warm-up, by this runtime's last launch — before any has reported: 16). rt may be NULL: the answer for a runtime yet to be made. */
int sar_runtime_batch_frames(const sar_config* cfg, sar_runtime* rt, uint32_t* out_frames);

/* Announces the NEXT sar_render_job_range_device call on this runtime — these start points, job count and iterations per
 * job, and the attractor's 30 coefficients; the view, render kind and colours of cfg may differ in the announced call (the
 * warm-up is the map alone: a sweep's next frame only turns the view) — so that the 1000 uncounted
 * warm-up iterations of its jobs (src/lib.rs:750-752) can run ahead, on a second stream, under the accumulate / fold /
 * colorize tail of the frame in flight (the CLI's frame loop, src/bin/main.rs:493-517, knows the next frame while it
 * renders this one; sar_render_parallel announces its own next frame this way). Results do not depend on it: a call that
 * does not match the announcement simply runs its own warm-up. The start points must be in place in device memory when this is called and stay unchanged until the announced
 * call; a reset in between is fine. Enqueues only. */
int sar_runtime_prefetch_device(const sar_config* cfg, sar_runtime* rt, uint32_t n_jobs,
                                uint64_t iters_per_job, const double* starts_xyz_dev);

/* ---- colorize (src/lib.rs:841-904) ---------------------------------------------------------------- */
/* Writes width*height*4 uint16 (RGBA16, FinalImage layout :625) to host memory. */
int sar_colorize(const sar_config* cfg, sar_runtime* rt, uint16_t* rgba_out_host);
/* Same, leaving the image in device memory (width*height*8 bytes); stream-ordered, no host sync. */
int sar_colorize_device(const sar_config* cfg, sar_runtime* rt, void* rgba_out_dev);
/* n of them at once (frame i: cfgs[i], rts[i] -> rgba_out_dev[i]): ONE launch for Gas frames of one palette on one stream. */
int sar_colorize_device_batch(uint32_t n, const sar_config* const* cfgs, sar_runtime* const* rts, void* const* rgba_out_dev);

/* ---- attractor extent: the "first pass" the reference leaves as a TODO (src/lib.rs:326-333) ----------------- *
 * n_jobs trajectories (start points from starts_xyz_host[n_jobs*3], or from the runtime's stream when NULL), each
 * 1000 warm-up iterations (:750-752) then iters_per_job iterations. out12[0..6) = xmin,xmax,ymin,ymax,zmin,zmax of the
 * screen-space points (cfg's rotation matrix applied, :773: the quantities the comment at :329-333 lists and from
 * which View::center_camera is chosen), out12[6..12) the same for the raw points. Bounds move through `<` / `>` only
 * (NaN never moves one), so the result is independent of the execution order. Does not touch the runtime's buffers. */
int sar_runtime_extent(const sar_config* cfg, sar_runtime* rt, uint32_t n_jobs, uint64_t iters_per_job,
                       const double* starts_xyz_host, double* out12);

/* ---- search for chaotic maps: Sprott's random search over the 30 coefficients ----------------------------------------- *
 * Candidate c under (seed, lo, hi) takes draws 30c .. 30c+29 of the SplitMix64 stream seeded with `seed` — draw k is
 * mix64(seed + (k+1) * 0x9E3779B97F4A7C15) with SplitMix64's finaliser, so no predecessor is drawn — each as
 * u = (d >> 11) * 2^-53, coeff = lo + (hi - lo) * u (a multiply, then an add: no FMA), filling coeff_x[0..10), coeff_y, coeff_z.
 * Every coefficient (generated or the caller's) goes through `0. + 1. * c` (-0.0 -> +0.0, as sar_render treats c0).
 *
 * Phase 1 (k_search_screen): `transient` steps of the map from `start`; a candidate dies once !(|x|, |y|, |z| <= bound)
 * (NaN included). Phase 2 (k_search_lyapunov): each survivor runs `steps` more steps carrying the tangent space: per step
 * V = J(p) Q, modified Gram-Schmidt V -> Q with norms n1, n2, n3 folded exactly as M_i *= n_i, (M_i, e) = frexp(M_i),
 * E_i += e; then p = next_point(p) and the raw bounds move (`<` / `>` only, as sar_runtime_extent). The first of n1, n2, n3
 * that is not positive and finite decides the step: exactly 0 -> DEGENERATE, otherwise (inf / NaN) -> DIVERGED; then a new
 * point beyond `bound` -> DIVERGED. A failing step is neither folded nor bounded; steps_done is its number (1-based), or
 * `steps` for a BOUNDED record. The raw fields are bit-exact (multiply, add, divide, sqrt and frexp only).
 * On the host: lambda_i = (E_i ln2 + ln M_i) / folded steps (steps_done, minus the failing one; none: NaN), sorted descending; the
 * Kaplan-Yorke dimension j + sum_{i<=j} lambda_i / |lambda_{j+1}| with j the largest index whose partial sum is >= 0 (0 or 3
 * at the ends; NaN without a folded step). Accepted: BOUNDED, lambda_1 >= min_lyapunov and ky_dim >= min_ky_dim. */
typedef struct sar_search_params {
    uint64_t seed;
    double   lo, hi;              /* coefficient box of generated candidates (default -1.2, 1.2: both presets lie in it) */
    double   start[3];            /* start point of every candidate (default 0.05, 0.05, 0.05: the middle of the start box) */
    uint32_t transient, steps;    /* phase-1 steps (default 1000, the render warm-up), phase-2 steps (default 20000); each <= 2^31 */
    double   bound;               /* default 1e6 */
    double   min_lyapunov;        /* default 0.005 (nats per iteration) */
    double   min_ky_dim;          /* default 0 */
    int32_t  keep_rejected;       /* 1: a record for every phase-2 candidate, whatever its status */
    int32_t  _pad;
} sar_search_params;
typedef struct sar_search_record {
    uint64_t candidate;           /* index (generated: the stream position; given: first + row) */
    int32_t  status;              /* SAR_SEARCH_* */
    uint32_t steps_done;
    int64_t  log2_exp[3];         /* raw accumulators E_i, M_i in Gram-Schmidt order: bit-exact */
    double   mant[3];
    double   lyapunov[3];         /* sorted descending, nats per iteration */
    double   ky_dim;
    double   extent[6];           /* xmin,xmax,ymin,ymax,zmin,zmax of the raw phase-2 points */
} sar_search_record;
typedef struct sar_search_stats {
    uint64_t tested, diverged_transient, diverged_late, degenerate, below_lyapunov, below_dim, accepted;
} sar_search_stats;
enum { SAR_SEARCH_BOUNDED = 0, SAR_SEARCH_DIVERGED = 1, SAR_SEARCH_DEGENERATE = 2 };
int sar_search_params_default(sar_search_params* out);
/* Candidate `index`'s 30 coefficients (host arithmetic, identical to the device's; no device needed). */
int sar_search_candidate(uint64_t seed, double lo, double hi, uint64_t index, double out30[30]);
/* Candidates [first, first + n): generated (coeffs_host == NULL) or the caller's [n][30] (x, y, z rows of 10). Runs on the
 * runtime's device and stream in chunks ("search_chunk" option, default 2^22 candidates); the image buffers are not touched.
 * Records (accepted ones, or every phase-2 candidate with keep_rejected) sorted by candidate: the first `cap` go to out_host,
 * *n_out is how many there are. stats_out may be NULL. With timing enabled, sar_runtime_last_timing reports the phases:
 * warmup_ms = k_search_screen, iterate_ms = k_search_lyapunov (iterate_launches = its launches). */
int sar_runtime_search(sar_runtime* rt, const sar_search_params* p, uint64_t first, uint32_t n,
                       const double* coeffs_host, sar_search_record* out_host, uint32_t cap, uint32_t* n_out,
                       sar_search_stats* stats_out);
/* Frames cfg's view on an extent (out12[0..6) of sar_runtime_extent: screen space under cfg's rotation), host arithmetic
 * on the reference's projection (src/lib.rs:774-789): center_camera = (-mid_x, -mid_z, -mid_y) and
 * scale = (1 - margin) * min(1 / range_x, height / (width * range_y)); with `sweep` range_x is the xz diagonal, so that every
 * angle of a turn stays in frame. Nothing else in cfg changes. */
int sar_frame_view(sar_config* cfg, const double screen_extent6[6], double margin, int sweep);

/* ---- Lyapunov planes: the largest exponent of a map family over a plane of two coefficients ------------------------------- *
 * A plane passes through the map `base` (30 coefficients: the x, y, z rows of sar_search_candidate) and sweeps two distinct
 * coefficients, axis[0] along the columns and axis[1] along the rows, over width x height pixels (row-major, y * width + x).
 * Pixel (x, y) is the map with
 *   coefficient axis[0] = lo[0] + (hi[0] - lo[0]) * t,  t = (double)x / (double)(width - 1)                (0 when width == 1)
 *   coefficient axis[1] = lo[1] + (hi[1] - lo[1]) * t,  t = (double)(height - 1 - y) / (double)(height - 1) (0 when height == 1)
 * (row 0 is the high end, as in a plot; hi - lo computed once, a multiply then an add, no FMA), every other coefficient base's,
 * and each one through `0. + 1. * c` as the search does: sar_plane_coeffs gives the device's doubles.
 * Each pixel runs the search's two phases fused in one lane: the transient from `start` — the first step outside the bound box is
 * DIVERGED with transient_done = that step (1-based) and steps_done = 0; a survivor has transient_done = transient — then `steps`
 * tangent steps. SAR_PLANE_SPECTRUM carries the whole tangent space with k_search_lyapunov's step: the record's status, steps_done,
 * log2_exp, mant, lyapunov and ky_dim are those sar_runtime_search gives the same map. SAR_PLANE_L1 carries q1 = e1 alone: per step
 * v = J(p) q1, n1 = |v|, q1 = v / n1 and the fold M *= n1, (M, e) = frexp(M), E += e, the status rules of the search applied to n1
 * alone, then the bound test — the first Gram-Schmidt column of the spectrum, to the bit. L1 measures the growth of e1: for a
 * generic map that is lambda_max, but for a map that keeps e1's direction invariant (a diagonal affine map, say) it is
 * ln|dx'/dx| instead; SPECTRUM gives the true maximum. In L1 records [1] and [2] hold E = 0, M = 1 and NaN exponents, and ky_dim is
 * NaN. The host finish is the search's: lambda = (E ln2 + ln M) / folded steps (sorted descending; NaN without a folded step). */
typedef struct sar_plane_params {
    double   base[30];            /* the map the plane passes through (default all 0) */
    uint32_t axis[2];             /* swept coefficients, distinct, each 0..29 (default 0, 1) */
    double   lo[2], hi[2];        /* ranges of axis[0] (columns) and axis[1] (rows), finite (default -1.2 .. 1.2 both) */
    uint32_t width, height;       /* pixels, width * height <= 2^24 (default 256 x 256) */
    double   start[3];            /* as sar_search_params: default 0.05, 0.05, 0.05 */
    uint32_t transient, steps;    /* default 1000, 20000; each <= 2^31 */
    double   bound;               /* default 1e6; finite and positive */
    int32_t  mode;                /* SAR_PLANE_L1 (default) or SAR_PLANE_SPECTRUM */
    int32_t  _pad;
} sar_plane_params;
typedef struct sar_plane_record {
    int32_t  status;              /* SAR_SEARCH_* */
    uint32_t transient_done, steps_done, _pad;
    int64_t  log2_exp[3];         /* raw accumulators E_i, M_i in Gram-Schmidt order: bit-exact */
    double   mant[3];
    double   lyapunov[3];         /* sorted descending, nats per iteration (L1: [0] only) */
    double   ky_dim;              /* SPECTRUM only */
} sar_plane_record;
typedef struct sar_plane_stats {
    uint64_t pixels, diverged_transient, diverged_late, degenerate, bounded;
} sar_plane_stats;
/* The colours of sar_runtime_plane_colorize, from cfg's palette through Palette::interpolate's arithmetic (as colorize blends a
 * pixel's colour), RGBA16 per pixel:
 *   DIVERGED                                    (0, 0, 0, 0)
 *   DEGENERATE, or BOUNDED without a folded step (0, 0, 0, 65535)
 *   BOUNDED, lambda_1 >= threshold              palette at v = (lambda_1 - threshold) / chaos_scale (clamped as interpolate
 *                                               clamps: v < 0 -> 0, v >= 1 -> 0.999999) times 65535, alpha 65535
 *   BOUNDED, lambda_1 < threshold               grey g = 0.5 * max(0, 1 - (threshold - lambda_1) / order_scale) times 65535
 * Each channel converts as colorize does (Rust `as u16`). lambda_1 is the largest exponent, evaluated on the device from the raw
 * fields with the device's log, which returns one of the two neighbouring doubles that enclose the true logarithm (measured, not only
 * documented: tests/test_gpu_device_log.py): a pixel's colour is one the expression above gives with such a value for log M — on the
 * planes the suite colours, the colour the host's logarithm gives. */
typedef struct sar_plane_colors {
    double threshold;             /* default 0 */
    double chaos_scale;           /* default 0.25; finite and positive */
    double order_scale;           /* default 1; finite and positive */
} sar_plane_colors;
enum { SAR_PLANE_L1 = 1, SAR_PLANE_SPECTRUM = 3 };
int sar_plane_params_default(sar_plane_params* out);
/* Pixel (x, y)'s 30 coefficients (host arithmetic, identical to the device's; no device needed). */
int sar_plane_coeffs(const sar_plane_params* p, uint32_t x, uint32_t y, double out30[30]);
/* The plane on the runtime's device and stream: one lane per pixel (k_plane, "plane_chunk" pixels per launch, default 2^20); the
 * image buffers are not touched. out_host: width * height records; stats_out may be NULL. The records stay on the device for
 * sar_runtime_plane_colorize until the next plane call. With timing enabled, sar_runtime_last_timing reports iterate_ms = k_plane
 * (iterate_launches = its launches). Refused (SAR_ERR_INVALID): equal axes or one above 29, a zero size or more than 2^24 pixels,
 * lo / hi / bound not finite or bound not positive, transient or steps above 2^31, an unknown mode. */
int sar_runtime_plane(sar_runtime* rt, const sar_plane_params* p, sar_plane_record* out_host, sar_plane_stats* stats_out);
int sar_plane_colors_default(sar_plane_colors* out);
/* Colours rt's last plane (colors NULL: the defaults) into rgba16_out_host[width * height * 4]; SAR_ERR_INVALID without one.
 * sar_runtime_set_width_height leaves the held records as they are — they have the plane's own size, not the runtime's —: the image
 * afterwards is the image before. */
int sar_runtime_plane_colorize(const sar_config* cfg, sar_runtime* rt, const sar_plane_colors* colors, uint16_t* rgba16_out_host);

/* ---- period planes: the period of the attractor at every pixel of a coefficient plane (the isoperiodic diagram) ------------------ *
 * The plane is sar_runtime_plane's, formula for formula: the map `base`, two distinct swept coefficients axis[0] (columns, from lo[0])
 * and axis[1] (rows, row 0 at the HIGH end), width x height pixels row-major, t = i / (n - 1) (0 when n == 1), lo + (hi - lo) * t with
 * hi - lo computed once, a multiply then an add, and every coefficient through `0. + 1. * c`; sar_period_coeffs gives a pixel's doubles
 * on the host. Alternatively the caller hands sar_runtime_period its own coefficient sets, [width * height][30] row-major (the x, y, z
 * rows of sar_search_candidate, each coefficient through `0. + 1. * c`): base, axis, lo and hi are then ignored — a line of maps
 * (height 1), an arbitrary list, a family that moves several coefficients together.
 * Per pixel, from `start`:
 *   transient  `transient` steps of next_point, each followed by the planes' bound test !(|x|, |y|, |z| <= bound), NaN included. The
 *              first point outside makes the pixel SAR_SEARCH_DIVERGED with transient_done = that step (1-based), steps_done = 0,
 *              period = 0 and residual NaN. A survivor has transient_done = transient.
 *   reference  r = the point after the transient.
 *   return     for k = 1 .. max_period: p = next_point(p); first the bound test — outside: DIVERGED, steps_done = k, period = 0,
 *              residual NaN, stop —; then d = max(max(|x - rx|, |y - ry|), |z - rz|), the differences and absolute values plain
 *              fp64, no FMA; d <= eps: SAR_SEARCH_BOUNDED, period = k, steps_done = k, residual = d, stop.
 *   no return  within max_period: BOUNDED, period = 0, steps_done = max_period, residual NaN.
 * What the number is: the FIRST RETURN of the orbit to within eps of r in the max norm, nothing more. period = 0 on a BOUNDED pixel says
 * "no period up to max_period at this resolution": chaos, a quasi-periodic orbit, or a cycle the transient has not yet settled on. A
 * cycle that converges slowly — next to a bifurcation — reads 0 (raise transient). A doubled cycle whose two branches are closer than
 * eps reads the undoubled period (lower eps). Nothing verifies that the orbit returns again after k more steps. Everything is an
 * integer, or one maximum of three absolute differences: a host restatement gives the same records bit for bit. */
typedef struct sar_period_params {
    double   base[30];            /* the map the plane passes through (default all 0) */
    uint32_t axis[2];             /* swept coefficients, distinct, each 0..29 (default 0, 1) */
    double   lo[2], hi[2];        /* ranges of axis[0] (columns) and axis[1] (rows), finite (default -1.2 .. 1.2 both) */
    uint32_t width, height;       /* pixels, width * height <= 2^24 (default 256 x 256) */
    double   start[3];            /* as sar_plane_params: default 0.05, 0.05, 0.05 */
    uint32_t transient;           /* default 2000; <= 2^31 */
    uint32_t max_period;          /* default 256; 1 .. 2^31 */
    double   bound;               /* default 1e6; finite and positive */
    double   eps;                 /* default 1e-9; finite, >= 0 (0: exact returns only) */
} sar_period_params;
typedef struct sar_period_record {
    int32_t  status;              /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t period;              /* the step of the first return; 0: none (or DIVERGED) */
    uint32_t transient_done, steps_done;
    double   residual;            /* d at the return; NaN without one */
} sar_period_record;
typedef struct sar_period_stats {
    uint64_t pixels, diverged_transient, diverged_late, periodic, aperiodic;   /* the last four sum to the first */
    uint64_t max_period_found;    /* the largest period of the plane (0: none) */
} sar_period_stats;
/* The colours of sar_runtime_period_colorize, RGBA16 per pixel:
 *   DIVERGED                  (0, 0, 0, 0)
 *   BOUNDED, period = 0       (0, 0, 0, 65535) — the black sea the literature draws
 *   BOUNDED, period = p >= 1  cfg's palette at v = ((double)((p - 1) % colours) + 0.5) / (double)colours through
 *                             Palette::interpolate's arithmetic as sar_runtime_plane_colorize applies it (clamp, blend, square root,
 *                             `as u16`), alpha 65535: periods p and p + colours share a colour
 * One division, three square roots and no logarithm: the image is bit for bit what a host restatement gives. */
typedef struct sar_period_colors {
    uint32_t colours;             /* default 16; at least 1 */
    uint32_t _pad;
} sar_period_colors;
int sar_period_params_default(sar_period_params* out);
/* Pixel (x, y)'s 30 coefficients of the sweep form (host arithmetic, identical to the device's; no device needed). */
int sar_period_coeffs(const sar_period_params* p, uint32_t x, uint32_t y, double out30[30]);
/* The period plane on the runtime's device and stream: one lane per pixel in 8 x 8 tiles (k_period, "period_chunk" pixels per launch,
 * default 2^20); the image buffers are not touched. coeffs_host: NULL for the sweep form, or the list form's [width * height][30].
 * records_out_host: width * height records; stats_out may be NULL. The records stay on the device for sar_runtime_period_colorize
 * until the next period call. With timing enabled, sar_runtime_last_timing reports iterate_ms = k_period (iterate_launches = its
 * launches). Refused (SAR_ERR_INVALID): a zero size or more than 2^24 pixels, bound not finite or not positive, transient above 2^31,
 * max_period 0 or above 2^31, eps negative or not finite, and — in the sweep form only — equal axes or one above 29, lo / hi not finite. */
int sar_runtime_period(sar_runtime* rt, const sar_period_params* p, const double* coeffs_host /* or NULL */,
                       sar_period_record* records_out_host, sar_period_stats* stats_out /* or NULL */);
int sar_period_colors_default(sar_period_colors* out);
/* Colours rt's last period plane (colors NULL: the defaults) into rgba16_out_host[width * height * 4]; SAR_ERR_INVALID without one
 * or with colours = 0. sar_runtime_set_width_height leaves the held records as they are — they have the plane's own size, not the
 * runtime's —: the image afterwards is the image before. */
int sar_runtime_period_colorize(const sar_config* cfg, sar_runtime* rt, const sar_period_colors* colors, uint16_t* rgba16_out_host);

/* ---- cycles: fixed points and periodic orbits of maps, stable or not, with their multipliers ---------------------------------------- *
 * The other analysis families see where orbits end up; this one solves F^p(x) = x by Newton's method from many starts per map and
 * merges what the starts find, so it also returns the saddles, the branch that goes on unstable after a period doubling and the
 * unstable cycles inside a chaotic attractor, each with M = D F^q at the orbit (its eigenvalues are the multipliers).
 * Input: n_maps coefficient sets [n_maps][30] (the x, y, z rows of sar_search_candidate, each coefficient through `0. + 1. * c`), one
 * `period` p, and starts shared by all maps: the caller's starts_xyz_host[jobs][3] (NaN refused, +-inf taken), or — NULL — the lattice
 * of grid^3 points over box_lo, box_hi: start j = (ix * grid + iy) * grid + iz has the coordinate lo + ((double)i + 0.5) * step per
 * axis, step = (hi - lo) / (double)grid computed once on the host (sar_cycles_starts gives these doubles); `jobs` is then ignored.
 * All norms are max norms, max(max(|a|, |b|), |c|) through `>`; all arithmetic is plain fp64, no FMA.
 *
 * Newton, per (map, start), iteration n = 0, 1, ... at the point x:
 *   steps      x_0 = x, M = I; p times: M <- J(x_k) M, then x_{k+1} = next_point(x_k). J's nine entries are tangent_eval's
 *              (x2 = x + x ...: jxx = ((cx1 + x2 cx2) + y cx3) + z cx4, jxy = ((x cx3 + cx5) + y2 cx6) + z cx7, jxz = ((x cx4 + y cx7) +
 *              cx8) + z2 cx9, likewise the y and z rows), and every column v of M becomes ((jrx v_x + jry v_y) + jrz v_z) per row r —
 *              the first product, with I, is made like the others.
 *   ESCAPED    one of x_1 .. x_p fails |x|, |y|, |z| <= bound (NaN fails): the start ends, iterations = n.
 *   CONVERGED  otherwise r = x_p - x, res = max|r_i|; res <= tol: the start ends at this x, iterations = n.
 *   NOT_CONVERGED  otherwise n == max_newton: the start ends, iterations = max_newton.
 *   SINGULAR   otherwise A = M - I (1 subtracted on the diagonal), row-major a b c / d e f / g h i; the cofactors
 *                c00 = e i - f h   c01 = f g - d i   c02 = d h - e g
 *                c10 = c h - b i   c11 = a i - c g   c12 = b g - a h
 *                c20 = b f - c e   c21 = c d - a f   c22 = a e - b d
 *              det = (a c00 + b c01) + c c02 and the numerators n_i = (c0i r_0 + c1i r_1) + c2i r_2 (adj A . r). det == 0 or not
 *              finite: the start ends, iterations = n.
 *   step       otherwise x_i <- x_i - n_i / det: three divisions, no reciprocal. Then iteration n + 1.
 * There is NO damping and NO line search: this is the plain Newton iteration. A start far from every root may wander, escape or run
 * out of iterations where a damped method would still arrive; the counts say how many did. `hits` is a share of this iteration's basin.
 *
 * Minimal period and representative of a CONVERGED start, from its x:
 *   pass 1     p steps of next_point from x. q is the first k = 1 .. p that divides p with max|x_k - x| <= same (p if none does). The
 *              representative is the lexicographically smallest of x_0 .. x_{q-1}: x_k replaces the one held when x_k.x < x, or
 *              x_k.x == x and (x_k.y < y, or x_k.y == y and x_k.z < z) — numeric compares, so of equal points the earlier stays.
 *   pass 2     q steps from the representative as in `steps`: M = D F^q there, row-major, and residual = max|F^q(rep) - rep|.
 * Merge, per map, over the starts in order: leader(j) is the smallest CONVERGED i <= j with q_i == q_j and max|rep_i - rep_j| <= merge;
 * head(j) = j if leader(j) == j, else head(leader(j)). An orbit is a head; its `hits` is the number of starts whose head it is. Orbits
 * are listed by ascending head; the first `cap` are kept (n_orbits), the others counted in orbits_lost and their hits in hits_lost.
 * This is a statement at merge's resolution, like the basin grid — and at a degenerate root (det A = 0 at the root) res <= tol only
 * gives |x - x*| of the order of sqrt(tol), so one double root can come back as two orbits: x' = x + x^2 with the defaults returns two
 * heads, near -8e-7 and +1e-6, for the one root 0. Raise `merge` for such a map; nothing here detects it.
 * Every field of the records and of the orbit slots is what a host restatement in plain IEEE arithmetic gives, bit for bit; nothing
 * depends on the launch shape, on "cycles_chunk" or on the order waves run in. */
#define SAR_CYCLE_CONVERGED 0
#define SAR_CYCLE_ESCAPED 1
#define SAR_CYCLE_SINGULAR 2
#define SAR_CYCLE_NOT_CONVERGED 3
typedef struct sar_cycles_params {
    uint32_t period;              /* p, 1 .. 64 (default 1) */
    uint32_t jobs;                /* starts of the caller's form, 1 .. 4096 (default 512); ignored with the lattice */
    uint32_t grid;                /* the lattice's points per axis, grid^3 <= 4096 (default 8); ignored with the caller's starts */
    uint32_t max_newton;          /* default 64; at most 65536 */
    uint32_t cap;                 /* orbit slots per map, 1 .. 4096 (default 64) */
    uint32_t _pad;
    double   box_lo[3], box_hi[3];   /* the lattice's box, finite, lo < hi (default -2 .. 2) */
    double   tol;                 /* default 1e-12; positive and finite */
    double   bound;               /* default 1e6; positive and finite */
    double   merge;               /* default 1e-6; finite, >= 0 (0: only equal representatives merge) */
    double   same;                /* default 1e-9; positive and finite */
} sar_cycles_params;
typedef struct sar_cycles_record {    /* one per map */
    uint32_t converged, escaped, singular, not_converged;   /* starts by outcome: they sum to the number of starts */
    uint32_t n_orbits, orbits_lost, hits_lost;              /* slots used; heads beyond cap, and the starts they stand for */
    uint32_t _pad;
    uint64_t newton_iterations;   /* the sum of the starts' iterations */
} sar_cycles_record;
typedef struct sar_cycle_orbit {      /* cap per map; the slots from n_orbits on are all zero */
    double   rep[3];              /* the representative */
    uint32_t period;              /* q, the minimal period at `same`'s resolution */
    uint32_t head;                /* the start that leads the orbit */
    uint32_t hits;                /* starts merged into it */
    uint32_t newton;              /* the head's iterations */
    double   residual;            /* max|F^q(rep) - rep| */
    double   M[9];                /* D F^q at rep, row-major */
} sar_cycle_orbit;
int sar_cycles_params_default(sar_cycles_params* out);
/* The lattice's starts, out_xyz_host[grid^3][3] (host arithmetic, the doubles the device starts from; no device needed). */
int sar_cycles_starts(const sar_cycles_params* p, double* out_xyz_host);
/* out3 = the coefficients of M's characteristic polynomial l^3 - out3[0] l^2 + out3[1] l - out3[2], M[9] row-major (host arithmetic):
 *   trace   (m0 + m4) + m8
 *   minors  ((m0 m4 - m1 m3) + (m0 m8 - m2 m6)) + (m4 m8 - m5 m7)
 *   det     (m0 (m4 m8 - m5 m7) + m1 (m5 m6 - m3 m8)) + m2 (m3 m7 - m4 m6)
 * The multipliers are its roots; solving for them is the caller's (eigenvalues are not part of this contract). */
int sar_cycle_charpoly(const double M[9], double out3[3]);
/* The cycles of n_maps maps on the runtime's device and stream: k_cycles_newton, one lane per (map, start) with a wave's lanes on one
 * map, then k_cycles_merge, one workgroup per map with the map's representatives in LDS; "cycles_chunk" lanes per launch, whole maps.
 * records_out_host[n_maps]; orbits_out_host[n_maps][cap]. p NULL: the defaults. n_maps == 0 succeeds and writes nothing. The runtime
 * lends its device, stream and timing spans: its image buffers, start-point stream and modes are neither read nor changed. With timing
 * enabled, sar_runtime_last_timing reports iterate_ms = k_cycles_newton (iterate_launches = its launches) and resolve_ms =
 * k_cycles_merge. Refused (SAR_ERR_INVALID): period 0 or above 64, max_newton above 65536, cap 0 or above 4096, tol or same not
 * positive and finite, merge negative or not finite, bound not positive and finite; with the caller's starts jobs 0 or above 4096 and
 * a NaN coordinate; with the lattice grid 0 or grid^3 above 4096, a box that is not finite or has lo >= hi on an axis. */
int sar_runtime_cycles(sar_runtime* rt, const sar_cycles_params* p, uint32_t n_maps, const double* coeffs_host /* [n_maps][30] */,
                       const double* starts_xyz_host /* [jobs][3] or NULL */, sar_cycles_record* records_out_host,
                       sar_cycle_orbit* orbits_out_host);

/* ---- unstable manifolds: the W^u of saddle cycles, rasterised as connected curves into a view's image ------------------------------ *
 * sar_runtime_cycles finds a map's saddles; this family draws what leaves them. A branch of a saddle cycle's unstable manifold is
 * grown from a short straight piece next to the cycle — a fundamental domain — by stepping every sample point of the piece and, at
 * every step, drawing the line segments between neighbouring samples into the image of `cfg`'s view.
 * Map, view and image come from ONE cfg: its 30 coefficients, each through `0. + 1. * c`, its camera (rotation, center_camera, scale,
 * angle) and its width x height, 1 to 2^24 pixels. All floating-point arithmetic is plain fp64, multiply then add, no FMA; everything
 * behind the fp64 steps is integers.
 *
 * Branch (sar_manifold_branch): base[3], a point of the cycle; dir[3], the direction, NOT normalised by the library; delta; period,
 * the map steps per return — q, or 2 q where the multiplier is negative. Eigenvectors are the caller's: not part of this contract.
 * Fundamental domain, per branch, on the host:
 *   a          base_k + delta * dir_k per coordinate k
 *   b          `period` steps of next_point from a. Every point on the way, a and b included, is tested with the planes' bound test
 *              (|x|, |y|, |z| <= bound, NaN fails); a failure makes the branch SAR_MANIFOLD_DOMAIN_ESCAPED: nothing of it is drawn,
 *              its counters are 0, first_long_step is 0xFFFFFFFF, and the record still carries a and b — b is whatever IEEE
 *              arithmetic gives after all `period` steps.
 *   samples    d_k = b_k - a_k once; point i of S = `samples` is a_k + d_k * t_i, t_i = (double)i / (double)(S - 1).
 * The straight piece stands in for the curved domain. That is an error of O(delta^2) at the cycle, which the map contracts onto the
 * manifold as it stretches along it: the picture is the manifold's in the limit delta -> 0, and at a finite delta the first steps'
 * segments lie beside it by that much. Nothing here measures it.
 *
 * Steps, n = 0 .. `steps`:  1. every point is tested: it is DEAD from the first n at which the bound test fails (also at n = 0),
 * for good; 2. every segment (i, i + 1), i = 0 .. S - 2, is classified and drawn; 3. every point takes one step of next_point.
 * Projection of a point (x, y, z) — the renderer's, operation for operation, with the constants render hoists:
 *   s_r        (m_r0 x + m_r1 y) + m_r2 z per row r of the rotation matrix
 *   ax, az     s_0 + center_camera_0, s_2 + center_camera_1
 *   x2         ax cos(angle) + az sin(angle)
 *   fi         (0.5 / scale - x2) * (width * scale)          fj   height / 2 - (s_1 + center_camera_2) * (width * scale)
 * The point is PLACED when -2^30 <= fi < 2^30 and -2^30 <= fj < 2^30 (NaN is not placed); then X = floor(fi), Y = floor(fj) as signed
 * integers. Where 0 <= X < width and 0 <= Y < height this is the pixel sar_render gives the same point. sar_manifold_pixel gives fi, fj.
 * Segment classes — the first rule that applies:
 *   dead       an endpoint is dead
 *   far        an endpoint is not placed
 *   long       L = max(|dX|, |dY|) > max_span, dX = X1 - X0, dY = Y1 - Y0: the curve is under-resolved there; counted, not drawn
 *   drawn      otherwise
 * Raster of a drawn segment: L = 0 plots (X0, Y0) once; L >= 1 plots k = 0 .. L - 1 at X0 + floor_div(2 k dX + L, 2 L),
 * Y0 + floor_div(2 k dY + L, 2 L), the division rounding toward -infinity (not as C truncates). The end pixel belongs to the next
 * segment. A plot inside the image does count[pix] += 1 and first[pix] = min(first[pix], n * 4096 + branch), pix = Y width + X; both
 * images are u32, first starts at 0xFFFFFFFF. A drawn segment visits a pixel at most once, so count cannot wrap while
 * n_branches (S - 1) (steps + 1) < 2^32, which is required. Of two equal branches the lower index keeps `first`.
 * Every word of count and first and every field of the records is what a host restatement in plain IEEE arithmetic gives, bit for
 * bit: the adds and the mins commute, so nothing depends on the launch shape or on the order waves run in. */
#define SAR_MANIFOLD_OK 0
#define SAR_MANIFOLD_DOMAIN_ESCAPED 1
typedef struct sar_manifold_params {
    uint32_t samples;             /* S, points of a fundamental domain, 2 .. 2^20 (default 4096) */
    uint32_t steps;               /* 0 .. 65535 (default 32) */
    uint32_t max_span;            /* the longest segment drawn, in pixels, 1 .. 4096 (default 16) */
    uint32_t _pad;
    double   bound;               /* default 1e6; positive and finite */
} sar_manifold_params;
typedef struct sar_manifold_branch {
    double   base[3];             /* a point of the cycle; finite */
    double   dir[3];              /* the direction, as given; finite, not all zero */
    double   delta;               /* finite, not zero */
    uint32_t period;              /* map steps per return, 1 .. 128 */
    uint32_t _pad;
} sar_manifold_branch;
typedef struct sar_manifold_record {  /* one per branch */
    int32_t  status;              /* SAR_MANIFOLD_* */
    uint32_t first_long_step;     /* the smallest n with a long segment; 0xFFFFFFFF: none */
    uint32_t alive_end;           /* points alive at n = steps */
    uint32_t _pad;
    double   a[3], b[3];          /* the fundamental domain's ends */
    uint64_t n_drawn, n_dead, n_far, n_long;   /* segments by class: they sum to (S - 1) (steps + 1), or are all 0 (DOMAIN_ESCAPED) */
    uint64_t pixels;              /* plots inside the image */
    uint64_t length_px;           /* the sum of L over the drawn segments */
} sar_manifold_record;
int sar_manifold_params_default(sar_manifold_params* out);
/* out_fi_fj[2] = fi, fj of the point xyz[3] in cfg's view (host arithmetic, the device's doubles; no device needed). The map's
 * coefficients are not used. */
int sar_manifold_pixel(const sar_config* cfg, const double xyz[3], double out_fi_fj[2]);
/* The branches' manifolds on the runtime's device and stream: both images are cleared on the stream, then k_manifold runs one lane
 * per sample and one wave per 63 segments of a branch — wave w holds the points 63 w .. 63 w + 63, lane l reads its right neighbour's
 * pixel across the wave and draws segment 63 w + l, the seam point is computed by both waves; nothing is stored per lane.
 * count_out_host[height][width], first_out_host[height][width], records_out_host[n_branches]. params NULL: the defaults.
 * n_branches == 0 succeeds and writes nothing. The runtime lends its device, stream and timing spans; a part of its own holds this
 * family's device buffers: the runtime's image buffers, start-point stream and modes are neither read nor changed, and cfg's size
 * need not be the runtime's. With timing enabled, sar_runtime_last_timing reports iterate_ms = k_manifold (iterate_launches = 1).
 * Refused (SAR_ERR_INVALID): a cfg that sar_config_validate refuses (with its status) or an image above 2^24 pixels; samples outside
 * 2 .. 2^20, steps above 65535, max_span outside 1 .. 4096, bound not positive and finite; n_branches above 4096;
 * n_branches (S - 1) (steps + 1) >= 2^32; more than 2^26 lanes (n_branches ceil((S - 1) / 63) 64); a branch whose base, dir or delta is
 * not finite, whose delta is zero, whose dir is all zero or whose period is outside 1 .. 128; a NULL runtime or buffer. */
int sar_runtime_manifold(sar_runtime* rt, const sar_config* cfg, const sar_manifold_params* params, uint32_t n_branches,
                         const sar_manifold_branch* branches_host, uint32_t* count_out_host, uint32_t* first_out_host,
                         sar_manifold_record* records_out_host);

/* ---- auto exposure: a levels stretch of the Gas tone curve from the frame's own counts ------------------------------------ *
 * Colorize writes (c F + brightness_offset) brightness_factor 65535 per channel c, F = ln(count+1) / ln(M+1) (src/lib.rs:858-866).
 * Exposure picks the two constants on the device:
 *   covered pixels   count != 0; n of them, their counts sorted ascending as s[0..n). (A count above M — only a state loaded with
 *                    sar_runtime_load and a smaller max has one — counts as M.)
 *   quantile count   k = floor(q * (double)n) (one IEEE product, then floor), clamped to n - 1; c(q) = s[k]: an exact order
 *                    statistic, independent of the launch shape and of the order of the atomics.
 *   F                F(c) = ln(c+1) / ln(M+1) with colorize's M (the wrap flag gives 0xFFFFFFFF) and colorize's ln: the host-libm
 *                    table below 2^20, device log above it — one of the two neighbouring doubles that enclose the true logarithm,
 *                    so offset and factor are what the expressions below give with such values (at most 8 candidates a record).
 *   constants        F_b = F(c(q_black)), F_w = F(c(q_white)); factor = (level_white - level_black) / (F_w - F_b), then
 *                    offset = level_black / factor - F_b (in that order, no contraction): a channel of 1 reaches level_black at the
 *                    black count and level_white at the white count.
 *   fallback         no covered pixel, F_w - F_b not positive and finite, or a constant not finite: the frame keeps cfg's
 *                    brightness_offset / brightness_factor and the record says applied = 0.
 * Parameters: 0 <= q_black <= q_white <= 1, finite levels, level_black < level_white (else SAR_ERR_INVALID). Alpha (F 65535 with
 * `transparent`) and Depth frames do not change. The selection is a radix select over the count buffer — the top 12 bits below
 * M's highest one, then 12 more and the last <= 8 inside each quantile's bucket — in a fixed number of launches on the runtime's
 * stream that never wait for the host (M stays on the device). */
typedef struct sar_exposure_params {
    double q_black, q_white;           /* default 0, 0.995 */
    double level_black, level_white;   /* default 0, 1 */
} sar_exposure_params;
typedef struct sar_exposure {
    double   offset, factor;           /* what colorize uses: the solved constants, or cfg's (applied == 0) */
    uint32_t black_count, white_count; /* c(q_black), c(q_white); 0 without a covered pixel */
    uint32_t covered;                  /* n */
    uint32_t max;                      /* M */
    int32_t  applied;
    int32_t  _pad;
} sar_exposure;
int sar_exposure_params_default(sar_exposure_params* out);
/* The exposure of rt's current buffers (params NULL: the defaults), computed with the same kernels as the mode below; waits for it.
 * A "hold" exposure: copy offset / factor into a config and colorize every frame of a sweep with it. */
int sar_runtime_exposure(const sar_config* cfg, sar_runtime* rt, const sar_exposure_params* params, sar_exposure* out);
/* The mode: while it is on (params != NULL), every whole-image Gas colorize of rt — sar_colorize, _device, _format, _format_async,
 * _device_batch — selects and solves on the device first and uses the result instead of cfg's constants (frames of a batch then
 * share one colorize launch whatever their constants). Colorizing part of the image (sar_colorize_range_device) fails with
 * SAR_ERR_INVALID while it is on. NULL turns it off. */
int sar_runtime_set_exposure(sar_runtime* rt, const sar_exposure_params* params);
/* The same for the renderer's shard-0 runtime, now or whenever it is made (sar_render_parallel colorizes through it on one
 * device). A render of a renderer over several devices with the mode on fails with SAR_ERR_INVALID. NULL turns it off. */
int sar_renderer_set_exposure(sar_renderer* r, const sar_exposure_params* params);

/* ---- auto colour range: the palette window of a Gas frame from the frame's own steps ---------------------------------------- *
 * Colorize takes a pixel's hue from Palette::interpolate(steps) (src/lib.rs:442-472), which clamps steps to [0, 1). A colour range
 * is an affine window on steps, chosen on the device from two exact quantiles of the frame's steps buffer:
 *   population       the pixels with count != 0 whose steps is not NaN; n of them.
 *   order            by the sortable 64-bit image of the double: its bits, all of them flipped when the sign bit is set, the sign bit
 *                    set otherwise (-0.0 below +0.0, -inf first, +inf last).
 *   quantile         the population sorted ascending by that key as s[0..n); k = floor(q * (double)n) (one IEEE product, then floor),
 *                    clamped to n - 1; v(q) = s[k]: an exact order statistic, independent of the launch shape, of the number of
 *                    workgroups and of the order of the atomics.
 *   window           lo = v(q_lo), hi = v(q_hi), span = hi - lo. (n = 0: lo = hi = 0.)
 *   position         pos = pos_lo + ((steps - lo) / span) * (pos_hi - pos_lo) — in exactly that order, no contraction — goes through
 *                    Palette::interpolate's clamp and blend, unchanged, in the place of steps. pos_lo > pos_hi reverses the palette.
 *   fallback         n = 0, span not positive and finite, or lo or hi not finite: the record says applied = 0 and colorize uses steps
 *                    as it is (bit for bit the image without a window).
 * Parameters: 0 <= q_lo <= q_hi <= 1, finite positions (else SAR_ERR_INVALID). Alpha, brightness and Depth frames do not change.
 * The selection is a radix select over the count and steps buffers — the keys' sign and exponent (12 bits), then the mantissa in
 * four digits of 13 bits inside each quantile's bucket — in a fixed number of launches on the runtime's stream that never wait for
 * the host. It is independent of auto exposure: a frame may have both, one or neither. */
typedef struct sar_color_range_params {
    double q_lo, q_hi;                 /* default 0.01, 0.99 */
    double pos_lo, pos_hi;             /* default 0, 1 */
} sar_color_range_params;
typedef struct sar_color_range {
    double   lo, hi;                   /* v(q_lo), v(q_hi); 0 without a population */
    double   pos_lo, pos_hi;           /* the parameters' */
    uint32_t covered;                  /* n */
    int32_t  applied;
} sar_color_range;
int sar_color_range_params_default(sar_color_range_params* out);
/* The colour range of rt's current buffers (params NULL: the defaults), computed with the same kernels as the mode below; waits
 * for it. */
int sar_runtime_color_range(const sar_config* cfg, sar_runtime* rt, const sar_color_range_params* params, sar_color_range* out);
/* The mode: while it is on (params != NULL), every whole-image Gas colorize of rt — sar_colorize, _device, _format, _format_async,
 * _device_batch — selects on the device first and colours through the frame's own window (frames of a batch share one colorize
 * launch whatever their windows). Colorizing part of the image (sar_colorize_range_device) fails with SAR_ERR_INVALID while it is
 * on. NULL turns it off. Turning it on ends a hold. */
int sar_runtime_set_color_range(sar_runtime* rt, const sar_color_range_params* params);
/* The hold: every whole-image Gas colorize of rt colours through this one window (a record of sar_runtime_color_range, or one made
 * by hand: finite positions; with applied != 0, finite lo < hi with a finite hi - lo — else SAR_ERR_INVALID), nothing is measured:
 * the frames of a sweep keep their colours. Refused where the mode is; NULL turns it off. Holding ends the mode. Waits for the
 * runtime's stream. */
int sar_runtime_hold_color_range(sar_runtime* rt, const sar_color_range* range);
/* The mode for the renderer's shard-0 runtime, now or whenever it is made (sar_render_parallel colorizes through it on one
 * device). A render of a renderer over several devices with the mode on fails with SAR_ERR_INVALID. NULL turns it off. */
int sar_renderer_set_color_range(sar_renderer* r, const sar_color_range_params* params);
/* The window as constants of the colour transform: for a SAR_CT_ADJUSTED_VELOCITY config, whose steps are (|dp| + ct_offset) ct_factor,
 * and a range with positions (0, 1), *out = *in with ct_offset' = ct_offset - lo / ct_factor and ct_factor' = ct_factor / span: a
 * render with *out carries the window in its steps (and the two constants fit the reference program's AdjustedVelocity { offset,
 * factor }). Algebraically the same window, not bit for bit: four roundings sit elsewhere. One kind of pixel is out of its reach: a
 * covered pixel no visit ever won the depth test on (count != 0, zbuf -1: pixel 0 of a map that loses trajectories to infinity,
 * where their NaN coordinates are counted) holds the steps the reset wrote, 0, in any render — the window moves it as it moves
 * every covered pixel, the transform's constants cannot. A range with applied == 0 gives
 * *out = *in. Another transform, other positions, a ct_factor of 0 or a constant that is not finite: SAR_ERR_INVALID. No device. */
int sar_color_range_to_velocity(const sar_config* in, const sar_color_range* range, sar_config* out);

/* ---- density estimation: an adaptive blur of the Gas histogram, in place, on the device ----------------------------------------- *
 * A frame is a histogram: filaments hold thousands of hits per pixel, the veil around them 0, 1 or 2, which shows as speckle. The
 * filter spreads each pixel's mass over a kernel that narrows as the pixel's count grows (the density estimation of flame-fractal
 * renderers): bright structure stays pixel-sharp, sparse regions become a haze. Everything is integers plus one fp64 sum in a fixed
 * order: a host restatement gives the same buffers bit for bit (tests/density_restatement.py). No pow, exp, sqrt or log anywhere.
 *   parameter  samples = S, 2 <= S <= 256 (default 64). A covered pixel with count c < S spreads over the lattice offsets (dx, dy) with
 *              d2 * c < S, d2 = dx*dx + dy*dy: a disc of area about pi S / c, the area that holds about S hits at that density (the
 *              k-nearest-neighbour bandwidth). A pixel with c >= S keeps all of its mass. The widest reach is R = floor(sqrt(S - 1)):
 *              7 at the default, 15 at S = 256.
 *   weights    one radial table per class c = 1 .. S-1, indexed by d2 in [0, S). A tap is live when d2 * c < S (an integer compare).
 *              For a live tap t = (double)(d2 * c) / (double)S, u = 1.0 - t, q[d2] = (int64)floor(u * u * 1048576.0), one IEEE
 *              operation each (the biweight shape). N = the integer sum of q[dx*dx + dy*dy] over the live lattice offsets in
 *              [-R, R]^2. For d2 > 0: W_c[d2] = (q[d2] << 16) / N (integer division; dead taps 0), and
 *              W_c[0] = 65536 - the sum of W_c[dx*dx + dy*dy] over the live offsets with d2 > 0: every class sums to exactly 2^16 over
 *              the lattice. (A live tap's weight may round down to 0: S = 256, c = 255 has W[1] = 0.) Class c >= S is the identity:
 *              65536 at d2 = 0 and nothing else. S = 2 gives W_1 = {32768, 8192}.
 *   count      for output pixel p the taps are visited in a fixed order, dy from -R to R (outer), dx from -R to R (inner); the source
 *              is q = p + (dx, dy). A source outside the image is skipped (mass that leaves the image is lost), and so is one with
 *              count[q] == 0. m = W_class(count[q])[d2] * count[q] as u64; acc = the sum of m (below 2^50);
 *              count'[p] = min((acc + 32768) >> 16, 0xFFFFFFFF).
 *   hue        steps is the colour value of the depth winner; the output is the mass-weighted mean of the sources' values: over the
 *              sources whose steps[q] is finite, den = the sum of m (u64) and num = num + (double)m * steps[q] in the tap order, no
 *              contraction (num starts at +0.0; a tap with m == 0 may be skipped or added, the bits are the same). When no source
 *              other than p itself has entered den — den == 0 included — steps'[p] = steps[p] with its bits untouched: the mean of one
 *              value is that value (the round trip (m s) / m is not s in fp64, and a pixel that nothing reaches must not change).
 *              Otherwise steps'[p] = num / (double)den, one conversion and one division.
 *   writes     count, steps and max (the maximum of count'). The wrap flag, zbuf, the depth keys and the depth hints stay as they
 *              are: a Depth colorize of the state does not change.
 *   statistics all integers, exact whatever the launch shape or the order of the atomics (sar_density_stats).
 * The call filters what the runtime holds NOW: it is not idempotent — calling it twice filters twice — and sar_runtime_merge must
 * come before it, not after (the sum of two filtered frames is not the filtered sum). The order of a frame is
 * render -> density -> exposure / colour range -> colorize: the two modes then measure the filtered buffers. */
typedef struct sar_density_params {
    uint32_t samples;                  /* S: default 64; 2 .. 256 */
    uint32_t _pad;
} sar_density_params;
typedef struct sar_density_stats {
    uint64_t mass_in;                  /* the sum of count */
    uint64_t mass_q16;                 /* the sum of acc, modulo 2^64: mass_in << 16 when no mass left the image */
    uint32_t covered_in, covered_out;  /* pixels with count != 0, count' != 0 */
    uint32_t spread;                   /* pixels with 0 < count < S */
    uint32_t saturated;                /* pixels whose (acc + 32768) >> 16 was above 0xFFFFFFFF */
    uint32_t max_in, max_out;          /* the maximum of count, of count' */
} sar_density_stats;
int sar_density_params_default(sar_density_params* out);
/* R = floor(sqrt(samples - 1)) in integers (params NULL: the defaults). Host only. */
int sar_density_radius(const sar_density_params* params, uint32_t* out_radius);
/* Class c's table W_c[0 .. samples) (the identity row for c >= samples; c == 0: SAR_ERR_INVALID). Host only; the device's plan is
 * made of these rows. */
int sar_density_weights(const sar_density_params* params, uint32_t c, uint32_t* out /* [samples] */);
/* Filters rt's count and steps in place on the runtime's stream (k_density reads a snapshot of both — 12 bytes per pixel of scratch
 * the runtime allocates on first use and frees with itself — and writes the live buffers). With stats_out == NULL the call never
 * waits for the host: a sweep enqueues it between a frame's render and its colorize; otherwise it waits once. Refused
 * (SAR_ERR_INVALID): samples outside 2 .. 256, a NULL runtime. The launch shape ("density_tile" option: rows of the 32-wide tile a
 * workgroup owns, 8, 16 or 32; 0 = 16) changes no bit of the result. With timing enabled, sar_runtime_last_timing reports
 * iterate_ms = k_density (iterate_launches = 1), as the analysis families book their main kernel: like them, a call that does not
 * accumulate timing starts the runtime's spans afresh, so read a render's timing before filtering. */
int sar_runtime_density(sar_runtime* rt, const sar_density_params* params /* NULL: defaults */, sar_density_stats* stats_out /* or NULL */);
/* Statistic of the launch shape of rt's last sar_runtime_density, not of the picture: the tiles it launched and how many of them
 * took the copy-through path (every source of the tile and its halo 0 or >= samples). Waits for the stream. */
int sar_runtime_density_tiles(sar_runtime* rt, uint32_t* tiles_out, uint32_t* copied_out);

/* ---- shaded rendering: a lit surface with ambient occlusion from the depth buffer ------------------------------------------------- *
 * zbuf is the nearest depth per pixel: a height field. The call turns a runtime's current count / zbuf / steps into RGBA16: the
 * surface lit from one direction (ambient + diffuse + a specular glint), darkened where neighbours stand in front of it, in the hue
 * the palette gives the pixel's steps. It is a third picture beside Gas and Depth, not a render_kind. All arithmetic is fp64 with
 * separate multiply and add; the only operations are + - * / sqrt, compares, the f32 -> f64 conversion and colorize's `as u16`: a
 * host restatement gives the same image and statistics bit for bit (tests/shade_restatement.py).
 *   host constants  k = (double)width * scale (the reference's width_scaled: one pixel is 1 / k world units, dz * k a height in pixels).
 *              L = light / sqrt((lx lx + ly ly) + lz lz), a division per component. H = (Lx, Ly, Lz + 1.0) normalised the same
 *              way; the view is orthographic, along +z; when H's length (that square root) is 0 the specular term is 0.
 *              inv_d[d2] = 1.0 / sqrt((double)d2) for 1 <= d2 <= R^2. N = the number of lattice offsets with 0 < dx^2 + dy^2 <= R^2.
 *              With a window: span = hi - lo, dpos = pos_hi - pos_lo.
 *   surface    a pixel is SURFACE when its zbuf is finite, is not the sentinel -1.0f, and count >= min_count. Every other pixel is
 *              BACKGROUND: +-inf and NaN depths, a covered pixel no visit ever won the depth test on, a pixel the density filter
 *              emptied. Background occludes nothing and lights nothing. (-0.0 and subnormal depths are surface.)
 *   smoothing  gives z~, an fp64 value per surface pixel. smooth == 0: z~ = (double)z. smooth == 1: the mean of (double)z_q over the
 *              3 x 3 window, dy = -1 .. 1 outside, dx = -1 .. 1 inside, centre included, over the q that are in the image, are surface
 *              and have |(double)z_q - (double)z_p| * k <= smooth_range; the fp64 sum runs in that order and is divided by their
 *              number as a double. The surface mask does not change.
 *   normal     on the x axis a = z~[x+1] - z~[x] if the right neighbour is surface, b = z~[x] - z~[x-1] if the left one is; with
 *              both, gx = |a| <= |b| ? a : b (the smaller difference keeps a depth step between two sheets from becoming a wall);
 *              with one, that one; with none, 0. The y axis is the same, the pixel below playing a. sx = gx * k, sy = gy * k,
 *              len = sqrt((sx sx + sy sy) + 1.0), n = (-sx / len, -sy / len, 1.0 / len). (x right, y down, z towards the viewer.)
 *   light      d = (nx Lx + ny Ly) + nz Lz, then d = d > 0 ? d : 0 (NaN gives 0). s = (nx Hx + ny Hy) + nz Hz, clamped the same
 *              way, then squared (s = s * s) shininess_log2 times.
 *   occlusion  the taps run dy = -R .. R outside, dx = -R .. R inside, over the offsets with 0 < d2 <= R^2, d2 = dx dx + dy dy. A tap
 *              outside the image or on background adds nothing. Otherwise h = (z~_q - z~_p) * k; if h > 0 and h <= ao_range then
 *              t = h * inv_d[d2] and occ = occ + (t < 1 ? t : 1). ao = 1 - ao_strength * (occ / (double)N), then
 *              ao = ao > 0 ? ao : 0. R = 0 means no taps and ao = 1.
 *   hue        (r, g, b) = Palette::interpolate's clamp, blend and square roots, as colorize applies them, at v = steps, or — with
 *              a window whose applied != 0 — at v = pos_lo + ((steps - lo) / span) * dpos, in exactly that order (the colour range's
 *              position expression). The runtime's exposure and colour-range MODES do not apply.
 *   pixel      lum = ao * (ambient + diffuse * d), glint = ao * (specular * s); per channel c = r * lum + glint, then
 *              c = c > 0 ? c : 0 (NaN gives 0), then c = c < 1 ? c : 1, then `as u16` of c * 65535.0. Alpha is 65535 on a surface
 *              pixel. A background pixel is background[0..3] with alpha cfg->transparent ? 0 : 65535.
 *   statistics all integers, exact whatever the launch shape or the order of the atomics (sar_shade_stats).
 * One rule added to the issue's text: the normal of a pixel reads z~ of its four neighbours whatever R is, so the workgroup's halo
 * of z~ is max(R, 1) wide — R = 0 turns the occlusion off, not the relief.
 * The call reads count, steps and the depth keys and writes only the image and its own reduction block: count, steps, zbuf, max and
 * the scalars keep their bits. The order of a frame is render -> [density] -> shade. The surface is the NEAREST hit of every pixel:
 * thin veils of single hits in front of a sheet look rough until min_count (with the density filter before it, or alone) or more
 * iterations thin them out. */
typedef struct sar_shade_params {
    double   light[3];                 /* direction TOWARDS the light, image space; finite, not all zero; default -0.5, -0.7, 0.6 */
    double   ambient, diffuse, specular; /* weights; finite, >= 0; default 0.25, 0.75, 0.25 */
    double   ao_strength;              /* finite, >= 0; default 1 */
    double   ao_range;                 /* pixels of height beyond which a neighbour no longer occludes; finite, >= 0; default 12 */
    double   smooth_range;             /* pixels of height; finite, >= 0; default 2 */
    uint32_t shininess_log2;           /* the specular term is squared this many times; 0 .. 10; default 5 */
    uint32_t ao_radius;                /* R, pixels; 0 .. 8; default 6 */
    int32_t  smooth;                   /* 0 / 1; default 1 */
    uint32_t min_count;                /* default 1 */
    uint16_t background[3];            /* r, g, b; default 0, 0, 0 */
    uint16_t _pad0;
    int32_t  has_window;               /* 0 / 1; default 0 */
    int32_t  _pad1;
    sar_color_range window;            /* read when has_window: as sar_runtime_hold_color_range validates a record */
} sar_shade_params;
typedef struct sar_shade_stats {
    uint32_t surface, background;      /* they sum to width * height */
    uint32_t isolated;                 /* surface pixels with no surface 4-neighbour */
    uint32_t occluded;                 /* surface pixels with occ > 0 */
    uint32_t smoothed;                 /* surface pixels whose 3 x 3 window took in any pixel beyond the centre */
    uint32_t _pad;
} sar_shade_stats;
int sar_shade_params_default(sar_shade_params* out);
/* Shades rt's current buffers into rgba_out_host[width * height * 4] (k_shade on the runtime's stream, then the read-back; waits).
 * params NULL: the defaults; stats_out may be NULL. Refused (SAR_ERR_INVALID unless said otherwise): a light that is not finite or is
 * all zero; a weight, ao_strength, ao_range or smooth_range that is negative or not finite; shininess_log2 above 10; ao_radius above
 * 8; smooth or has_window other than 0 / 1; a window sar_runtime_hold_color_range would refuse; a NULL config, runtime or output; a
 * config colorize would refuse, among them one whose size is not the runtime's (SAR_ERR_DIM_MISMATCH); k = (double)width * scale not
 * finite or not positive. With timing enabled, sar_runtime_last_timing reports colorize_ms = k_shade. */
int sar_shade(const sar_config* cfg, sar_runtime* rt, const sar_shade_params* params /* NULL: defaults */,
              sar_shade_stats* stats_out /* or NULL */, uint16_t* rgba_out_host);
/* The same, leaving the image in device memory (width * height * 8 bytes); stream-ordered. With stats_out == NULL the call never
 * waits for the host; otherwise it waits once, for the statistics. */
int sar_shade_device(const sar_config* cfg, sar_runtime* rt, const sar_shade_params* params /* NULL: defaults */,
                     sar_shade_stats* stats_out /* or NULL */, void* rgba_out_dev);

/* ---- volume rendering: the hit histogram resolved along the view ray, marched front to back ------------------------------------ *
 * Gas sums every hit along a pixel's ray, Depth and shade keep the nearest one. The VOLUME keeps the histogram along the ray: D depth
 * slabs of height x width u32 voxels in device memory the runtime holds, vol[k][j][i]. It is filled by sar_runtime_volume and read by
 * sar_runtime_volume_section (slab sections: tomography), sar_runtime_volume_read and sar_runtime_volume_march (emission-absorption
 * compositing) — any number of times, with new windows and opacities, without iterating the map again. The volume is in VIEW space:
 * with the whole depth range covered its sum along the ray is render's count, and the nearest non-empty slab is the slab of
 * render's zbuf. A host restatement gives every byte below (tests/volume_restatement.py).
 *   slab       D = slabs (1 .. 1024), z_lo < z_hi finite; the host computes dscale = (double)D / (z_hi - z_lo) once. A visit with
 *              render's f32 depth zf (the value zbuf stores) has u = ((double)zf - z_lo) * dscale, a subtraction, then a
 *              multiplication. u != u: class NAN. u < 0: BELOW. u >= D: ABOVE. Otherwise its slab is k = (uint32_t)u. Render's depth
 *              test is zf > zbuf, so slab D - 1 is nearest to the viewer. +-inf depths are ABOVE / BELOW. sar_volume_slab is the host
 *              form: *k_out = k, or -1 / -2 / -3 for BELOW / ABOVE / NAN.
 *   accumulate job j starts at starts[j], runs render's 1000 uncounted warm-up steps and then iters_per_job counted iterations of
 *              render's loop body up to the visit: next_point, screen_space, the projection and the bounds test, operation for
 *              operation. NaN passes the bounds test and lands on pixel (0, 0), as in render. Every in-bounds visit is one of
 *              `visits`; one whose depth has a slab adds 1 to vol[k][j][i] (u32, wrapping as count does), the others add to below,
 *              above or nan. Everything is a sum, a max or a min: nothing depends on the launch shape or the order of the atomics.
 *   section    per pixel, count = the wrapping sum of the slabs k0 <= k < k1 and nearest = the largest non-empty k of them, or -1.
 *   march      slab k has the colour (r_k, g_k, b_k) = Palette::interpolate's clamp, blend and square roots, as colorize applies them,
 *              at v_k = pos_lo + (((double)k + 0.5) / (double)D) * (pos_hi - pos_lo). half = half_count, or where that is 0
 *              (double)vmax * 0.125, or 1.0 when vmax is 0 too. Per pixel T = 1, R = G = B = 0, seen = 0, then for k = k1 - 1 down
 *              to k0: n = vol[k][p]; n == 0: next k; otherwise seen += 1, nd = (double)n, a = nd / (nd + half), w = T * a,
 *              R = R + w * r_k (multiply, then add; likewise G, B), T = T * (1.0 - a), and if T < t_min the pixel is `stopped` and
 *              leaves the loop. With cfg->transparent a channel is R / (1.0 - T) when T < 1, else 0, and alpha is 1.0 - T; without,
 *              a channel is R + T * ((double)background[c] / 65535.0) and alpha is 1. Every value then goes through c > 0 ? c : 0,
 *              c < 1 ? c : 1 and `as u16` of c * 65535.0. All fp64 + - * / and sqrt in this order: image and statistics are the
 *              restatement's bit for bit.
 * The runtime is lent: count, steps, zbuf, max, the start-point stream, the modes and a held basin picture keep their bits. The
 * volume is held until the next add = 0 call (which reuses the allocation where it is large enough), sar_runtime_volume_free,
 * sar_runtime_set_width_height or sar_runtime_free. A refused call leaves the held volume as it was; a call that fails after
 * touching the volume leaves none held. This first accumulate is bound by the chip's rate of scattered atomics, one per stored
 * visit. Not here: a world-space volume, hue from the hits' steps, lighting, depth of field. */
typedef struct sar_volume_params {
    double   z_lo, z_hi;               /* the depth range the slabs divide; default -1, 1 */
    uint32_t slabs;                    /* D, 1 .. 1024; default 64 */
    int32_t  add;                      /* 0: zero the volume and replace it; 1: add to the held volume (same width, height, slabs and
                                          bit-equal z_lo, z_hi, or the call is refused) */
} sar_volume_params;
typedef struct sar_volume_stats {
    uint64_t visits;                   /* in-bounds visits = stored + below + above + nan */
    uint64_t stored, below, above, nan;
    uint64_t nonempty;                 /* voxels != 0 */
    uint32_t vmax;                     /* the largest voxel */
    float    z_min, z_max;             /* over the in-bounds visits with a finite depth; +inf / -inf without one; of -0.0 and +0.0
                                          either may be reported */
    uint32_t _pad;
} sar_volume_stats;
typedef struct sar_volume_march_params {
    double   half_count;               /* the count at which a voxel is half opaque; finite, >= 0; 0 (default): from vmax */
    double   t_min;                    /* the transmittance below which a ray stops; in [0, 1); default 0 */
    double   pos_lo, pos_hi;           /* palette positions of the farthest and the nearest end; finite; default 0, 1 */
    uint32_t k0, k1;                   /* the slabs marched, 0 <= k0 < k1 <= D; k1 = 0 (default) stands for D */
    uint16_t background[3];            /* r, g, b behind an opaque image; default 0, 0, 0 */
    uint16_t _pad;
} sar_volume_march_params;
typedef struct sar_volume_march_stats {
    uint64_t slabs_seen;               /* non-empty voxels the rays read before they ended */
    uint32_t covered;                  /* pixels that saw any */
    uint32_t stopped;                  /* pixels whose ray stopped at t_min */
} sar_volume_march_stats;
int sar_volume_params_default(sar_volume_params* out);
int sar_volume_march_params_default(sar_volume_march_params* out);
/* The slab of depth zf under params (host arithmetic, the device's doubles): *k_out = k, -1 (BELOW), -2 (ABOVE) or -3 (NAN). Refused:
 * NULLs and parameters sar_runtime_volume would refuse. */
int sar_volume_slab(const sar_volume_params* params, float zf, int32_t* k_out);
/* Fills the runtime's volume from n_jobs jobs of iters_per_job counted iterations each, starts_xyz_host[n_jobs][3] (k_volume_warm,
 * then k_volume_accumulate in launches of "volume_chunk" jobs by "volume_steps" iterations: a longer job continues in the next launch
 * from its point saved in device memory; neither option changes a bit of the result), then one reduction pass over the volume for
 * nonempty and vmax; waits. The two options go through sar_runtime_set_option like the ones listed there, 0 restoring the default:
 * "volume_chunk" jobs per launch (default 2^17, at most 2^24) and "volume_steps" counted iterations per job and launch (default 2^16,
 * at most 2^24); their purpose is that no single dispatch runs long on a shared card. With add = 1 the statistics are the held volume's plus this call's visit classes. params NULL: the
 * defaults. Refused (SAR_ERR_INVALID unless said otherwise): slabs outside 1 .. 1024; z_lo or z_hi not finite, z_hi - z_lo not
 * positive or dscale not finite; add other than 0 / 1; a config render would refuse, one whose size is not the runtime's among them
 * (SAR_ERR_DIM_MISMATCH); width * height * slabs above 2^30; n_jobs 0 or above 2^24; iters_per_job 0 or above 2^40; a start point
 * that is not finite; NULLs; add = 1 without a held volume of the same shape and range; no room (SAR_ERR_OOM). With timing enabled,
 * sar_runtime_last_timing reports warmup_ms = k_volume_warm and iterate_ms = k_volume_accumulate (iterate_launches = its launches). */
int sar_runtime_volume(const sar_config* cfg, sar_runtime* rt, const sar_volume_params* params /* NULL: defaults */, uint32_t n_jobs,
                       uint64_t iters_per_job, const double* starts_xyz_host, sar_volume_stats* stats_out);
/* Frees the held volume (none held: nothing to do). Waits for the stream. */
int sar_runtime_volume_free(sar_runtime* rt);
/* The section of the slabs k0 <= k < k1 of the held volume into count_out_host[width * height] and nearest_out_host[width * height]
 * (k_volume_section, then the read-back; waits); either may be NULL. Refused: no held volume, a window outside 0 <= k0 < k1 <= D.
 * With timing enabled, colorize_ms = k_volume_section. */
int sar_runtime_volume_section(sar_runtime* rt, uint32_t k0, uint32_t k1, uint32_t* count_out_host /* or NULL */,
                               int32_t* nearest_out_host /* or NULL */);
/* Copies the slabs k0 <= k < k1 themselves into out_host[(k1 - k0) * width * height]; waits. Refused as the section. */
int sar_runtime_volume_read(sar_runtime* rt, uint32_t k0, uint32_t k1, uint32_t* out_host);
/* Marches the held volume into rgba_out_host[width * height * 4] (k_volume_march on the runtime's stream, then the read-back; waits).
 * params NULL: the defaults; stats_out may be NULL. Refused: half_count negative or not finite; t_min outside [0, 1); pos_lo or
 * pos_hi not finite; a config colorize would refuse, one whose size is not the runtime's among them (SAR_ERR_DIM_MISMATCH); no held
 * volume; a window outside 0 <= k0 < k1 <= D; a NULL output. With timing enabled, colorize_ms = k_volume_march. */
int sar_runtime_volume_march(const sar_config* cfg, sar_runtime* rt, const sar_volume_march_params* params /* NULL: defaults */,
                             sar_volume_march_stats* stats_out /* or NULL */, uint16_t* rgba_out_host);
/* The same, leaving the image in device memory (width * height * 8 bytes); stream-ordered. With stats_out == NULL the call never
 * waits for the host; otherwise it waits once, for the statistics. */
int sar_runtime_volume_march_device(const sar_config* cfg, sar_runtime* rt, const sar_volume_march_params* params /* NULL: defaults */,
                                    sar_volume_march_stats* stats_out /* or NULL */, void* rgba_out_dev);

/* ---- flows: quadratic ODE systems p' = P(p), integrated by RK4 and rendered into the runtime's frame ---------------------------- *
 * Everything else here iterates the MAP p <- P(p). The same 30 coefficients read as a VECTOR FIELD p' = P(p) are Lorenz, Roessler,
 * Chen, Nose-Hoover, Sprott's flows A .. S. sar_runtime_render_flow integrates such a field and plots the trajectory into the
 * runtime's count, zbuf, steps and max, so that colorize (both kinds), auto exposure, auto colour range, sar_runtime_density,
 * sar_shade and the export work on a flow as on a map. A host restatement gives every byte below (tests/flow_restatement.py).
 *   step       classical RK4 with the fixed step h = dt; the host computes h2 = h * 0.5 and h6 = h / 6.0 once. eval(p) is next_point's
 *              polynomial, operand for operand. k1 = eval(p), k2 = eval(p + h2 * k1), k3 = eval(p + h2 * k2), k4 = eval(p + h * k3),
 *              p' = p + h6 * (((k1 + 2.0 * k2) + 2.0 * k3) + k4) per component: multiplies and adds, each its own IEEE operation,
 *              nothing fused, no division on the device. sar_flow_step is the host form.
 *   escape     after EVERY step, the transient's included: max(|x'|, |y'|, |z'|) <= bound, false for a NaN. A job that fails has
 *              escaped: the failing point is neither plotted nor counted, and the job takes no further step. (Render's rule that a
 *              NaN lands on pixel (0, 0) is NOT carried over.) Start points are not tested.
 *   plotting   job j runs `transient` uncounted steps, then steps_per_job counted ones; counted step t = 0, 1, .. is plotted where
 *              (t + 1) % stride == 0. A plotted point goes through render's screen_space, projection and bounds test
 *              (src/lib.rs:773-802) with render's f32 depth zf + 0.0f. Inside the image it is a VISIT: count[pix] += 1 (u32, wrapping
 *              as render's). Outside it is one of `outside`.
 *   depth, hue the key of a visit is (sortable(zf) << 32) | sortable((float)c), sortable() the order-preserving u32 image of an f32,
 *              c = color_transform(d) of render's colour transform with d = p' - p, the displacement of this ONE RK4 step (not the
 *              distance to the previous plotted point): under AdjustedVelocity the hue is speed * h. The LARGEST key of a pixel
 *              wins: the nearest depth, and among visits of exactly that depth the largest (float)c. This tie rule is the flow's own
 *              — render lets the earliest visit win — and makes the result independent of the order of the visits by construction;
 *              its price is a hue rounded to f32. A visit whose zf is NaN is counted and offers no key. After the last step a pixel
 *              with a key whose depth passes render's strict test zf > zbuf[pix] (against what the frame held before the call: an
 *              earlier render's depth, or the sentinel -1) takes zbuf[pix] = zf and steps[pix] = (double)(float)c. max becomes the
 *              larger of itself and the largest count.
 *   launches   one lane per job, the job's point in device memory between launches of chunk_jobs jobs by chunk_steps steps; their
 *              purpose is that no single dispatch runs long on a shared card. A lane merges consecutive visits of one pixel into a
 *              run and sends ONE atomic add per run: when the pixel changes, when a plotted point is outside, at the end of a launch.
 *              count_atomics counts those. key_atomics counts the runs that held a visit with a depth: the key raises OFFERED — a
 *              relaxed load spares the atomic max where the key can no longer win, and how often that happens depends on timing and
 *              is not reported. Neither chunk changes a bit of the frame or any other statistic; the two counters are exact for a
 *              given pair.
 * The call ACCUMULATES onto an un-reset runtime, on top of an earlier sar_render* or sar_runtime_render_flow, and leaves the runtime
 * as sar_runtime_load leaves it (the depth hints cleared), so a render call may follow. With plot = 0 nothing of the frame is
 * written: the statistics alone (the extent, for framing a view) — visits and outside as with plot = 1, the two atomics counters 0.
 * Not here: adaptive or other integrators, non-autonomous or non-quadratic fields, Lyapunov spectra of flows, line segments between
 * plotted points, an LDS-binned accumulate. Poincare sections are sar_runtime_section's, below. */
typedef struct sar_flow_params {
    double   dt;                       /* the step h; finite, > 0; default 0.01 */
    double   bound;                    /* finite, > 0; default 1e6 */
    uint32_t transient;                /* uncounted steps first; default 1000 */
    uint32_t stride;                   /* every stride-th counted step is plotted; >= 1; default 1 */
    int32_t  plot;                     /* 1 (default); 0: measure only, the frame untouched */
    uint32_t chunk_jobs;               /* jobs per launch, at most 2^24; 0 (default): 2^17 */
    uint32_t chunk_steps;              /* steps per job and launch, at most 2^24; 0 (default): 2^12 */
    uint32_t _pad;
} sar_flow_params;
typedef struct sar_flow_stats {
    uint64_t steps;                    /* counted steps whose point stayed within the bound */
    uint64_t visits, outside;          /* plotted points inside / outside the image */
    uint64_t escaped_transient;        /* jobs that escaped during the transient */
    uint64_t escaped;                  /* jobs that escaped during the counted steps */
    uint64_t alive;                    /* n_jobs less the two */
    uint64_t count_atomics, key_atomics;
    double   extent[6];                /* xmin, xmax, ymin, ymax, zmin, zmax of the counted points (plotted or not), raw coordinates:
                                          what sar_frame_view_box takes; +inf, -inf without one */
    uint32_t max;                      /* the runtime's max after the call */
    uint32_t _pad;
} sar_flow_stats;
int sar_flow_params_default(sar_flow_params* out);
/* One RK4 step of cfg's field from xyz, in place, on the host in the device's arithmetic; *within_out (or NULL) = 1 where the new point
 * passes the bound test, else 0 (the failing point is left in xyz). Uses params' dt and bound only; params NULL: the defaults.
 * Refused: a NULL config or point, a config render would refuse, dt or bound not finite or not positive. No device needed. */
int sar_flow_step(const sar_config* cfg, const sar_flow_params* params /* NULL: defaults */, double xyz[3], int32_t* within_out /* or NULL */);
/* Integrates n_jobs trajectories of cfg's field from starts_xyz_host[n_jobs][3] and plots them into rt's frame in cfg's view
 * (k_flow_transient, k_flow_render, then k_flow_resolve once); waits. Refused (SAR_ERR_INVALID unless said otherwise), the frame left as
 * it was: dt or bound not finite or not positive; stride 0; plot other than 0 / 1; chunk_jobs or chunk_steps above 2^24; a config render
 * would refuse, one whose size is not the runtime's among them (SAR_ERR_DIM_MISMATCH); n_jobs 0; steps_per_job / stride above 2^32 - 1
 * (what one job may add to a pixel); a start point that is not finite; NULLs; no room (SAR_ERR_OOM). With timing enabled,
 * sar_runtime_last_timing reports warmup_ms = k_flow_transient, iterate_ms = k_flow_render (iterate_launches = its launches) and
 * colorize_ms = k_flow_resolve. */
int sar_runtime_render_flow(const sar_config* cfg, sar_runtime* rt, const sar_flow_params* params /* NULL: defaults */, uint32_t n_jobs,
                            uint64_t steps_per_job, const double* starts_xyz_host, sar_flow_stats* stats_out);

/* ---- Poincare sections of flows: the crossings of a trajectory with a surface, refined by Henon's step ---------------------------- *
 * A section turns a flow into a map, the first-return map: sar_runtime_section integrates cfg's field as sar_runtime_render_flow does
 * and records where the trajectories cross a surface g = 0, with the time between consecutive crossings. The recorded crossings of a
 * job are a point set of the shape sar_runtime_pairs, sar_runtime_boxes, sar_runtime_spectra and sar_runtime_recurrence take; with
 * plot = 1 they are also plotted into the runtime's frame, the hue their return time. A host restatement gives every bit below
 * (tests/section_restatement.py).
 *   surface    g(p) = s . [1, x, x^2, xy, xz, y, y^2, yz, z, z^2]: ten doubles in the coefficient rows' monomial order, summed as
 *              next_point sums a row: g = s0, then g = g + t[k] * s[k + 1], left to right. A plane n . p = d is
 *              s = (-d, nx, 0, 0, 0, ny, 0, 0, nz, 0). Row a of the field itself is the surface p_a' = 0, the extrema of coordinate
 *              a: Lorenz's map of successive maxima of z is surface = the field's z row, direction = -1.
 *   crossing   side(p) = (g(p) >= 0). Counted step t = 0, 1, .. takes p0 -> p1 by flows' RK4 step. Where p1 fails flows' bound test
 *              the job has escaped: the failing point is dropped and no crossing is looked for in that step. Otherwise, with
 *              g0 = g(p0) and g1 = g(p1): an up-crossing is !side(p0) && side(p1), a down-crossing side(p0) && !side(p1), either
 *              only where g0 and g1 are both finite. direction +1 takes up-crossings, -1 down-crossings, 0 both. A point exactly
 *              on the surface is on the side g >= 0.
 *   refinement Henon 1982: with g as the independent variable, dp/dg = P(p) * w and dt/dg = w, w = 1.0 / gdot,
 *              gdot = (gx * Px + gy * Py) + gz * Pz, gx = ((s1 + d2 * x) + s3 * y) + s4 * z, gy = ((s5 + s3 * x) + d6 * y) + s7 * z,
 *              gz = ((s8 + s4 * x) + s7 * y) + d9 * z, d2 = 2 * s2, d6 = 2 * s6, d9 = 2 * s9 doubled on the host (exact). ONE classical
 *              RK4 step of these four components from (p0, t = 0) with the step D = -g0, D2 = D * 0.5, D6 = D / 6.0, in the flow
 *              step's operand order — k1 = F(p0), k2 = F(p0 + D2 * k1), k3 = F(p0 + D2 * k2), k4 = F(p0 + D * k3),
 *              q = p0 + D6 * (((k1 + 2.0 * k2) + 2.0 * k3) + k4) per component, dt = 0.0 + D6 * (the same sum of the fourth
 *              components) — gives the crossing q and the time dt from p0 to it. Every operation is its own IEEE operation, nothing
 *              fused; the five divisions are correctly rounded. It is accepted where 0 <= dt && dt <= h and q passes the bound
 *              test (both false for a NaN). Otherwise the crossing is ROUGH: theta = g0 / (g0 - g1), q = p0 + theta * (p1 - p0),
 *              dt = theta * h. The limit: one Henon step leaves a residual |g(q)| of rounding size for a plane and of O(D^5) for a
 *              quadric, and a crossing is only ever as good as the RK4 trajectory it lies on; residual_max reports the largest.
 *   clock      a job runs `transient` uncounted steps (flows' transient), then at most max_steps counted ones. Its first qualifying
 *              crossing after the transient is the CLOCK crossing: it sets (t_prev, dt_prev) and is not recorded. Every later one is
 *              recorded, until the job holds `samples` of them and stops. A recorded crossing of counted step t stores q and the
 *              return time r = ((double)(t - t_prev) * h + dt) - dt_prev, and then becomes the previous crossing. No accumulated
 *              time is kept anywhere: r does not depend on how the steps are cut into launches.
 *   picture    with plot = 1 every recorded crossing goes through render's projection and bounds test in cfg's view: inside the
 *              image it is one of `visits` and count[pix] += 1, outside one of `outside`. Its key is
 *              (sortable(zf + 0.0f) << 32) | sortable((float)r); the largest key of a pixel wins and a NaN depth offers no key
 *              (flows' rule), and flows' resolve then writes zbuf, steps = (double)(float)r and max. The call accumulates onto an
 *              un-reset runtime and clears the depth hints, as sar_runtime_render_flow does. A section seen face-on is all one
 *              depth, so the tie rule decides every pixel and the hue is the return time: sar_runtime_set_color_range spreads it
 *              over the palette. With plot = 0 the frame keeps its bits, and visits and outside are 0.
 * Not here: Lyapunov spectra of flows; sections in sar_render_sequence, sar_render_parallel, the gallery and the volume; a second
 * refinement step; non-quadratic surfaces; plotting arbitrary point sets; an LDS-binned plot. */
#define SAR_SECTION_FULL              0   /* the job holds `samples` recorded crossings */
#define SAR_SECTION_SHORT             1   /* max_steps ran out first */
#define SAR_SECTION_ESCAPED           2   /* it escaped during the counted steps; what it found before stays */
#define SAR_SECTION_ESCAPED_TRANSIENT 3   /* it escaped during the transient */
#define SAR_SECTION_NO_CLOCK 0xFFFFFFFFu  /* clock_step of a job without a clock crossing */
typedef struct sar_section_params {
    double   surface[10];              /* s; every entry finite, s1 .. s9 not all zero; sar_section_params_default leaves it zero */
    double   dt;                       /* the step h; finite, > 0; default 0.01 */
    double   bound;                    /* finite, > 0; default 1e6 */
    uint32_t transient;                /* uncounted steps first; default 1000 */
    int32_t  direction;                /* +1 (default) up-crossings, -1 down-crossings, 0 both */
    uint32_t samples;                  /* recorded crossings per job, 1 .. 2^20; default 1024 */
    uint32_t max_steps;                /* counted steps per job at most, 1 .. 2^32 - 1; default 2^20 */
    int32_t  plot;                     /* 0 (default); 1: the recorded crossings also go into the runtime's frame */
    uint32_t chunk_jobs;               /* jobs per launch, at most 2^24; 0 (default): flows' 2^17 */
    uint32_t chunk_steps;              /* steps per job and launch, at most 2^24; 0 (default): flows' 2^12 */
    uint32_t _pad;
} sar_section_params;
typedef struct sar_section_record {
    uint32_t status;                   /* SAR_SECTION_* */
    uint32_t found;                    /* recorded crossings */
    uint32_t rough;                    /* those of them that are rough */
    uint32_t steps;                    /* counted steps taken, the one of the last recorded crossing included, an escaping one not */
    uint32_t clock_step;               /* the counted step of the clock crossing; SAR_SECTION_NO_CLOCK without one */
    uint32_t _pad;
} sar_section_record;
typedef struct sar_section_stats {
    uint64_t steps;                    /* the records' steps, summed */
    uint64_t crossings, rough;         /* the records' found and rough, summed */
    uint64_t clocked;                  /* jobs with a clock crossing */
    uint64_t full, short_jobs, escaped, escaped_transient;   /* jobs by status */
    uint64_t visits, outside;          /* plot = 1: recorded crossings inside / outside the image */
    double   extent[6];                /* xmin, xmax, ymin, ymax, zmin, zmax of the recorded q, raw coordinates: what sar_frame_view_box
                                          takes; +inf, -inf without one */
    double   ret_min, ret_max;         /* of the recorded return times; +inf, -inf without one */
    double   residual_max;             /* the largest |g(q)| of a recorded crossing, g summed as above; 0 without one */
    uint32_t max;                      /* the runtime's max after the call */
    uint32_t _pad;
} sar_section_stats;
int sar_section_params_default(sar_section_params* out);
/* One counted step on the host in the device's arithmetic: xyz is p0 on entry and p1 on return; *kind_out = 0 no crossing, 1 a
 * crossing refined by Henon's step, 2 a rough one, -1 escaped (the failing point is left in xyz). On 1 and 2 crossing[3] takes q and
 * *dt_out the time from p0 to it; otherwise both are left alone. crossing, dt_out and kind_out may each be NULL. Uses params' surface,
 * dt, bound and direction only. Refused: a NULL config, parameters or point, a config render would refuse, a surface entry that is not
 * finite or s1 .. s9 all zero, dt or bound not finite or not positive, a direction other than +1, -1, 0. No device needed. */
int sar_section_step(const sar_config* cfg, const sar_section_params* params, double xyz[3] /* p0 in, p1 out */, double crossing[3],
                     double* dt_out, int32_t* kind_out);
/* The section of n_jobs trajectories of cfg's field from starts_xyz_host[n_jobs][3] (k_flow_transient, k_flow_section, with plot = 1
 * k_section_plot and k_flow_resolve); waits. points_out[n_jobs][samples][3] takes the recorded crossings, ret_out[n_jobs][samples]
 * their return times — unfilled entries are NaN —, records_out[n_jobs] the jobs' records. Jobs run in chunks of chunk_jobs, each
 * chunk's counted steps in launches of chunk_steps, and a chunk's outputs are copied out before the next begins: device memory is
 * bounded by chunk_jobs * samples. Neither chunk changes a bit of any output. Refused (SAR_ERR_INVALID unless said otherwise), the
 * frame left as it was: a surface entry that is not finite; s1 .. s9 all zero; dt or bound not finite or not positive; a direction
 * other than +1, -1, 0; plot other than 0 / 1; samples 0 or above 2^20; max_steps 0; chunk_jobs or chunk_steps above 2^24; n_jobs 0;
 * n_jobs * samples above 2^24; a start point that is not finite; a config render would refuse, one whose size is not the runtime's
 * among them (SAR_ERR_DIM_MISMATCH); NULLs (params included: there is no default surface); no room (SAR_ERR_OOM). With timing enabled,
 * sar_runtime_last_timing reports warmup_ms = k_flow_transient, iterate_ms = k_flow_section (iterate_launches = its launches) and
 * colorize_ms = k_flow_resolve; k_section_plot is not booked. */
int sar_runtime_section(const sar_config* cfg, sar_runtime* rt, const sar_section_params* params, uint32_t n_jobs,
                        const double* starts_xyz_host, double* points_out, double* ret_out, sar_section_record* records_out,
                        sar_section_stats* stats_out);

/* ---- gallery: many maps rendered as small tiles of one atlas, in one call ------------------------------------------------------ *
 * What the search found, seen: tile i is an ordinary small render — what the library gives for cfg_i = *base with item i's
 * coefficients, center_camera and scale, width / height the tile's, iterations = p->iterations and jobs_total = p->jobs; everything
 * else (palette, brightness constants, colour transform, render kind, transparent, rotation, angle) is base's. Its count, zbuf,
 * steps, max and RGBA16 are those of a fresh runtime, sar_render_jobs(cfg_i, rt, starts) and sar_colorize(cfg_i, rt), bit for bit:
 * the warm-up of 1000 steps with its dropped trajectories, job-major depth ties, the colour transform at the winner, the ln table,
 * Gas and Depth (with the tile's own z range). One workgroup renders one tile with its image in the CU's LDS (k_gallery): no visit
 * is scattered to device memory, which is what limits a tile to 16 384 pixels. */
typedef struct sar_gallery_item {     /* what differs from tile to tile */
    double coeff[30];                 /* x, y, z rows of 10, as sar_search_candidate */
    double center_camera[3];
    double scale;
} sar_gallery_item;
typedef struct sar_gallery_params {
    uint32_t tile_width, tile_height; /* 1 .. , tile_width * tile_height <= 16384 */
    uint32_t cols;                    /* tiles per atlas row, >= 1 */
    uint32_t jobs;                    /* trajectories per tile */
    uint64_t iterations;              /* per tile; iterations per job = iterations / jobs (floor), as sar_render_jobs */
    uint64_t seed;                    /* start points = sar_start_points(seed, 0, jobs) when starts == NULL */
} sar_gallery_params;
typedef struct sar_gallery_stats {    /* one per tile */
    uint32_t max;                     /* Runtime::max of the tile */
    uint32_t covered;                 /* pixels with count > 0 */
    uint64_t hits;                    /* sum of count (visits that landed in the tile) */
    uint32_t dead_jobs;               /* trajectories dropped in the warm-up: x not finite after it (they left for infinity) */
    uint32_t _pad;
} sar_gallery_stats;
/* 128 x 128 tiles, 8 per row, 1024 jobs, 2^20 iterations, seed 0. */
int sar_gallery_params_default(sar_gallery_params* out);
/* n tiles into an atlas of cols * tile_width by ceil(n / cols) * tile_height pixels (RGBA16, row-major): tile i at column i % cols,
 * row i / cols; the cells of a last row that hold no tile are all-zero pixels. Every tile runs the same start points
 * (starts_xyz_host: jobs * 3 doubles, or NULL for the stream of p->seed). count / zbuf / steps_out_host (each [n][tile_height]
 * [tile_width], tile-major, or NULL) receive the raw tiles — sar_runtime_load takes one, for sar_runtime_exposure /
 * sar_runtime_color_range on it — and stats_out_host ([n] or NULL) every tile's scalars. Runs on the runtime's device and stream in
 * chunks ("gallery_chunk" option, default 512 tiles per launch: bounds the raw scratch, results do not depend on it); the runtime's
 * image buffers, start-point stream and exposure / colour-range modes are neither read nor changed: tiles are colorized with base's
 * constants. With timing enabled, sar_runtime_last_timing reports iterate_ms = k_gallery (iterate_launches = its launches).
 * Refused (SAR_ERR_INVALID): a zero tile side or more than 16 384 pixels per tile, cols == 0, jobs == 0,
 * jobs * (iterations / jobs) >= 2^32 (the visit ordinal is 32 bits, as in the frame path), an invalid base, items_host == NULL
 * with n > 0. n == 0 succeeds and writes nothing. */
int sar_runtime_gallery(sar_runtime* rt, const sar_config* base, const sar_gallery_params* p,
                        uint32_t n, const sar_gallery_item* items_host, const double* starts_xyz_host /* [jobs*3] or NULL */,
                        uint16_t* atlas_rgba16_out_host,
                        uint32_t* count_out_host, float* zbuf_out_host, double* steps_out_host, /* each [n][th][tw], or NULL */
                        sar_gallery_stats* stats_out_host /* [n] or NULL */);
/* sar_frame_view from a RAW bounding box (xmin,xmax,ymin,ymax,zmin,zmax of the map's own coordinates: what sar_search_record.extent
 * and out12[6..12) of sar_runtime_extent hold), so that a search result is framed without another pass over the map. Host
 * arithmetic: the box's 8 corners go through cfg's rotation (sar_rotation_matrix, applied as sar_runtime_extent applies it), their
 * componentwise min / max is the screen-space extent handed to sar_frame_view(cfg, ., margin, sweep). Conservative: the rotated box
 * bounds the rotated attractor, so the view is never too tight and usually a little loose. */
int sar_frame_view_box(sar_config* cfg, const double raw_extent6[6], double margin, int sweep);

/* ---- orbit diagrams: where a map family settles, along a line in coefficient space ---------------------------------------------- *
 * The orbit (bifurcation) diagram of the line from map a to map b (30 coefficients each: the x, y, z rows of sar_search_candidate).
 * Column c of `width` is the map with
 *   coeff_k = a_k + (b_k - a_k) * t,  t = (double)c / (double)(width - 1)                                  (0 when width == 1)
 * (b_k - a_k computed once, a multiply then an add, no FMA), each one then through `0. + 1. * c` as the search and the planes do:
 * sar_orbit_coeffs gives the device's doubles. An entry with b_k == a_k stays exactly a_k; a single-axis sweep is b == a but for
 * one entry, a family whose entries move together (the logistic x' = r x - r x^2: entries 1 and 2 of the x row) moves several.
 * Every column runs the same `jobs` trajectories (start points starts_xyz_host[jobs * 3], or sar_start_points(seed, 0, jobs) when
 * that is NULL): several per column let coexisting attractors show in one column. A job's life:
 *   transient   `transient` steps of next_point; the first point outside the bound box — !(|x|, |y|, |z| <= bound), NaN included, the
 *               planes' test — kills the job (dead_transient).
 *   steps       `steps` steps, each advancing the point first. A point outside the box kills the job (dead_late): that step and all
 *               later ones contribute nothing, earlier visits stay. Otherwise the visit is live, with the plotted value
 *               v = (proj[0] * x + proj[1] * y) + proj[2] * z (left to right, no FMA) and u = (v - v_lo) * scale (a subtract, then a
 *               multiply), scale = (double)height / (v_hi - v_lo) computed once on the host.
 *   hit         u >= 0 && u < (double)height: count[(height - 1 - (uint32_t)u) * width + c] += 1 — row 0 is the high end, as in a
 *               plot. Any other live visit (NaN u included) is a miss.
 *   vmin, vmax  of the column move on every live visit, hit or miss, through `<` / `>` only (a NaN v never moves one).
 * Everything is a sum or a minimum / maximum over the visits: the result does not depend on the launch shape, on "orbit_chunk" or on
 * the order of the atomics (vmin / vmax as values: of -0.0 and +0.0, which compare equal, either may be reported). The map, v and u
 * are multiplies and adds only, so a host restatement gives the same counts bit for bit. */
typedef struct sar_orbit_params {
    double   a[30], b[30];        /* the ends of the line (default all 0) */
    uint32_t width, height;       /* columns 1..65536, bins 1..32768: a column's histogram lives in LDS (default 1024 x 512) */
    uint32_t jobs;                /* trajectories per column, 1..1024 (default 256) */
    uint32_t transient, steps;    /* default 1000, 4096; each <= 2^31, jobs * steps < 2^32 (a bin is 32 bits) */
    uint32_t _pad;
    uint64_t seed;                /* start points = sar_start_points(seed, 0, jobs) when starts == NULL (default 0) */
    double   bound;               /* default 1e6; finite and positive */
    double   proj[3];             /* default 1, 0, 0: the diagram plots x */
    double   v_lo, v_hi;          /* the plotted range, finite, v_lo < v_hi (default -1, 1) */
} sar_orbit_params;
typedef struct sar_orbit_column {     /* one per column */
    uint32_t dead_transient, dead_late, alive;   /* jobs by fate: they sum to `jobs` */
    uint32_t occupied;                /* bins > 0 */
    uint32_t max;                     /* the column's largest bin */
    uint32_t _pad;
    uint64_t hits, misses;            /* live visits inside / outside [v_lo, v_hi) */
    double   vmin, vmax;              /* of v over the live visits; +inf / -inf without one */
} sar_orbit_column;
int sar_orbit_params_default(sar_orbit_params* out);
/* Column `column`'s 30 coefficients (host arithmetic, identical to the device's; no device needed). */
int sar_orbit_coeffs(const sar_orbit_params* p, uint32_t column, double out30[30]);
/* The diagram on the runtime's device and stream: one workgroup per column (k_orbit, "orbit_chunk" columns per launch), the column's
 * histogram in LDS, every visit one LDS add. count_out_host[height][width] (row-major); *max_out the largest bin of the whole
 * diagram and stats_out_host[width] every column's scalars (either may be NULL). The runtime lends its device, stream and timing
 * spans: its image buffers, start-point stream and exposure / colour-range modes are neither read nor changed. With timing enabled,
 * sar_runtime_last_timing reports iterate_ms = k_orbit (iterate_launches = its launches). Refused (SAR_ERR_INVALID): a zero width or
 * height, a width above 65536 or a height above 32768, jobs 0 or above 1024, jobs * steps >= 2^32, transient or steps above 2^31, an
 * a, b, proj, v_lo, v_hi or bound that is not finite, bound <= 0, v_lo >= v_hi, a scale that is not finite. */
int sar_runtime_orbit(sar_runtime* rt, const sar_orbit_params* p, const double* starts_xyz_host /* [jobs*3] or NULL */,
                      uint32_t* count_out_host /* [height][width] */, sar_orbit_column* stats_out_host /* [width] or NULL */,
                      uint32_t* max_out /* or NULL */);

/* ---- correlation dimension: exact pair-distance histograms of point sets and of maps' attractors --------------------------------- *
 * The measured counterpart of the Kaplan-Yorke dimension (Grassberger & Procaccia): D2 is the slope of ln C(r) against ln r, C(r)
 * the share of point pairs closer than r. The device counts, exactly; the slope is host arithmetic on the counts.
 *   sets       n_sets sets of n points, doubles [set][n][3]. Point i belongs to trajectory i / samples and is its sample i % samples
 *              (samples divides n; samples == 0 in sar_pairs_params stands for n: one trajectory).
 *   pairs      every unordered pair i < j of one set is counted once, except a pair of the SAME trajectory with j - i <= theiler
 *              (the Theiler window, default 0), which is skipped.
 *   distance   r2 = (dx * dx + dy * dy) + dz * dz with dx = x_j - x_i, dy, dz alike: subtracts, multiplies and adds in that order,
 *              no FMA. (r2 is never negative; with infinite coordinates it may be NaN, whose sign bit is ignored below.)
 *   key        with s = sub_bits (0..4): key = ((bits(r2) & ~sign) >> (52 - s)) - ((1023 + e_min) << s), as a signed value;
 *              bin = 0 for key < 0 (underflow: r2 == 0 and everything below 2^e_min, subnormals included);
 *              bin = key + 1 for 0 <= key < (e_max - e_min) << s; bin = bins - 1 otherwise (overflow: r2 >= 2^e_max, inf, NaN);
 *              bins = ((e_max - e_min) << s) + 2. No logarithm runs anywhere: a bin is the exponent and the top s mantissa bits of
 *              r2, so bins are piecewise linear within a binade of r2.
 *   edges      the upper edge of bin b < bins - 1 is r2_b = (1 + m / 2^s) * 2^(e_min + e), (e, m) the quotient and remainder of b
 *              by 2^s — exact in a double; bin b holds r2_(b-1) <= r2 < r2_b. sar_pairs_edges gives r_b = sqrt(r2_b), and +inf for
 *              the overflow bin.
 *   output     hist[set][bins] as uint64, and per set the pairs counted (the sum of its histogram) and skipped by the window:
 *              counted + skipped = n (n - 1) / 2.
 * Every result is a sum of integers (or, below, a minimum / maximum): nothing depends on the launch shape, on "corr_chunk" or on the
 * order of the atomics, and a host restatement gives the same integers bit for bit.
 * Limits (SAR_ERR_INVALID otherwise): 1 <= n <= 2^20, samples dividing n, sub_bits <= 4, -1022 <= e_min < e_max <= 1023,
 * bins <= 1024, no NaN coordinate anywhere (infinities are taken). */
typedef struct sar_pairs_params {
    uint32_t samples;                 /* points per trajectory; 0 = n (default 0) */
    uint32_t theiler;                 /* default 0 */
    uint32_t sub_bits;                /* s, default 2 */
    int32_t  e_min, e_max;            /* default -64, 8: 290 bins */
    uint32_t _pad;
} sar_pairs_params;
typedef struct sar_pairs_counts {     /* one per set */
    uint64_t counted, skipped;
} sar_pairs_counts;
int sar_pairs_params_default(sar_pairs_params* out);
/* *bins_out = the number of bins of p's binning (p NULL: the defaults') and, with r_out != NULL, r_out[b] = r_b for every bin
 * ([bins]; the last is +inf). Host arithmetic; refuses what sar_runtime_pairs refuses of sub_bits, e_min, e_max. */
int sar_pairs_edges(const sar_pairs_params* p, uint32_t* bins_out, double* r_out);
/* The pair histograms of n_sets caller-supplied sets on the runtime's device and stream (k_corr_pairs: one workgroup per pair of
 * 256-point tiles I <= J of a set, "corr_chunk" workgroups per launch; sets beyond 2^24 points of device memory go in groups).
 * hist_out_host[n_sets][bins]; counts_out_host[n_sets] or NULL. p NULL: the defaults. n_sets == 0 succeeds and writes nothing.
 * The runtime lends its device, stream and timing spans: its image buffers, start-point stream and modes are neither read nor
 * changed. With timing enabled, sar_runtime_last_timing reports iterate_ms = k_corr_pairs (iterate_launches = its launches). */
int sar_runtime_pairs(sar_runtime* rt, const sar_pairs_params* p, uint32_t n_sets, uint32_t n, const double* points_host /* [n_sets][n][3] */,
                      uint64_t* hist_out_host /* [n_sets][bins] */, sar_pairs_counts* counts_out_host /* [n_sets] or NULL */);

/* The least-squares line of ln C against ln r over a window of one histogram: host arithmetic only, no device.
 *   C_b      the cumulative count through bin b, the underflow bin included.
 *   window   the bins b in 1 .. bins - 2 with C_b >= c_lo and r_b <= r_hi (contiguous: both grow with b).
 *   line     ordinary least squares of y_b = ln C_b on x_b = 0.5 * ln r2_b over the window, in bin order: the means of x and y, then
 *            slope = sum (x - mx)(y - my) / sum (x - mx)^2, intercept = my - slope * mx, rms = sqrt(sum (y - intercept - slope x)^2 / k).
 *            slope is the correlation dimension D2. rms says how straight the window is; it is not an error bar of D2.
 *   status   SAR_CORRDIM_NO_WINDOW with NaN slope, intercept and rms where the window holds fewer than three bins.
 * Refused: c_lo not >= 1, r_hi not > 0 (+inf is taken: no upper limit), a binning sar_pairs_edges refuses. */
enum { SAR_CORRDIM_FIT_OK = 0, SAR_CORRDIM_NO_WINDOW = 1 };
typedef struct sar_corrdim_line {
    double   slope, intercept, rms;
    uint32_t first_bin, last_bin;     /* the window's ends; 0, 0 without a window */
    uint32_t used;                    /* bins in the window */
    int32_t  status;
} sar_corrdim_line;
int sar_corrdim_fit(const uint64_t* hist /* [bins] */, const sar_pairs_params* binning /* or NULL */, double c_lo, double r_hi,
                    sar_corrdim_line* out);

/* The same for maps: n_maps coefficient sets [n_maps][30] in the search's row order (x, y, z rows of 10), each coefficient through
 * `0. + 1. * c` as everywhere — sar_search_candidate's output goes in as it is. Every map runs the same `jobs` start points
 * (starts_xyz_host[jobs * 3], or sar_start_points(seed, 0, jobs) when that is NULL). A job runs `transient` steps of next_point, then
 * `samples` times `stride` steps and a recorded point: n = jobs * samples points per map, point job * samples + sample, so a job is
 * a trajectory of the Theiler window. Steps are numbered from 1, the transient included.
 *   status   a point outside the bound box — !(|x|, |y|, |z| <= bound), NaN included, the planes' test — at any step of any job makes
 *            the map SAR_SEARCH_DIVERGED: fail_job is the lowest job that left the box and fail_step the step at which it did; its
 *            histogram is all zero, counted = skipped = 0, its extent is (+inf, -inf) three times, its line has no window and its
 *            returned points are all zero. Otherwise the map is SAR_SEARCH_BOUNDED with fail_job = fail_step = 0.
 *   extent   xmin, xmax, ymin, ymax, zmin, zmax of the recorded points, through `<` / `>` only, as sar_runtime_extent (as values: of
 *            -0.0 and +0.0 the smaller is -0.0).
 *   line     sar_corrdim_fit of the map's histogram with c_lo = p->c_lo and r_hi = p->r_hi_fraction * the extent's diagonal,
 *            sqrt((dx * dx + dy * dy) + dz * dz) of its three spans; r_hi is in the record.
 * points_out_host ([n_maps][n][3], or NULL) receives the recorded points: sar_runtime_pairs on them, with samples and theiler as
 * here, gives the same histograms. hist_out_host[n_maps][bins]; records_out_host[n_maps]. Runs on the runtime's device and stream
 * (k_corr_orbit: one lane per map and job; then k_corr_pairs), chunked by "corr_chunk"; maps beyond 2^24 points of device memory
 * go in groups. The runtime is lent as to sar_runtime_pairs. With timing enabled, sar_runtime_last_timing reports warmup_ms =
 * k_corr_orbit and iterate_ms = k_corr_pairs (iterate_launches = the latter's launches).
 * Refused (SAR_ERR_INVALID): jobs 0 or above 2^16, samples or stride 0, n = jobs * samples above 2^20, transient or
 * stride * samples above 2^31, a bound that is not positive and finite, a coefficient or start coordinate that is not finite, c_lo
 * not >= 1, r_hi_fraction not > 0, and what sar_runtime_pairs refuses of the binning. n_maps == 0 succeeds and writes nothing. */
typedef struct sar_corrdim_params {
    uint32_t jobs, samples;           /* default 256, 128: 32768 points */
    uint32_t stride, transient;       /* default 4, 1000 */
    uint32_t theiler;                 /* default 0 */
    uint32_t sub_bits;                /* default 2 */
    int32_t  e_min, e_max;            /* default -64, 8 */
    uint64_t seed;                    /* start points = sar_start_points(seed, 0, jobs) when starts == NULL (default 0) */
    double   bound;                   /* default 1e6 */
    double   c_lo;                    /* default 100 pairs */
    double   r_hi_fraction;           /* default 2^-4 of the extent's diagonal */
} sar_corrdim_params;
typedef struct sar_corrdim_record {   /* one per map */
    int32_t  status;                  /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t fail_job;
    uint64_t fail_step;
    uint64_t counted, skipped;
    double   extent[6];
    double   r_hi;                    /* the window's upper limit; NaN for a DIVERGED map */
    sar_corrdim_line line;            /* line.slope is D2 */
} sar_corrdim_record;
int sar_corrdim_params_default(sar_corrdim_params* out);
int sar_runtime_corrdim(sar_runtime* rt, const sar_corrdim_params* p, uint32_t n_maps, const double* coeffs_host /* [n_maps][30] */,
                        const double* starts_xyz_host /* [jobs*3] or NULL */, uint64_t* hist_out_host /* [n_maps][bins] */,
                        sar_corrdim_record* records_out_host /* [n_maps] */, double* points_out_host /* [n_maps][n][3] or NULL */);

/* ---- box counting: the dimensions D0, D1, D2 of point sets and of maps' attractors from exact cell counts ----------------------------- *
 * The start of the Renyi spectrum from boxes of edge eps: the capacity dimension D0 from the number of occupied boxes, the
 * information dimension D1 (what the Kaplan-Yorke conjecture speaks about) from the entropy of their occupancies, and the box form
 * of the correlation dimension D2 from the sum of their squares. O(n * levels), where the pair histogram is O(n^2). The device counts,
 * exactly, at levels + 1 scales at once; the three slopes are host arithmetic on the counts.
 *   box        a cube: origin[3] and size. L = levels (1..16) halvings: the edge at level l (0..L) is size * 2^-l; level 0 is the cube.
 *   cell       scale = (double)(1u << L) / size, computed once on the host. For a coordinate p on axis k: u = (p - origin_k) * scale
 *              (a subtract, then a multiply, no FMA); c_k = !(u >= 0) ? 0 : (u >= 2^L ? 2^L - 1 : (uint32_t)u) — points outside the
 *              cube fall into its border cells, infinities included. The cell of a point at level l is (c_x, c_y, c_z) >> (L - l).
 *   level      per set and level one sar_box_level over the occupied cells, n_i the points in cell i: the cells, those with n_i = 1,
 *              the sum of n_i^2 and the sum of n_i * lg32(n_i). The n_i of a level sum to n; level 0 is (1, n == 1, n^2, n lg32(n)).
 *   lg32       log2(n) in fixed point with 32 fraction bits, truncated, in integers only: e = the index of n's top bit,
 *              y = n << (63 - e); 32 times y = (y * y) >> 63 through the 128-bit product, the next fraction bit is whether that
 *              reached 2^64, and y is halved when it did; lg32 = (e << 32) | fraction. No logarithm runs on the device.
 *              sar_box_log2_q32 is the host form.
 * Every result is a sum of integers: nothing depends on the launch shape, on "box_chunk", on "box_slots" or on the order of the
 * atomics, and a host restatement gives the same integers bit for bit.
 * Limits (SAR_ERR_INVALID otherwise): 1 <= n <= 2^20 — with which every sum fits 64 bits: sum_sq <= n^2 <= 2^40 and
 * n_log_n <= n lg32(n) <= 2^20 * 20 * 2^32 < 2^57 —, 1 <= levels <= 16, an origin that is finite, a size that is finite and
 * positive with a finite scale, no NaN coordinate anywhere (infinities are taken). */
typedef struct sar_box_params {
    uint32_t levels;                  /* L, default 16 */
    uint32_t _pad;
    double   origin[3];               /* default 0, 0, 0 */
    double   size;                    /* default 1 */
} sar_box_params;
typedef struct sar_box_level {        /* one per set and level 0..L */
    uint64_t cells;                   /* occupied cells */
    uint64_t singles;                 /* cells with exactly one point */
    uint64_t sum_sq;                  /* sum of n_i^2 */
    uint64_t n_log_n;                 /* sum of n_i * lg32(n_i) */
} sar_box_level;
int sar_box_params_default(sar_box_params* out);
/* *out = lg32(n) as defined above. Host arithmetic; refuses n == 0. */
int sar_box_log2_q32(uint32_t n, uint64_t* out);
/* The box counts of n_sets caller-supplied sets in one cube, on the runtime's device and stream: k_box_insert, one lane per point,
 * puts the points' finest cells into a hash table per set in device memory, and k_box_level, once per level L .. 1, sums a level's
 * table and folds it into the next coarser one — no sort and no dense grid. "box_chunk" sets per launch;
 * sets beyond 2^24 points of device memory go in groups. levels_out_host[n_sets][L + 1]. p NULL: the defaults. n_sets == 0 succeeds
 * and writes nothing. The runtime is lent as to sar_runtime_pairs. With timing enabled, sar_runtime_last_timing reports iterate_ms =
 * the box kernels (iterate_launches = their launches: L + 1 per launch group). */
int sar_runtime_boxes(sar_runtime* rt, const sar_box_params* p, uint32_t n_sets, uint32_t n, const double* points_host /* [n_sets][n][3] */,
                      sar_box_level* levels_out_host /* [n_sets][L + 1] */);

/* Three least-squares lines over a window of one set's levels: host arithmetic only, no device.
 *   window   the levels l >= l_min with (double)n >= min_occupancy * (double)cells_l: the mean occupancy of a box is at least
 *            min_occupancy (contiguous: cells never shrinks with l). A level without a cell (a DIVERGED map's rows) is outside it.
 *   points   x_l = l * ln 2 (minus the logarithm of the edge, up to the cube's size),
 *            y0_l = ln cells, y1_l = ln n - (n_log_n / 2^32) * ln 2 / n (the entropy of the occupancies), y2_l = 2 ln n - ln sum_sq.
 *   lines    ordinary least squares of each y on x over the window, in level order, with sar_corrdim_fit's formula and order of
 *            operations. The slopes are D0, D1 and D2; rms says how straight the window is and is not an error bar.
 *   status   SAR_BOXDIM_NO_WINDOW with NaN lines where the window holds fewer than three levels.
 * Refused: levels NULL, L outside 1..16, n outside 1..2^20, min_occupancy not > 0. */
enum { SAR_BOXDIM_FIT_OK = 0, SAR_BOXDIM_NO_WINDOW = 1 };
typedef struct sar_boxdim_line {
    double slope, intercept, rms;
} sar_boxdim_line;
typedef struct sar_boxdim_lines {
    sar_boxdim_line d0, d1, d2;
    uint32_t first_level, last_level; /* the window's ends; 0, 0 without a window */
    uint32_t used;                    /* levels in the window */
    int32_t  status;
} sar_boxdim_lines;
int sar_boxdim_fit(const sar_box_level* levels /* [L + 1] */, uint32_t L, uint32_t n, uint32_t l_min, double min_occupancy,
                   sar_boxdim_lines* out);

/* The same for maps. Coefficients, start points, jobs, the recorded points, status, fail_job, fail_step and extent are exactly
 * sar_runtime_corrdim's (k_corr_orbit, launched as it is): n = jobs * samples points per map.
 *   cube     of a BOUNDED map: origin = the extent's three minima, size = the largest of its three spans — 1.0 where that is 0 (a
 *            fixed point). Both are in the record. sar_runtime_boxes on the returned points with that cube gives the same rows.
 *   lines    sar_boxdim_fit of the map's rows with p->l_min and p->min_occupancy.
 *   DIVERGED all-zero levels, NaN origin and size, no window, returned points all zero.
 * levels_out_host[n_maps][L + 1]; records_out_host[n_maps]; points_out_host [n_maps][n][3] or NULL. "box_chunk" maps per launch;
 * maps beyond 2^24 points of device memory go in groups. The runtime is lent as to sar_runtime_pairs. With timing enabled,
 * sar_runtime_last_timing reports warmup_ms = k_corr_orbit and iterate_ms = the box kernels (iterate_launches = their launches).
 * Refused (SAR_ERR_INVALID): what sar_runtime_corrdim refuses of jobs, samples, stride, transient, bound, coefficients and start
 * points; levels outside 1..16; min_occupancy not > 0. n_maps == 0 succeeds and writes nothing. */
typedef struct sar_boxdim_params {
    uint32_t jobs, samples;           /* default 256, 128: 32768 points */
    uint32_t stride, transient;       /* default 4, 1000 */
    uint32_t levels;                  /* default 16 */
    uint32_t l_min;                   /* default 3 */
    uint64_t seed;                    /* start points = sar_start_points(seed, 0, jobs) when starts == NULL (default 0) */
    double   bound;                   /* default 1e6 */
    double   min_occupancy;           /* default 16 points per occupied box */
} sar_boxdim_params;
typedef struct sar_boxdim_record {    /* one per map */
    int32_t  status;                  /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t fail_job;
    uint64_t fail_step;
    double   extent[6];
    double   origin[3];               /* the cube; NaN for a DIVERGED map */
    double   size;
    sar_boxdim_lines lines;           /* lines.d0.slope, .d1.slope, .d2.slope are D0, D1, D2 */
} sar_boxdim_record;
int sar_boxdim_params_default(sar_boxdim_params* out);
int sar_runtime_boxdim(sar_runtime* rt, const sar_boxdim_params* p, uint32_t n_maps, const double* coeffs_host /* [n_maps][30] */,
                       const double* starts_xyz_host /* [jobs*3] or NULL */, sar_box_level* levels_out_host /* [n_maps][L + 1] */,
                       sar_boxdim_record* records_out_host /* [n_maps] */, double* points_out_host /* [n_maps][n][3] or NULL */);

/* ---- basins of attraction: the fate and the attractor of every start point on a plane through state space --------------------------- *
 * One map (`coeffs`: the x, y, z rows of sar_search_candidate, each coefficient through `0. + 1. * c` as the search does) and a plane
 * of width x height START POINTS (row-major, pixel index y * width + x). Pixel (x, y) starts at
 *   start_k = (origin_k + du_k * tu) + dv_k * tv,   tu = (double)x / (double)(width - 1)                   (0 when width == 1)
 *                                                   tv = (double)(height - 1 - y) / (double)(height - 1)    (0 when height == 1)
 * (row 0 is the high end, as in the planes; two multiplies and two adds in that order, no FMA; an entry with du_k == 0 and
 * dv_k == 0 stays origin_k). sar_basin_start gives the device's doubles on the host.
 *   fate       the pixel runs transient + steps steps of next_point; the start point itself is not tested. The first point outside the
 *              bound box — !(|x|, |y|, |z| <= bound), NaN included, the planes' test — makes the pixel SAR_SEARCH_DIVERGED with
 *              escape_step = that step's number, 1-based and counted from the start (<= transient: it escaped in the transient;
 *              above: in its tail). Otherwise the pixel is SAR_SEARCH_BOUNDED with escape_step = 0.
 *   tail       a BOUNDED pixel's tail is its steps + 1 points: the one after the transient and the `steps` that follow. Only bounded
 *              pixels have a tail: a pixel that escapes during its tail contributes nothing to what follows.
 *   node       of a point p: u_k = (p_k - box_lo_k) * scale_k (a subtract, then a multiply), scale_k = (double)grid / (box_hi_k -
 *              box_lo_k) computed once on the host; cell_k = u_k < 0 ? 0 : u_k >= grid ? grid - 1 : (uint32_t)u_k — points outside the
 *              box land in its border cells —; node = (cell_z * grid + cell_y) * grid + cell_x.
 *   attractor  the graph whose nodes are the cells some tail visits and whose edges join the cells of consecutive tail points of one
 *              pixel; an attractor is a connected component of it and its `root` the component's smallest node. All cells of one
 *              pixel lie in one component: that component's root is the pixel's `root`.
 * The partition is a property of the SET of edges: it does not depend on the launch shape, on "basin_chunk" or on the order of the
 * atomics. It is a statement at the grid's resolution and no finer: two attractors closer than a cell merge into one, and a tail too
 * short to overlap its neighbours' tails splits one attractor into several (raise `steps`, or lower `grid`). With grid = 1 every
 * bounded pixel has root 0 and the call is a cheap first pass that learns the extent of the tails for the box.
 * The attractors are sorted by `pixels` descending, then by `root` ascending; a pixel's `label` is its attractor's index in that
 * order. Everything is an integer, or a minimum / maximum moved through `<` / `>` only as in sar_runtime_extent (a -0.0 can only be a
 * start point's own coordinate with transient = 0; every later coordinate is a sum that begins with a canonical coefficient). The map
 * and the node are multiplies, adds and compares, so a host restatement gives the same records bit for bit. */
typedef struct sar_basin_params {
    double   coeffs[30];          /* the map (default all 0) */
    double   origin[3];           /* the plane: start = origin + du * tu + dv * tv (default (-1, -1, 0), du (2, 0, 0), dv (0, 2, 0)) */
    double   du[3], dv[3];
    uint32_t width, height;       /* pixels, width * height <= 2^24 (default 256 x 256) */
    uint32_t transient, steps;    /* default 1000, 256; each <= 2^31 and transient + steps < 2^32 (escape_step is 32 bits) */
    double   bound;               /* default 1e6; finite and positive */
    uint32_t grid;                /* G: cells per axis of the box, 1..128 (default 32) */
    uint32_t _pad;
    double   box_lo[3], box_hi[3]; /* the box the grid divides: finite, lo < hi, grid / (hi - lo) finite (default -1 .. 1) */
} sar_basin_params;
typedef struct sar_basin_pixel {      /* one per pixel */
    int32_t  status;              /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t escape_step;         /* DIVERGED: the 1-based step of the first point outside the bound box; BOUNDED: 0 */
    uint32_t root;                /* the smallest node of the pixel's attractor; 0xFFFFFFFF for a DIVERGED pixel */
    uint32_t label;               /* the attractor's index in the sorted table; 0xFFFFFFFF for a DIVERGED pixel */
} sar_basin_pixel;
typedef struct sar_basin_attractor {  /* one per attractor, sorted by pixels descending, then root ascending */
    uint32_t root;
    uint32_t pixels;              /* the size of its basin within the plane */
    uint32_t cells;               /* grid cells its tails visit */
    uint32_t first_pixel;         /* the lowest pixel index of the basin */
    uint32_t cell_lo[3], cell_hi[3]; /* the bounding cells (x, y, z), inclusive */
} sar_basin_attractor;
typedef struct sar_basin_stats {
    uint64_t pixels, escaped_transient, escaped_tail, bounded;   /* the last three sum to the first */
    uint64_t attractors, cells;   /* components, and occupied cells over all of them */
    double   extent[6];           /* xmin, xmax, ymin, ymax, zmin, zmax of all tail points, raw; +inf / -inf without a bounded pixel */
} sar_basin_stats;
typedef struct sar_basin_colors {
    double fade;                  /* default 32; finite and positive: the escape step at which the grey is half its ceiling */
} sar_basin_colors;
int sar_basin_params_default(sar_basin_params* out);
/* Pixel (x, y)'s start point (host arithmetic, identical to the device's; no device needed). */
int sar_basin_start(const sar_basin_params* p, uint32_t x, uint32_t y, double out3[3]);
/* The basins on the runtime's device and stream, "basin_chunk" pixels per launch: k_basin_screen, one lane per pixel in 8 x 8 tiles,
 * finds every pixel's fate and packs the survivors; k_basin_mark, one lane per survivor, walks the tail and unites the cells of
 * consecutive points in a lock-free union-find over the grid; k_basin_finish resolves every pixel's and every cell's root, and the
 * host builds the table, the labels and the statistics. pixels_out_host: width * height records. attractors_out_host: the first `cap`
 * attractors (may be NULL with cap 0); *n_out says how many there are (the search's convention); n_out and stats_out may be NULL.
 * The records and labels stay on the device for sar_runtime_basin_colorize until the next basin call. The runtime lends its device,
 * stream and timing spans: its image buffers, start-point stream and exposure / colour-range modes are neither read nor changed. With
 * timing enabled, sar_runtime_last_timing reports warmup_ms = k_basin_screen and iterate_ms = k_basin_mark (iterate_launches = the
 * latter's launches). Refused (SAR_ERR_INVALID): a zero size or more than 2^24 pixels, transient or steps above 2^31 or a sum of
 * 2^32 or more, grid 0 or above 128, a coefficient, origin, du, dv, box_lo, box_hi or bound that is not finite, bound <= 0,
 * box_lo >= box_hi, a scale that is not finite. */
int sar_runtime_basin(sar_runtime* rt, const sar_basin_params* p, sar_basin_pixel* pixels_out_host,
                      sar_basin_attractor* attractors_out_host /* [cap] or NULL */, uint32_t cap, uint32_t* n_out /* or NULL */,
                      sar_basin_stats* stats_out /* or NULL */);
int sar_basin_colors_default(sar_basin_colors* out);
/* Colours rt's last basin call (colors NULL: the defaults) into rgba16_out_host[width * height * 4]; SAR_ERR_INVALID without one.
 *   DIVERGED   grey g = 0.5 * (e / (e + fade)), e = (double)escape_step: channels `as u16` of g * 65535, alpha 65535 — the escape-time
 *              field, darkest where a start point leaves at once
 *   BOUNDED    cfg's palette at v = ((double)label + 0.5) / (double)attractors through Palette::interpolate's arithmetic as
 *              sar_runtime_plane_colorize applies it (clamp, blend, square root, `as u16`), alpha 65535
 * One division, three square roots and no logarithm: the image is bit for bit what a host restatement gives.
 * sar_runtime_set_width_height leaves the held picture as it is — it has the basin call's own size, not the runtime's —: the image
 * afterwards is the image before. */
int sar_runtime_basin_colorize(const sar_config* cfg, sar_runtime* rt, const sar_basin_colors* colors, uint16_t* rgba16_out_host);

/* ---- basin probes: the fate of ANY start point in the held basin picture, and the uncertainty exponent of its boundary --------------- *
 * THE HELD PICTURE is that of the runtime's last sar_runtime_basin call, if that call succeeded: its canonical map, `transient`,
 * `steps`, `bound`, `grid` and box, and its table label[node] — the label of the attractor whose component holds the cell, 0xFFFFFFFF
 * for a cell no tail of the picture visited. A basin call that fails, a refused one included, leaves the runtime without a held
 * picture (sar_runtime_basin_colorize keeps its own rule). A picture with grid = 1 is valid: every bounded probe then has label 0, the
 * escape-versus-stay question, and it is cheap.
 *   fate       of a point s: s runs exactly as a pixel runs — transient + steps steps of next_point, the start not tested, the bound
 *              test !(|x|, |y|, |z| <= bound) at every step. The first point outside makes it SAR_SEARCH_DIVERGED with the 1-based
 *              escape_step, label = 0xFFFFFFFF and hit = 0. Otherwise it is SAR_SEARCH_BOUNDED with escape_step = 0, its tail is the
 *              steps + 1 points from the one after the transient on, `hit` is the smallest j for which the cell of tail point j (the
 *              basins' node, in the held box) has a label, and `label` is that label. If no tail point's cell has one: label =
 *              SAR_BASIN_UNKNOWN and hit = steps + 1. A pixel's own start point (sar_basin_start) has that pixel's status,
 *              escape_step and label, and hit = 0.
 *   class      of a fate: 0xFFFFFFFF where DIVERGED (all escapes are ONE class), else its label; SAR_BASIN_UNKNOWN is a class of its own.
 *   ladder     n base points, a direction dir and K = `levels` perturbations e_k = ldexp(eps0, -(k - 1)), k = 1..K (an exact table made
 *              on the host). The probes of base point b are b, b_c + dir_c * e_k and b_c - dir_c * e_k per coordinate c: one multiply
 *              and one add or subtract, no FMA. Level k of a base point is UNKNOWN if any of its three classes is SAR_BASIN_UNKNOWN;
 *              else UNCERTAIN if the + or the - class differs from the base's; else certain. tested = n - unknown per level, and
 *              f(e_k) = uncertain / tested scales as e^alpha where the boundary is fractal: its dimension is D - alpha.
 * A fate is a statement at the held grid's resolution and no finer; UNKNOWN is counted, never guessed; a call takes one direction.
 * Everything the device produces is an integer; the map, the probe points and the node are multiplies, adds and compares, so a host
 * restatement gives every field bit for bit, whatever the launch shape or `chunk`. */
#define SAR_BASIN_UNKNOWN 0xFFFFFFFEu
#define SAR_BASIN_MAX_LEVELS 31
typedef struct sar_basin_fate {
    int32_t  status;              /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t escape_step;         /* DIVERGED: the 1-based step of the first point outside the bound box; BOUNDED: 0 */
    uint32_t label;               /* BOUNDED: the label found, or SAR_BASIN_UNKNOWN; DIVERGED: 0xFFFFFFFF */
    uint32_t hit;                 /* BOUNDED: the tail point whose cell gave the label (steps + 1 for UNKNOWN); DIVERGED: 0 */
} sar_basin_fate;
typedef struct sar_basin_fate_counts {
    uint64_t points, diverged, labelled, unknown;   /* the last three sum to the first */
} sar_basin_fate_counts;
typedef struct sar_basin_ladder_params {
    double   dir[3];              /* default (1, 0, 0); finite, not all zero; used as given (not normalised) */
    double   eps0;                /* default 0.125; finite and positive: e_1 */
    uint32_t levels;              /* K, 1..31 (default 24) */
    uint32_t chunk;               /* base points per launch; 0: 2^16. No result depends on it */
} sar_basin_ladder_params;
typedef struct sar_basin_uncertainty_level {
    double   eps;                 /* e_k */
    uint64_t tested, uncertain, unknown;   /* tested = n - unknown */
} sar_basin_uncertainty_level;
typedef struct sar_basin_ladder_mask {
    uint32_t uncertain_bits, unknown_bits;   /* bit k - 1: level k of this base point */
} sar_basin_ladder_mask;
int sar_basin_ladder_params_default(sar_basin_ladder_params* out);
/* The fates of n <= 2^24 points (points_host[n][3]) in rt's held picture: k_basin_fate, one lane per point, 2^20 points per launch.
 * counts_out may be NULL. The runtime is lent as to sar_runtime_basin: its image buffers, start-point stream, modes and the held
 * picture are neither changed nor invalidated (the first probe call after a basin call uploads the label table).
 * sar_runtime_basin_colorize after a probe call returns the bytes it returned before. sar_runtime_set_width_height leaves the held
 * picture and its label table as they are: the fates afterwards are the fates before. With timing enabled, iterate_ms and
 * iterate_launches are k_basin_fate's. Refused (SAR_ERR_INVALID): no held picture, n = 0 or above 2^24, a point that is not finite,
 * a NULL runtime or buffer. */
int sar_runtime_basin_fates(sar_runtime* rt, uint32_t n, const double* points_host /* [n][3] */, sar_basin_fate* fates_out_host /* [n] */,
                            sar_basin_fate_counts* counts_out /* or NULL */);
/* The ladder over n <= 2^20 base points (base_host[n][3]): k_basin_ladder, one group of 1 + 2K neighbouring lanes per base point,
 * `chunk` base points per launch. levels_out_host: K records. fate0_out_host (the base points' own fates) and masks_out_host (per base
 * point) may be NULL; p NULL: the defaults. The runtime is lent as above; iterate_ms and iterate_launches are k_basin_ladder's.
 * Refused as above, and: n above 2^20, a dir or eps0 that is not finite, eps0 <= 0, dir all zero, levels 0 or above 31. */
int sar_runtime_basin_uncertainty(sar_runtime* rt, const sar_basin_ladder_params* p, uint32_t n, const double* base_host /* [n][3] */,
                                  sar_basin_uncertainty_level* levels_out_host /* [levels] */, sar_basin_fate* fate0_out_host /* [n] or NULL */,
                                  sar_basin_ladder_mask* masks_out_host /* [n] or NULL */);

/* ---- FTLE maps: the finite-time stretching of the flow map F^N over a plane of start points ------------------------------------------ *
 * One map and a plane of width x height start points, as the basins take them: `coeffs`, `origin`, `du`, `dv`, `width`, `height` and
 * `bound` mean what they mean in sar_basin_params, and pixel (x, y) starts where sar_basin_start puts it, bit for bit (the same
 * expression over the same two tables tu[], tv[]; sar_ftle_start is its host twin). The field is taken by FINITE DIFFERENCES between
 * the end points of neighbouring pixels, not by tangent dynamics: a sheet that passes between two pixel centres cannot be missed, and
 * the picture states the stretching at the plane's resolution and no finer. Its ridges are the stable manifolds cut by the plane.
 *   fate       the pixel runs N = `steps` steps of next_point; the start point itself is not tested. The first point outside the bound
 *              box — !(|x|, |y|, |z| <= bound), NaN included: the basins' test — makes the pixel SAR_SEARCH_DIVERGED with escape_step =
 *              that step's number, 1-based (the basins' numbering with transient = 0), and end = (0, 0, 0). Otherwise the pixel is
 *              SAR_SEARCH_BOUNDED with escape_step = 0 and end = F^N(start).
 *   usable     a neighbour of a pixel is usable if it lies inside the picture and is BOUNDED.
 *   a, b       for a BOUNDED pixel with end point e, along u with R = (x + 1, y) and L = (x - 1, y):
 *                both usable   a_k = (e_R,k - e_L,k) * 0.5
 *                only R        a_k = e_R,k - e_k                       SAR_FTLE_ONE_SIDED_U
 *                only L        a_k = e_k - e_L,k                       SAR_FTLE_ONE_SIDED_U
 *                neither       a = 0                                   SAR_FTLE_NO_U (every pixel of a picture one pixel wide)
 *              and b along v the same with (x, y - 1) as the "plus" side R and (x, y + 1) as the "minus" side L — row 0 is the high
 *              end of tv — and SAR_FTLE_ONE_SIDED_V / SAR_FTLE_NO_V.
 *   Gram       g11 = (a0 * a0 + a1 * a1) + a2 * a2, g12 = (a0 * b0 + a1 * b1) + a2 * b2, g22 = (b0 * b0 + b1 * b1) + b2 * b2, no FMA.
 *   EDGE       SAR_FTLE_EDGE: some 4-neighbour inside the picture is DIVERGED — the pixel lies on the basin boundary.
 * A DIVERGED pixel has zero Gram entries and zero flags. Every field up to g22 is the device's, and only multiplies, adds,
 * subtractions and compares: a host restatement gives the same bits, whatever `chunk` is.
 * The host finishes each record in this order of operations (double, no FMA; N as a double, exact):
 *   hu_k = du_k / (double)(width - 1), hv_k = dv_k / (double)(height - 1)      — the plane's step per pixel, where the axis has one
 *   m11 = (hu0 * hu0 + hu1 * hu1) + hu2 * hu2, m12 and m22 likewise from hu . hv and hv . hv
 *   both axes present (neither NO flag): stretch2 = the larger root s of det(G - s M) = 0 — the largest squared singular value of
 *   the flow map's difference quotient over the plane:
 *     A = m11 * m22 - m12 * m12,  B = (g11 * m22 + g22 * m11) - 2 * (g12 * m12),  C = g11 * g22 - g12 * g12,
 *     disc = B * B - 4 * (A * C), a negative or NaN disc taken as 0;   stretch2 = (B + sqrt(disc)) / (2 * A)
 *   SAR_FTLE_NO_V only: stretch2 = g11 / m11;  SAR_FTLE_NO_U only: stretch2 = g22 / m22
 *   both NO flags, or a DIVERGED pixel: stretch2 = NaN
 *   ftle = log(stretch2) / (2 * N)     — nats per step; -inf for stretch2 == 0, NaN for NaN
 * stretch2 is a division and a correctly rounded square root over the device's bits; ftle is the host libm's log of it. */
#define SAR_FTLE_EDGE 1u
#define SAR_FTLE_ONE_SIDED_U 2u
#define SAR_FTLE_ONE_SIDED_V 4u
#define SAR_FTLE_NO_U 8u
#define SAR_FTLE_NO_V 16u
typedef struct sar_ftle_params {
    double   coeffs[30];          /* the map (default all 0) */
    double   origin[3];           /* the plane: start = origin + du * tu + dv * tv (default (-1, -1, 0), du (2, 0, 0), dv (0, 2, 0)) */
    double   du[3], dv[3];
    uint32_t width, height;       /* pixels, width * height <= 2^24 (default 256 x 256) */
    uint32_t steps;               /* N, 1 .. 2^31 (default 16) */
    uint32_t chunk;               /* pixels per launch of k_ftle_flow: 0 = 2^20, at most 2^30; whole 8 x 8 tiles, at least one. A field,
                                   * not a runtime option: no result depends on it */
    double   bound;               /* default 1e6; finite and positive */
} sar_ftle_params;
typedef struct sar_ftle_pixel {       /* one per pixel */
    int32_t  status;              /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t escape_step;         /* DIVERGED: the 1-based step of the first point outside the bound box; BOUNDED: 0 */
    uint32_t flags;               /* SAR_FTLE_* */
    uint32_t _pad;
    double   end[3];              /* BOUNDED: F^N(start); DIVERGED: 0 */
    double   g11, g12, g22;       /* the device's fields end here */
    double   stretch2;            /* the host finish */
    double   ftle;
} sar_ftle_pixel;
typedef struct sar_ftle_stats {
    uint64_t pixels, escaped, bounded;   /* escaped + bounded == pixels */
    uint64_t edge;                /* pixels with SAR_FTLE_EDGE */
    uint64_t one_sided;           /* pixels with SAR_FTLE_ONE_SIDED_U or SAR_FTLE_ONE_SIDED_V */
    uint64_t isolated;            /* pixels with SAR_FTLE_NO_U and SAR_FTLE_NO_V */
    double   ftle_min, ftle_max;  /* over the finite ftle; +inf / -inf without one */
} sar_ftle_stats;
typedef struct sar_ftle_colors {
    double lo, hi;                /* the palette's window of ftle (default 0 .. 1); finite, lo < hi, hi - lo finite */
    double fade;                  /* default 32; finite and positive: sar_basin_colors' fade, for the DIVERGED pixels */
} sar_ftle_colors;
int sar_ftle_params_default(sar_ftle_params* out);
/* Pixel (x, y)'s start point (host arithmetic, identical to the device's and to sar_basin_start's; no device needed). */
int sar_ftle_start(const sar_ftle_params* p, uint32_t x, uint32_t y, double out3[3]);
/* The FTLE map on the runtime's device and stream. k_ftle_flow, one lane per pixel in 8 x 8 tiles, `chunk` pixels per launch, writes
 * status, escape_step and end; k_ftle_gram, ONE launch over the whole picture behind every band, one lane per pixel, reads the four
 * neighbours' records from memory and writes the Gram entries and the flags — the kernel boundary is what makes every band's stores
 * visible to it —; the host finishes the records and counts the statistics. pixels_out_host: width * height records; stats_out may be
 * NULL. The records stay on the device for sar_runtime_ftle_colorize until the next FTLE call. The runtime lends its device, stream
 * and timing spans: its image buffers, start-point stream, exposure / colour-range modes and the records it holds for the other
 * families are neither read nor changed. With timing enabled, sar_runtime_last_timing reports iterate_ms = k_ftle_flow
 * (iterate_launches = its launches, the bands) and resolve_ms = k_ftle_gram.
 * Refused (SAR_ERR_INVALID): a zero size or more than 2^24 pixels, steps 0 or above 2^31, chunk above 2^30, a coefficient, origin, du
 * or dv that is not finite, bound not finite or <= 0; with width > 1, m11 == 0 (du is zero); with height > 1, m22 == 0; with both,
 * A not positive and finite (du and dv parallel, or their Gram determinant under- or overflows). */
int sar_runtime_ftle(sar_runtime* rt, const sar_ftle_params* p, sar_ftle_pixel* pixels_out_host, sar_ftle_stats* stats_out /* or NULL */);
int sar_ftle_colors_default(sar_ftle_colors* out);
/* Colours rt's last FTLE call (colors NULL: the defaults) into rgba16_out_host[width * height * 4]; SAR_ERR_INVALID without one. In
 * this order:
 *   DIVERGED                    the basins' escape-time grey g = 0.5 * (e / (e + fade)), e = (double)escape_step, alpha 65535
 *   BOUNDED with SAR_FTLE_EDGE  white (65535, 65535, 65535, 65535): the basin boundary itself
 *   BOUNDED, ftle finite        cfg's palette at v = (ftle - lo) / (hi - lo) through Palette::interpolate's arithmetic as
 *                               sar_runtime_plane_colorize applies it (clamp, blend, square root, `as u16`), alpha 65535
 *   BOUNDED, ftle not finite    (0, 0, 0, 65535)
 * ftle is evaluated on the device as log(stretch2) / (2 * N) from the record's stretch2 with the device's log, which returns one of the
 * two neighbouring doubles that enclose the true logarithm: a pixel's colour is one the expression gives with such a value (held per
 * pixel by tests/test_gpu_device_log.py). DIVERGED and EDGE pixels are bit for bit what a host restatement gives.
 * sar_runtime_set_width_height leaves the held records as they are — they have the map's own size, not the runtime's —: the image
 * afterwards is the image before. */
int sar_runtime_ftle_colorize(const sar_config* cfg, sar_runtime* rt, const sar_ftle_colors* colors, uint16_t* rgba16_out_host);

/* ---- power spectra: Welch periodograms of one observable of point sets and of maps' orbits ------------------------------------------- *
 * The frequency content of an orbit: a period-p cycle has lines at the multiples of 1 / p only, a torus at incommensurate
 * frequencies and their combinations, chaos is broadband. A trajectory is cut into overlapping segments, every segment is tapered
 * and transformed, and the squared magnitudes are added up. All arithmetic is fp64 multiplies, adds and subtractions in the order
 * written here, no FMA; the device holds no division, square root or logarithm, and a host restatement gives every output double
 * bit for bit.
 *   series      v_t = (proj[0] * x_t + proj[1] * y_t) + proj[2] * z_t, as sar_runtime_orbit plots it.
 *   segments    a trajectory (job) has `samples` values; segment s = 0 .. S - 1 is v[s * hop .. s * hop + N - 1] with
 *               S = (samples - N) / hop + 1 (floor). Values behind the last segment are unused.
 *   tree        tree(a) of N values: a <- a[0::2] + a[1::2], log2 N times — the pairwise sum.
 *   mean        m = tree(v) * inv_n with inv_n = 1.0 / N, exact, computed on the host.
 *   taper       a_t = (v_t - m) * w_t with the table w of sar_spectrum_window: SAR_WINDOW_RECT all 1.0 (the multiply is still done),
 *               SAR_WINDOW_HANN 0.5 - 0.5 * cos(2.0 * M_PI * (double)t / (double)N).
 *   energy      e_s = tree(a o a), the squares taken first.
 *   transform   the plain complex radix-2 decimation-in-time FFT of (a, 0): the input in bit-reversed order, the stages
 *               len = 2, 4, .., N; for every block i = 0, len, .. and j < len / 2: W = tw[j * N / len], b = A[i + j + len / 2],
 *               tr = W.re * b.re - W.im * b.im, ti = W.re * b.im + W.im * b.re, then with u = A[i + j]: A[i + j] = u + t and
 *               A[i + j + len / 2] = u - t. tw[k] = (cos(2.0 * M_PI * (double)k / (double)N), -sin(the same)), k < N / 2, is the
 *               table of sar_spectrum_twiddles. No butterfly is skipped or simplified, those on zeros and on W = 1 included.
 *   periodogram p_s[k] = re * re + im * im for k = 0 .. N / 2.
 *   sums        per job P_j[k] = the left fold of p_0[k], p_1[k], .. from +0.0 and E_j that of e_s; per set P[k] = the left fold of
 *               P_0[k], P_1[k], .. in job order from +0.0 and E that of E_j. Nothing depends on the launch shape, on `chunk` or on
 *               the order the workgroups run in.
 * A spectrum is N / 2 + 1 doubles and raw: unnormalised sums. Parseval: sum_k c_k P[k] = N * E up to rounding, c = 1 at k = 0 and
 * N / 2 and 2 elsewhere. Bin k is the frequency k / N cycles per sample. Inputs whose squares overflow give infinite or NaN bins
 * as the arithmetic gives them. */
#define SAR_WINDOW_RECT 0u
#define SAR_WINDOW_HANN 1u
typedef struct sar_spectra_params {
    uint32_t n;                       /* N: a power of two, 8..4096 (default 1024) */
    uint32_t hop;                     /* 1..N (default 512) */
    uint32_t window;                  /* SAR_WINDOW_* (default SAR_WINDOW_HANN) */
    uint32_t samples;                 /* per trajectory; 0: the whole set is one trajectory */
    uint32_t chunk;                   /* (set, job) workgroups per launch of k_spectrum: 0 = 2^16, at most 2^30. A field, not a
                                         runtime option, as sar_ftle_params' */
    uint32_t _pad;
    double   proj[3];                 /* default 1, 0, 0 */
} sar_spectra_params;
typedef struct sar_spectra_record {   /* one per set */
    uint32_t jobs, segments;          /* trajectories of the set, segments of a trajectory */
    double   energy;                  /* E */
} sar_spectra_record;
int sar_spectra_params_default(sar_spectra_params* out);
/* The tables the kernel reads: out[n / 2][2] = (re, im) of tw; out[n] = w. Host arithmetic, no device. Refused: n not a power of two
 * in 8..4096, an unknown window, out NULL. */
int sar_spectrum_twiddles(uint32_t n, double* out /* [n / 2][2] */);
int sar_spectrum_window(uint32_t window, uint32_t n, double* out /* [n] */);
/* The trajectories of a set of n_points points and the segments of each, behind the checks of p (NULL: the defaults) and n_points
 * that sar_runtime_spectra makes; either result may be NULL. */
int sar_spectra_segments(const sar_spectra_params* p, uint32_t n_points, uint32_t* jobs_out, uint32_t* segments_out);
/* The spectra of n_sets caller-supplied sets on the runtime's device and stream, the way sar_runtime_pairs and sar_runtime_boxes
 * take them: point i of a set is sample i % samples of trajectory i / samples. k_spectrum: one 256-lane workgroup per (set, job)
 * keeps a segment as re[] and im[] in LDS and the job's sums in registers, `chunk` workgroups per launch; k_spectrum_fold, one launch
 * per group, adds the jobs in order. Sets beyond 2^24 points of device memory go in groups.
 * power_out_host[n_sets][n / 2 + 1]; records_out_host[n_sets] or NULL. p NULL: the defaults. n_sets == 0 succeeds and writes
 * nothing. The runtime is lent as to sar_runtime_pairs: its image buffers, start-point stream and modes are neither read nor changed.
 * With timing enabled, sar_runtime_last_timing reports iterate_ms = k_spectrum (iterate_launches = its launches) and resolve_ms =
 * k_spectrum_fold.
 * Refused (SAR_ERR_INVALID): n not a power of two in 8..4096, hop 0 or above n, an unknown window, a proj that is not finite, a
 * chunk above 2^30, n_points 0 or above 2^20, samples that does not divide n_points or is below n, a coordinate that is not finite. */
int sar_runtime_spectra(sar_runtime* rt, const sar_spectra_params* p, uint32_t n_sets, uint32_t n_points,
                        const double* points_host /* [n_sets][n_points][3] */, double* power_out_host /* [n_sets][n / 2 + 1] */,
                        sar_spectra_record* records_out_host /* [n_sets] or NULL */);

/* The same for maps. Coefficients, start points, jobs, the recorded points, status, fail_job, fail_step and extent are exactly
 * sar_runtime_corrdim's (k_corr_orbit, launched as it is) with samples = (segments - 1) * hop + n per job, so that every job has
 * `segments` segments and no tail. sar_runtime_spectra on the returned points with samples set gives the same power.
 *   DIVERGED all-+0.0 power, energy 0, segments 0, returned points all zero.
 * power_out_host[n_maps][n / 2 + 1]; records_out_host[n_maps]; points_out_host [n_maps][jobs * samples][3] or NULL. Maps beyond 2^24
 * points of device memory go in groups. Bin k is k / (n * stride) cycles per step. The runtime is lent as to sar_runtime_pairs. With
 * timing enabled, sar_runtime_last_timing reports warmup_ms = k_corr_orbit, iterate_ms = k_spectrum (iterate_launches = its
 * launches) and resolve_ms = k_spectrum_fold.
 * Refused (SAR_ERR_INVALID): what sar_runtime_spectra refuses of n, hop, window, proj and chunk; segments 0; what sar_runtime_corrdim
 * refuses of jobs, samples, stride, transient, bound, coefficients and start points. n_maps == 0 succeeds and writes nothing. */
typedef struct sar_spectrum_params {
    uint32_t jobs, segments;          /* default 16, 15 */
    uint32_t n, hop;                  /* default 1024, 512 */
    uint32_t window;                  /* default SAR_WINDOW_HANN */
    uint32_t stride, transient;       /* default 1, 1000 */
    uint32_t chunk;                   /* as sar_spectra_params' */
    uint64_t seed;                    /* start points = sar_start_points(seed, 0, jobs) when starts == NULL (default 0) */
    double   bound;                   /* default 1e6 */
    double   proj[3];                 /* default 1, 0, 0 */
} sar_spectrum_params;
typedef struct sar_spectrum_record {  /* one per map */
    int32_t  status;                  /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t fail_job;
    uint64_t fail_step;
    double   extent[6];
    uint32_t segments;                /* per job; 0 for a DIVERGED map */
    uint32_t _pad;
    double   energy;                  /* E; 0 for a DIVERGED map */
} sar_spectrum_record;
int sar_spectrum_params_default(sar_spectrum_params* out);
int sar_runtime_spectrum(sar_runtime* rt, const sar_spectrum_params* p, uint32_t n_maps, const double* coeffs_host /* [n_maps][30] */,
                         const double* starts_xyz_host /* [jobs*3] or NULL */, double* power_out_host /* [n_maps][n / 2 + 1] */,
                         sar_spectrum_record* records_out_host /* [n_maps] */, double* points_out_host /* [n_maps][jobs * samples][3] or NULL */);

/* ---- recurrence analysis: exact line-length histograms of the recurrence plots of point sets and of maps' orbits ------------------------ *
 * When an orbit comes back near where it has been, and for how long it then follows its own past (Eckmann, Kamphorst & Ruelle;
 * Zbilut & Webber; Marwan et al.). The T x T recurrence matrix of a trajectory is never stored: the device counts the lengths of
 * its maximal diagonal and vertical runs, exactly; the measures (determinism, laminarity, trapping time, ..) are host arithmetic on
 * the counts.
 *   trajectories  as sar_runtime_pairs: point i of a set of n points is sample i % T of trajectory i / T, T = samples, 0 standing for
 *                 n. A trajectory is p_0 .. p_(T-1). Only pairs of the same trajectory are looked at.
 *   distance      r2(i, j) = (dx * dx + dy * dy) + dz * dz with dx = x_j - x_i, dy, dz alike: sar_runtime_pairs' arithmetic in its
 *                 order, no FMA. Symmetric bit for bit: (-d) * (-d) = d * d.
 *   recurrence    R(i, j) = |i - j| > theiler && r2(i, j) < eps2. `<` is strict — the pair histogram's bin convention: with eps2 on a
 *                 bin edge the recurrences are the cumulative pair count. A NaN r2 (from infinite coordinates) and r2 = +inf are not
 *                 recurrent; r2 = 0 is, a product that underflows to 0 included.
 *   diagonals     for every k in theiler + 1 .. T - 1 the sequence R(i, i + k), i = 0 .. T - k - 1: every maximal run of ones of
 *                 length l adds 1 to diag[min(l, B)]. The upper triangle only; the lower one mirrors it.
 *   verticals     for every column j the sequence R(i, j), i = 0 .. T - 1, over the full matrix; the Theiler band's entries are zeros
 *                 and cut a run. Every maximal run of length l adds 1 to vert[min(l, B)].
 *   bins          B = line_bins, 2 .. 4096, default 256. Both histograms are uint64[B + 1]; entry 0 is always 0, entry B collects l >= B.
 *   per set       summed over its trajectories: recurrences = the sum of R over i < j (also the sum of l over all diagonal lines, and
 *                 half of that over all vertical lines); pairs = the sum over trajectories of (T - theiler - 1)(T - theiler) / 2, 0
 *                 where T <= theiler + 1; diag_lines and vert_lines; diag_longest and vert_longest, exact, not clamped.
 * Every result is a sum of integers or a maximum: nothing depends on the launch shape, on `chunk` or on the order of the atomics, and
 * a host restatement gives the same integers bit for bit. */
typedef struct sar_recurrence_params {
    uint32_t samples;                 /* T, points per trajectory; 0 = n (default 0) */
    uint32_t theiler;                 /* any value; with theiler >= T - 1 everything is zero (default 0) */
    uint32_t line_bins;               /* B, 2..4096 (default 256) */
    uint32_t chunk;                   /* workgroups per launch of k_rqa_diag and of k_rqa_vert: 0 = 2^16, at most 2^30. A field, not a
                                         runtime option, as sar_ftle_params' */
    double   eps2;                    /* the squared threshold, positive and finite. The default 0 is refused: there is no natural one */
} sar_recurrence_params;
typedef struct sar_recurrence_record {   /* one per set */
    uint64_t recurrences, pairs;
    uint64_t diag_lines, vert_lines;
    uint64_t diag_longest, vert_longest;
} sar_recurrence_record;
int sar_recurrence_params_default(sar_recurrence_params* out);
/* The line-length histograms of n_sets caller-supplied sets on the runtime's device and stream. k_rqa_diag: a lane owns one diagonal
 * and walks it from end to end with the run length in a register, a 256-lane workgroup takes a band of 256 neighbouring diagonals
 * and the band that mirrors it, `chunk` workgroups per launch over (set, trajectory, folded band). k_rqa_vert: a lane owns one column
 * (DESIGN.md section 26). Sets beyond 2^24 points of device memory go in groups. diag_out_host and vert_out_host [n_sets][B + 1];
 * records_out_host[n_sets] or NULL. n_sets == 0 succeeds and writes nothing. The runtime is lent as to sar_runtime_pairs: its image
 * buffers, start-point stream, modes and the records it holds for other families are neither read nor changed. With timing enabled,
 * sar_runtime_last_timing reports iterate_ms = k_rqa_diag (iterate_launches = its launches) and resolve_ms = k_rqa_vert.
 * Refused (SAR_ERR_INVALID): line_bins outside 2..4096, an eps2 that is not positive and finite, a chunk above 2^30, n 0 or above
 * 2^20, samples that does not divide n, a NaN coordinate (infinities are taken). */
int sar_runtime_recurrence(sar_runtime* rt, const sar_recurrence_params* p, uint32_t n_sets, uint32_t n,
                           const double* points_host /* [n_sets][n][3] */, uint64_t* diag_out_host /* [n_sets][B + 1] */,
                           uint64_t* vert_out_host /* [n_sets][B + 1] */, sar_recurrence_record* records_out_host /* [n_sets] or NULL */);
/* A window of the recurrence matrix of trajectory `job` of one set: out_host[y][x] = R(i0 + y, j0 + x), 1 or 0 (k_rqa_plot: one lane
 * per entry). Refused: what sar_runtime_recurrence refuses, a job the set does not have, a window of 0 or more than 2^24 entries, a
 * window that leaves the trajectory (i0 + height or j0 + width above T). */
int sar_runtime_recurrence_plot(sar_runtime* rt, const sar_recurrence_params* p, uint32_t n, const double* points_host /* [n][3] */,
                                uint32_t job, uint32_t i0, uint32_t j0, uint32_t height, uint32_t width, uint8_t* out_host /* [height][width] */);

/* The same for maps. Coefficients, start points, jobs, samples, stride, transient, seed, bound, the recorded points, status,
 * fail_job, fail_step and extent are exactly sar_runtime_corrdim's (k_corr_orbit, launched as it is): a job is a trajectory of
 * T = samples points.
 *   eps2      p->eps2 > 0 is used as given for every map. Otherwise a map's own eps2 = (eps_fraction * eps_fraction) *
 *             ((dx * dx + dy * dy) + dz * dz) of its extent's three spans, on the host in that order: the threshold is eps_fraction
 *             of the extent's diagonal. The record holds it.
 *   zero      a BOUNDED map whose own eps2 is 0 (a fixed point: no extent) or not finite has all-zero histograms and counts and
 *             eps2 = 0 in its record; so has a DIVERGED map, whose returned points are all zero too.
 * sar_runtime_recurrence on the returned points with samples, theiler, line_bins and the record's eps2 gives the same histograms and
 * counts. diag_out_host and vert_out_host [n_maps][B + 1]; records_out_host[n_maps]; points_out_host [n_maps][jobs * samples][3] or
 * NULL. Maps beyond 2^24 points of device memory go in groups. The runtime is lent as to sar_runtime_pairs. With timing enabled,
 * sar_runtime_last_timing reports warmup_ms = k_corr_orbit, iterate_ms = k_rqa_diag (iterate_launches = its launches) and
 * resolve_ms = k_rqa_vert.
 * Refused (SAR_ERR_INVALID): what sar_runtime_corrdim refuses of jobs, samples, stride, transient, bound, coefficients and start
 * points; line_bins outside 2..4096; a chunk above 2^30; an eps2 that is negative or not finite; with eps2 == 0 an eps_fraction that
 * is not positive and finite. n_maps == 0 succeeds and writes nothing. */
typedef struct sar_rqa_params {
    uint32_t jobs, samples;           /* default 16, 1024 */
    uint32_t stride, transient;       /* default 1, 1000 */
    uint64_t seed;                    /* start points = sar_start_points(seed, 0, jobs) when starts == NULL (default 0) */
    double   bound;                   /* default 1e6 */
    uint32_t theiler;                 /* default 0 */
    uint32_t line_bins;               /* default 256 */
    uint32_t chunk;                   /* as sar_recurrence_params' */
    uint32_t _pad;
    double   eps2;                    /* default 0: every map's own, from eps_fraction */
    double   eps_fraction;            /* default 0.05 */
} sar_rqa_params;
typedef struct sar_rqa_record {       /* one per map */
    int32_t  status;                  /* SAR_SEARCH_BOUNDED or SAR_SEARCH_DIVERGED */
    uint32_t fail_job;
    uint64_t fail_step;
    double   extent[6];
    double   eps2;                    /* the threshold used; 0: nothing was counted */
    sar_recurrence_record counts;
} sar_rqa_record;
int sar_rqa_params_default(sar_rqa_params* out);
int sar_runtime_rqa(sar_runtime* rt, const sar_rqa_params* p, uint32_t n_maps, const double* coeffs_host /* [n_maps][30] */,
                    const double* starts_xyz_host /* [jobs*3] or NULL */, uint64_t* diag_out_host /* [n_maps][B + 1] */,
                    uint64_t* vert_out_host /* [n_maps][B + 1] */, sar_rqa_record* records_out_host /* [n_maps] */,
                    double* points_out_host /* [n_maps][jobs * samples][3] or NULL */);

/* The measures of recurrence quantification from one set's or map's histograms and counts: host arithmetic only, no device, in this
 * order, every integer converted to double where it meets a division.
 *   rr      recurrences / pairs.
 *   det     (recurrences - S) / recurrences with S = the sum of l * diag[l] over l < l_min, in integers: the share of recurrent
 *           points on diagonal lines of at least l_min.
 *   l_mean  (recurrences - S) / N with N = the sum of diag[l] over l_min <= l <= B.
 *   l_max   diag_longest; div = 1 / l_max.
 *   entr    the Shannon entropy, natural logarithm, of the line lengths l >= l_min: h = h - p * log(p) with p = diag[l] / N, a left
 *           fold over l = l_min .. B from 0.0 that skips empty bins. The clamp bin B counts as one class: lengths beyond B are not
 *           told apart.
 *   lam, tt, v_max   the same from vert with v_min, against 2 * recurrences: the laminarity, the trapping time, vert_longest.
 * A quotient with an empty denominator is NaN. Refused: a NULL, line_bins outside 2..4096, l_min or v_min outside 1..B. */
typedef struct sar_rqa_measures_out {
    double   rr, det, l_mean, div, entr, lam, tt;
    uint64_t l_max, v_max;
} sar_rqa_measures_out;
int sar_rqa_measures(const uint64_t* diag /* [B + 1] */, const uint64_t* vert /* [B + 1] */, const sar_recurrence_record* record,
                     uint32_t line_bins, uint32_t l_min, uint32_t v_min, sar_rqa_measures_out* out);

/* ---- image export (src/bin/main.rs:40-100, write_image_matches) ------------------------------------ *
 * The CLI converts FinalImage (RGBA16) by (--transparent, --8bit) before it encodes (:52-57):
 *   (true,false) RGBA16 as is | (false,false) to_rgb16 | (true,true) to_rgba8 | (false,true) to_rgb8
 * and writes PNG (default compression, adaptive filter, :84-92), BMP (:71-77) or PAM (:64-70; both need --8bit,
 * :256-258). The conversions and encoders live in the `image` crate (Cargo.toml: image = "0.25", no lockfile,
 * not vendored): restated here from its published algorithm — 16 -> 8 bit is ((c + 128) / 257), alpha is
 * dropped without pre-multiplication — PARITY UNPINNED beyond "the file decodes to these samples".
 */
#define SAR_FMT_RGBA16 0
#define SAR_FMT_RGB16  1
#define SAR_FMT_RGBA8  2
#define SAR_FMT_RGB8   3
/* The format write_image_matches picks for (--transparent, --8bit) (:52-57). */
int sar_image_format(int transparent, int eight_bit);
/* Bytes of a width x height image in `format` (0 for an unknown format). */
size_t sar_image_bytes(int format, uint32_t width, uint32_t height);
/* RGBA16 (device) -> format (device), stream-ordered on rt's stream; in and out must not overlap. */
int sar_image_convert_device(sar_runtime* rt, const void* rgba16_dev, int format, void* out_dev);
/* colorize + conversion on the device, then ONE device-to-host copy of the converted image
 * (sar_image_bytes(format) bytes: 12 MiB instead of 32 MiB for RGB8 at 2048x2048). Samples are host-endian. */
int sar_colorize_format(const sar_config* cfg, sar_runtime* rt, int format, void* out_host);
/* The same, returning as soon as the work is ENQUEUED: the image is in out_host once sar_runtime_wait_image(rt, ticket) has returned
 * (sar_runtime_image_done asks without waiting). A `sequence` sweep (src/bin/main.rs:493-517 hands frame k to its writer threads
 * and goes on with frame k+1) reads frame k back while frame k+1 renders. out_host should be page-locked (sar_host_alloc; pageable
 * memory is staged by the HIP runtime and the call may block) and stay untouched until the ticket is done; the runtime may be reset
 * and rendered into again before that. out_host == NULL: colorize + conversion only — the image stays in device memory until
 * sar_runtime_read_image_async fetches it (page-locking a host image takes 1-3 ms, a frame renders in 0.7). */
int sar_colorize_format_async(const sar_config* cfg, sar_runtime* rt, int format, void* out_host, uint64_t* ticket_out);
int sar_runtime_read_image_async(sar_runtime* rt, void* out_host, uint64_t* ticket_out);
int sar_runtime_image_done(sar_runtime* rt, uint64_t ticket, int* done_out);
int sar_runtime_wait_image(sar_runtime* rt, uint64_t ticket);
/* Page-locked host memory for those read-backs (4 MiB and more: mapped with huge pages, touched, hipHostRegister'ed). */
int sar_host_alloc(size_t bytes, void** out);
int sar_host_free(void* p);
/* Announces `count` sar_host_alloc(bytes) calls to come (a sweep's ring of images): helper threads map and zero the blocks ahead —
 * most of what page-locking costs, and no HIP call — and sar_host_alloc only locks them. One announcement per process at a time; a
 * new one, or count 0, releases what the last one left. */
int sar_host_reserve(size_t bytes, uint32_t count);
/* Encoders (host only; no device needed). `pixels` is a host image in `format`, host-endian samples.
 * PNG: 8/16-bit RGB(A), zlib default compression, per-row adaptive filter (minimum sum of absolute differences).
 * BMP / PAM: SAR_FMT_RGBA8 or SAR_FMT_RGB8 only (the CLI requires --8bit for them); BMP 24 bpp BI_RGB or
 * 32 bpp BI_BITFIELDS (V4 header) bottom-up; PAM "P7" with TUPLTYPE RGB / RGB_ALPHA. */
int sar_write_png(const char* path, int format, uint32_t width, uint32_t height, const void* pixels);
int sar_write_bmp(const char* path, int format, uint32_t width, uint32_t height, const void* pixels);
int sar_write_pam(const char* path, int format, uint32_t width, uint32_t height, const void* pixels);

/* ---- read-back accessors (the reference keeps these fields private, :633-643) ---------------------- */
int sar_runtime_count(sar_runtime* rt, uint32_t* out_host);   /* width*height */
int sar_runtime_steps(sar_runtime* rt, double* out_host);     /* width*height */
int sar_runtime_zbuf(sar_runtime* rt, float* out_host);       /* width*height */
int sar_runtime_max(sar_runtime* rt, uint32_t* out_max);
/* Upload a full state (used to move a partial render between processes / devices). */
int sar_runtime_load(sar_runtime* rt, const uint32_t* count_host, const double* steps_host,
                     const float* zbuf_host, uint32_t max);

/* ---- multi-GPU exchange, one process per GPU: Runtime::merge (:708-738) folded in rank order (:1068-1076) -----------------------
 * ONE context object per runtime and world; the collectives (RCCL through torch.distributed, or anything else) are the caller's,
 * on buffers the caller owns (device memory the collective library can address); everything between them happens here.
 * Every rank OWNS the slice [rank*S, min(npix, (rank+1)*S)) of the image, S a multiple of 2048 (sar_exchange_slice_pixels):
 *
 *   sar_exchange_flags   flags[g] = 1 for every 64-pixel GRANULE of this rank's partial buffers with a count or a depth  -> all-gather (1 B / granule)
 *   sar_exchange_pack    from every rank's flags the library PLANS the exchange on the device (two block scans: where each of my
 *                        records goes, where each record I receive arrives) and packs the send buffer — records of 1 KiB
 *                        [count u32 x 64 | sortable(zbuf) u32 x 64 | steps f64 x 64], owner by owner (a frame touches a fifth of
 *                        its pixels: 21 % of the granules of BASELINE configs[1]); a rank without a record holds the reset state
 *                        there, the fold skips it, same result bit for bit. A frame whose flags cover more than dense_above of
 *                        the image — or flags_all == NULL — goes DENSE: `world` blocks of S*16 bytes [count x S | zbuf x S |
 *                        steps x S]. send_bytes / recv_bytes[world] are the split sizes of the all-to-all: the call waits for
 *                        them (2 world + 1 numbers), the ONE host wait of a frame's exchange                    -> all-to-all (split sizes)
 *   sar_exchange_merge   the owner folds what arrived in rank order (rank 0 = the accumulator of :1070, the earlier rank wins depth
 *                        ties, `max` follows every intermediate sum) into rt's own buffers at its slice, and writes {max, wrap
 *                        flag, depth range} as 4 x int64                                                         -> all-reduce MAX (32 B)
 *   sar_exchange_finish  the reduced scalars become the runtime's; sar_colorize_range_device on my slice         -> gather (8 B/px)
 *
 * After merge a runtime holds the merged frame only inside its own slice. strange_attractor_renderer_amd/distributed.py
 * (SlicedExchange) is this sequence around torch.distributed. */
typedef struct sar_exchange sar_exchange;
typedef struct sar_exchange_layout {
    uint32_t world, rank;
    uint32_t slice_pixels;    /* S */
    uint32_t first_px, n_px;  /* this rank's slice */
    uint32_t granules;        /* ceil(npix / 64): the bytes of one rank's flags */
    uint64_t block_bytes;     /* world * S * 16: the size of the send and of the receive buffer */
} sar_exchange_layout;
#define SAR_EXCHANGE_GRANULE 64
int sar_exchange_slice_pixels(uint32_t npix, uint32_t world, uint32_t* out_slice_pixels);   /* host arithmetic only */
/* rt is borrowed: every call on the exchange but sar_exchange_free needs it alive, at the image size it had here (a resized
 * runtime: SAR_ERR_DIM_MISMATCH, make a new context); layout_out may be NULL. */
int sar_exchange_new(sar_runtime* rt, uint32_t world, uint32_t rank, sar_exchange** out, sar_exchange_layout* layout_out);
int sar_exchange_free(sar_exchange* ex);
int sar_exchange_flags(sar_exchange* ex, uint8_t* flags_out_dev /* [granules] */);
int sar_exchange_pack(sar_exchange* ex, const uint8_t* flags_all_dev /* [world][granules], or NULL */, double dense_above,
                      void* send_dev /* block_bytes */, uint64_t* send_bytes /* [world] */, uint64_t* recv_bytes /* [world] */, int* sparse_out);
int sar_exchange_merge(sar_exchange* ex, const void* recv_dev /* block_bytes */, int64_t* scalars_out_dev /* [4] */);
int sar_exchange_finish(sar_exchange* ex, const int64_t* scalars_reduced_dev /* [4] */);
/* The ROOTED form, for a caller that wants the whole merged Runtime on one rank (20 B/px through two ring collectives):
 *   step 0  key[p] = sortable int64 of (zbuf[p], lowest-rank-wins)                                        -> all-reduce MAX
 *   step 1  sum[0..npix) = count[p] as int32 (wrapping == u32 add), sum[npix..3 npix) = the two int32 halves of steps[p] where this
 *           rank holds the winning key, else 0                                                            -> reduce SUM (int32)
 *   step 2  (the root) count / zbuf / steps / max of rt replaced by the reduced buffers. */
int sar_exchange_rooted(sar_exchange* ex, uint32_t step, void* key_i64_dev /* [npix] */, void* sum_i32_dev /* [3 npix]; step 0: NULL */);
/* colorize (:841-904) of the pixel range [first_px, first_px + n_px) into out_dev (n_px*8 bytes, RGBA16), using the
 * max / depth range the runtime's scalars hold (made global by step 3); stream-ordered. */
int sar_colorize_range_device(const sar_config* cfg, sar_runtime* rt, uint32_t first_px, uint32_t n_px, void* rgba_out_dev);

/* ---- ParallelRenderer / render_parallel (src/lib.rs:908-1082) -------------------------------------- */
/* ParallelRenderer::new (:919-1004). `units` plays the role of num_threads (:920-922): the number of
 * execution units the job split divides by; 0 selects the device default, 64 per CU (16 384 on MI355X), so that the
 * CLI's default of 12 jobs per thread (src/bin/main.rs:305) becomes 196 608 trajectories = three waves per SIMD.
 * The renderer owns one runtime on `device`, seeded with `seed`. */
int sar_renderer_new(int device, uint32_t units, uint64_t seed, sar_renderer** out);
/* The same over SEVERAL GPUs of one node, behind this ABI alone (no Python, no RCCL): ParallelRenderer::new owns every execution
 * unit of the machine (:919-1004). devices[n_devices] are HIP device ordinals in FOLD ORDER (device 0 is the accumulator of :1070;
 * a device may be listed more than once — each entry is its own shard). units == 0: 64 per CU summed over the devices.
 * render_parallel then cuts the units*jobs_per_unit jobs into contiguous slices, one per device (one host thread + one stream
 * each), lets every device own one slice of the image, exchanges the partial buffers point-to-point (sar_renderer_set_exchange),
 * folds them with Runtime::merge in device order, colorizes each slice where it lives and copies it into rgba_out_host. The
 * result is bit-identical to the single-device renderer's for the same units. (Validated with one physical GPU listed several
 * times; a node with several GPUs has not been available to this build.) */
int sar_renderer_new_multi(const int* devices, uint32_t n_devices, uint32_t units, uint64_t seed, sar_renderer** out);
int sar_renderer_num_devices(const sar_renderer* r, uint32_t* out_devices);
int sar_renderer_num_units(const sar_renderer* r, uint32_t* out_units);
/* ParallelRenderer::shutdown (:1020-1025). */
int sar_renderer_shutdown(sar_renderer* r);
/* render_parallel (:1051-1082): iterations/units/jobs_per_unit per job (:1058), units*jobs_per_unit
 * jobs (:1062), reset, render, colorize. rgba_out_host: width*height*4 uint16. */
int sar_render_parallel(sar_renderer* r, const sar_config* cfg, uint32_t jobs_per_unit,
                        uint16_t* rgba_out_host);
/* The renderer's runtime (borrowed; device 0's), e.g. to read the count buffer after render_parallel. With several
 * devices the merged slices are first gathered into it (20 B/px over xGMI, once per frame, only when asked). */
int sar_renderer_runtime(sar_renderer* r, sar_runtime** out_borrowed);
/* Phases of the last sar_render_parallel on a multi-device renderer: the slowest device's stream time per phase. */
typedef struct sar_parallel_timing {
    float    total_ms;      /* host wall time of the call */
    float    render_ms;     /* reset + warm-up + iterate + accumulate + fold + pack */
    float    exchange_ms;   /* records / peer copies + merge of the owned slice + the scalar reduce (includes waiting for the slowest peer) */
    float    colorize_ms;   /* colorize of the own slice + its copy to the host image (from behind the scalar reduce) */
    uint32_t n_devices;
    uint32_t peer_access_failures;  /* ordered pairs of distinct devices WITHOUT direct peer access (hipDeviceCanAccessPeer said
                                       no, or hipDeviceEnablePeerAccess failed; sar_last_error keeps the last reason): their
                                       copies are staged through host memory by the HIP runtime */
    uint64_t exchange_bytes_per_device;  /* bytes every device pulls over xGMI per frame */
    float    host_ms_before_exchange;    /* host time between the last device's render being enqueued and the first pull of the
                                            exchange being enqueued (one device: entry to render enqueued) — the next frame's
                                            start points are drawn on helper threads meanwhile, off this path */
    float    host_ms_enqueue;            /* host time from entry until the whole frame (render, exchange, colorize, copies) is enqueued */
    float    draw_ahead_ms;              /* a helper thread's time to draw one device's slice of the next frame's start points */
    float    _pad;
} sar_parallel_timing;
int sar_renderer_last_timing(const sar_renderer* r, sar_parallel_timing* out);
/* How a multi-device renderer exchanges its partial buffers before colorize. 2 = sparse: every device writes the records of the
 * 64-pixel granules it has touched (1 KiB each: count, zbuf, steps) straight into their owners' buffers — kernels storing to
 * peer memory over xGMI — and the owners fold what arrived (a fifth of a frame at the BASELINE shapes); 1 = dense: whole slices,
 * 16 B/px, by hipMemcpyPeerAsync; 0 (default) = sparse when every pair of devices has direct peer access AND every device could
 * give its receive buffers fine-grained (device-coherent) memory, dense otherwise — where either is missing, a render call under
 * mode 2 fails with SAR_ERR_INVALID instead of folding what may be stale. The merged frame is the same bit for bit. */
int sar_renderer_set_exchange(sar_renderer* r, uint32_t mode);

/* ---- measurement ----------------------------------------------------------------------------------- */
int sar_runtime_enable_timing(sar_runtime* rt, int enabled);
int sar_runtime_last_timing(sar_runtime* rt, sar_timing* out);
/* What the last render call launched, as one line of text for logs and bench records — e.g.
 * "k_iterate_split R=60 bins=128x32768px interleaved hints=f32 pipe=2 park=8 phase=2 | k_bin_accumulate splits=4 lists=4
 * counters=u32 | chunks=1 warmup_ahead=19": the iterate kernel the library really chose (not a guess of the caller), its chunk
 * size and bin geometry, the accumulate mode, the launch chunks of the call and how many render calls so far found their warm-up
 * already done (sar_runtime_prefetch_device). phase: the iterations per barrier phase of the wave-pair kernel that was launched,
 * single or batched (2, or 1 where the LDS staging leaves room for 1 KiB of visits in flight only), 0 for k_iterate_lean. Writes
 * at most cap bytes including the terminating 0. */
int sar_runtime_describe_last_launch(const sar_runtime* rt, char* out, size_t cap);
/* Options by name (value 0 restores the default):
 *   "block_threads"      lanes per workgroup of the iterate kernel (64, 128, 192, 256)
 *   "checkpoint_stride"  iterations between trajectory checkpoints used by the payload resolve (default 32)
 *   "hint_bits"          per-XCD depth hints of the iterate kernel: 16 (fixed point over the depth range the warm-up saw) or
 *                        32 (the depth itself as f32); 0 = by image size
 *   "split_waves"        the iterate kernel as producer / consumer wave pairs: 1 never, 2 wherever the kernel exists; 0 = 2 for
 *                        launches whose jobs are all resident at once (512 per CU), 1 for larger ones
 *   "tail_overlap"       1: the depth resolve of a launch chunk runs on the runtime's side stream beside the accumulate kernel,
 *                        and the launch stream waits for both; 0 (the default): it follows the accumulate kernel on the launch
 *                        stream. The same result either way; an A/B switch (1 measured slower at 2048^2)
 *   "timing_accumulate"  1: the spans of successive render calls add up (sar_timing sums, iterate_launches counts
 *                        them) until sar_runtime_last_timing reads and clears them; 0: last render call only
 *   "search_chunk"       candidates per launch of sar_runtime_search (default 2^22, at most 2^30): bounds its device scratch
 *   "plane_chunk"        pixels per launch of sar_runtime_plane (default 2^20, at most 2^30; whole 8 x 8 tiles, at least one)
 *   "gallery_chunk"      tiles per launch of sar_runtime_gallery (default 512, at most 2^16): bounds its raw scratch
 *   "orbit_chunk"        columns per launch of sar_runtime_orbit (default 4096, at most 2^16): keeps one dispatch short
 *   "basin_chunk"        pixels per launch of sar_runtime_basin's two kernels (default 2^20, at most 2^30; whole 8 x 8 tiles, at least one)
 *   "period_chunk"       pixels per launch of sar_runtime_period (default 2^20, at most 2^30; whole 8 x 8 tiles, at least one)
 *   "cycles_chunk"       (map, start) lanes per launch of sar_runtime_cycles' two kernels (default 2^21, at most 2^30; whole maps, at
 *                        least one): bounds its device scratch, the result does not depend on it
 *   "density_tile"       rows of the 32-pixel-wide tile a workgroup of sar_runtime_density's kernel owns: 8, 16 or 32 (default 16); the
 *                        result does not depend on it
 *   "corr_chunk"         workgroups (pairs of 256-point tiles) per launch of sar_runtime_pairs / sar_runtime_corrdim's pair kernel, and
 *                        256-job blocks per launch of its orbit kernel, whole maps and at least one (default 2^18, at most 2^30)
 *   "box_chunk"          sets (maps) per launch of sar_runtime_boxes / sar_runtime_boxdim's kernels (default and at most 65535)
 *   "box_slots"          slots of a set's hash tables in sar_runtime_boxes / sar_runtime_boxdim: 0 = the smallest power of two
 *                        >= 2 n; otherwise a power of two > n and at most 2^24 (refused by the call where it is not > n)
 * Everything else a laboratory wants to turn — accumulate path, bin geometry, chunk sizes, hint layout, launch-chunk caps,
 * the batched launch's variants — is NOT in this library: include/sar_test_hooks.h declares sar_runtime_set_test_option, which
 * only the hooks build of the test-suite links (tests/hooks/libsar_hip_hooks.so: the same object files plus that one function).
 *
 * Jobs of more than 2^32-2 iterations (Config::iterations is a usize, :267): a launch orders its visits with a 32-bit
 * ordinal, so such a job runs as successive launches that hand its state on — and it runs them ALONE, one lane of the
 * chip at ~1e6 iterations per second: the reference's tie rule is job-major (an earlier JOB wins an exact depth tie
 * whatever the iteration), and two jobs advancing through their segments side by side would fold a later job's early
 * visit before an earlier job's late one. Correct, but ~1e5 times slower than the same iterations cut into more jobs;
 * use jobs_total / jobs_per_unit so that a job stays below 2^32-2 iterations. */
int sar_runtime_set_option(sar_runtime* rt, const char* name, uint64_t value);
/* Diagnostic (host arithmetic only, no device needed): the pixel -> (bin, 16-bit record) map the LDS-binned path uses for
 * a width x height image with "bin_shift" / "bin_interleave" as given (0 = the defaults of a runtime without forced
 * options and 131072 jobs). out = {ok, bins, bin_shift, interleaved, seg_shift, bin_bits, hi_shift, low_mask}:
 *   bin = (idx >> seg_shift) & ((1 << bin_bits) - 1);  record = (idx & low_mask) | ((idx >> hi_shift) & ~low_mask)
 *   idx = (record & low_mask) | (bin << seg_shift) | ((record & ~low_mask) << hi_shift)
 * ok = 0: the image has no binned geometry (the one-atomic-per-visit path renders it). */
int sar_bin_geometry(uint32_t width, uint32_t height, uint32_t bin_shift, uint32_t bin_interleave, uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* SAR_H */
