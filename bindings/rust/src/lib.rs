//! Raw bindings to `include/sar.h` (the C ABI of the MI355X iterate/accumulate path).
//!
//! SOURCE ONLY: the image this repository is built in has no Rust toolchain, so this crate has never been
//! compiled there. `#[repr(C)] SarConfig` mirrors `struct sar_config` field by field; the layout the C side
//! expects is pinned by `tests/test_abi_and_host.py::test_struct_layout_matches_c`.
//! Each function names the item of Icelk/strange-attractor-renderer (`src/lib.rs`) it replaces.
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

pub const SAR_OK: c_int = 0;
pub const SAR_ERR_INVALID: c_int = 1;
pub const SAR_ERR_DIM_MISMATCH: c_int = 2;
pub const SAR_ERR_NO_DEVICE: c_int = 3;
pub const SAR_ERR_HIP: c_int = 4;
pub const SAR_ERR_OOM: c_int = 5;
pub const SAR_ERR_RANGE: c_int = 6;
pub const SAR_ERR_IO: c_int = 7;
pub const SAR_ERR_INTERNAL: c_int = 8;

pub const SAR_RENDER_GAS: i32 = 0; // RenderKind::Gas   (:233-239)
pub const SAR_RENDER_DEPTH: i32 = 1; // RenderKind::Depth
pub const SAR_CT_POISSON_SATURNE: i32 = 0; // color_transforms::poisson_saturne (:520)
pub const SAR_CT_ADJUSTED_VELOCITY: i32 = 1; // color_transforms::AdjustedVelocity (:507)
pub const SAR_PALETTE_MAX: usize = 15;
pub const SAR_FMT_RGBA16: c_int = 0;
pub const SAR_FMT_RGB16: c_int = 1;
pub const SAR_FMT_RGBA8: c_int = 2;
pub const SAR_FMT_RGB8: c_int = 3;

#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SarConfig {
    pub iterations: u64,
    pub width: u32,
    pub height: u32,
    pub render_kind: i32,
    pub transparent: i32,
    pub angle: f64,
    pub silent: i32,
    pub attractor_kind: i32,
    pub coeff_x: [f64; 10],
    pub coeff_y: [f64; 10],
    pub coeff_z: [f64; 10],
    pub palette_len: u32,
    pub _pad0: u32,
    pub palette_rgb: [[f64; 3]; SAR_PALETTE_MAX],
    pub brightness_offset: f64,
    pub brightness_factor: f64,
    pub center_camera: [f64; 3],
    pub rotation_axis: [f64; 3],
    pub rotation_angle: f64,
    pub scale: f64,
    pub color_transform: i32,
    pub _pad1: i32,
    pub ct_offset: f64,
    pub ct_factor: f64,
    pub seed: u64,
    pub jobs_total: u32,
    pub _pad2: u32,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarTiming {
    pub iterate_ms: f32,
    pub resolve_ms: f32,
    pub colorize_ms: f32,
    pub merge_ms: f32,
    pub iterate_launches: u32,
    pub warmup_ms: f32,
    pub iterations_counted: u64,
    pub depth_atomics: u64,
    pub depth_candidates: u64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarParallelTiming {
    pub total_ms: f32,
    pub render_ms: f32,
    pub exchange_ms: f32,
    pub colorize_ms: f32,
    pub n_devices: u32,
    pub peer_access_failures: u32,
    pub exchange_bytes_per_device: u64,
    pub host_ms_before_exchange: f32,
    pub host_ms_enqueue: f32,
    pub draw_ahead_ms: f32,
    pub _pad: f32,
}

/// Parameters of the chaotic-map search (sar_runtime_search); sar_search_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSearchParams {
    pub seed: u64,
    pub lo: f64,
    pub hi: f64,
    pub start: [f64; 3],
    pub transient: u32,
    pub steps: u32,
    pub bound: f64,
    pub min_lyapunov: f64,
    pub min_ky_dim: f64,
    pub keep_rejected: i32,
    pub _pad: i32,
}

/// One phase-2 candidate of the search: raw accumulators (bit-exact), Lyapunov spectrum, Kaplan-Yorke dimension, extent.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSearchRecord {
    pub candidate: u64,
    pub status: i32,
    pub steps_done: u32,
    pub log2_exp: [i64; 3],
    pub mant: [f64; 3],
    pub lyapunov: [f64; 3],
    pub ky_dim: f64,
    pub extent: [f64; 6],
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSearchStats {
    pub tested: u64,
    pub diverged_transient: u64,
    pub diverged_late: u64,
    pub degenerate: u64,
    pub below_lyapunov: u64,
    pub below_dim: u64,
    pub accepted: u64,
}
/// A Lyapunov plane (sar_runtime_plane); sar_plane_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SarPlaneParams {
    pub base: [f64; 30],
    pub axis: [u32; 2],
    pub lo: [f64; 2],
    pub hi: [f64; 2],
    pub width: u32,
    pub height: u32,
    pub start: [f64; 3],
    pub transient: u32,
    pub steps: u32,
    pub bound: f64,
    pub mode: i32,
    pub _pad: i32,
}

/// One pixel of a Lyapunov plane: raw accumulators (bit-exact), exponents (L1: [0] only), Kaplan-Yorke dimension (spectrum).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPlaneRecord {
    pub status: i32,
    pub transient_done: u32,
    pub steps_done: u32,
    pub _pad: u32,
    pub log2_exp: [i64; 3],
    pub mant: [f64; 3],
    pub lyapunov: [f64; 3],
    pub ky_dim: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPlaneStats {
    pub pixels: u64,
    pub diverged_transient: u64,
    pub diverged_late: u64,
    pub degenerate: u64,
    pub bounded: u64,
}

/// The colours of sar_runtime_plane_colorize; sar_plane_colors_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPlaneColors {
    pub threshold: f64,
    pub chaos_scale: f64,
    pub order_scale: f64,
}

pub const SAR_PLANE_L1: i32 = 1;
pub const SAR_PLANE_SPECTRUM: i32 = 3;

/// Density estimation (sar_runtime_density): `samples` = S, 2..=256; sar_density_params_default fills the default, 64.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarDensityParams {
    pub samples: u32,
    pub _pad: u32,
}

/// What one call of the density filter did: the mass before (the sum of count) and after (Q16, modulo 2^64), the covered pixels
/// before and after, the pixels that spread (0 < count < S), the pixels that saturated at 0xFFFFFFFF, the maxima before and after.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarDensityStats {
    pub mass_in: u64,
    pub mass_q16: u64,
    pub covered_in: u32,
    pub covered_out: u32,
    pub spread: u32,
    pub saturated: u32,
    pub max_in: u32,
    pub max_out: u32,
}

/// Auto exposure (sar_runtime_exposure / sar_runtime_set_exposure): the quantiles of the covered counts that become the black
/// and white levels; sar_exposure_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarExposureParams {
    pub q_black: f64,
    pub q_white: f64,
    pub level_black: f64,
    pub level_white: f64,
}

/// What an exposure found: the constants colorize uses (the config's when `applied` is 0), the quantile counts, n and M.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarExposure {
    pub offset: f64,
    pub factor: f64,
    pub black_count: u32,
    pub white_count: u32,
    pub covered: u32,
    pub max: u32,
    pub applied: i32,
    pub _pad: i32,
}

/// Auto colour range (sar_runtime_color_range / sar_runtime_set_color_range): the quantiles of the covered steps that become the
/// palette positions pos_lo and pos_hi; sar_color_range_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarColorRangeParams {
    pub q_lo: f64,
    pub q_hi: f64,
    pub pos_lo: f64,
    pub pos_hi: f64,
}

/// A palette window: steps in [lo, hi] map to the palette positions [pos_lo, pos_hi]; `applied` 0: colorize uses steps as they are.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarColorRange {
    pub lo: f64,
    pub hi: f64,
    pub pos_lo: f64,
    pub pos_hi: f64,
    pub covered: u32,
    pub applied: i32,
}

/// Shaded rendering (sar_shade): the light (towards it, image space), the weights, the occlusion disc, the pre-smoothing, the
/// surface test's min_count, the background and an optional palette window; sar_shade_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarShadeParams {
    pub light: [f64; 3],
    pub ambient: f64,
    pub diffuse: f64,
    pub specular: f64,
    pub ao_strength: f64,
    pub ao_range: f64,
    pub smooth_range: f64,
    pub shininess_log2: u32,
    pub ao_radius: u32,
    pub smooth: i32,
    pub min_count: u32,
    pub background: [u16; 3],
    pub _pad0: u16,
    pub has_window: i32,
    pub _pad1: i32,
    pub window: SarColorRange,
}

/// What one shade call saw: surface and background pixels (they sum to the image), surface pixels without a surface 4-neighbour,
/// with any occlusion, and whose smoothing window took in more than the centre.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarShadeStats {
    pub surface: u32,
    pub background: u32,
    pub isolated: u32,
    pub occluded: u32,
    pub smoothed: u32,
    pub _pad: u32,
}

/// Flows (sar_runtime_render_flow): the 30 coefficients read as the vector field p' = P(p), integrated by RK4 with the fixed step
/// `dt`; a job that leaves the `bound` box has escaped. sar_flow_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarFlowParams {
    pub dt: f64,
    pub bound: f64,
    pub transient: u32,
    pub stride: u32,
    pub plot: i32,
    pub chunk_jobs: u32,
    pub chunk_steps: u32,
    pub _pad: u32,
}

/// What one flow call did: the counted steps, the plotted points inside and outside the image, the jobs by fate, the atomics it
/// sent or offered, the raw extent [xmin, xmax, ymin, ymax, zmin, zmax] of the counted points and the runtime's max after it.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarFlowStats {
    pub steps: u64,
    pub visits: u64,
    pub outside: u64,
    pub escaped_transient: u64,
    pub escaped: u64,
    pub alive: u64,
    pub count_atomics: u64,
    pub key_atomics: u64,
    pub extent: [f64; 6],
    pub max: u32,
    pub _pad: u32,
}

/// Poincare sections of flows (sar_runtime_section): the surface g = surface . [1, x, x^2, xy, xz, y, y^2, yz, z, z^2], the flow's step
/// and bound, which crossings count (`direction` +1 up, -1 down, 0 both), how many each job records and how long it may look.
/// sar_section_params_default fills everything but the surface.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSectionParams {
    pub surface: [f64; 10],
    pub dt: f64,
    pub bound: f64,
    pub transient: u32,
    pub direction: i32,
    pub samples: u32,
    pub max_steps: u32,
    pub plot: i32,
    pub chunk_jobs: u32,
    pub chunk_steps: u32,
    pub _pad: u32,
}

/// One job of a section: its status (SAR_SECTION_*), the recorded crossings and the rough ones among them, the counted steps it
/// took and the step of its clock crossing (SAR_SECTION_NO_CLOCK without one).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSectionRecord {
    pub status: u32,
    pub found: u32,
    pub rough: u32,
    pub steps: u32,
    pub clock_step: u32,
    pub _pad: u32,
}

/// What one section call did: the steps and crossings, the jobs by status, the plotted crossings inside and outside the image, the
/// raw extent of the recorded crossings, the extrema of the return times, the largest residual |g(q)| and the runtime's max.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSectionStats {
    pub steps: u64,
    pub crossings: u64,
    pub rough: u64,
    pub clocked: u64,
    pub full: u64,
    pub short_jobs: u64,
    pub escaped: u64,
    pub escaped_transient: u64,
    pub visits: u64,
    pub outside: u64,
    pub extent: [f64; 6],
    pub ret_min: f64,
    pub ret_max: f64,
    pub residual_max: f64,
    pub max: u32,
    pub _pad: u32,
}

pub const SAR_SECTION_FULL: u32 = 0;
pub const SAR_SECTION_SHORT: u32 = 1;
pub const SAR_SECTION_ESCAPED: u32 = 2;
pub const SAR_SECTION_ESCAPED_TRANSIENT: u32 = 3;
pub const SAR_SECTION_NO_CLOCK: u32 = 0xFFFF_FFFF;

/// Volume rendering (sar_runtime_volume): the depth range [z_lo, z_hi) cut into `slabs` slabs, and whether the call replaces the
/// held volume (add = 0) or adds to it (add = 1); sar_volume_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarVolumeParams {
    pub z_lo: f64,
    pub z_hi: f64,
    pub slabs: u32,
    pub add: i32,
}

/// What the held volume holds: in-bounds visits = stored + below + above + nan, the non-empty voxels, the largest voxel and the
/// range of the finite depths.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarVolumeStats {
    pub visits: u64,
    pub stored: u64,
    pub below: u64,
    pub above: u64,
    pub nan: u64,
    pub nonempty: u64,
    pub vmax: u32,
    pub z_min: f32,
    pub z_max: f32,
    pub _pad: u32,
}

/// The march (sar_runtime_volume_march): the half-opacity count (0: from vmax), the transmittance at which a ray stops, the palette
/// positions of the two ends, the slabs marched (k1 = 0: all of them) and the background of an opaque image.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarVolumeMarchParams {
    pub half_count: f64,
    pub t_min: f64,
    pub pos_lo: f64,
    pub pos_hi: f64,
    pub k0: u32,
    pub k1: u32,
    pub background: [u16; 3],
    pub _pad: u16,
}

/// What one march saw: the non-empty voxels its rays read, the pixels that saw any and those whose ray stopped at t_min.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarVolumeMarchStats {
    pub slabs_seen: u64,
    pub covered: u32,
    pub stopped: u32,
}

/// One tile of a gallery (sar_runtime_gallery): what differs from tile to tile — the map (x, y, z rows of 10) and its view.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarGalleryItem {
    pub coeff: [f64; 30],
    pub center_camera: [f64; 3],
    pub scale: f64,
}

/// The shape of a gallery: tile size (at most 16 384 pixels), tiles per atlas row, trajectories and iterations per tile, the seed of
/// the shared start points; sar_gallery_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarGalleryParams {
    pub tile_width: u32,
    pub tile_height: u32,
    pub cols: u32,
    pub jobs: u32,
    pub iterations: u64,
    pub seed: u64,
}

/// A tile's scalars: Runtime::max, covered pixels, visits that landed in the tile, trajectories dropped in the warm-up.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarGalleryStats {
    pub max: u32,
    pub covered: u32,
    pub hits: u64,
    pub dead_jobs: u32,
    pub _pad: u32,
}

/// An orbit diagram (sar_runtime_orbit): the line of maps from `a` to `b` (x, y, z rows of 10), `width` columns of `height` bins,
/// `jobs` trajectories per column, the projection and the plotted range; sar_orbit_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarOrbitParams {
    pub a: [f64; 30],
    pub b: [f64; 30],
    pub width: u32,
    pub height: u32,
    pub jobs: u32,
    pub transient: u32,
    pub steps: u32,
    pub _pad: u32,
    pub seed: u64,
    pub bound: f64,
    pub proj: [f64; 3],
    pub v_lo: f64,
    pub v_hi: f64,
}

/// A column's scalars: its jobs by fate, occupied bins, largest bin, live visits inside / outside the range, the extent of v.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarOrbitColumn {
    pub dead_transient: u32,
    pub dead_late: u32,
    pub alive: u32,
    pub occupied: u32,
    pub max: u32,
    pub _pad: u32,
    pub hits: u64,
    pub misses: u64,
    pub vmin: f64,
    pub vmax: f64,
}

/// A basin picture (sar_runtime_basin): the map (x, y, z rows of 10), the plane of start points origin + du * tu + dv * tv over
/// `width` x `height` pixels, the steps, and the box whose `grid`^3 cells are the nodes of the attractors; sar_basin_params_default
/// fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinParams {
    pub coeffs: [f64; 30],
    pub origin: [f64; 3],
    pub du: [f64; 3],
    pub dv: [f64; 3],
    pub width: u32,
    pub height: u32,
    pub transient: u32,
    pub steps: u32,
    pub bound: f64,
    pub grid: u32,
    pub _pad: u32,
    pub box_lo: [f64; 3],
    pub box_hi: [f64; 3],
}

/// A pixel's fate: status (SAR_SEARCH_BOUNDED / SAR_SEARCH_DIVERGED), the escape step, and its attractor by root and by label
/// (0xFFFFFFFF both for an escaped pixel).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinPixel {
    pub status: i32,
    pub escape_step: u32,
    pub root: u32,
    pub label: u32,
}

/// One attractor of the table: its root, the size of its basin, its cells, the basin's lowest pixel index and the bounding cells.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinAttractor {
    pub root: u32,
    pub pixels: u32,
    pub cells: u32,
    pub first_pixel: u32,
    pub cell_lo: [u32; 3],
    pub cell_hi: [u32; 3],
}

/// The pixels by fate, the attractors, the occupied cells and the raw extent of all tail points.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinStats {
    pub pixels: u64,
    pub escaped_transient: u64,
    pub escaped_tail: u64,
    pub bounded: u64,
    pub attractors: u64,
    pub cells: u64,
    pub extent: [f64; 6],
}

/// The colours of sar_runtime_basin_colorize: the escape step at which the grey is half its ceiling.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinColors {
    pub fade: f64,
}

/// Label of a BOUNDED probe none of whose tail points lies in a labelled cell of the held basin picture.
pub const SAR_BASIN_UNKNOWN: u32 = 0xFFFF_FFFE;
pub const SAR_BASIN_MAX_LEVELS: u32 = 31;

/// The fate of one start point in the held basin picture (sar_runtime_basin_fates): status, the escape step, the label found along
/// the tail (SAR_BASIN_UNKNOWN: none; 0xFFFFFFFF: DIVERGED) and the tail point that gave it.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinFate {
    pub status: i32,
    pub escape_step: u32,
    pub label: u32,
    pub hit: u32,
}

/// The fates of a call counted: diverged + labelled + unknown = points.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinFateCounts {
    pub points: u64,
    pub diverged: u64,
    pub labelled: u64,
    pub unknown: u64,
}

/// An uncertainty ladder (sar_runtime_basin_uncertainty): the direction, e_1 = eps0, K = levels with e_k = eps0 / 2^(k - 1), and the
/// base points per launch; sar_basin_ladder_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinLadderParams {
    pub dir: [f64; 3],
    pub eps0: f64,
    pub levels: u32,
    pub chunk: u32,
}

/// One level of a ladder: e_k and the exact counts, tested = n - unknown.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinUncertaintyLevel {
    pub eps: f64,
    pub tested: u64,
    pub uncertain: u64,
    pub unknown: u64,
}

/// One base point of a ladder: bit k - 1 of each word is level k.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBasinLadderMask {
    pub uncertain_bits: u32,
    pub unknown_bits: u32,
}

/// Flags of a pixel of an FTLE map (SarFtlePixel::flags).
pub const SAR_FTLE_EDGE: u32 = 1;
pub const SAR_FTLE_ONE_SIDED_U: u32 = 2;
pub const SAR_FTLE_ONE_SIDED_V: u32 = 4;
pub const SAR_FTLE_NO_U: u32 = 8;
pub const SAR_FTLE_NO_V: u32 = 16;

/// An FTLE map (sar_runtime_ftle): the map (x, y, z rows of 10), the plane of start points origin + du * tu + dv * tv over
/// `width` x `height` pixels as in SarBasinParams, the steps N of the flow map and the pixels per launch; sar_ftle_params_default
/// fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarFtleParams {
    pub coeffs: [f64; 30],
    pub origin: [f64; 3],
    pub du: [f64; 3],
    pub dv: [f64; 3],
    pub width: u32,
    pub height: u32,
    pub steps: u32,
    pub chunk: u32,
    pub bound: f64,
}

/// One pixel of an FTLE map: its fate, its end point F^N(start), the Gram entries of the differences between its neighbours' end
/// points (the device's fields), and the host finish: the largest squared stretching and ftle = ln(stretch2) / (2 N).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarFtlePixel {
    pub status: i32,
    pub escape_step: u32,
    pub flags: u32,
    pub _pad: u32,
    pub end: [f64; 3],
    pub g11: f64,
    pub g12: f64,
    pub g22: f64,
    pub stretch2: f64,
    pub ftle: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarFtleStats {
    pub pixels: u64,
    pub escaped: u64,
    pub bounded: u64,
    pub edge: u64,
    pub one_sided: u64,
    pub isolated: u64,
    pub ftle_min: f64,
    pub ftle_max: f64,
}

/// The colours of sar_runtime_ftle_colorize: the palette's window of ftle and the basins' fade for the escaped pixels.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarFtleColors {
    pub lo: f64,
    pub hi: f64,
    pub fade: f64,
}

/// The windows of the power spectra (SarSpectraParams::window, SarSpectrumParams::window).
pub const SAR_WINDOW_RECT: u32 = 0;
pub const SAR_WINDOW_HANN: u32 = 1;

/// The power spectra of point sets (sar_runtime_spectra): the transform size N, the hop between segments, the window, the samples
/// of a trajectory (0: the whole set), the (set, job) workgroups per launch and the plotted projection; sar_spectra_params_default
/// fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSpectraParams {
    pub n: u32,
    pub hop: u32,
    pub window: u32,
    pub samples: u32,
    pub chunk: u32,
    pub _pad: u32,
    pub proj: [f64; 3],
}

/// One set's record of sar_runtime_spectra: its trajectories, the segments of each, and the energy E (sum c_k P[k] = N E).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSpectraRecord {
    pub jobs: u32,
    pub segments: u32,
    pub energy: f64,
}

/// The power spectra of maps (sar_runtime_spectrum): every job records (segments - 1) * hop + n points; sar_spectrum_params_default
/// fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSpectrumParams {
    pub jobs: u32,
    pub segments: u32,
    pub n: u32,
    pub hop: u32,
    pub window: u32,
    pub stride: u32,
    pub transient: u32,
    pub chunk: u32,
    pub seed: u64,
    pub bound: f64,
    pub proj: [f64; 3],
}

/// One map's record of sar_runtime_spectrum: the common header of the recorded orbits, then the segments per job and the energy
/// (both 0 for a DIVERGED map).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarSpectrumRecord {
    pub status: i32,
    pub fail_job: u32,
    pub fail_step: u64,
    pub extent: [f64; 6],
    pub segments: u32,
    pub _pad: u32,
    pub energy: f64,
}

/// The recurrence analysis of point sets (sar_runtime_recurrence, sar_runtime_recurrence_plot): the samples of a trajectory (0: the
/// whole set), the Theiler window, the bins B of the line-length histograms, the workgroups per launch and the squared threshold;
/// sar_recurrence_params_default fills the defaults (eps2 = 0 is refused: set it).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarRecurrenceParams {
    pub samples: u32,
    pub theiler: u32,
    pub line_bins: u32,
    pub chunk: u32,
    pub eps2: f64,
}

/// One set's counts of sar_runtime_recurrence: the recurrences in the upper triangle, the pairs outside the Theiler window, the
/// diagonal and vertical lines and the longest of each, exact.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarRecurrenceRecord {
    pub recurrences: u64,
    pub pairs: u64,
    pub diag_lines: u64,
    pub vert_lines: u64,
    pub diag_longest: u64,
    pub vert_longest: u64,
}

/// The recurrence analysis of maps (sar_runtime_rqa): the recorded orbits as sar_runtime_corrdim's, then the Theiler window, the
/// bins, the workgroups per launch and the threshold — eps2, or where that is 0 eps_fraction of the diagonal of every map's extent;
/// sar_rqa_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarRqaParams {
    pub jobs: u32,
    pub samples: u32,
    pub stride: u32,
    pub transient: u32,
    pub seed: u64,
    pub bound: f64,
    pub theiler: u32,
    pub line_bins: u32,
    pub chunk: u32,
    pub _pad: u32,
    pub eps2: f64,
    pub eps_fraction: f64,
}

/// One map's record of sar_runtime_rqa: the common header of the recorded orbits, the eps2 used (0: nothing was counted) and the
/// counts.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarRqaRecord {
    pub status: i32,
    pub fail_job: u32,
    pub fail_step: u64,
    pub extent: [f64; 6],
    pub eps2: f64,
    pub counts: SarRecurrenceRecord,
}

/// The measures of sar_rqa_measures: RR, DET, the mean diagonal line, 1 / l_max, the entropy of the diagonal lines, LAM, the
/// trapping time, and the longest diagonal and vertical line.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarRqaMeasures {
    pub rr: f64,
    pub det: f64,
    pub l_mean: f64,
    pub div: f64,
    pub entr: f64,
    pub lam: f64,
    pub tt: f64,
    pub l_max: u64,
    pub v_max: u64,
}

/// A period plane (sar_runtime_period): the Lyapunov planes' plane (base, two swept coefficients, ranges, size), the start point,
/// the transient, the longest period looked for, the bound box and the tolerance of a return; sar_period_params_default fills the
/// defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SarPeriodParams {
    pub base: [f64; 30],
    pub axis: [u32; 2],
    pub lo: [f64; 2],
    pub hi: [f64; 2],
    pub width: u32,
    pub height: u32,
    pub start: [f64; 3],
    pub transient: u32,
    pub max_period: u32,
    pub bound: f64,
    pub eps: f64,
}

/// One pixel of a period plane: status (SAR_SEARCH_BOUNDED / SAR_SEARCH_DIVERGED), the step of the orbit's first return (0: none),
/// the steps run and the max-norm distance at the return (NaN without one).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPeriodRecord {
    pub status: i32,
    pub period: u32,
    pub transient_done: u32,
    pub steps_done: u32,
    pub residual: f64,
}

#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPeriodStats {
    pub pixels: u64,
    pub diverged_transient: u64,
    pub diverged_late: u64,
    pub periodic: u64,
    pub aperiodic: u64,
    pub max_period_found: u64,
}

pub const SAR_CYCLE_CONVERGED: i32 = 0;
pub const SAR_CYCLE_ESCAPED: i32 = 1;
pub const SAR_CYCLE_SINGULAR: i32 = 2;
pub const SAR_CYCLE_NOT_CONVERGED: i32 = 3;

/// The cycles of maps (sar_runtime_cycles): the period p, the starts (the caller's `jobs`, or the lattice of grid^3 points over the
/// box), the Newton iteration's limits and the merge's resolutions; sar_cycles_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SarCyclesParams {
    pub period: u32,
    pub jobs: u32,
    pub grid: u32,
    pub max_newton: u32,
    pub cap: u32,
    pub _pad: u32,
    pub box_lo: [f64; 3],
    pub box_hi: [f64; 3],
    pub tol: f64,
    pub bound: f64,
    pub merge: f64,
    pub same: f64,
}

/// One map's starts by outcome, its orbits kept and lost, and the sum of the starts' Newton iterations.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarCyclesRecord {
    pub converged: u32,
    pub escaped: u32,
    pub singular: u32,
    pub not_converged: u32,
    pub n_orbits: u32,
    pub orbits_lost: u32,
    pub hits_lost: u32,
    pub _pad: u32,
    pub newton_iterations: u64,
}

/// One orbit slot: the representative, the minimal period, the leading start, the starts merged into it, the head's iterations,
/// max|F^q(rep) - rep| and M = D F^q at rep, row-major.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarCycleOrbit {
    pub rep: [f64; 3],
    pub period: u32,
    pub head: u32,
    pub hits: u32,
    pub newton: u32,
    pub residual: f64,
    pub m: [f64; 9],
}

pub const SAR_MANIFOLD_OK: i32 = 0;
pub const SAR_MANIFOLD_DOMAIN_ESCAPED: i32 = 1;

/// The unstable manifolds (sar_runtime_manifold): the samples of a fundamental domain, the steps, the longest segment drawn and
/// the bound; sar_manifold_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct SarManifoldParams {
    pub samples: u32,
    pub steps: u32,
    pub max_span: u32,
    pub _pad: u32,
    pub bound: f64,
}

/// One branch: a point of the cycle, the direction (not normalised by the library), delta and the map steps per return.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarManifoldBranch {
    pub base: [f64; 3],
    pub dir: [f64; 3],
    pub delta: f64,
    pub period: u32,
    pub _pad: u32,
}

/// One branch's outcome: the status, the fundamental domain's ends, the segments by class, the plots inside the image, the drawn
/// length in pixels, the first step with a long segment (0xFFFFFFFF: none) and the points alive at the last step.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarManifoldRecord {
    pub status: i32,
    pub first_long_step: u32,
    pub alive_end: u32,
    pub _pad: u32,
    pub a: [f64; 3],
    pub b: [f64; 3],
    pub n_drawn: u64,
    pub n_dead: u64,
    pub n_far: u64,
    pub n_long: u64,
    pub pixels: u64,
    pub length_px: u64,
}

/// The colours of sar_runtime_period_colorize: the palette slots the periods cycle through.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPeriodColors {
    pub colours: u32,
    pub _pad: u32,
}

/// The binning and the trajectories of a pair histogram (sar_runtime_pairs); sar_pairs_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPairsParams {
    pub samples: u32,
    pub theiler: u32,
    pub sub_bits: u32,
    pub e_min: i32,
    pub e_max: i32,
    pub _pad: u32,
}

/// A set's pairs: counted (the sum of its histogram) and skipped by the Theiler window.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarPairsCounts {
    pub counted: u64,
    pub skipped: u64,
}

/// The least-squares line of ln C on ln r over a window (sar_corrdim_fit): `slope` is the correlation dimension D2.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarCorrdimLine {
    pub slope: f64,
    pub intercept: f64,
    pub rms: f64,
    pub first_bin: u32,
    pub last_bin: u32,
    pub used: u32,
    pub status: i32,
}

/// The correlation dimension of maps (sar_runtime_corrdim); sar_corrdim_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarCorrdimParams {
    pub jobs: u32,
    pub samples: u32,
    pub stride: u32,
    pub transient: u32,
    pub theiler: u32,
    pub sub_bits: u32,
    pub e_min: i32,
    pub e_max: i32,
    pub seed: u64,
    pub bound: f64,
    pub c_lo: f64,
    pub r_hi_fraction: f64,
}

/// One map's record: status (SAR_SEARCH_BOUNDED / SAR_SEARCH_DIVERGED), the first failure, the pairs, the extent and the line.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarCorrdimRecord {
    pub status: i32,
    pub fail_job: u32,
    pub fail_step: u64,
    pub counted: u64,
    pub skipped: u64,
    pub extent: [f64; 6],
    pub r_hi: f64,
    pub line: SarCorrdimLine,
}

pub const SAR_BOXDIM_FIT_OK: i32 = 0;
pub const SAR_BOXDIM_NO_WINDOW: i32 = 1;

/// The cube of a box count (sar_runtime_boxes) and its halvings; sar_box_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBoxParams {
    pub levels: u32,
    pub _pad: u32,
    pub origin: [f64; 3],
    pub size: f64,
}

/// One level of one set: the occupied cells, those with one point, the sum of n_i^2 and of n_i lg32(n_i).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBoxLevel {
    pub cells: u64,
    pub singles: u64,
    pub sum_sq: u64,
    pub n_log_n: u64,
}

/// One least-squares line over a window of levels (sar_boxdim_fit).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBoxdimLine {
    pub slope: f64,
    pub intercept: f64,
    pub rms: f64,
}

/// The three lines of a set: the slopes of d0, d1 and d2 are the capacity, information and correlation dimensions.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBoxdimLines {
    pub d0: SarBoxdimLine,
    pub d1: SarBoxdimLine,
    pub d2: SarBoxdimLine,
    pub first_level: u32,
    pub last_level: u32,
    pub used: u32,
    pub status: i32,
}

/// The box-counting dimensions of maps (sar_runtime_boxdim); sar_boxdim_params_default fills the defaults.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBoxdimParams {
    pub jobs: u32,
    pub samples: u32,
    pub stride: u32,
    pub transient: u32,
    pub levels: u32,
    pub l_min: u32,
    pub seed: u64,
    pub bound: f64,
    pub min_occupancy: f64,
}

/// One map's record: status (SAR_SEARCH_BOUNDED / SAR_SEARCH_DIVERGED), the first failure, the extent, the cube and the lines.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarBoxdimRecord {
    pub status: i32,
    pub fail_job: u32,
    pub fail_step: u64,
    pub extent: [f64; 6],
    pub origin: [f64; 3],
    pub size: f64,
    pub lines: SarBoxdimLines,
}

pub const SAR_CORRDIM_FIT_OK: i32 = 0;
pub const SAR_CORRDIM_NO_WINDOW: i32 = 1;

pub const SAR_SEARCH_BOUNDED: i32 = 0;
pub const SAR_SEARCH_DIVERGED: i32 = 1;
pub const SAR_SEARCH_DEGENERATE: i32 = 2;

#[repr(C)]
pub struct SarRuntime {
    _private: [u8; 0],
}
#[repr(C)]
pub struct SarRenderer {
    _private: [u8; 0],
}
#[repr(C)]
pub struct SarExchange {
    _private: [u8; 0],
}
/// Geometry of the sliced exchange (sar_exchange_new).
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct SarExchangeLayout {
    pub world: u32,
    pub rank: u32,
    pub slice_pixels: u32,
    pub first_px: u32,
    pub n_px: u32,
    pub granules: u32,
    pub block_bytes: u64,
}

extern "C" {
    pub fn sar_abi_version() -> c_int;
    pub fn sar_build_id() -> *const c_char;
    pub fn sar_device_pci_bus_id(device: c_int, out: *mut c_char, cap: usize) -> c_int;
    pub fn sar_checksum_fnv1a64(data_host: *const c_void, nbytes: usize, out: *mut u64) -> c_int;
    pub fn sar_status_string(status: c_int) -> *const c_char;
    pub fn sar_last_error() -> *const c_char;
    pub fn sar_device_count(out_count: *mut c_int) -> c_int;

    pub fn sar_config_poisson_saturne(out: *mut SarConfig) -> c_int; // Config::poisson_saturne (:310)
    pub fn sar_config_solar_sail(out: *mut SarConfig) -> c_int; // Config::solar_sail (:355)
    pub fn sar_config_validate(cfg: *const SarConfig) -> c_int;
    pub fn sar_rotation_matrix(cfg: *const SarConfig, m_out: *mut f64) -> c_int; // to_rotation_matrix (:176)
    pub fn sar_start_points(seed: u64, first_job: u64, n_jobs: u32, xyz_out_host: *mut f64) -> c_int;

    pub fn sar_runtime_new(cfg: *const SarConfig, device: c_int, out: *mut *mut SarRuntime) -> c_int; // Runtime::new (:660)
    pub fn sar_runtime_free(rt: *mut SarRuntime) -> c_int;
    pub fn sar_runtime_reset(rt: *mut SarRuntime) -> c_int; // Runtime::reset (:682)
    pub fn sar_runtime_set_width_height(rt: *mut SarRuntime, width: u32, height: u32) -> c_int; // (:667)
    pub fn sar_runtime_seed(rt: *mut SarRuntime, seed: u64) -> c_int;
    pub fn sar_runtime_merge(dst: *mut SarRuntime, src: *const SarRuntime) -> c_int; // Runtime::merge (:708)
    pub fn sar_runtime_synchronize(rt: *mut SarRuntime) -> c_int;
    pub fn sar_runtime_dims(rt: *const SarRuntime, width: *mut u32, height: *mut u32) -> c_int;
    pub fn sar_runtime_set_stream(rt: *mut SarRuntime, hip_stream: *mut c_void) -> c_int;
    pub fn sar_runtime_get_stream(rt: *const SarRuntime, hip_stream_out: *mut *mut c_void) -> c_int;

    pub fn sar_render(cfg: *const SarConfig, rt: *mut SarRuntime) -> c_int; // render (:747)
    pub fn sar_render_jobs(cfg: *const SarConfig, rt: *mut SarRuntime, starts_xyz_host: *const f64) -> c_int;
    pub fn sar_render_job_range(cfg: *const SarConfig, rt: *mut SarRuntime, n_jobs: u32, iters_per_job: u64,
                                starts_xyz_host: *const f64) -> c_int;
    pub fn sar_colorize(cfg: *const SarConfig, rt: *mut SarRuntime, rgba_out_host: *mut u16) -> c_int; // colorize (:841)
    pub fn sar_render_job_range_device(cfg: *const SarConfig, rt: *mut SarRuntime, n_jobs: u32, iters_per_job: u64,
                                       starts_xyz_dev: *const f64) -> c_int;
    pub fn sar_runtime_prefetch_device(cfg: *const SarConfig, rt: *mut SarRuntime, n_jobs: u32, iters_per_job: u64,
                                       starts_xyz_dev: *const f64) -> c_int;
    /// F frames of a sweep (src/bin/main.rs:493-517) through one set of launches: frame i == sar_render_jobs(cfgs[i], rts[i], starts[i]).
    pub fn sar_render_jobs_batch(n_frames: u32, cfgs: *const *const SarConfig, rts: *const *mut SarRuntime,
                                 starts_xyz_host: *const *const f64) -> c_int;
    /// n runtimes for the frames of one batch: one stream, one device and one page-locked allocation for all of them.
    pub fn sar_runtime_new_group(cfg: *const SarConfig, device: c_int, n: u32, out: *mut *mut SarRuntime) -> c_int;
    pub fn sar_runtime_reset_batch(n: u32, rts: *const *mut SarRuntime) -> c_int;
    pub fn sar_colorize_device_batch(n: u32, cfgs: *const *const SarConfig, rts: *const *mut SarRuntime, rgba_out_dev: *const *mut c_void) -> c_int;
    pub fn sar_runtime_batch_frames(cfg: *const SarConfig, rt: *mut SarRuntime, out_frames: *mut u32) -> c_int;
    pub fn sar_renderer_set_exchange(r: *mut SarRenderer, mode: u32) -> c_int;
    pub fn sar_runtime_get_copy_stream(rt: *mut SarRuntime, hip_stream_out: *mut *mut c_void) -> c_int;
    pub fn sar_runtime_set_copy_stream(rt: *mut SarRuntime, hip_stream: *mut c_void) -> c_int;
    pub fn sar_colorize_device(cfg: *const SarConfig, rt: *mut SarRuntime, rgba_out_dev: *mut c_void) -> c_int;
    pub fn sar_runtime_describe_last_launch(rt: *const SarRuntime, out: *mut c_char, cap: usize) -> c_int;

    pub fn sar_runtime_extent(cfg: *const SarConfig, rt: *mut SarRuntime, n_jobs: u32, iters_per_job: u64,
                              starts_xyz_host: *const f64, out12: *mut f64) -> c_int;
    // image export (src/bin/main.rs:40-100)
    pub fn sar_image_format(transparent: c_int, eight_bit: c_int) -> c_int;
    pub fn sar_image_bytes(format: c_int, width: u32, height: u32) -> usize;
    pub fn sar_image_convert_device(rt: *mut SarRuntime, rgba16_dev: *const c_void, format: c_int, out_dev: *mut c_void) -> c_int;
    pub fn sar_colorize_format(cfg: *const SarConfig, rt: *mut SarRuntime, format: c_int, out_host: *mut c_void) -> c_int;
    pub fn sar_colorize_format_async(cfg: *const SarConfig, rt: *mut SarRuntime, format: c_int, out_host: *mut c_void, ticket_out: *mut u64) -> c_int;
    pub fn sar_runtime_wait_image(rt: *mut SarRuntime, ticket: u64) -> c_int;
    pub fn sar_runtime_read_image_async(rt: *mut SarRuntime, out_host: *mut c_void, ticket_out: *mut u64) -> c_int;
    pub fn sar_runtime_image_done(rt: *mut SarRuntime, ticket: u64, done_out: *mut c_int) -> c_int;
    pub fn sar_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn sar_host_free(p: *mut c_void) -> c_int;
    pub fn sar_host_reserve(bytes: usize, count: u32) -> c_int;
    pub fn sar_write_png(path: *const c_char, format: c_int, width: u32, height: u32, pixels: *const c_void) -> c_int;
    pub fn sar_write_bmp(path: *const c_char, format: c_int, width: u32, height: u32, pixels: *const c_void) -> c_int;
    pub fn sar_write_pam(path: *const c_char, format: c_int, width: u32, height: u32, pixels: *const c_void) -> c_int;
    pub fn sar_runtime_count(rt: *mut SarRuntime, out_host: *mut u32) -> c_int;
    pub fn sar_runtime_steps(rt: *mut SarRuntime, out_host: *mut f64) -> c_int;
    pub fn sar_runtime_zbuf(rt: *mut SarRuntime, out_host: *mut f32) -> c_int;
    pub fn sar_runtime_max(rt: *mut SarRuntime, out_max: *mut u32) -> c_int;
    pub fn sar_runtime_load(rt: *mut SarRuntime, count_host: *const u32, steps_host: *const f64,
                            zbuf_host: *const f32, max: u32) -> c_int;

    // The ONE exchange step before colorize of a one-process-per-GPU host (Runtime::merge folded in rank order, :708-738, :1068-1076)
    // behind one context object; the collectives between the steps are the caller's.
    pub fn sar_exchange_slice_pixels(npix: u32, world: u32, out_slice_pixels: *mut u32) -> c_int;
    pub fn sar_exchange_new(rt: *mut SarRuntime, world: u32, rank: u32, out: *mut *mut SarExchange, layout_out: *mut SarExchangeLayout) -> c_int;
    pub fn sar_exchange_free(ex: *mut SarExchange) -> c_int;
    pub fn sar_exchange_flags(ex: *mut SarExchange, flags_out_dev: *mut u8) -> c_int;
    pub fn sar_exchange_pack(ex: *mut SarExchange, flags_all_dev: *const u8, dense_above: f64, send_dev: *mut c_void,
                             send_bytes: *mut u64, recv_bytes: *mut u64, sparse_out: *mut c_int) -> c_int;
    pub fn sar_exchange_merge(ex: *mut SarExchange, recv_dev: *const c_void, scalars_out_dev: *mut i64) -> c_int;
    pub fn sar_exchange_finish(ex: *mut SarExchange, scalars_reduced_dev: *const i64) -> c_int;
    pub fn sar_exchange_rooted(ex: *mut SarExchange, step: u32, key_i64_dev: *mut c_void, sum_i32_dev: *mut c_void) -> c_int;
    pub fn sar_colorize_range_device(cfg: *const SarConfig, rt: *mut SarRuntime, first_px: u32, n_px: u32,
                                     rgba_out_dev: *mut c_void) -> c_int;

    pub fn sar_renderer_new_multi(devices: *const c_int, n_devices: u32, units: u32, seed: u64,
                                  out: *mut *mut SarRenderer) -> c_int; // ParallelRenderer::new over several GPUs (:919)
    pub fn sar_renderer_num_devices(r: *const SarRenderer, out_devices: *mut u32) -> c_int;
    pub fn sar_renderer_last_timing(r: *const SarRenderer, out: *mut SarParallelTiming) -> c_int;
    pub fn sar_renderer_new(device: c_int, units: u32, seed: u64, out: *mut *mut SarRenderer) -> c_int; // ParallelRenderer::new (:919)
    pub fn sar_renderer_num_units(r: *const SarRenderer, out_units: *mut u32) -> c_int;
    pub fn sar_renderer_shutdown(r: *mut SarRenderer) -> c_int; // ParallelRenderer::shutdown (:1020)
    pub fn sar_render_parallel(r: *mut SarRenderer, cfg: *const SarConfig, jobs_per_unit: u32,
                               rgba_out_host: *mut u16) -> c_int; // render_parallel (:1051)
    pub fn sar_renderer_runtime(r: *mut SarRenderer, out_borrowed: *mut *mut SarRuntime) -> c_int;

    pub fn sar_runtime_enable_timing(rt: *mut SarRuntime, enabled: c_int) -> c_int;
    pub fn sar_runtime_last_timing(rt: *mut SarRuntime, out: *mut SarTiming) -> c_int;
    pub fn sar_runtime_set_option(rt: *mut SarRuntime, name: *const c_char, value: u64) -> c_int;
    pub fn sar_bin_geometry(width: u32, height: u32, bin_shift: u32, bin_interleave: u32, out: *mut u32) -> c_int;
    // the chaotic-map search
    pub fn sar_search_params_default(out: *mut SarSearchParams) -> c_int;
    pub fn sar_search_candidate(seed: u64, lo: f64, hi: f64, index: u64, out30: *mut f64) -> c_int;
    pub fn sar_runtime_search(rt: *mut SarRuntime, p: *const SarSearchParams, first: u64, n: u32, coeffs_host: *const f64,
                              out_host: *mut SarSearchRecord, cap: u32, n_out: *mut u32, stats_out: *mut SarSearchStats) -> c_int;
    pub fn sar_frame_view(cfg: *mut SarConfig, screen_extent6: *const f64, margin: f64, sweep: c_int) -> c_int;
    // Lyapunov planes
    pub fn sar_plane_params_default(out: *mut SarPlaneParams) -> c_int;
    pub fn sar_plane_coeffs(p: *const SarPlaneParams, x: u32, y: u32, out30: *mut f64) -> c_int;
    pub fn sar_runtime_plane(rt: *mut SarRuntime, p: *const SarPlaneParams, out_host: *mut SarPlaneRecord,
                             stats_out: *mut SarPlaneStats) -> c_int;
    pub fn sar_plane_colors_default(out: *mut SarPlaneColors) -> c_int;
    pub fn sar_runtime_plane_colorize(cfg: *const SarConfig, rt: *mut SarRuntime, colors: *const SarPlaneColors,
                                      rgba16_out_host: *mut u16) -> c_int;
    // auto exposure
    pub fn sar_exposure_params_default(out: *mut SarExposureParams) -> c_int;
    pub fn sar_runtime_exposure(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarExposureParams, out: *mut SarExposure) -> c_int;
    pub fn sar_runtime_set_exposure(rt: *mut SarRuntime, params: *const SarExposureParams) -> c_int;
    pub fn sar_renderer_set_exposure(r: *mut SarRenderer, params: *const SarExposureParams) -> c_int;
    // auto colour range
    pub fn sar_color_range_params_default(out: *mut SarColorRangeParams) -> c_int;
    pub fn sar_runtime_color_range(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarColorRangeParams, out: *mut SarColorRange) -> c_int;
    pub fn sar_runtime_set_color_range(rt: *mut SarRuntime, params: *const SarColorRangeParams) -> c_int;
    pub fn sar_runtime_hold_color_range(rt: *mut SarRuntime, range: *const SarColorRange) -> c_int;
    pub fn sar_renderer_set_color_range(r: *mut SarRenderer, params: *const SarColorRangeParams) -> c_int;
    pub fn sar_gallery_params_default(out: *mut SarGalleryParams) -> c_int;
    pub fn sar_runtime_gallery(rt: *mut SarRuntime, base: *const SarConfig, p: *const SarGalleryParams, n: u32, items_host: *const SarGalleryItem,
                               starts_xyz_host: *const f64, atlas_rgba16_out_host: *mut u16, count_out_host: *mut u32, zbuf_out_host: *mut f32,
                               steps_out_host: *mut f64, stats_out_host: *mut SarGalleryStats) -> c_int;
    pub fn sar_frame_view_box(cfg: *mut SarConfig, raw_extent6: *const f64, margin: f64, sweep: c_int) -> c_int;
    pub fn sar_orbit_params_default(out: *mut SarOrbitParams) -> c_int;
    pub fn sar_orbit_coeffs(p: *const SarOrbitParams, column: u32, out30: *mut f64) -> c_int;
    pub fn sar_pairs_params_default(out: *mut SarPairsParams) -> c_int;
    pub fn sar_pairs_edges(p: *const SarPairsParams, bins_out: *mut u32, r_out: *mut f64) -> c_int;
    pub fn sar_runtime_pairs(rt: *mut SarRuntime, p: *const SarPairsParams, n_sets: u32, n: u32, points_host: *const f64,
                             hist_out_host: *mut u64, counts_out_host: *mut SarPairsCounts) -> c_int;
    pub fn sar_corrdim_fit(hist: *const u64, binning: *const SarPairsParams, c_lo: f64, r_hi: f64, out: *mut SarCorrdimLine) -> c_int;
    pub fn sar_corrdim_params_default(out: *mut SarCorrdimParams) -> c_int;
    pub fn sar_runtime_corrdim(rt: *mut SarRuntime, p: *const SarCorrdimParams, n_maps: u32, coeffs_host: *const f64,
                               starts_xyz_host: *const f64, hist_out_host: *mut u64, records_out_host: *mut SarCorrdimRecord,
                               points_out_host: *mut f64) -> c_int;
    pub fn sar_box_params_default(out: *mut SarBoxParams) -> c_int;
    pub fn sar_box_log2_q32(n: u32, out: *mut u64) -> c_int;
    pub fn sar_runtime_boxes(rt: *mut SarRuntime, p: *const SarBoxParams, n_sets: u32, n: u32, points_host: *const f64,
                             levels_out_host: *mut SarBoxLevel) -> c_int;
    pub fn sar_boxdim_fit(levels: *const SarBoxLevel, l: u32, n: u32, l_min: u32, min_occupancy: f64, out: *mut SarBoxdimLines) -> c_int;
    pub fn sar_boxdim_params_default(out: *mut SarBoxdimParams) -> c_int;
    pub fn sar_runtime_boxdim(rt: *mut SarRuntime, p: *const SarBoxdimParams, n_maps: u32, coeffs_host: *const f64,
                              starts_xyz_host: *const f64, levels_out_host: *mut SarBoxLevel, records_out_host: *mut SarBoxdimRecord,
                              points_out_host: *mut f64) -> c_int;
    pub fn sar_runtime_orbit(rt: *mut SarRuntime, p: *const SarOrbitParams, starts_xyz_host: *const f64, count_out_host: *mut u32,
                             stats_out_host: *mut SarOrbitColumn, max_out: *mut u32) -> c_int;
    pub fn sar_basin_params_default(out: *mut SarBasinParams) -> c_int;
    pub fn sar_basin_start(p: *const SarBasinParams, x: u32, y: u32, out3: *mut f64) -> c_int;
    pub fn sar_runtime_basin(rt: *mut SarRuntime, p: *const SarBasinParams, pixels_out_host: *mut SarBasinPixel,
                             attractors_out_host: *mut SarBasinAttractor, cap: u32, n_out: *mut u32, stats_out: *mut SarBasinStats) -> c_int;
    pub fn sar_basin_colors_default(out: *mut SarBasinColors) -> c_int;
    pub fn sar_runtime_basin_colorize(cfg: *const SarConfig, rt: *mut SarRuntime, colors: *const SarBasinColors,
                                      rgba16_out_host: *mut u16) -> c_int;
    // basin probes
    pub fn sar_basin_ladder_params_default(out: *mut SarBasinLadderParams) -> c_int;
    pub fn sar_runtime_basin_fates(rt: *mut SarRuntime, n: u32, points_host: *const f64, fates_out_host: *mut SarBasinFate,
                                   counts_out: *mut SarBasinFateCounts) -> c_int;
    pub fn sar_runtime_basin_uncertainty(rt: *mut SarRuntime, p: *const SarBasinLadderParams, n: u32, base_host: *const f64,
                                         levels_out_host: *mut SarBasinUncertaintyLevel, fate0_out_host: *mut SarBasinFate,
                                         masks_out_host: *mut SarBasinLadderMask) -> c_int;
    // FTLE maps
    pub fn sar_ftle_params_default(out: *mut SarFtleParams) -> c_int;
    pub fn sar_ftle_start(p: *const SarFtleParams, x: u32, y: u32, out3: *mut f64) -> c_int;
    pub fn sar_runtime_ftle(rt: *mut SarRuntime, p: *const SarFtleParams, pixels_out_host: *mut SarFtlePixel,
                            stats_out: *mut SarFtleStats) -> c_int;
    pub fn sar_ftle_colors_default(out: *mut SarFtleColors) -> c_int;
    pub fn sar_runtime_ftle_colorize(cfg: *const SarConfig, rt: *mut SarRuntime, colors: *const SarFtleColors,
                                     rgba16_out_host: *mut u16) -> c_int;
    // power spectra
    pub fn sar_spectra_params_default(out: *mut SarSpectraParams) -> c_int;
    pub fn sar_spectrum_twiddles(n: u32, out: *mut f64) -> c_int;
    pub fn sar_spectrum_window(window: u32, n: u32, out: *mut f64) -> c_int;
    pub fn sar_spectra_segments(p: *const SarSpectraParams, n_points: u32, jobs_out: *mut u32, segments_out: *mut u32) -> c_int;
    pub fn sar_runtime_spectra(rt: *mut SarRuntime, p: *const SarSpectraParams, n_sets: u32, n_points: u32, points_host: *const f64,
                               power_out_host: *mut f64, records_out_host: *mut SarSpectraRecord) -> c_int;
    pub fn sar_spectrum_params_default(out: *mut SarSpectrumParams) -> c_int;
    pub fn sar_runtime_spectrum(rt: *mut SarRuntime, p: *const SarSpectrumParams, n_maps: u32, coeffs_host: *const f64,
                                starts_xyz_host: *const f64, power_out_host: *mut f64, records_out_host: *mut SarSpectrumRecord,
                                points_out_host: *mut f64) -> c_int;
    // recurrence analysis
    pub fn sar_recurrence_params_default(out: *mut SarRecurrenceParams) -> c_int;
    pub fn sar_runtime_recurrence(rt: *mut SarRuntime, p: *const SarRecurrenceParams, n_sets: u32, n: u32, points_host: *const f64,
                                  diag_out_host: *mut u64, vert_out_host: *mut u64, records_out_host: *mut SarRecurrenceRecord) -> c_int;
    pub fn sar_runtime_recurrence_plot(rt: *mut SarRuntime, p: *const SarRecurrenceParams, n: u32, points_host: *const f64, job: u32,
                                       i0: u32, j0: u32, height: u32, width: u32, out_host: *mut u8) -> c_int;
    pub fn sar_rqa_params_default(out: *mut SarRqaParams) -> c_int;
    pub fn sar_runtime_rqa(rt: *mut SarRuntime, p: *const SarRqaParams, n_maps: u32, coeffs_host: *const f64, starts_xyz_host: *const f64,
                           diag_out_host: *mut u64, vert_out_host: *mut u64, records_out_host: *mut SarRqaRecord,
                           points_out_host: *mut f64) -> c_int;
    pub fn sar_rqa_measures(diag: *const u64, vert: *const u64, record: *const SarRecurrenceRecord, line_bins: u32, l_min: u32, v_min: u32,
                            out: *mut SarRqaMeasures) -> c_int;
    // period planes
    pub fn sar_period_params_default(out: *mut SarPeriodParams) -> c_int;
    pub fn sar_period_coeffs(p: *const SarPeriodParams, x: u32, y: u32, out30: *mut f64) -> c_int;
    pub fn sar_runtime_period(rt: *mut SarRuntime, p: *const SarPeriodParams, coeffs_host: *const f64, records_out_host: *mut SarPeriodRecord,
                              stats_out: *mut SarPeriodStats) -> c_int;
    pub fn sar_period_colors_default(out: *mut SarPeriodColors) -> c_int;
    pub fn sar_runtime_period_colorize(cfg: *const SarConfig, rt: *mut SarRuntime, colors: *const SarPeriodColors,
                                       rgba16_out_host: *mut u16) -> c_int;
    // cycles
    pub fn sar_cycles_params_default(out: *mut SarCyclesParams) -> c_int;
    pub fn sar_cycles_starts(p: *const SarCyclesParams, out_xyz_host: *mut f64) -> c_int;
    pub fn sar_cycle_charpoly(m: *const f64, out3: *mut f64) -> c_int;
    pub fn sar_runtime_cycles(rt: *mut SarRuntime, p: *const SarCyclesParams, n_maps: u32, coeffs_host: *const f64,
                              starts_xyz_host: *const f64, records_out_host: *mut SarCyclesRecord,
                              orbits_out_host: *mut SarCycleOrbit) -> c_int;
    // unstable manifolds
    pub fn sar_manifold_params_default(out: *mut SarManifoldParams) -> c_int;
    pub fn sar_manifold_pixel(cfg: *const SarConfig, xyz: *const f64, out_fi_fj: *mut f64) -> c_int;
    pub fn sar_runtime_manifold(rt: *mut SarRuntime, cfg: *const SarConfig, params: *const SarManifoldParams, n_branches: u32,
                                branches_host: *const SarManifoldBranch, count_out_host: *mut u32, first_out_host: *mut u32,
                                records_out_host: *mut SarManifoldRecord) -> c_int;
    // density estimation
    pub fn sar_density_params_default(out: *mut SarDensityParams) -> c_int;
    pub fn sar_density_radius(params: *const SarDensityParams, out_radius: *mut u32) -> c_int;
    pub fn sar_density_weights(params: *const SarDensityParams, c: u32, out: *mut u32) -> c_int;
    pub fn sar_runtime_density(rt: *mut SarRuntime, params: *const SarDensityParams, stats_out: *mut SarDensityStats) -> c_int;
    pub fn sar_runtime_density_tiles(rt: *mut SarRuntime, tiles_out: *mut u32, copied_out: *mut u32) -> c_int;
    // shaded rendering
    pub fn sar_shade_params_default(out: *mut SarShadeParams) -> c_int;
    pub fn sar_shade(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarShadeParams, stats_out: *mut SarShadeStats,
                     rgba_out_host: *mut u16) -> c_int;
    pub fn sar_shade_device(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarShadeParams, stats_out: *mut SarShadeStats,
                            rgba_out_dev: *mut c_void) -> c_int;
    // flows
    pub fn sar_flow_params_default(out: *mut SarFlowParams) -> c_int;
    pub fn sar_flow_step(cfg: *const SarConfig, params: *const SarFlowParams, xyz: *mut f64, within_out: *mut i32) -> c_int;
    pub fn sar_runtime_render_flow(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarFlowParams, n_jobs: u32, steps_per_job: u64,
                                   starts_xyz_host: *const f64, stats_out: *mut SarFlowStats) -> c_int;
    // Poincare sections of flows
    pub fn sar_section_params_default(out: *mut SarSectionParams) -> c_int;
    pub fn sar_section_step(cfg: *const SarConfig, params: *const SarSectionParams, xyz: *mut f64, crossing: *mut f64, dt_out: *mut f64,
                            kind_out: *mut i32) -> c_int;
    pub fn sar_runtime_section(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarSectionParams, n_jobs: u32,
                               starts_xyz_host: *const f64, points_out: *mut f64, ret_out: *mut f64, records_out: *mut SarSectionRecord,
                               stats_out: *mut SarSectionStats) -> c_int;
    // volume rendering
    pub fn sar_volume_params_default(out: *mut SarVolumeParams) -> c_int;
    pub fn sar_volume_march_params_default(out: *mut SarVolumeMarchParams) -> c_int;
    pub fn sar_volume_slab(params: *const SarVolumeParams, zf: f32, k_out: *mut i32) -> c_int;
    pub fn sar_runtime_volume(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarVolumeParams, n_jobs: u32, iters_per_job: u64,
                              starts_xyz_host: *const f64, stats_out: *mut SarVolumeStats) -> c_int;
    pub fn sar_runtime_volume_free(rt: *mut SarRuntime) -> c_int;
    pub fn sar_runtime_volume_section(rt: *mut SarRuntime, k0: u32, k1: u32, count_out_host: *mut u32, nearest_out_host: *mut i32) -> c_int;
    pub fn sar_runtime_volume_read(rt: *mut SarRuntime, k0: u32, k1: u32, out_host: *mut u32) -> c_int;
    pub fn sar_runtime_volume_march(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarVolumeMarchParams,
                                    stats_out: *mut SarVolumeMarchStats, rgba_out_host: *mut u16) -> c_int;
    pub fn sar_runtime_volume_march_device(cfg: *const SarConfig, rt: *mut SarRuntime, params: *const SarVolumeMarchParams,
                                           stats_out: *mut SarVolumeMarchStats, rgba_out_dev: *mut c_void) -> c_int;
    pub fn sar_color_range_to_velocity(input: *const SarConfig, range: *const SarColorRange, out: *mut SarConfig) -> c_int;
}
