"""ctypes mirror of include/sar.h (the C ABI of the HIP library).

Plumbing only: struct layouts, prototypes and the loader for ``libsar_hip.so``. The library is the
product; there is NO CPU fallback — loading fails loudly when the shared object is missing.
"""
from __future__ import annotations

import ctypes as C
import os

SAR_OK = 0
SAR_ERR_INVALID = 1
SAR_ERR_DIM_MISMATCH = 2
SAR_ERR_NO_DEVICE = 3
SAR_ERR_HIP = 4
SAR_ERR_OOM = 5
SAR_ERR_RANGE = 6
SAR_ERR_IO = 7
SAR_ERR_INTERNAL = 8

SAR_RENDER_GAS = 0
SAR_RENDER_DEPTH = 1
SAR_ATTRACTOR_SPROTT2 = 0
SAR_CT_POISSON_SATURNE = 0
SAR_CT_ADJUSTED_VELOCITY = 1
SAR_PALETTE_MAX = 15
SAR_FMT_RGBA16 = 0
SAR_FMT_RGB16 = 1
SAR_FMT_RGBA8 = 2
SAR_FMT_RGB8 = 3


class SarConfig(C.Structure):
    """``struct sar_config`` — POD mirror of the reference's Config/View/Colors (src/lib.rs:253-308)."""

    _fields_ = [
        ("iterations", C.c_uint64),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("render_kind", C.c_int32),
        ("transparent", C.c_int32),
        ("angle", C.c_double),
        ("silent", C.c_int32),
        ("attractor_kind", C.c_int32),
        ("coeff_x", C.c_double * 10),
        ("coeff_y", C.c_double * 10),
        ("coeff_z", C.c_double * 10),
        ("palette_len", C.c_uint32),
        ("_pad0", C.c_uint32),
        ("palette_rgb", (C.c_double * 3) * SAR_PALETTE_MAX),
        ("brightness_offset", C.c_double),
        ("brightness_factor", C.c_double),
        ("center_camera", C.c_double * 3),
        ("rotation_axis", C.c_double * 3),
        ("rotation_angle", C.c_double),
        ("scale", C.c_double),
        ("color_transform", C.c_int32),
        ("_pad1", C.c_int32),
        ("ct_offset", C.c_double),
        ("ct_factor", C.c_double),
        ("seed", C.c_uint64),
        ("jobs_total", C.c_uint32),
        ("_pad2", C.c_uint32),
    ]


class SarParallelTiming(C.Structure):
    _fields_ = [
        ("total_ms", C.c_float),
        ("render_ms", C.c_float),
        ("exchange_ms", C.c_float),
        ("colorize_ms", C.c_float),
        ("n_devices", C.c_uint32),
        ("peer_access_failures", C.c_uint32),
        ("exchange_bytes_per_device", C.c_uint64),
        ("host_ms_before_exchange", C.c_float),
        ("host_ms_enqueue", C.c_float),
        ("draw_ahead_ms", C.c_float),
        ("_pad", C.c_float),
    ]


class SarExchangeLayout(C.Structure):
    _fields_ = [("world", C.c_uint32), ("rank", C.c_uint32), ("slice_pixels", C.c_uint32), ("first_px", C.c_uint32), ("n_px", C.c_uint32),
                ("granules", C.c_uint32), ("block_bytes", C.c_uint64)]


class SarTiming(C.Structure):
    _fields_ = [
        ("iterate_ms", C.c_float),
        ("resolve_ms", C.c_float),
        ("colorize_ms", C.c_float),
        ("merge_ms", C.c_float),
        ("iterate_launches", C.c_uint32),
        ("warmup_ms", C.c_float),
        ("iterations_counted", C.c_uint64),
        ("depth_atomics", C.c_uint64),
        ("depth_candidates", C.c_uint64),
    ]


SAR_SEARCH_BOUNDED = 0
SAR_SEARCH_DIVERGED = 1
SAR_SEARCH_DEGENERATE = 2


class SarSearchParams(C.Structure):
    _fields_ = [
        ("seed", C.c_uint64),
        ("lo", C.c_double),
        ("hi", C.c_double),
        ("start", C.c_double * 3),
        ("transient", C.c_uint32),
        ("steps", C.c_uint32),
        ("bound", C.c_double),
        ("min_lyapunov", C.c_double),
        ("min_ky_dim", C.c_double),
        ("keep_rejected", C.c_int32),
        ("_pad", C.c_int32),
    ]


class SarSearchRecord(C.Structure):
    _fields_ = [
        ("candidate", C.c_uint64),
        ("status", C.c_int32),
        ("steps_done", C.c_uint32),
        ("log2_exp", C.c_int64 * 3),
        ("mant", C.c_double * 3),
        ("lyapunov", C.c_double * 3),
        ("ky_dim", C.c_double),
        ("extent", C.c_double * 6),
    ]


class SarSearchStats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("tested", "diverged_transient", "diverged_late", "degenerate", "below_lyapunov",
                                           "below_dim", "accepted")]


SAR_PLANE_L1 = 1
SAR_PLANE_SPECTRUM = 3


class SarPlaneParams(C.Structure):
    _fields_ = [
        ("base", C.c_double * 30),
        ("axis", C.c_uint32 * 2),
        ("lo", C.c_double * 2),
        ("hi", C.c_double * 2),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("start", C.c_double * 3),
        ("transient", C.c_uint32),
        ("steps", C.c_uint32),
        ("bound", C.c_double),
        ("mode", C.c_int32),
        ("_pad", C.c_int32),
    ]


class SarPlaneRecord(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("transient_done", C.c_uint32),
        ("steps_done", C.c_uint32),
        ("_pad", C.c_uint32),
        ("log2_exp", C.c_int64 * 3),
        ("mant", C.c_double * 3),
        ("lyapunov", C.c_double * 3),
        ("ky_dim", C.c_double),
    ]


class SarPlaneStats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("pixels", "diverged_transient", "diverged_late", "degenerate", "bounded")]


class SarPlaneColors(C.Structure):
    _fields_ = [("threshold", C.c_double), ("chaos_scale", C.c_double), ("order_scale", C.c_double)]


class SarDensityParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("_pad", C.c_uint32)]


class SarDensityStats(C.Structure):
    _fields_ = [
        ("mass_in", C.c_uint64),
        ("mass_q16", C.c_uint64),
        ("covered_in", C.c_uint32),
        ("covered_out", C.c_uint32),
        ("spread", C.c_uint32),
        ("saturated", C.c_uint32),
        ("max_in", C.c_uint32),
        ("max_out", C.c_uint32),
    ]


class SarExposureParams(C.Structure):
    _fields_ = [("q_black", C.c_double), ("q_white", C.c_double), ("level_black", C.c_double), ("level_white", C.c_double)]


class SarExposure(C.Structure):
    _fields_ = [
        ("offset", C.c_double),
        ("factor", C.c_double),
        ("black_count", C.c_uint32),
        ("white_count", C.c_uint32),
        ("covered", C.c_uint32),
        ("max", C.c_uint32),
        ("applied", C.c_int32),
        ("_pad", C.c_int32),
    ]


class SarColorRangeParams(C.Structure):
    _fields_ = [("q_lo", C.c_double), ("q_hi", C.c_double), ("pos_lo", C.c_double), ("pos_hi", C.c_double)]


class SarColorRange(C.Structure):
    _fields_ = [
        ("lo", C.c_double),
        ("hi", C.c_double),
        ("pos_lo", C.c_double),
        ("pos_hi", C.c_double),
        ("covered", C.c_uint32),
        ("applied", C.c_int32),
    ]


class SarShadeParams(C.Structure):
    _fields_ = [
        ("light", C.c_double * 3),
        ("ambient", C.c_double),
        ("diffuse", C.c_double),
        ("specular", C.c_double),
        ("ao_strength", C.c_double),
        ("ao_range", C.c_double),
        ("smooth_range", C.c_double),
        ("shininess_log2", C.c_uint32),
        ("ao_radius", C.c_uint32),
        ("smooth", C.c_int32),
        ("min_count", C.c_uint32),
        ("background", C.c_uint16 * 3),
        ("_pad0", C.c_uint16),
        ("has_window", C.c_int32),
        ("_pad1", C.c_int32),
        ("window", SarColorRange),
    ]


class SarShadeStats(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("surface", "background", "isolated", "occluded", "smoothed", "_pad")]


class SarVolumeParams(C.Structure):
    _fields_ = [("z_lo", C.c_double), ("z_hi", C.c_double), ("slabs", C.c_uint32), ("add", C.c_int32)]


class SarVolumeStats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("visits", "stored", "below", "above", "nan", "nonempty")] + [
        ("vmax", C.c_uint32), ("z_min", C.c_float), ("z_max", C.c_float), ("_pad", C.c_uint32)]


class SarVolumeMarchParams(C.Structure):
    _fields_ = [
        ("half_count", C.c_double),
        ("t_min", C.c_double),
        ("pos_lo", C.c_double),
        ("pos_hi", C.c_double),
        ("k0", C.c_uint32),
        ("k1", C.c_uint32),
        ("background", C.c_uint16 * 3),
        ("_pad", C.c_uint16),
    ]


class SarVolumeMarchStats(C.Structure):
    _fields_ = [("slabs_seen", C.c_uint64), ("covered", C.c_uint32), ("stopped", C.c_uint32)]


class SarFlowParams(C.Structure):
    _fields_ = [("dt", C.c_double), ("bound", C.c_double), ("transient", C.c_uint32), ("stride", C.c_uint32), ("plot", C.c_int32),
                ("chunk_jobs", C.c_uint32), ("chunk_steps", C.c_uint32), ("_pad", C.c_uint32)]


class SarFlowStats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("steps", "visits", "outside", "escaped_transient", "escaped", "alive", "count_atomics", "key_atomics")] + [
        ("extent", C.c_double * 6), ("max", C.c_uint32), ("_pad", C.c_uint32)]


class SarSectionParams(C.Structure):
    _fields_ = [("surface", C.c_double * 10), ("dt", C.c_double), ("bound", C.c_double), ("transient", C.c_uint32), ("direction", C.c_int32),
                ("samples", C.c_uint32), ("max_steps", C.c_uint32), ("plot", C.c_int32), ("chunk_jobs", C.c_uint32), ("chunk_steps", C.c_uint32),
                ("_pad", C.c_uint32)]


class SarSectionRecord(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("status", "found", "rough", "steps", "clock_step", "_pad")]


class SarSectionStats(C.Structure):
    _fields_ = [(f, C.c_uint64) for f in ("steps", "crossings", "rough", "clocked", "full", "short_jobs", "escaped", "escaped_transient", "visits",
                                          "outside")] + [
        ("extent", C.c_double * 6), ("ret_min", C.c_double), ("ret_max", C.c_double), ("residual_max", C.c_double), ("max", C.c_uint32),
        ("_pad", C.c_uint32)]


class SarGalleryItem(C.Structure):
    _fields_ = [("coeff", C.c_double * 30), ("center_camera", C.c_double * 3), ("scale", C.c_double)]


class SarGalleryParams(C.Structure):
    _fields_ = [
        ("tile_width", C.c_uint32),
        ("tile_height", C.c_uint32),
        ("cols", C.c_uint32),
        ("jobs", C.c_uint32),
        ("iterations", C.c_uint64),
        ("seed", C.c_uint64),
    ]


class SarGalleryStats(C.Structure):
    _fields_ = [
        ("max", C.c_uint32),
        ("covered", C.c_uint32),
        ("hits", C.c_uint64),
        ("dead_jobs", C.c_uint32),
        ("_pad", C.c_uint32),
    ]


class SarOrbitParams(C.Structure):
    _fields_ = [
        ("a", C.c_double * 30),
        ("b", C.c_double * 30),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("jobs", C.c_uint32),
        ("transient", C.c_uint32),
        ("steps", C.c_uint32),
        ("_pad", C.c_uint32),
        ("seed", C.c_uint64),
        ("bound", C.c_double),
        ("proj", C.c_double * 3),
        ("v_lo", C.c_double),
        ("v_hi", C.c_double),
    ]


class SarOrbitColumn(C.Structure):
    _fields_ = [
        ("dead_transient", C.c_uint32),
        ("dead_late", C.c_uint32),
        ("alive", C.c_uint32),
        ("occupied", C.c_uint32),
        ("max", C.c_uint32),
        ("_pad", C.c_uint32),
        ("hits", C.c_uint64),
        ("misses", C.c_uint64),
        ("vmin", C.c_double),
        ("vmax", C.c_double),
    ]


class SarPairsParams(C.Structure):
    _fields_ = [
        ("samples", C.c_uint32),
        ("theiler", C.c_uint32),
        ("sub_bits", C.c_uint32),
        ("e_min", C.c_int32),
        ("e_max", C.c_int32),
        ("_pad", C.c_uint32),
    ]


class SarPairsCounts(C.Structure):
    _fields_ = [("counted", C.c_uint64), ("skipped", C.c_uint64)]


class SarCorrdimLine(C.Structure):
    _fields_ = [
        ("slope", C.c_double),
        ("intercept", C.c_double),
        ("rms", C.c_double),
        ("first_bin", C.c_uint32),
        ("last_bin", C.c_uint32),
        ("used", C.c_uint32),
        ("status", C.c_int32),
    ]


class SarCorrdimParams(C.Structure):
    _fields_ = [
        ("jobs", C.c_uint32),
        ("samples", C.c_uint32),
        ("stride", C.c_uint32),
        ("transient", C.c_uint32),
        ("theiler", C.c_uint32),
        ("sub_bits", C.c_uint32),
        ("e_min", C.c_int32),
        ("e_max", C.c_int32),
        ("seed", C.c_uint64),
        ("bound", C.c_double),
        ("c_lo", C.c_double),
        ("r_hi_fraction", C.c_double),
    ]


class SarCorrdimRecord(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("fail_job", C.c_uint32),
        ("fail_step", C.c_uint64),
        ("counted", C.c_uint64),
        ("skipped", C.c_uint64),
        ("extent", C.c_double * 6),
        ("r_hi", C.c_double),
        ("line", SarCorrdimLine),
    ]


SAR_CORRDIM_FIT_OK, SAR_CORRDIM_NO_WINDOW = 0, 1


class SarBoxParams(C.Structure):
    _fields_ = [
        ("levels", C.c_uint32),
        ("_pad", C.c_uint32),
        ("origin", C.c_double * 3),
        ("size", C.c_double),
    ]


class SarBoxLevel(C.Structure):
    _fields_ = [("cells", C.c_uint64), ("singles", C.c_uint64), ("sum_sq", C.c_uint64), ("n_log_n", C.c_uint64)]


class SarBoxdimLine(C.Structure):
    _fields_ = [("slope", C.c_double), ("intercept", C.c_double), ("rms", C.c_double)]


class SarBoxdimLines(C.Structure):
    _fields_ = [
        ("d0", SarBoxdimLine),
        ("d1", SarBoxdimLine),
        ("d2", SarBoxdimLine),
        ("first_level", C.c_uint32),
        ("last_level", C.c_uint32),
        ("used", C.c_uint32),
        ("status", C.c_int32),
    ]


class SarBoxdimParams(C.Structure):
    _fields_ = [
        ("jobs", C.c_uint32),
        ("samples", C.c_uint32),
        ("stride", C.c_uint32),
        ("transient", C.c_uint32),
        ("levels", C.c_uint32),
        ("l_min", C.c_uint32),
        ("seed", C.c_uint64),
        ("bound", C.c_double),
        ("min_occupancy", C.c_double),
    ]


class SarBoxdimRecord(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("fail_job", C.c_uint32),
        ("fail_step", C.c_uint64),
        ("extent", C.c_double * 6),
        ("origin", C.c_double * 3),
        ("size", C.c_double),
        ("lines", SarBoxdimLines),
    ]


SAR_BOXDIM_FIT_OK, SAR_BOXDIM_NO_WINDOW = 0, 1


class SarBasinParams(C.Structure):
    _fields_ = [
        ("coeffs", C.c_double * 30),
        ("origin", C.c_double * 3),
        ("du", C.c_double * 3),
        ("dv", C.c_double * 3),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("transient", C.c_uint32),
        ("steps", C.c_uint32),
        ("bound", C.c_double),
        ("grid", C.c_uint32),
        ("_pad", C.c_uint32),
        ("box_lo", C.c_double * 3),
        ("box_hi", C.c_double * 3),
    ]


class SarBasinPixel(C.Structure):
    _fields_ = [("status", C.c_int32), ("escape_step", C.c_uint32), ("root", C.c_uint32), ("label", C.c_uint32)]


class SarBasinAttractor(C.Structure):
    _fields_ = [
        ("root", C.c_uint32),
        ("pixels", C.c_uint32),
        ("cells", C.c_uint32),
        ("first_pixel", C.c_uint32),
        ("cell_lo", C.c_uint32 * 3),
        ("cell_hi", C.c_uint32 * 3),
    ]


class SarBasinStats(C.Structure):
    _fields_ = [
        ("pixels", C.c_uint64),
        ("escaped_transient", C.c_uint64),
        ("escaped_tail", C.c_uint64),
        ("bounded", C.c_uint64),
        ("attractors", C.c_uint64),
        ("cells", C.c_uint64),
        ("extent", C.c_double * 6),
    ]


class SarBasinColors(C.Structure):
    _fields_ = [("fade", C.c_double)]


SAR_BASIN_UNKNOWN, SAR_BASIN_MAX_LEVELS = 0xFFFFFFFE, 31


class SarBasinFate(C.Structure):
    _fields_ = [("status", C.c_int32), ("escape_step", C.c_uint32), ("label", C.c_uint32), ("hit", C.c_uint32)]


class SarBasinFateCounts(C.Structure):
    _fields_ = [("points", C.c_uint64), ("diverged", C.c_uint64), ("labelled", C.c_uint64), ("unknown", C.c_uint64)]


class SarBasinLadderParams(C.Structure):
    _fields_ = [("dir", C.c_double * 3), ("eps0", C.c_double), ("levels", C.c_uint32), ("chunk", C.c_uint32)]


class SarBasinUncertaintyLevel(C.Structure):
    _fields_ = [("eps", C.c_double), ("tested", C.c_uint64), ("uncertain", C.c_uint64), ("unknown", C.c_uint64)]


class SarBasinLadderMask(C.Structure):
    _fields_ = [("uncertain_bits", C.c_uint32), ("unknown_bits", C.c_uint32)]


SAR_FTLE_EDGE, SAR_FTLE_ONE_SIDED_U, SAR_FTLE_ONE_SIDED_V, SAR_FTLE_NO_U, SAR_FTLE_NO_V = 1, 2, 4, 8, 16


class SarFtleParams(C.Structure):
    _fields_ = [
        ("coeffs", C.c_double * 30),
        ("origin", C.c_double * 3),
        ("du", C.c_double * 3),
        ("dv", C.c_double * 3),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("steps", C.c_uint32),
        ("chunk", C.c_uint32),
        ("bound", C.c_double),
    ]


class SarFtlePixel(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("escape_step", C.c_uint32),
        ("flags", C.c_uint32),
        ("_pad", C.c_uint32),
        ("end", C.c_double * 3),
        ("g11", C.c_double),
        ("g12", C.c_double),
        ("g22", C.c_double),
        ("stretch2", C.c_double),
        ("ftle", C.c_double),
    ]


class SarFtleStats(C.Structure):
    _fields_ = [
        ("pixels", C.c_uint64),
        ("escaped", C.c_uint64),
        ("bounded", C.c_uint64),
        ("edge", C.c_uint64),
        ("one_sided", C.c_uint64),
        ("isolated", C.c_uint64),
        ("ftle_min", C.c_double),
        ("ftle_max", C.c_double),
    ]


class SarFtleColors(C.Structure):
    _fields_ = [("lo", C.c_double), ("hi", C.c_double), ("fade", C.c_double)]


SAR_WINDOW_RECT, SAR_WINDOW_HANN = 0, 1


class SarSpectraParams(C.Structure):
    _fields_ = [
        ("n", C.c_uint32),
        ("hop", C.c_uint32),
        ("window", C.c_uint32),
        ("samples", C.c_uint32),
        ("chunk", C.c_uint32),
        ("_pad", C.c_uint32),
        ("proj", C.c_double * 3),
    ]


class SarSpectraRecord(C.Structure):
    _fields_ = [("jobs", C.c_uint32), ("segments", C.c_uint32), ("energy", C.c_double)]


class SarSpectrumParams(C.Structure):
    _fields_ = [
        ("jobs", C.c_uint32),
        ("segments", C.c_uint32),
        ("n", C.c_uint32),
        ("hop", C.c_uint32),
        ("window", C.c_uint32),
        ("stride", C.c_uint32),
        ("transient", C.c_uint32),
        ("chunk", C.c_uint32),
        ("seed", C.c_uint64),
        ("bound", C.c_double),
        ("proj", C.c_double * 3),
    ]


class SarSpectrumRecord(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("fail_job", C.c_uint32),
        ("fail_step", C.c_uint64),
        ("extent", C.c_double * 6),
        ("segments", C.c_uint32),
        ("_pad", C.c_uint32),
        ("energy", C.c_double),
    ]


class SarRecurrenceParams(C.Structure):
    _fields_ = [
        ("samples", C.c_uint32),
        ("theiler", C.c_uint32),
        ("line_bins", C.c_uint32),
        ("chunk", C.c_uint32),
        ("eps2", C.c_double),
    ]


class SarRecurrenceRecord(C.Structure):
    _fields_ = [
        ("recurrences", C.c_uint64),
        ("pairs", C.c_uint64),
        ("diag_lines", C.c_uint64),
        ("vert_lines", C.c_uint64),
        ("diag_longest", C.c_uint64),
        ("vert_longest", C.c_uint64),
    ]


class SarRqaParams(C.Structure):
    _fields_ = [
        ("jobs", C.c_uint32),
        ("samples", C.c_uint32),
        ("stride", C.c_uint32),
        ("transient", C.c_uint32),
        ("seed", C.c_uint64),
        ("bound", C.c_double),
        ("theiler", C.c_uint32),
        ("line_bins", C.c_uint32),
        ("chunk", C.c_uint32),
        ("_pad", C.c_uint32),
        ("eps2", C.c_double),
        ("eps_fraction", C.c_double),
    ]


class SarRqaRecord(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("fail_job", C.c_uint32),
        ("fail_step", C.c_uint64),
        ("extent", C.c_double * 6),
        ("eps2", C.c_double),
        ("counts", SarRecurrenceRecord),
    ]


class SarRqaMeasures(C.Structure):
    _fields_ = [
        ("rr", C.c_double),
        ("det", C.c_double),
        ("l_mean", C.c_double),
        ("div", C.c_double),
        ("entr", C.c_double),
        ("lam", C.c_double),
        ("tt", C.c_double),
        ("l_max", C.c_uint64),
        ("v_max", C.c_uint64),
    ]


class SarPeriodParams(C.Structure):
    _fields_ = [
        ("base", C.c_double * 30),
        ("axis", C.c_uint32 * 2),
        ("lo", C.c_double * 2),
        ("hi", C.c_double * 2),
        ("width", C.c_uint32),
        ("height", C.c_uint32),
        ("start", C.c_double * 3),
        ("transient", C.c_uint32),
        ("max_period", C.c_uint32),
        ("bound", C.c_double),
        ("eps", C.c_double),
    ]


class SarPeriodRecord(C.Structure):
    _fields_ = [("status", C.c_int32), ("period", C.c_uint32), ("transient_done", C.c_uint32), ("steps_done", C.c_uint32),
                ("residual", C.c_double)]


class SarPeriodStats(C.Structure):
    _fields_ = [
        ("pixels", C.c_uint64),
        ("diverged_transient", C.c_uint64),
        ("diverged_late", C.c_uint64),
        ("periodic", C.c_uint64),
        ("aperiodic", C.c_uint64),
        ("max_period_found", C.c_uint64),
    ]


class SarPeriodColors(C.Structure):
    _fields_ = [("colours", C.c_uint32), ("_pad", C.c_uint32)]


SAR_CYCLE_CONVERGED, SAR_CYCLE_ESCAPED, SAR_CYCLE_SINGULAR, SAR_CYCLE_NOT_CONVERGED = 0, 1, 2, 3


class SarCyclesParams(C.Structure):
    _fields_ = [
        ("period", C.c_uint32),
        ("jobs", C.c_uint32),
        ("grid", C.c_uint32),
        ("max_newton", C.c_uint32),
        ("cap", C.c_uint32),
        ("_pad", C.c_uint32),
        ("box_lo", C.c_double * 3),
        ("box_hi", C.c_double * 3),
        ("tol", C.c_double),
        ("bound", C.c_double),
        ("merge", C.c_double),
        ("same", C.c_double),
    ]


class SarCyclesRecord(C.Structure):
    _fields_ = [(f, C.c_uint32) for f in ("converged", "escaped", "singular", "not_converged", "n_orbits", "orbits_lost", "hits_lost",
                                          "_pad")] + [("newton_iterations", C.c_uint64)]


class SarCycleOrbit(C.Structure):
    _fields_ = [
        ("rep", C.c_double * 3),
        ("period", C.c_uint32),
        ("head", C.c_uint32),
        ("hits", C.c_uint32),
        ("newton", C.c_uint32),
        ("residual", C.c_double),
        ("M", C.c_double * 9),
    ]


SAR_MANIFOLD_OK, SAR_MANIFOLD_DOMAIN_ESCAPED = 0, 1
SAR_SECTION_FULL, SAR_SECTION_SHORT, SAR_SECTION_ESCAPED, SAR_SECTION_ESCAPED_TRANSIENT = 0, 1, 2, 3
SAR_SECTION_NO_CLOCK = 0xFFFFFFFF


class SarManifoldParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("steps", C.c_uint32), ("max_span", C.c_uint32), ("_pad", C.c_uint32), ("bound", C.c_double)]


class SarManifoldBranch(C.Structure):
    _fields_ = [("base", C.c_double * 3), ("dir", C.c_double * 3), ("delta", C.c_double), ("period", C.c_uint32), ("_pad", C.c_uint32)]


class SarManifoldRecord(C.Structure):
    _fields_ = [("status", C.c_int32), ("first_long_step", C.c_uint32), ("alive_end", C.c_uint32), ("_pad", C.c_uint32),
                ("a", C.c_double * 3), ("b", C.c_double * 3)] + [(f, C.c_uint64) for f in ("n_drawn", "n_dead", "n_far", "n_long", "pixels",
                                                                                          "length_px")]


_P = C.POINTER
_cfg_p = _P(SarConfig)
_vp = C.c_void_p

# name -> (restype, argtypes); every symbol include/sar.h declares
PROTOTYPES = {
    "sar_abi_version": (C.c_int, []),
    "sar_build_id": (C.c_char_p, []),
    "sar_device_pci_bus_id": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "sar_checksum_fnv1a64": (C.c_int, [_vp, C.c_size_t, _P(C.c_uint64)]),
    "sar_status_string": (C.c_char_p, [C.c_int]),
    "sar_last_error": (C.c_char_p, []),
    "sar_device_count": (C.c_int, [_P(C.c_int)]),
    "sar_config_poisson_saturne": (C.c_int, [_cfg_p]),
    "sar_config_solar_sail": (C.c_int, [_cfg_p]),
    "sar_config_validate": (C.c_int, [_cfg_p]),
    "sar_rotation_matrix": (C.c_int, [_cfg_p, _P(C.c_double)]),
    "sar_start_points": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint32, _P(C.c_double)]),
    "sar_runtime_new": (C.c_int, [_cfg_p, C.c_int, _P(_vp)]),
    "sar_runtime_new_group": (C.c_int, [_cfg_p, C.c_int, C.c_uint32, _P(_vp)]),
    "sar_runtime_reset_batch": (C.c_int, [C.c_uint32, _P(_vp)]),
    "sar_colorize_device_batch": (C.c_int, [C.c_uint32, _P(_cfg_p), _P(_vp), _P(_vp)]),
    "sar_runtime_free": (C.c_int, [_vp]),
    "sar_runtime_reset": (C.c_int, [_vp]),
    "sar_runtime_set_width_height": (C.c_int, [_vp, C.c_uint32, C.c_uint32]),
    "sar_runtime_seed": (C.c_int, [_vp, C.c_uint64]),
    "sar_runtime_merge": (C.c_int, [_vp, _vp]),
    "sar_runtime_synchronize": (C.c_int, [_vp]),
    "sar_runtime_dims": (C.c_int, [_vp, _P(C.c_uint32), _P(C.c_uint32)]),
    "sar_runtime_set_stream": (C.c_int, [_vp, _vp]),
    "sar_runtime_get_stream": (C.c_int, [_vp, _P(_vp)]),
    "sar_runtime_get_copy_stream": (C.c_int, [_vp, _P(_vp)]),
    "sar_runtime_set_copy_stream": (C.c_int, [_vp, _vp]),
    "sar_render": (C.c_int, [_cfg_p, _vp]),
    "sar_render_jobs": (C.c_int, [_cfg_p, _vp, _P(C.c_double)]),
    "sar_render_job_range": (C.c_int, [_cfg_p, _vp, C.c_uint32, C.c_uint64, _P(C.c_double)]),
    "sar_render_job_range_device": (C.c_int, [_cfg_p, _vp, C.c_uint32, C.c_uint64, _vp]),
    "sar_render_jobs_batch": (C.c_int, [C.c_uint32, _P(_cfg_p), _P(_vp), _P(_P(C.c_double))]),
    "sar_runtime_batch_frames": (C.c_int, [_cfg_p, _vp, _P(C.c_uint32)]),
    "sar_runtime_prefetch_device": (C.c_int, [_cfg_p, _vp, C.c_uint32, C.c_uint64, _vp]),
    "sar_runtime_describe_last_launch": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "sar_colorize": (C.c_int, [_cfg_p, _vp, _P(C.c_uint16)]),
    "sar_colorize_device": (C.c_int, [_cfg_p, _vp, _vp]),
    "sar_runtime_extent": (C.c_int, [_cfg_p, _vp, C.c_uint32, C.c_uint64, _P(C.c_double), _P(C.c_double)]),
    "sar_image_format": (C.c_int, [C.c_int, C.c_int]),
    "sar_image_bytes": (C.c_size_t, [C.c_int, C.c_uint32, C.c_uint32]),
    "sar_image_convert_device": (C.c_int, [_vp, _vp, C.c_int, _vp]),
    "sar_colorize_format": (C.c_int, [_cfg_p, _vp, C.c_int, _vp]),
    "sar_colorize_format_async": (C.c_int, [_cfg_p, _vp, C.c_int, _vp, _P(C.c_uint64)]),
    "sar_runtime_wait_image": (C.c_int, [_vp, C.c_uint64]),
    "sar_runtime_read_image_async": (C.c_int, [_vp, _vp, _P(C.c_uint64)]),
    "sar_runtime_image_done": (C.c_int, [_vp, C.c_uint64, _P(C.c_int)]),
    "sar_host_alloc": (C.c_int, [C.c_size_t, _P(C.c_void_p)]),
    "sar_host_free": (C.c_int, [_vp]),
    "sar_host_reserve": (C.c_int, [C.c_size_t, C.c_uint32]),
    "sar_write_png": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, _vp]),
    "sar_write_bmp": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, _vp]),
    "sar_write_pam": (C.c_int, [C.c_char_p, C.c_int, C.c_uint32, C.c_uint32, _vp]),
    "sar_runtime_count": (C.c_int, [_vp, _P(C.c_uint32)]),
    "sar_runtime_steps": (C.c_int, [_vp, _P(C.c_double)]),
    "sar_runtime_zbuf": (C.c_int, [_vp, _P(C.c_float)]),
    "sar_runtime_max": (C.c_int, [_vp, _P(C.c_uint32)]),
    "sar_runtime_load": (C.c_int, [_vp, _P(C.c_uint32), _P(C.c_double), _P(C.c_float), C.c_uint32]),
    "sar_exchange_slice_pixels": (C.c_int, [C.c_uint32, C.c_uint32, _P(C.c_uint32)]),
    "sar_exchange_new": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _P(_vp), _P(SarExchangeLayout)]),
    "sar_exchange_free": (C.c_int, [_vp]),
    "sar_exchange_flags": (C.c_int, [_vp, _vp]),
    "sar_exchange_pack": (C.c_int, [_vp, _vp, C.c_double, _vp, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_int)]),
    "sar_exchange_merge": (C.c_int, [_vp, _vp, _vp]),
    "sar_exchange_finish": (C.c_int, [_vp, _vp]),
    "sar_exchange_rooted": (C.c_int, [_vp, C.c_uint32, _vp, _vp]),
    "sar_colorize_range_device": (C.c_int, [_cfg_p, _vp, C.c_uint32, C.c_uint32, _vp]),
    "sar_renderer_new": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, _P(_vp)]),
    "sar_renderer_new_multi": (C.c_int, [_P(C.c_int), C.c_uint32, C.c_uint32, C.c_uint64, _P(_vp)]),
    "sar_renderer_num_devices": (C.c_int, [_vp, _P(C.c_uint32)]),
    "sar_renderer_last_timing": (C.c_int, [_vp, _P(SarParallelTiming)]),
    "sar_renderer_set_exchange": (C.c_int, [_vp, C.c_uint32]),
    "sar_renderer_num_units": (C.c_int, [_vp, _P(C.c_uint32)]),
    "sar_renderer_shutdown": (C.c_int, [_vp]),
    "sar_render_parallel": (C.c_int, [_vp, _cfg_p, C.c_uint32, _P(C.c_uint16)]),
    "sar_renderer_runtime": (C.c_int, [_vp, _P(_vp)]),
    "sar_runtime_enable_timing": (C.c_int, [_vp, C.c_int]),
    "sar_runtime_last_timing": (C.c_int, [_vp, _P(SarTiming)]),
    "sar_runtime_set_option": (C.c_int, [_vp, C.c_char_p, C.c_uint64]),
    "sar_search_params_default": (C.c_int, [_P(SarSearchParams)]),
    "sar_search_candidate": (C.c_int, [C.c_uint64, C.c_double, C.c_double, C.c_uint64, _P(C.c_double)]),
    "sar_runtime_search": (C.c_int, [_vp, _P(SarSearchParams), C.c_uint64, C.c_uint32, _P(C.c_double), _P(SarSearchRecord),
                                     C.c_uint32, _P(C.c_uint32), _P(SarSearchStats)]),
    "sar_frame_view": (C.c_int, [_cfg_p, _P(C.c_double), C.c_double, C.c_int]),
    "sar_plane_params_default": (C.c_int, [_P(SarPlaneParams)]),
    "sar_plane_coeffs": (C.c_int, [_P(SarPlaneParams), C.c_uint32, C.c_uint32, _P(C.c_double)]),
    "sar_runtime_plane": (C.c_int, [_vp, _P(SarPlaneParams), _vp, _P(SarPlaneStats)]),
    "sar_plane_colors_default": (C.c_int, [_P(SarPlaneColors)]),
    "sar_runtime_plane_colorize": (C.c_int, [_cfg_p, _vp, _P(SarPlaneColors), _P(C.c_uint16)]),
    "sar_exposure_params_default": (C.c_int, [_P(SarExposureParams)]),
    "sar_runtime_exposure": (C.c_int, [_cfg_p, _vp, _P(SarExposureParams), _P(SarExposure)]),
    "sar_runtime_set_exposure": (C.c_int, [_vp, _P(SarExposureParams)]),
    "sar_renderer_set_exposure": (C.c_int, [_vp, _P(SarExposureParams)]),
    "sar_color_range_params_default": (C.c_int, [_P(SarColorRangeParams)]),
    "sar_runtime_color_range": (C.c_int, [_cfg_p, _vp, _P(SarColorRangeParams), _P(SarColorRange)]),
    "sar_runtime_set_color_range": (C.c_int, [_vp, _P(SarColorRangeParams)]),
    "sar_runtime_hold_color_range": (C.c_int, [_vp, _P(SarColorRange)]),
    "sar_renderer_set_color_range": (C.c_int, [_vp, _P(SarColorRangeParams)]),
    "sar_color_range_to_velocity": (C.c_int, [_cfg_p, _P(SarColorRange), _cfg_p]),
    "sar_gallery_params_default": (C.c_int, [_P(SarGalleryParams)]),
    "sar_runtime_gallery": (C.c_int, [_vp, _cfg_p, _P(SarGalleryParams), C.c_uint32, _P(SarGalleryItem), _P(C.c_double), _P(C.c_uint16),
                                      _P(C.c_uint32), _P(C.c_float), _P(C.c_double), _P(SarGalleryStats)]),
    "sar_frame_view_box": (C.c_int, [_cfg_p, _P(C.c_double), C.c_double, C.c_int]),
    "sar_orbit_params_default": (C.c_int, [_P(SarOrbitParams)]),
    "sar_orbit_coeffs": (C.c_int, [_P(SarOrbitParams), C.c_uint32, _P(C.c_double)]),
    "sar_runtime_orbit": (C.c_int, [_vp, _P(SarOrbitParams), _P(C.c_double), _P(C.c_uint32), _P(SarOrbitColumn), _P(C.c_uint32)]),
    "sar_pairs_params_default": (C.c_int, [_P(SarPairsParams)]),
    "sar_pairs_edges": (C.c_int, [_P(SarPairsParams), _P(C.c_uint32), _P(C.c_double)]),
    "sar_runtime_pairs": (C.c_int, [_vp, _P(SarPairsParams), C.c_uint32, C.c_uint32, _P(C.c_double), _P(C.c_uint64), _P(SarPairsCounts)]),
    "sar_corrdim_fit": (C.c_int, [_P(C.c_uint64), _P(SarPairsParams), C.c_double, C.c_double, _P(SarCorrdimLine)]),
    "sar_corrdim_params_default": (C.c_int, [_P(SarCorrdimParams)]),
    "sar_runtime_corrdim": (C.c_int, [_vp, _P(SarCorrdimParams), C.c_uint32, _P(C.c_double), _P(C.c_double), _P(C.c_uint64),
                                      _P(SarCorrdimRecord), _P(C.c_double)]),
    "sar_box_params_default": (C.c_int, [_P(SarBoxParams)]),
    "sar_box_log2_q32": (C.c_int, [C.c_uint32, _P(C.c_uint64)]),
    "sar_runtime_boxes": (C.c_int, [_vp, _P(SarBoxParams), C.c_uint32, C.c_uint32, _P(C.c_double), _P(SarBoxLevel)]),
    "sar_boxdim_fit": (C.c_int, [_P(SarBoxLevel), C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, _P(SarBoxdimLines)]),
    "sar_boxdim_params_default": (C.c_int, [_P(SarBoxdimParams)]),
    "sar_runtime_boxdim": (C.c_int, [_vp, _P(SarBoxdimParams), C.c_uint32, _P(C.c_double), _P(C.c_double), _P(SarBoxLevel),
                                     _P(SarBoxdimRecord), _P(C.c_double)]),
    "sar_basin_params_default": (C.c_int, [_P(SarBasinParams)]),
    "sar_basin_start": (C.c_int, [_P(SarBasinParams), C.c_uint32, C.c_uint32, _P(C.c_double)]),
    "sar_runtime_basin": (C.c_int, [_vp, _P(SarBasinParams), _P(SarBasinPixel), _P(SarBasinAttractor), C.c_uint32, _P(C.c_uint32),
                                    _P(SarBasinStats)]),
    "sar_basin_colors_default": (C.c_int, [_P(SarBasinColors)]),
    "sar_runtime_basin_colorize": (C.c_int, [_cfg_p, _vp, _P(SarBasinColors), _P(C.c_uint16)]),
    "sar_basin_ladder_params_default": (C.c_int, [_P(SarBasinLadderParams)]),
    "sar_runtime_basin_fates": (C.c_int, [_vp, C.c_uint32, _P(C.c_double), _P(SarBasinFate), _P(SarBasinFateCounts)]),
    "sar_runtime_basin_uncertainty": (C.c_int, [_vp, _P(SarBasinLadderParams), C.c_uint32, _P(C.c_double), _P(SarBasinUncertaintyLevel),
                                                _P(SarBasinFate), _P(SarBasinLadderMask)]),
    "sar_ftle_params_default": (C.c_int, [_P(SarFtleParams)]),
    "sar_ftle_start": (C.c_int, [_P(SarFtleParams), C.c_uint32, C.c_uint32, _P(C.c_double)]),
    "sar_runtime_ftle": (C.c_int, [_vp, _P(SarFtleParams), _P(SarFtlePixel), _P(SarFtleStats)]),
    "sar_ftle_colors_default": (C.c_int, [_P(SarFtleColors)]),
    "sar_runtime_ftle_colorize": (C.c_int, [_cfg_p, _vp, _P(SarFtleColors), _P(C.c_uint16)]),
    "sar_spectra_params_default": (C.c_int, [_P(SarSpectraParams)]),
    "sar_spectrum_twiddles": (C.c_int, [C.c_uint32, _P(C.c_double)]),
    "sar_spectrum_window": (C.c_int, [C.c_uint32, C.c_uint32, _P(C.c_double)]),
    "sar_spectra_segments": (C.c_int, [_P(SarSpectraParams), C.c_uint32, _P(C.c_uint32), _P(C.c_uint32)]),
    "sar_runtime_spectra": (C.c_int, [_vp, _P(SarSpectraParams), C.c_uint32, C.c_uint32, _P(C.c_double), _P(C.c_double),
                                      _P(SarSpectraRecord)]),
    "sar_spectrum_params_default": (C.c_int, [_P(SarSpectrumParams)]),
    "sar_runtime_spectrum": (C.c_int, [_vp, _P(SarSpectrumParams), C.c_uint32, _P(C.c_double), _P(C.c_double), _P(C.c_double),
                                       _P(SarSpectrumRecord), _P(C.c_double)]),
    "sar_recurrence_params_default": (C.c_int, [_P(SarRecurrenceParams)]),
    "sar_runtime_recurrence": (C.c_int, [_vp, _P(SarRecurrenceParams), C.c_uint32, C.c_uint32, _P(C.c_double), _P(C.c_uint64), _P(C.c_uint64),
                                         _P(SarRecurrenceRecord)]),
    "sar_runtime_recurrence_plot": (C.c_int, [_vp, _P(SarRecurrenceParams), C.c_uint32, _P(C.c_double), C.c_uint32, C.c_uint32, C.c_uint32,
                                              C.c_uint32, C.c_uint32, _P(C.c_uint8)]),
    "sar_rqa_params_default": (C.c_int, [_P(SarRqaParams)]),
    "sar_runtime_rqa": (C.c_int, [_vp, _P(SarRqaParams), C.c_uint32, _P(C.c_double), _P(C.c_double), _P(C.c_uint64), _P(C.c_uint64),
                                  _P(SarRqaRecord), _P(C.c_double)]),
    "sar_rqa_measures": (C.c_int, [_P(C.c_uint64), _P(C.c_uint64), _P(SarRecurrenceRecord), C.c_uint32, C.c_uint32, C.c_uint32,
                                   _P(SarRqaMeasures)]),
    "sar_period_params_default": (C.c_int, [_P(SarPeriodParams)]),
    "sar_period_coeffs": (C.c_int, [_P(SarPeriodParams), C.c_uint32, C.c_uint32, _P(C.c_double)]),
    "sar_runtime_period": (C.c_int, [_vp, _P(SarPeriodParams), _P(C.c_double), _P(SarPeriodRecord), _P(SarPeriodStats)]),
    "sar_period_colors_default": (C.c_int, [_P(SarPeriodColors)]),
    "sar_runtime_period_colorize": (C.c_int, [_cfg_p, _vp, _P(SarPeriodColors), _P(C.c_uint16)]),
    "sar_cycles_params_default": (C.c_int, [_P(SarCyclesParams)]),
    "sar_cycles_starts": (C.c_int, [_P(SarCyclesParams), _P(C.c_double)]),
    "sar_cycle_charpoly": (C.c_int, [_P(C.c_double), _P(C.c_double)]),
    "sar_runtime_cycles": (C.c_int, [_vp, _P(SarCyclesParams), C.c_uint32, _P(C.c_double), _P(C.c_double), _P(SarCyclesRecord),
                                     _P(SarCycleOrbit)]),
    "sar_manifold_params_default": (C.c_int, [_P(SarManifoldParams)]),
    "sar_manifold_pixel": (C.c_int, [_cfg_p, _P(C.c_double), _P(C.c_double)]),
    "sar_runtime_manifold": (C.c_int, [_vp, _cfg_p, _P(SarManifoldParams), C.c_uint32, _P(SarManifoldBranch), _P(C.c_uint32), _P(C.c_uint32),
                                       _P(SarManifoldRecord)]),
    "sar_density_params_default": (C.c_int, [_P(SarDensityParams)]),
    "sar_density_radius": (C.c_int, [_P(SarDensityParams), _P(C.c_uint32)]),
    "sar_density_weights": (C.c_int, [_P(SarDensityParams), C.c_uint32, _P(C.c_uint32)]),
    "sar_runtime_density": (C.c_int, [_vp, _P(SarDensityParams), _P(SarDensityStats)]),
    "sar_runtime_density_tiles": (C.c_int, [_vp, _P(C.c_uint32), _P(C.c_uint32)]),
    "sar_shade_params_default": (C.c_int, [_P(SarShadeParams)]),
    "sar_shade": (C.c_int, [_cfg_p, _vp, _P(SarShadeParams), _P(SarShadeStats), _P(C.c_uint16)]),
    "sar_shade_device": (C.c_int, [_cfg_p, _vp, _P(SarShadeParams), _P(SarShadeStats), _vp]),
    "sar_volume_params_default": (C.c_int, [_P(SarVolumeParams)]),
    "sar_volume_march_params_default": (C.c_int, [_P(SarVolumeMarchParams)]),
    "sar_volume_slab": (C.c_int, [_P(SarVolumeParams), C.c_float, _P(C.c_int32)]),
    "sar_runtime_volume": (C.c_int, [_cfg_p, _vp, _P(SarVolumeParams), C.c_uint32, C.c_uint64, _P(C.c_double), _P(SarVolumeStats)]),
    "sar_runtime_volume_free": (C.c_int, [_vp]),
    "sar_runtime_volume_section": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _P(C.c_uint32), _P(C.c_int32)]),
    "sar_runtime_volume_read": (C.c_int, [_vp, C.c_uint32, C.c_uint32, _P(C.c_uint32)]),
    "sar_runtime_volume_march": (C.c_int, [_cfg_p, _vp, _P(SarVolumeMarchParams), _P(SarVolumeMarchStats), _P(C.c_uint16)]),
    "sar_runtime_volume_march_device": (C.c_int, [_cfg_p, _vp, _P(SarVolumeMarchParams), _P(SarVolumeMarchStats), _vp]),
    "sar_flow_params_default": (C.c_int, [_P(SarFlowParams)]),
    "sar_flow_step": (C.c_int, [_cfg_p, _P(SarFlowParams), _P(C.c_double), _P(C.c_int32)]),
    "sar_runtime_render_flow": (C.c_int, [_cfg_p, _vp, _P(SarFlowParams), C.c_uint32, C.c_uint64, _P(C.c_double), _P(SarFlowStats)]),
    "sar_section_params_default": (C.c_int, [_P(SarSectionParams)]),
    "sar_section_step": (C.c_int, [_cfg_p, _P(SarSectionParams), _P(C.c_double), _P(C.c_double), _P(C.c_double), _P(C.c_int32)]),
    "sar_runtime_section": (C.c_int, [_cfg_p, _vp, _P(SarSectionParams), C.c_uint32, _P(C.c_double), _P(C.c_double), _P(C.c_double),
                                      _P(SarSectionRecord), _P(SarSectionStats)]),
    "sar_bin_geometry": (C.c_int, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _P(C.c_uint32)]),
}

# the hooks build only (include/sar_test_hooks.h): attached when the loaded library exports it
OPTIONAL_PROTOTYPES = {
    "sar_runtime_set_test_option": (C.c_int, [_vp, C.c_char_p, C.c_uint64]),
    "sar_runtime_debug_spans": (C.c_int, [_vp, C.c_uint32, _P(C.c_float), C.c_uint32, _P(C.c_uint32)]),
    "sar_runtime_debug_colorize_launches": (C.c_int, [_vp, _P(C.c_uint64)]),
    "sar_runtime_debug_volume_load": (C.c_int, [_vp, C.c_uint32, C.c_double, C.c_double, _P(C.c_uint32)]),
    "sar_runtime_debug_volume_stats": (C.c_int, [_vp, _P(SarVolumeStats)]),
    "sar_runtime_debug_device_log": (C.c_int, [_vp, C.c_uint32, _vp, C.c_uint32, _P(C.c_double)]),
}
STABLE_OPTIONS = ("block_threads", "checkpoint_stride", "hint_bits", "split_waves", "tail_overlap", "timing_accumulate", "search_chunk", "plane_chunk", "gallery_chunk", "orbit_chunk", "corr_chunk", "basin_chunk", "period_chunk", "cycles_chunk", "box_chunk", "box_slots", "density_tile")

# sar_runtime_set_option's names of volume rendering: stable as well, listed apart from the record the names above are held to
VOLUME_OPTIONS = ("volume_chunk", "volume_steps")

LIB_NAME = "libsar_hip.so"
_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG_DIR, LIB_NAME)
HOOKS_PATH = os.path.join(os.path.dirname(_PKG_DIR), "tests", "hooks", "libsar_hip_hooks.so")   # product objects + the test hooks

_lib = None
_default_path = LIB_PATH


def use_hooks_build():
    """From now on load_library() loads the hooks build (the product's object files + sar_runtime_set_test_option): what the
    test-suite and the A/B tools do before their first call. The product is never replaced on disk."""
    global _default_path, _lib
    if not os.path.exists(HOOKS_PATH):
        raise SarLibraryMissing(f"{HOOKS_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    if _default_path != HOOKS_PATH:
        _default_path, _lib = HOOKS_PATH, None


class SarLibraryMissing(RuntimeError):
    pass


def load_library(path: str | None = None) -> C.CDLL:
    """dlopen the in-tree HIP library and attach prototypes. Raises if it is missing — by design
    there is no fallback path."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("SAR_LIBRARY") or _default_path  # SAR_LIBRARY: A/B timing of another build of the same ABI
    if not os.path.exists(p):
        raise SarLibraryMissing(
            f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback."
        )
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in OPTIONAL_PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    if p in (LIB_PATH, HOOKS_PATH):
        verify_library(lib)  # a variant named explicitly (path / SAR_LIBRARY) is the caller's business
    if path is None:
        _lib = lib
    return lib


class SarLibraryStale(RuntimeError):
    pass


def verify_library(lib, csrc: str | None = None):
    """The product library must have been built from the sources that lie next to it: its embedded id (sar_build_id) against
    build.source_id() of the tree. Raises SarLibraryStale on a mismatch; silent where there is no source tree (an installed copy)."""
    from . import build
    if not os.path.isdir(csrc or build.CSRC):
        return
    want = build.source_id(csrc, extra_flags=[])
    got = lib.sar_build_id().decode()
    if got != want:
        raise SarLibraryStale(f"{LIB_NAME} was built from other sources (its id {got}, the tree's {want}): run "
                              "`python -c 'import __graft_entry__ as g; g.build()'` — or name a variant through SAR_LIBRARY")
