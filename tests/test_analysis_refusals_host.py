"""CPU: every refusal the analysis entry points (include/sar.h: sar_runtime_search .. sar_runtime_density) and their host-only
companions make before they touch a device, as a table. Every call goes in with a NULL runtime. A row is one call with one bad
argument — or with two, to pin which of them is reported — and expects the status and the exact sar_last_error text that
tests/golden/analysis_refusals.json records. Before every call the error text is set to SENTINEL, so a refusal without a text of
its own reads SENTINEL, and so does a call that succeeds.

The golden file is a record of the library BEFORE a change to the host code, not of the tree under test:

    python tests/test_analysis_refusals_host.py --record path/to/the/parent's/libsar_hip.so

The cap: FORMATS below lists every set_error format string of the nine family files and of the shared sar_analysis.{hpp,cpp} that
a call can reach with a NULL runtime; NEEDS_A_RUNTIME lists the others with the reason. test_every_format_is_listed holds the two
lists to the sources, test_every_format_has_a_row holds FORMATS to the table. No device needed.

Last, tests/c/sar_analysis_host.c — the calls that succeed: fits, edges, coefficients — is built against the product and run."""
import ctypes as C
import json
import math
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from strange_attractor_renderer_amd import _abi as A  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "analysis_refusals.json")
CSRC = os.path.join(ROOT, "strange_attractor_renderer_amd", "csrc")
FILES = [f"sar_{f}.cpp" for f in ("search", "plane", "gallery", "orbit", "corr", "box", "basin", "period", "density", "analysis")] + ["sar_analysis.hpp"]
SENTINEL = "sar_start_points: first_job beyond 2^36"
NAN, INF = math.nan, math.inf

# ---- the cap ----------------------------------------------------------------------------------------------------------------
FORMATS = [
    # shared (sar_analysis.cpp)
    "%s: transient and steps must be at most 2^31 (%u, %u)",
    "%s: bound must be positive and finite",
    "%s: the plane must hold 1 to 2^24 pixels (%u x %u)",
    "%s: a set must hold 1 to 2^20 points (%u)",
    "%s: the axes must be two distinct coefficients 0..29 (%u, %u)",
    "%s: lo and hi must be finite",
    "%s: coordinate %zu of point %zu of set %zu is NaN",
    # several families
    "%s: the parameters are NULL",
    "%s: the runtime is NULL",
    # search
    "sar_runtime_search: bound must be positive, lo and hi finite",
    "sar_frame_view: extent[%d] is not finite (a trajectory diverged?)",
    "sar_frame_view: the extent is empty or a single point",
    # planes
    "%s: mode must be SAR_PLANE_L1 or SAR_PLANE_SPECTRUM (%d)",
    # gallery
    "sar_runtime_gallery: the parameters are NULL",
    "sar_runtime_gallery: a tile side is 0 (%u x %u)",
    "sar_runtime_gallery: a tile holds at most %u pixels (%u x %u)",
    "sar_runtime_gallery: cols is 0",
    "sar_runtime_gallery: jobs is 0",
    "sar_runtime_gallery: jobs * (iterations / jobs) must stay below 2^32, the visit ordinal is 32 bits (%u jobs, %llu iterations)",
    "sar_runtime_gallery: base is NULL",
    "sar_runtime_gallery: items_host is NULL",
    "sar_runtime_gallery: the runtime or the atlas is NULL",
    "sar_frame_view_box: extent[%d] is not finite (a trajectory diverged?)",
    # orbit diagrams
    "%s: the diagram must hold 1 to %u columns of 1 to %u bins (%u x %u)",
    "%s: jobs must be 1 to %u (%u)",
    "%s: jobs * steps must stay below 2^32, a bin is 32 bits (%u jobs, %u steps)",
    "%s: a and b must be finite (entry %u)",
    "%s: proj must be finite",
    "%s: v_lo and v_hi must be finite with v_lo < v_hi",
    "%s: height / (v_hi - v_lo) is not finite",
    "sar_runtime_orbit: the runtime or the count buffer is NULL",
    # correlation dimension
    "%s: sub_bits must be at most %u (%u)",
    "%s: the exponents must hold -1022 <= e_min < e_max <= 1023 (%d, %d)",
    "%s: at most %u bins (%u)",
    "%s: c_lo must be at least 1 pair",
    "%s: %s must be positive",
    "%s: jobs must be 1 to 2^16 (%u)",
    "%s: samples and stride must be at least 1",
    "%s: jobs * samples must be at most 2^20 points (%u, %u)",
    "%s: transient and stride * samples must be at most 2^31 (%u, %u * %u)",
    "%s: the coefficients must be finite (map %zu, entry %zu)",
    "%s: the start points must be finite (job %zu)",
    "sar_corrdim_fit: the histogram or the result is NULL",
    "sar_runtime_pairs: samples must divide n (%u, %u)",
    "sar_runtime_pairs: the points or the histogram buffer is NULL",
    "sar_runtime_pairs: the runtime is NULL",
    "%s: the coefficients, the histogram buffer or the records are NULL",
    # box counting
    "%s: levels must be 1 to %u (%u)",
    "%s: min_occupancy must be positive",
    "%s: the origin must be finite",
    "%s: size must be finite and positive",
    "%s: the scale 2^levels / size must be finite",
    "sar_box_log2_q32: n must be at least 1 and the result not NULL",
    "%s: the levels or the result is NULL",
    "%s: the points or the levels buffer is NULL",
    "%s: the coefficients, the levels buffer or the records are NULL",
    # basins
    "%s: transient + steps must stay below 2^32, escape_step is 32 bits (%u, %u)",
    "%s: grid must be 1 to %u (%u)",
    "%s: the coefficients must be finite (entry %u)",
    "%s: origin, du and dv must be finite",
    "%s: box_lo and box_hi must be finite with box_lo < box_hi",
    "%s: grid / (box_hi - box_lo) is not finite",
    "sar_runtime_basin: the runtime or the pixel buffer is NULL",
    # period planes
    "%s: max_period must be 1 to 2^31",
    "%s: eps must be finite and not negative",
    "sar_runtime_period: the runtime or the record buffer is NULL",
    # density
    "%s: samples must be %u to %u (%u)",
    "sar_density_weights: class 0 has no table (an empty pixel spreads nothing)",
    "sar_runtime_density: the runtime is NULL",
]
NEEDS_A_RUNTIME = {
    # behind the entry's refusal of a NULL runtime, which has no text or another one
    "sar_runtime_gallery: the atlas is wider than 2^32-1 pixels": "behind the NULL-runtime refusal",
    "sar_runtime_basin: cap is %u and the attractor buffer NULL": "behind the NULL-runtime refusal",
    "sar_runtime_plane_colorize: threshold must be finite, chaos_scale and order_scale positive and finite": "behind the NULL-runtime refusal",
    "sar_runtime_basin_colorize: fade must be positive and finite": "behind the NULL-runtime refusal",
    "sar_runtime_period_colorize: colours must be at least 1": "behind the NULL-runtime refusal",
    "%s: the palette must hold 1 to %d entries (%u)": "colorize_tail: behind the NULL-runtime refusal",
    "%s: the runtime has no %s (%s first)": "colorize_tail: reads the runtime (the GPU tests of the three colorize calls)",
    "%s: box_slots (%u) must be above the points of a set (%u)": "reads the runtime's option (tests/test_gpu_box.py)",
    "sar_runtime_density_tiles: the runtime has not filtered yet (sar_runtime_density first)": "reads the runtime",
    # behind the first HIP call
    "hipFuncSetAttribute(max dynamic LDS) failed: %d": "a HIP failure",
    "sar_runtime_density: the plan outgrew its buffer": "internal, behind the device selection",
    "%s: a hash table of %u slots overflowed with %u points (internal)": "internal, read back from the device",
    "sar_runtime_basin: pixel %u has root %u outside the grid": "internal, read back from the device",
    "sar_runtime_basin: cell %u has root %u outside the grid": "internal, read back from the device",
}


def F(part):
    """the one format string of FORMATS that holds `part`"""
    (fmt,) = [f for f in FORMATS if part in f]
    return fmt


# ---- arguments ---------------------------------------------------------------------------------------------------------------
def _set(obj, path, value):
    """obj.a = v, obj.a[2] = v for path "a" / ("a", 2)"""
    if isinstance(path, tuple):
        getattr(obj, path[0])[path[1]] = value
    else:
        setattr(obj, path, value)


def _params(lib, cls, default, changes):
    p = cls()
    assert getattr(lib, default)(C.byref(p)) == A.SAR_OK
    for path, value in changes:
        _set(p, path, value)
    return p


def _dbl(values):
    return (C.c_double * len(values))(*values)


OUT30 = (C.c_double * 30)()
BIG = C.create_string_buffer(1 << 16)   # any output a call that is refused further down could be handed
COEFFS2 = [0.1] * 60                    # two maps
POINTS = [0.25 * k for k in range(2 * 4 * 3)]  # two sets of four points


def _big(cls=None):
    return C.cast(BIG, C.POINTER(cls)) if cls else C.cast(BIG, C.c_void_p)


def _with(values, at, v):
    values = list(values)
    values[at] = v
    return values


# Every row: (id, format string it reaches or None, call(lib) -> status). The expected status and text are the golden file's.
def _rows():
    R = []

    def row(name, fmt, call):
        R.append((name, fmt, call))

    AXES, SIZE, RANGES = F("the axes"), F("the plane"), F("%s: lo and")
    STEPS, BOUND, SETPTS, NANPT = F("transient and steps"), F("%s: bound must"), F("a set"), F("coordinate %zu")
    PNULL, RTNULL = F("%s: the parameters"), F("%s: the runtime")

    # -- search
    def search(changes, n_out=True, rt=None):
        return lambda lib: lib.sar_runtime_search(rt, C.byref(_params(lib, A.SarSearchParams, "sar_search_params_default", changes)), 0, 4, None,
                                                  None, 0, C.byref(C.c_uint32()) if n_out else None, None)
    row("search.params_null", None, lambda lib: lib.sar_runtime_search(None, None, 0, 4, None, None, 0, C.byref(C.c_uint32()), None))
    row("search.bound_zero", F("sar_runtime_search: bound must"), search([("bound", 0.)]))
    row("search.bound_nan", F("sar_runtime_search: bound must"), search([("bound", NAN)]))
    row("search.lo_inf", F("sar_runtime_search: bound must"), search([("lo", -INF)]))
    row("search.hi_nan", F("sar_runtime_search: bound must"), search([("hi", NAN)]))
    row("search.transient", STEPS, search([("transient", (1 << 31) + 1)]))
    row("search.steps", STEPS, search([("steps", 0xFFFFFFFF)]))
    row("search.bound_and_steps", F("sar_runtime_search: bound must"), search([("bound", -1.), ("steps", 0xFFFFFFFF)]))
    row("search.steps_and_runtime_null", STEPS, search([("steps", 0xFFFFFFFF)], n_out=False))
    row("search.runtime_null", None, search([]))
    row("search.bound_inf_is_accepted", None, search([("bound", INF)]))

    def view(extent, margin=0.1, cfg=True, entry="sar_frame_view"):
        def call(lib):
            c = A.SarConfig()
            assert lib.sar_config_poisson_saturne(C.byref(c)) == A.SAR_OK
            return getattr(lib, entry)(C.byref(c) if cfg else None, _dbl(extent) if extent else None, margin, 0)
        return call
    row("frame_view.cfg_null", None, view([0, 1, 0, 1, 0, 1], cfg=False))
    row("frame_view.extent_null", None, view(None))
    row("frame_view.margin", None, view([0, 1, 0, 1, 0, 1], margin=1.))
    row("frame_view.extent_nan", F("sar_frame_view: extent[%d] is"), view([0, 1, 0, NAN, 0, 1]))
    row("frame_view.extent_inf_first_of_two", F("sar_frame_view: extent[%d] is"), view([0, INF, 0, 1, NAN, 1]))
    row("frame_view.extent_empty", F("the extent"), view([0, 0, 0, 0, 0, 0]))
    row("frame_view.extent_reversed", F("the extent"), view([1, 0, 1, 0, 0, 1]))
    row("frame_view_box.cfg_null", None, view([0, 1, 0, 1, 0, 1], cfg=False, entry="sar_frame_view_box"))
    row("frame_view_box.extent_inf", F("sar_frame_view_box: extent[%d] is"), view([0, 1, 0, 1, 0, INF], entry="sar_frame_view_box"))
    row("frame_view_box.extent_empty", F("the extent"), view([0, 0, 0, 0, 0, 0], entry="sar_frame_view_box"))

    # -- planes: the same faults through sar_plane_coeffs and sar_runtime_plane
    def plane_coeffs(changes, x=0, y=0, out=OUT30):
        return lambda lib: lib.sar_plane_coeffs(C.byref(_params(lib, A.SarPlaneParams, "sar_plane_params_default", changes)), x, y, out)

    def plane_run(changes, out=True):
        return lambda lib: lib.sar_runtime_plane(None, C.byref(_params(lib, A.SarPlaneParams, "sar_plane_params_default", changes)),
                                                 _big() if out else None, None)
    row("plane_coeffs.params_null", None, lambda lib: lib.sar_plane_coeffs(None, 0, 0, OUT30))
    row("plane.params_null", None, lambda lib: lib.sar_runtime_plane(None, None, _big(), None))
    for name, make in (("plane_coeffs", plane_coeffs), ("plane", plane_run)):
        row(f"{name}.axes_equal", AXES, make([(("axis", 0), 3), (("axis", 1), 3)]))
        row(f"{name}.axis0_30", AXES, make([(("axis", 0), 30)]))
        row(f"{name}.axis1_30", AXES, make([(("axis", 1), 30)]))
        row(f"{name}.width_zero", SIZE, make([("width", 0)]))
        row(f"{name}.height_zero", SIZE, make([("height", 0)]))
        row(f"{name}.too_large", SIZE, make([("width", 4097), ("height", 4096)]))
        row(f"{name}.lo0_nan", RANGES, make([(("lo", 0), NAN)]))
        row(f"{name}.lo1_inf", RANGES, make([(("lo", 1), INF)]))
        row(f"{name}.hi0_inf", RANGES, make([(("hi", 0), -INF)]))
        row(f"{name}.hi1_nan", RANGES, make([(("hi", 1), NAN)]))
        row(f"{name}.bound_zero", BOUND, make([("bound", 0.)]))
        row(f"{name}.bound_inf", BOUND, make([("bound", INF)]))
        row(f"{name}.bound_nan", BOUND, make([("bound", NAN)]))
        row(f"{name}.transient", STEPS, make([("transient", (1 << 31) + 1)]))
        row(f"{name}.steps", STEPS, make([("steps", (1 << 31) + 1)]))
        row(f"{name}.mode", F("mode must"), make([("mode", 2)]))
        row(f"{name}.axes_and_size", AXES, make([(("axis", 0), 30), ("width", 0)]))
        row(f"{name}.size_and_ranges", SIZE, make([("width", 0), (("lo", 0), NAN)]))
        row(f"{name}.ranges_and_bound", RANGES, make([(("hi", 1), NAN), ("bound", 0.)]))
        row(f"{name}.bound_and_steps", BOUND, make([("bound", 0.), ("steps", (1 << 31) + 1)]))
        row(f"{name}.steps_and_mode", STEPS, make([("steps", (1 << 31) + 1), ("mode", 0)]))
    row("plane_coeffs.x", None, plane_coeffs([("width", 5), ("height", 4)], x=5))
    row("plane_coeffs.y", None, plane_coeffs([("width", 5), ("height", 4)], y=4))
    row("plane_coeffs.out_null", None, plane_coeffs([], out=None))
    row("plane_coeffs.mode_and_out_null", F("mode must"), plane_coeffs([("mode", 2)], out=None))
    row("plane_coeffs.ok", None, plane_coeffs([("width", 5), ("height", 4)], x=4, y=3))
    row("plane.runtime_null", None, plane_run([]))
    row("plane.mode_and_out_null", F("mode must"), plane_run([("mode", 2)], out=False))
    row("plane_colorize.runtime_null", None, lambda lib: lib.sar_runtime_plane_colorize(C.byref(A.SarConfig()), None, None, _big(C.c_uint16)))

    # -- period planes: the size first, the sweep's axes and ranges last and only without a coefficient list
    def period_coeffs(changes, x=0, y=0, out=OUT30):
        return lambda lib: lib.sar_period_coeffs(C.byref(_params(lib, A.SarPeriodParams, "sar_period_params_default", changes)), x, y, out)

    def period_run(changes, coeffs=False, out=True):
        return lambda lib: lib.sar_runtime_period(None, C.byref(_params(lib, A.SarPeriodParams, "sar_period_params_default", changes)),
                                                  _big(C.c_double) if coeffs else None, _big(A.SarPeriodRecord) if out else None, None)
    row("period_coeffs.params_null", PNULL, lambda lib: lib.sar_period_coeffs(None, 0, 0, OUT30))
    row("period.params_null", PNULL, lambda lib: lib.sar_runtime_period(None, None, None, _big(A.SarPeriodRecord), None))
    for name, make in (("period_coeffs", period_coeffs), ("period", period_run)):
        row(f"{name}.width_zero", SIZE, make([("width", 0)]))
        row(f"{name}.too_large", SIZE, make([("width", 4096), ("height", 4097)]))
        row(f"{name}.bound_zero", BOUND, make([("bound", 0.)]))
        row(f"{name}.bound_inf", BOUND, make([("bound", INF)]))
        row(f"{name}.transient", STEPS, make([("transient", (1 << 31) + 1)]))
        row(f"{name}.max_period_large", STEPS, make([("max_period", (1 << 31) + 1)]))
        row(f"{name}.max_period_zero", F("max_period must"), make([("max_period", 0)]))
        row(f"{name}.eps_negative", F("%s: eps must"), make([("eps", -1e-9)]))
        row(f"{name}.eps_nan", F("%s: eps must"), make([("eps", NAN)]))
        row(f"{name}.eps_inf", F("%s: eps must"), make([("eps", INF)]))
        row(f"{name}.axes_equal", AXES, make([(("axis", 0), 7), (("axis", 1), 7)]))
        row(f"{name}.axis1_30", AXES, make([(("axis", 1), 30)]))
        row(f"{name}.lo0_nan", RANGES, make([(("lo", 0), NAN)]))
        row(f"{name}.hi1_inf", RANGES, make([(("hi", 1), INF)]))
        row(f"{name}.size_and_bound", SIZE, make([("height", 0), ("bound", 0.)]))
        row(f"{name}.bound_and_steps", BOUND, make([("bound", NAN), ("transient", (1 << 31) + 1)]))
        row(f"{name}.steps_and_max_period", STEPS, make([("transient", (1 << 31) + 1), ("max_period", 0)]))
        row(f"{name}.max_period_and_eps", F("max_period must"), make([("max_period", 0), ("eps", -1.)]))
        row(f"{name}.eps_and_axes", F("%s: eps must"), make([("eps", -1.), (("axis", 0), 30)]))
        row(f"{name}.axes_and_ranges", AXES, make([(("axis", 0), 30), (("lo", 0), NAN)]))
        row(f"{name}.size_and_axes", SIZE, make([("width", 0), (("axis", 0), 30)]))
    row("period_coeffs.x", None, period_coeffs([("width", 5), ("height", 4)], x=5))
    row("period_coeffs.y", None, period_coeffs([("width", 5), ("height", 4)], y=4))
    row("period_coeffs.out_null", None, period_coeffs([], out=None))
    row("period_coeffs.ranges_and_out_null", RANGES, period_coeffs([(("hi", 0), NAN)], out=None))
    row("period_coeffs.ok", None, period_coeffs([("width", 5), ("height", 4)], x=4, y=3))
    row("period.runtime_null", F("sar_runtime_period: the runtime"), period_run([]))
    row("period.out_null", F("sar_runtime_period: the runtime"), period_run([], out=False))
    row("period.list_skips_the_axes", F("sar_runtime_period: the runtime"), period_run([(("axis", 0), 30)], coeffs=True))
    row("period.list_skips_the_ranges", F("sar_runtime_period: the runtime"), period_run([(("lo", 1), NAN)], coeffs=True))
    row("period.list_keeps_the_size", SIZE, period_run([("width", 0)], coeffs=True))
    row("period.ranges_and_runtime_null", RANGES, period_run([(("lo", 1), NAN)], out=False))
    row("period_colorize.runtime_null", None, lambda lib: lib.sar_runtime_period_colorize(C.byref(A.SarConfig()), None, None, _big(C.c_uint16)))

    # -- basins
    def basin_start(changes, x=0, y=0, out=OUT30):
        return lambda lib: lib.sar_basin_start(C.byref(_params(lib, A.SarBasinParams, "sar_basin_params_default", changes)), x, y, out)

    def basin_run(changes, out=True):
        return lambda lib: lib.sar_runtime_basin(None, C.byref(_params(lib, A.SarBasinParams, "sar_basin_params_default", changes)),
                                                 _big(A.SarBasinPixel) if out else None, None, 0, None, None)
    row("basin_start.params_null", PNULL, lambda lib: lib.sar_basin_start(None, 0, 0, OUT30))
    row("basin.params_null", PNULL, lambda lib: lib.sar_runtime_basin(None, None, _big(A.SarBasinPixel), None, 0, None, None))
    for name, make in (("basin_start", basin_start), ("basin", basin_run)):
        row(f"{name}.width_zero", SIZE, make([("width", 0)]))
        row(f"{name}.too_large", SIZE, make([("width", 8192), ("height", 2049)]))
        row(f"{name}.steps", STEPS, make([("steps", (1 << 31) + 1)]))
        row(f"{name}.transient_plus_steps", F("transient +"), make([("transient", 1 << 31), ("steps", 1 << 31)]))
        row(f"{name}.grid_zero", F("grid must"), make([("grid", 0)]))
        row(f"{name}.grid_large", F("grid must"), make([("grid", 129)]))
        row(f"{name}.coeff_nan", F("the coefficients must be finite (entry"), make([(("coeffs", 7), NAN)]))
        row(f"{name}.coeff_inf_first_of_two", F("the coefficients must be finite (entry"), make([(("coeffs", 29), NAN), (("coeffs", 11), INF)]))
        row(f"{name}.origin_nan", F("origin, du"), make([(("origin", 2), NAN)]))
        row(f"{name}.du_inf", F("origin, du"), make([(("du", 0), INF)]))
        row(f"{name}.dv_nan", F("origin, du"), make([(("dv", 1), NAN)]))
        row(f"{name}.bound_zero", BOUND, make([("bound", 0.)]))
        row(f"{name}.box_reversed", F("box_lo and"), make([(("box_lo", 1), 1.), (("box_hi", 1), 1.)]))
        row(f"{name}.box_nan", F("box_lo and"), make([(("box_hi", 2), NAN)]))
        row(f"{name}.box_scale", F("grid /"), make([(("box_lo", 0), 0.), (("box_hi", 0), 5e-324)]))
        row(f"{name}.size_and_steps", SIZE, make([("height", 0), ("steps", (1 << 31) + 1)]))
        row(f"{name}.steps_and_grid", STEPS, make([("steps", (1 << 31) + 1), ("grid", 0)]))
        row(f"{name}.grid_and_coeff", F("grid must"), make([("grid", 0), (("coeffs", 0), NAN)]))
        row(f"{name}.coeff_and_origin", F("the coefficients must be finite (entry"), make([(("coeffs", 0), NAN), (("origin", 0), NAN)]))
        row(f"{name}.origin_and_bound", F("origin, du"), make([(("origin", 0), NAN), ("bound", 0.)]))
        row(f"{name}.bound_and_box", BOUND, make([("bound", INF), (("box_hi", 0), NAN)]))
    row("basin_start.x", None, basin_start([("width", 5), ("height", 4)], x=5))
    row("basin_start.out_null", None, basin_start([], out=None))
    row("basin_start.ok", None, basin_start([("width", 5), ("height", 4)], x=4, y=3))
    row("basin.runtime_null", F("sar_runtime_basin: the runtime"), basin_run([]))
    row("basin.box_and_runtime_null", F("box_lo and"), basin_run([(("box_hi", 2), NAN)], out=False))
    row("basin_colorize.runtime_null", None, lambda lib: lib.sar_runtime_basin_colorize(C.byref(A.SarConfig()), None, None, _big(C.c_uint16)))

    # -- orbit diagrams
    def orbit_coeffs(changes, column=0, out=OUT30):
        return lambda lib: lib.sar_orbit_coeffs(C.byref(_params(lib, A.SarOrbitParams, "sar_orbit_params_default", changes)), column, out)

    def orbit_run(changes, out=True):
        return lambda lib: lib.sar_runtime_orbit(None, C.byref(_params(lib, A.SarOrbitParams, "sar_orbit_params_default", changes)), None,
                                                 _big(C.c_uint32) if out else None, None, None)
    row("orbit_coeffs.params_null", PNULL, lambda lib: lib.sar_orbit_coeffs(None, 0, OUT30))
    row("orbit.params_null", PNULL, lambda lib: lib.sar_runtime_orbit(None, None, None, _big(C.c_uint32), None, None))
    for name, make in (("orbit_coeffs", orbit_coeffs), ("orbit", orbit_run)):
        row(f"{name}.width_zero", F("the diagram"), make([("width", 0)]))
        row(f"{name}.width_large", F("the diagram"), make([("width", 65537)]))
        row(f"{name}.height_zero", F("the diagram"), make([("height", 0)]))
        row(f"{name}.height_large", F("the diagram"), make([("height", 32769)]))
        row(f"{name}.jobs_zero", F("jobs must be 1 to %u"), make([("jobs", 0)]))
        row(f"{name}.jobs_large", F("jobs must be 1 to %u"), make([("jobs", 1025)]))
        row(f"{name}.transient", STEPS, make([("transient", (1 << 31) + 1)]))
        row(f"{name}.jobs_times_steps", F("jobs * steps"), make([("jobs", 1024), ("steps", 1 << 22)]))
        row(f"{name}.a_nan", F("a and"), make([(("a", 4), NAN)]))
        row(f"{name}.b_inf_first_of_two", F("a and"), make([(("b", 9), INF), (("a", 12), NAN)]))
        row(f"{name}.bound_nan", BOUND, make([("bound", NAN)]))
        row(f"{name}.proj_nan", F("proj must"), make([(("proj", 1), NAN)]))
        row(f"{name}.v_reversed", F("v_lo and"), make([("v_lo", 1.), ("v_hi", 1.)]))
        row(f"{name}.v_inf", F("v_lo and"), make([("v_hi", INF)]))
        row(f"{name}.v_scale", F("height /"), make([("v_lo", 0.), ("v_hi", 5e-324)]))
        row(f"{name}.size_and_jobs", F("the diagram"), make([("width", 0), ("jobs", 0)]))
        row(f"{name}.jobs_and_steps", F("jobs must be 1 to %u"), make([("jobs", 0), ("steps", (1 << 31) + 1)]))
        row(f"{name}.steps_and_a", STEPS, make([("steps", (1 << 31) + 1), (("a", 0), NAN)]))
        row(f"{name}.a_and_bound", F("a and"), make([(("a", 0), NAN), ("bound", 0.)]))
        row(f"{name}.bound_and_proj", BOUND, make([("bound", 0.), (("proj", 0), NAN)]))
        row(f"{name}.proj_and_v", F("proj must"), make([(("proj", 0), NAN), ("v_hi", NAN)]))
    row("orbit_coeffs.column", None, orbit_coeffs([("width", 5)], column=5))
    row("orbit_coeffs.out_null", None, orbit_coeffs([], out=None))
    row("orbit_coeffs.ok", None, orbit_coeffs([("width", 5)], column=4))
    row("orbit.runtime_null", F("sar_runtime_orbit: the runtime"), orbit_run([]))
    row("orbit.v_and_runtime_null", F("v_lo and"), orbit_run([("v_hi", NAN)], out=False))

    # -- gallery
    def gallery(changes, base=True, n=1, items=True, atlas=True, cfg_changes=()):
        def call(lib):
            c = A.SarConfig()
            assert lib.sar_config_poisson_saturne(C.byref(c)) == A.SAR_OK
            for path, value in cfg_changes:
                _set(c, path, value)
            p = _params(lib, A.SarGalleryParams, "sar_gallery_params_default", changes)
            return lib.sar_runtime_gallery(None, C.byref(c) if base else None, C.byref(p), n, _big(A.SarGalleryItem) if items else None, None,
                                           _big(C.c_uint16) if atlas else None, None, None, None, None)
        return call
    row("gallery.params_null", F("sar_runtime_gallery: the parameters"), lambda lib: lib.sar_runtime_gallery(None, C.byref(A.SarConfig()), None, 1, _big(A.SarGalleryItem),
                                                                                 None, _big(C.c_uint16), None, None, None, None))
    row("gallery.tile_width_zero", F("a tile side"), gallery([("tile_width", 0)]))
    row("gallery.tile_height_zero", F("a tile side"), gallery([("tile_height", 0)]))
    row("gallery.tile_pixels", F("a tile holds"), gallery([("tile_width", 129), ("tile_height", 128)]))
    row("gallery.tile_pixels_wrap", F("a tile holds"), gallery([("tile_width", 1 << 16), ("tile_height", 1 << 16)]))
    row("gallery.cols_zero", F("cols is"), gallery([("cols", 0)]))
    row("gallery.jobs_zero", F("jobs is"), gallery([("jobs", 0)]))
    row("gallery.iterations", F("sar_runtime_gallery: jobs *"), gallery([("iterations", 1 << 32)]))
    row("gallery.iterations_per_job", F("sar_runtime_gallery: jobs *"), gallery([("jobs", 1), ("iterations", 1 << 63)]))
    row("gallery.base_null", F("base is"), gallery([], base=False))
    row("gallery.base_invalid", None, gallery([], cfg_changes=[("palette_len", 0)]))
    row("gallery.items_null", F("items_host is"), gallery([], items=False))
    row("gallery.no_tiles", None, gallery([], n=0, items=False, atlas=False))
    row("gallery.runtime_null", F("sar_runtime_gallery: the runtime"), gallery([]))
    row("gallery.atlas_null", F("sar_runtime_gallery: the runtime"), gallery([], atlas=False))
    row("gallery.tile_and_cols", F("a tile side"), gallery([("tile_width", 0), ("cols", 0)]))
    row("gallery.cols_and_jobs", F("cols is"), gallery([("cols", 0), ("jobs", 0)]))
    row("gallery.jobs_and_base_null", F("jobs is"), gallery([("jobs", 0)], base=False))
    row("gallery.iterations_and_base_null", F("sar_runtime_gallery: jobs *"), gallery([("iterations", 1 << 32)], base=False))
    row("gallery.base_invalid_and_items_null", None, gallery([], items=False, cfg_changes=[("palette_len", 0)]))
    row("gallery.items_null_and_runtime_null", F("items_host is"), gallery([], items=False, atlas=False))

    # -- correlation dimension: the edges, the fit, the pair counts of given sets, the maps
    def pairs_params(lib, changes):
        return C.byref(_params(lib, A.SarPairsParams, "sar_pairs_params_default", changes))
    BINNING = [("sub_bits", F("sub_bits must"), [("sub_bits", 5)]), ("exponents_equal", F("the exponents"), [("e_min", 3), ("e_max", 3)]),
               ("e_min_low", F("the exponents"), [("e_min", -1023)]), ("e_max_high", F("the exponents"), [("e_max", 1024)]),
               ("bins", F("%s: at most"), [("sub_bits", 4)]), ("sub_bits_and_exponents", F("sub_bits must"), [("sub_bits", 5), ("e_max", -64)]),
               ("exponents_and_bins", F("the exponents"), [("sub_bits", 4), ("e_max", 1024)])]
    HIST = (C.c_uint64 * 1154)()
    LINE = A.SarCorrdimLine()

    def pairs(changes, n_sets=2, n=4, points=POINTS, hist=True):
        return lambda lib: lib.sar_runtime_pairs(None, pairs_params(lib, changes), n_sets, n, _dbl(points) if points else None,
                                                 _big(C.c_uint64) if hist else None, None)

    def corrdim(changes, n_maps=2, coeffs=COEFFS2, starts=None, hist=True, records=True):
        def call(lib):
            p = _params(lib, A.SarCorrdimParams, "sar_corrdim_params_default", [("jobs", 2), ("samples", 4)] + changes)
            return lib.sar_runtime_corrdim(None, C.byref(p), n_maps, _dbl(coeffs) if coeffs else None, _dbl(starts) if starts else None,
                                           _big(C.c_uint64) if hist else None, _big(A.SarCorrdimRecord) if records else None, None)
        return call
    for name, fmt, changes in BINNING:
        row(f"pairs_edges.{name}", fmt, lambda lib, ch=changes: lib.sar_pairs_edges(pairs_params(lib, ch), C.byref(C.c_uint32()), None))
        row(f"corrdim_fit.{name}", fmt, lambda lib, ch=changes: lib.sar_corrdim_fit(HIST, pairs_params(lib, ch), 10., 1., C.byref(LINE)))
        row(f"pairs.{name}", fmt, pairs(changes))
        row(f"corrdim.{name}", fmt, corrdim(changes))
    row("pairs_edges.defaults", None, lambda lib: lib.sar_pairs_edges(None, C.byref(C.c_uint32()), None))
    row("corrdim_fit.c_lo", F("c_lo must"), lambda lib: lib.sar_corrdim_fit(HIST, None, 0.5, 1., C.byref(LINE)))
    row("corrdim_fit.c_lo_nan", F("c_lo must"), lambda lib: lib.sar_corrdim_fit(HIST, None, NAN, 1., C.byref(LINE)))
    row("corrdim_fit.r_hi", F("%s must"), lambda lib: lib.sar_corrdim_fit(HIST, None, 10., 0., C.byref(LINE)))
    row("corrdim_fit.r_hi_nan", F("%s must"), lambda lib: lib.sar_corrdim_fit(HIST, None, 10., NAN, C.byref(LINE)))
    row("corrdim_fit.hist_null", F("sar_corrdim_fit: the histogram"), lambda lib: lib.sar_corrdim_fit(None, None, 10., 1., C.byref(LINE)))
    row("corrdim_fit.out_null", F("sar_corrdim_fit: the histogram"), lambda lib: lib.sar_corrdim_fit(HIST, None, 10., 1., None))
    row("corrdim_fit.binning_and_c_lo", F("sub_bits must"), lambda lib: lib.sar_corrdim_fit(HIST, pairs_params(lib, [("sub_bits", 5)]), 0., 1., C.byref(LINE)))
    row("corrdim_fit.c_lo_and_r_hi", F("c_lo must"), lambda lib: lib.sar_corrdim_fit(HIST, None, 0., 0., C.byref(LINE)))
    row("corrdim_fit.r_hi_and_hist_null", F("%s must"), lambda lib: lib.sar_corrdim_fit(None, None, 10., 0., C.byref(LINE)))
    row("corrdim_fit.ok", None, lambda lib: lib.sar_corrdim_fit(HIST, None, 10., 1., C.byref(LINE)))
    row("pairs.n_zero", SETPTS, pairs([], n=0))
    row("pairs.n_large", SETPTS, pairs([], n=(1 << 20) + 1, n_sets=0))
    row("pairs.samples", F("sar_runtime_pairs: samples must"), pairs([("samples", 3)]))
    row("pairs.no_sets", None, pairs([], n_sets=0, points=None, hist=False))
    row("pairs.points_null", F("sar_runtime_pairs: the points"), pairs([], points=None))
    row("pairs.hist_null", F("sar_runtime_pairs: the points"), pairs([], hist=False))
    row("pairs.nan", NANPT, pairs([], points=_with(POINTS, 1 * 12 + 2 * 3 + 1, NAN)))
    row("pairs.nan_first_of_two", NANPT, pairs([], points=_with(_with(POINTS, 23, NAN), 2, NAN)))
    row("pairs.inf_is_accepted", F("sar_runtime_pairs: the runtime"), pairs([], points=_with(POINTS, 5, INF)))
    row("pairs.runtime_null", F("sar_runtime_pairs: the runtime"), pairs([]))
    row("pairs.defaults_runtime_null", F("sar_runtime_pairs: the runtime"), lambda lib: lib.sar_runtime_pairs(None, None, 2, 4, _dbl(POINTS), _big(C.c_uint64), None))
    row("pairs.binning_and_n", F("sub_bits must"), pairs([("sub_bits", 5)], n=0))
    row("pairs.n_and_samples", SETPTS, pairs([("samples", 3)], n=0))
    row("pairs.samples_and_points_null", F("sar_runtime_pairs: samples must"), pairs([("samples", 3)], points=None))
    row("pairs.samples_and_no_sets", F("sar_runtime_pairs: samples must"), pairs([("samples", 3)], n_sets=0))
    row("pairs.points_null_and_runtime_null", F("sar_runtime_pairs: the points"), pairs([], points=None))
    row("pairs.nan_and_runtime_null", NANPT, pairs([], points=_with(POINTS, 0, NAN)))
    row("corrdim.params_null", PNULL, lambda lib: lib.sar_runtime_corrdim(None, None, 2, _dbl(COEFFS2), None, _big(C.c_uint64),
                                                                          _big(A.SarCorrdimRecord), None))
    SHAPE = [("jobs_zero", F("jobs must be 1 to 2^16"), [("jobs", 0)]), ("jobs_large", F("jobs must be 1 to 2^16"), [("jobs", (1 << 16) + 1)]),
             ("samples_zero", F("samples and"), [("samples", 0)]), ("stride_zero", F("samples and"), [("stride", 0)]),
             ("points", F("jobs * samples"), [("jobs", 1 << 16), ("samples", 17)]), ("transient", F("transient and stride"), [("transient", (1 << 31) + 1)]),
             ("stride_times_samples", F("transient and stride"), [("jobs", 1), ("samples", 1 << 20), ("stride", 1 << 12)]),
             ("bound_zero", BOUND, [("bound", 0.)]), ("bound_inf", BOUND, [("bound", INF)]),
             ("jobs_and_samples", F("jobs must be 1 to 2^16"), [("jobs", 0), ("samples", 0)]), ("samples_and_transient", F("samples and"), [("stride", 0), ("transient", 0xFFFFFFFF)]),
             ("points_and_transient", F("jobs * samples"), [("jobs", 1 << 16), ("samples", 17), ("transient", 0xFFFFFFFF)]),
             ("transient_and_bound", F("transient and stride"), [("transient", 0xFFFFFFFF), ("bound", 0.)])]

    def boxdim(changes, n_maps=2, coeffs=COEFFS2, starts=None, levels=True, records=True):
        def call(lib):
            p = _params(lib, A.SarBoxdimParams, "sar_boxdim_params_default", [("jobs", 2), ("samples", 4)] + changes)
            return lib.sar_runtime_boxdim(None, C.byref(p), n_maps, _dbl(coeffs) if coeffs else None, _dbl(starts) if starts else None,
                                          _big(A.SarBoxLevel) if levels else None, _big(A.SarBoxdimRecord) if records else None, None)
        return call
    for name, fmt, changes in SHAPE:
        row(f"corrdim.{name}", fmt, corrdim(changes))
        row(f"boxdim.{name}", fmt, boxdim(changes))
    for name, make, nulls in (("corrdim", corrdim, F("the coefficients, the histogram")), ("boxdim", boxdim, F("the coefficients, the levels"))):
        row(f"{name}.no_maps", None, make([], n_maps=0, coeffs=None, records=False))
        row(f"{name}.coeffs_null", nulls, make([], coeffs=None))
        row(f"{name}.records_null", nulls, make([], records=False))
        row(f"{name}.coeff_nan", F("the coefficients must be finite (map"), make([], coeffs=_with(COEFFS2, 33, NAN)))
        row(f"{name}.coeff_inf_first_of_two", F("the coefficients must be finite (map"), make([], coeffs=_with(_with(COEFFS2, 59, NAN), 4, -INF)))
        row(f"{name}.start_nan", F("the start"), make([], starts=[0.1, 0.1, 0.1, 0.1, 0.1, NAN]))
        row(f"{name}.start_inf", F("the start"), make([], starts=[0.1, INF, 0.1, 0.1, 0.1, 0.1]))
        row(f"{name}.coeff_and_start", F("the coefficients must be finite (map"), make([], coeffs=_with(COEFFS2, 33, NAN), starts=[NAN] * 6))
        row(f"{name}.runtime_null", RTNULL, make([]))
        row(f"{name}.runtime_null_with_starts", RTNULL, make([], starts=[0.1] * 6))
        row(f"{name}.bound_and_no_maps", BOUND, make([("bound", 0.)], n_maps=0))
        row(f"{name}.nulls_and_coeff", nulls, make([], coeffs=_with(COEFFS2, 0, NAN), records=False))
    row("corrdim.hist_null", F("the coefficients, the histogram"), corrdim([], hist=False))
    row("corrdim.c_lo", F("c_lo must"), corrdim([("c_lo", 0.5)]))
    row("corrdim.r_hi_fraction", F("%s must"), corrdim([("r_hi_fraction", 0.)]))
    row("corrdim.binning_and_shape", F("sub_bits must"), corrdim([("sub_bits", 5), ("jobs", 0)]))
    row("corrdim.bound_and_c_lo", BOUND, corrdim([("bound", 0.), ("c_lo", 0.)]))
    row("corrdim.c_lo_and_no_maps", F("c_lo must"), corrdim([("c_lo", 0.)], n_maps=0))
    row("corrdim.r_hi_fraction_and_nulls", F("%s must"), corrdim([("r_hi_fraction", -1.)], coeffs=None))

    # -- box counting
    def box_params(lib, changes):
        return C.byref(_params(lib, A.SarBoxParams, "sar_box_params_default", changes))

    def boxes(changes, n_sets=2, n=4, points=POINTS, levels=True):
        return lambda lib: lib.sar_runtime_boxes(None, box_params(lib, changes), n_sets, n, _dbl(points) if points else None,
                                                 _big(A.SarBoxLevel) if levels else None)
    LEVELS = (A.SarBoxLevel * 17)()
    LINES = A.SarBoxdimLines()

    def boxdim_fit(L=16, n=1000, occupancy=4., levels=True, out=True):
        return lambda lib: lib.sar_boxdim_fit(LEVELS if levels else None, L, n, 1, occupancy, C.byref(LINES) if out else None)
    row("box_log2.n_zero", F("sar_box_log2_q32: n must"), lambda lib: lib.sar_box_log2_q32(0, C.byref(C.c_uint64())))
    row("box_log2.out_null", F("sar_box_log2_q32: n must"), lambda lib: lib.sar_box_log2_q32(5, None))
    row("boxdim_fit.levels_zero", F("levels must"), boxdim_fit(L=0))
    row("boxdim_fit.levels_large", F("levels must"), boxdim_fit(L=17))
    row("boxdim_fit.n_zero", SETPTS, boxdim_fit(n=0))
    row("boxdim_fit.n_large", SETPTS, boxdim_fit(n=(1 << 20) + 1))
    row("boxdim_fit.occupancy_zero", F("min_occupancy must"), boxdim_fit(occupancy=0.))
    row("boxdim_fit.occupancy_nan", F("min_occupancy must"), boxdim_fit(occupancy=NAN))
    row("boxdim_fit.levels_null", F("%s: the levels"), boxdim_fit(levels=False))
    row("boxdim_fit.out_null", F("%s: the levels"), boxdim_fit(out=False))
    row("boxdim_fit.levels_and_n", F("levels must"), boxdim_fit(L=0, n=0))
    row("boxdim_fit.n_and_occupancy", SETPTS, boxdim_fit(n=0, occupancy=0.))
    row("boxdim_fit.occupancy_and_null", F("min_occupancy must"), boxdim_fit(occupancy=0., out=False))
    row("boxdim_fit.ok", None, boxdim_fit())
    row("boxes.levels_zero", F("levels must"), boxes([("levels", 0)]))
    row("boxes.levels_large", F("levels must"), boxes([("levels", 17)]))
    row("boxes.origin_nan", F("the origin"), boxes([(("origin", 1), NAN)]))
    row("boxes.size_zero", F("%s: size must"), boxes([("size", 0.)]))
    row("boxes.size_inf", F("%s: size must"), boxes([("size", INF)]))
    row("boxes.scale", F("the scale"), boxes([("size", 5e-324)]))
    row("boxes.n_zero", SETPTS, boxes([], n=0))
    row("boxes.n_large", SETPTS, boxes([], n=(1 << 20) + 1, n_sets=0))
    row("boxes.no_sets", None, boxes([], n_sets=0, points=None, levels=False))
    row("boxes.points_null", F("%s: the points"), boxes([], points=None))
    row("boxes.levels_null", F("%s: the points"), boxes([], levels=False))
    row("boxes.nan", NANPT, boxes([], points=_with(POINTS, 1 * 12 + 3 * 3 + 2, NAN)))
    row("boxes.nan_first_of_two", NANPT, boxes([], points=_with(_with(POINTS, 22, NAN), 4, NAN)))
    row("boxes.runtime_null", RTNULL, boxes([]))
    row("boxes.defaults_runtime_null", RTNULL, lambda lib: lib.sar_runtime_boxes(None, None, 2, 4, _dbl(POINTS), _big(A.SarBoxLevel)))
    row("boxes.levels_and_origin", F("levels must"), boxes([("levels", 0), (("origin", 0), NAN)]))
    row("boxes.origin_and_size", F("the origin"), boxes([(("origin", 0), NAN), ("size", 0.)]))
    row("boxes.size_and_n", F("%s: size must"), boxes([("size", 0.)], n=0))
    row("boxes.n_and_points_null", SETPTS, boxes([], n=0, points=None))
    row("boxes.points_null_and_runtime_null", F("%s: the points"), boxes([], points=None))
    row("boxes.nan_and_runtime_null", NANPT, boxes([], points=_with(POINTS, 0, NAN)))
    row("boxdim.params_null", PNULL, lambda lib: lib.sar_runtime_boxdim(None, None, 2, _dbl(COEFFS2), None, _big(A.SarBoxLevel),
                                                                        _big(A.SarBoxdimRecord), None))
    row("boxdim.levels_zero", F("levels must"), boxdim([("levels", 0)]))
    row("boxdim.levels_large", F("levels must"), boxdim([("levels", 17)]))
    row("boxdim.levels_null", F("the coefficients, the levels"), boxdim([], levels=False))
    row("boxdim.occupancy", F("min_occupancy must"), boxdim([("min_occupancy", 0.)]))
    row("boxdim.levels_and_shape", F("levels must"), boxdim([("levels", 0), ("jobs", 0)]))
    row("boxdim.bound_and_occupancy", BOUND, boxdim([("bound", 0.), ("min_occupancy", 0.)]))
    row("boxdim.occupancy_and_no_maps", F("min_occupancy must"), boxdim([("min_occupancy", 0.)], n_maps=0))

    # -- density
    def density_params(lib, changes):
        return C.byref(_params(lib, A.SarDensityParams, "sar_density_params_default", changes))
    W = (C.c_uint32 * 256)()
    row("density_radius.samples_low", F("%s: samples must"), lambda lib: lib.sar_density_radius(density_params(lib, [("samples", 1)]), C.byref(C.c_uint32())))
    row("density_radius.samples_high", F("%s: samples must"), lambda lib: lib.sar_density_radius(density_params(lib, [("samples", 257)]), C.byref(C.c_uint32())))
    row("density_radius.out_null", None, lambda lib: lib.sar_density_radius(None, None))
    row("density_radius.samples_and_out_null", F("%s: samples must"), lambda lib: lib.sar_density_radius(density_params(lib, [("samples", 0)]), None))
    row("density_radius.defaults", None, lambda lib: lib.sar_density_radius(None, C.byref(C.c_uint32())))
    row("density_weights.samples", F("%s: samples must"), lambda lib: lib.sar_density_weights(density_params(lib, [("samples", 257)]), 1, W))
    row("density_weights.class_zero", F("class 0"), lambda lib: lib.sar_density_weights(None, 0, W))
    row("density_weights.out_null", None, lambda lib: lib.sar_density_weights(None, 1, None))
    row("density_weights.samples_and_class", F("%s: samples must"), lambda lib: lib.sar_density_weights(density_params(lib, [("samples", 1)]), 0, W))
    row("density_weights.class_and_out_null", F("class 0"), lambda lib: lib.sar_density_weights(None, 0, None))
    row("density.samples", F("%s: samples must"), lambda lib: lib.sar_runtime_density(None, density_params(lib, [("samples", 1)]), None))
    row("density.runtime_null", F("sar_runtime_density: the runtime"), lambda lib: lib.sar_runtime_density(None, None, None))
    row("density_tiles.runtime_null", None, lambda lib: lib.sar_runtime_density_tiles(None, C.byref(C.c_uint32()), C.byref(C.c_uint32())))
    return R


ROWS = _rows()


def _run(lib, call):
    assert lib.sar_start_points(0, 1 << 37, 0, None) == A.SAR_ERR_RANGE and lib.sar_last_error().decode() == SENTINEL
    status = call(lib)
    return [int(status), lib.sar_last_error().decode()]


def _format_regex(fmt):
    """the texts a printf format can produce, as a regular expression"""
    out = re.escape(fmt)
    for spec, pattern in ((r"%llu", r"\d+"), (r"%zu", r"\d+"), (r"%u", r"\d+"), (r"%d", r"-?\d+"), (r"%s", r".+")):
        out = out.replace(re.escape(spec), pattern)
    return re.compile(out + r"\Z", re.S)


def _source_formats():
    found = set()
    for name in FILES:
        text = open(os.path.join(CSRC, name)).read()
        for m in re.finditer(r'set_error\(\s*((?:"(?:[^"\\]|\\.)*"\s*)+)', text):
            found.add("".join(re.findall(r'"((?:[^"\\]|\\.)*)"', m.group(1))))
    return found


# ---- the tests ---------------------------------------------------------------------------------------------------------------
def test_every_format_is_listed():
    """FORMATS and NEEDS_A_RUNTIME together are the set_error format strings of the family files and the shared file, no more, no less."""
    assert len(set(FORMATS)) == len(FORMATS) and not set(FORMATS) & set(NEEDS_A_RUNTIME)
    assert _source_formats() == set(FORMATS) | set(NEEDS_A_RUNTIME)


def test_every_format_has_a_row():
    assert len({name for name, _, _ in ROWS}) == len(ROWS)
    assert set(FORMATS) - {fmt for _, fmt, _ in ROWS} == set()
    assert {fmt for _, fmt, _ in ROWS} - {None} <= set(FORMATS)


def test_the_golden_file_holds_the_table():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(name for name, _, _ in ROWS)
    for name, fmt, _ in ROWS:
        status, text = golden[name]
        if fmt is None:  # no text of the family's own: a success, a bare refusal, or a text from elsewhere (sar_config_validate's)
            assert text == SENTINEL or name.startswith("gallery.base_invalid"), name
        else:
            assert status != A.SAR_OK and _format_regex(fmt).match(text), (name, fmt, text)


@pytest.mark.parametrize("name,call", [(name, call) for name, _, call in ROWS], ids=[name for name, _, _ in ROWS])
def test_refusal(sar, name, call):
    assert _run(sar.load_library(), call) == json.load(open(GOLDEN))[name]


def test_c_program_of_the_host_companions(sar, tmp_path):
    """tests/c/sar_analysis_host.c: the fits over windows of 0, 2 and 3 usable bins, the edges, and one sweep through sar_plane_coeffs
    and sar_period_coeffs, from C99 against the product library."""
    pkg = os.path.dirname(A.LIB_PATH)
    exe = str(tmp_path / "sar_analysis_host")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "sar_analysis_host.c"), "-o", exe, "-L", pkg, "-l:libsar_hip.so", "-lm",
                    f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    recorded = {name: _run(A.load_library(sys.argv[2]), call) for name, _, call in ROWS}
    with open(GOLDEN, "w") as f:
        json.dump(recorded, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(recorded)} rows recorded from {sys.argv[2]}")
