"""CPU: Poincare sections of flows without a device (include/sar.h: sar_section_*, sar_runtime_section) — the prototypes, the
defaults, the layouts and every refusal that needs no device; sar_section_step against the numpy restatement bit for bit on every
kind of step; and the restatement itself held to facts that do not come from this code: the harmonic oscillator's period and radius,
Roessler's period doubling, Lorenz's cusp map of successive maxima of z, a surface the trajectory never leaves, a grazing plane, and
the identity between the three directions."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import flow_restatement as R
import section_restatement as P
from test_abi_and_host import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OSCILLATOR = np.zeros((3, 10))
OSCILLATOR[0, 5], OSCILLATOR[1, 1] = 1.0, -1.0                # x' = y, y' = -x
Y_PLANE = P.plane((0.0, 1.0, 0.0))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _config(sar, rows):
    return sar.Config.from_coefficients(rows).replace(width=64, height=48)


# ---- (a) prototypes, defaults, layouts, refusals ----------------------------------------------------------------------------------
def test_the_entries_and_their_mirrors(sar):
    from strange_attractor_renderer_amd import _abi
    names = [n for n in declared_functions() if "section" in n and "volume" not in n]
    assert names == ["sar_runtime_section", "sar_section_params_default", "sar_section_step"]
    lib = sar.load_library()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    for n in names:
        assert n in _abi.PROTOTYPES and hasattr(lib, n) and re.search(rf"pub fn {n}\s*\(", rs) and f"{n}(" in hpp, n
    for struct, mirror in (("SarSectionParams", _abi.SarSectionParams), ("SarSectionRecord", _abi.SarSectionRecord),
                           ("SarSectionStats", _abi.SarSectionStats)):
        body = rs[rs.index(f"pub struct {struct} {{"):]
        assert re.findall(r"pub (\w+):", body[:body.index("}")]) == [f for f, _ in mirror._fields_]
    header = open(os.path.join(ROOT, "include", "sar.h")).read()
    for word in ("g = g + t[k] * s[k + 1]", "side(p) = (g(p) >= 0)", "w = 1.0 / gdot", "gdot = (gx * Px + gy * Py) + gz * Pz",
                 "theta = g0 / (g0 - g1)", "r = ((double)(t - t_prev) * h + dt) - dt_prev", "(sortable(zf + 0.0f) << 32) | sortable((float)r)",
                 "a second\n * refinement step"):
        assert word in header, word
    for fn in ("section_params", "section_plane", "section_extremum", "section_step", "flow_section"):
        assert callable(getattr(sar, fn))
    assert (sar.SAR_SECTION_FULL, sar.SAR_SECTION_SHORT, sar.SAR_SECTION_ESCAPED, sar.SAR_SECTION_ESCAPED_TRANSIENT) == (
        P.FULL, P.SHORT, P.ESCAPED, P.ESCAPED_TRANSIENT) and sar.SAR_SECTION_NO_CLOCK == P.NONE
    for name in ("FULL", "SHORT", "ESCAPED", "ESCAPED_TRANSIENT"):
        assert re.search(rf"#define SAR_SECTION_{name}\s+{getattr(P, name)}\b", header)


def test_defaults_and_layouts(sar):
    from strange_attractor_renderer_amd import _abi
    p = sar.section_params()
    assert list(p.surface) == [0.0] * 10
    assert {f: getattr(p, f) for f in P.DEFAULTS} == P.DEFAULTS
    assert (p.dt, p.bound, p.transient, p.direction, p.samples, p.max_steps, p.plot) == (0.01, 1e6, 1000, 1, 1024, 1 << 20, 0)
    structs = (("sar_section_params", _abi.SarSectionParams), ("sar_section_record", _abi.SarSectionRecord),
               ("sar_section_stats", _abi.SarSectionStats))
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    want = []
    for cname, mirror in structs:
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        want.append(C.sizeof(mirror))
        for f, _ in mirror._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
            want.append(getattr(mirror, f).offset)
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out == want and [C.sizeof(m) for _, m in structs] == [128, 24, 160]
    assert sar.SECTION_RECORD_DTYPE.itemsize == 24 and P.RECORD_DTYPE.itemsize == 24
    assert not [o for o in _abi.STABLE_OPTIONS if "section" in o]     # the launch bounds are fields of the parameters


def test_surfaces(sar):
    assert np.array_equal(sar.section_plane((1.0, 2.0, 3.0), 4.0), [-4.0, 1.0, 0, 0, 0, 2.0, 0, 0, 3.0, 0])
    assert np.array_equal(sar.section_plane((0.0, 0.0, 2.0), point=(5.0, 6.0, 7.0)), [-14.0, 0, 0, 0, 0, 0, 0, 0, 2.0, 0])
    assert np.array_equal(sar.section_plane((0.0, 1.0, 0.0)), Y_PLANE) and np.array_equal(P.plane((0.0, 0.0, 1.0), 27.0), sar.section_plane((0, 0, 1), 27.0))
    lorenz = sar.flow_coefficients("lorenz")
    assert np.array_equal(sar.section_extremum(lorenz, 2), lorenz[2]) and np.array_equal(sar.section_extremum(_config(sar, lorenz), 1), lorenz[1])
    with pytest.raises(ValueError):
        sar.section_extremum(lorenz, 3)


def test_refusals_that_need_no_device(sar):
    from strange_attractor_renderer_amd import _abi
    lib = sar.load_library()
    cfg = _config(sar, sar.flow_coefficients("lorenz"))
    jobs, samples = 4, 8
    starts = np.full((jobs, 3), 0.1)
    points, ret = np.zeros((jobs, samples, 3)), np.zeros((jobs, samples))
    records, st = np.zeros(jobs, dtype=sar.SECTION_RECORD_DTYPE), _abi.SarSectionStats()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))  # noqa: E731
    plane = P.plane((0.0, 0.0, 1.0), 27.0)

    def call(cfg_=cfg, jobs_=jobs, s=starts, pts=points, rets=ret, recs=records, stats=st, params=True, **fields):
        p = sar.section_params(**{"surface": plane, "samples": samples, **fields})
        status = lib.sar_runtime_section(C.byref(cfg_.c) if cfg_ is not None else None, None, C.byref(p) if params else None, jobs_,
                                         dp(s) if s is not None else None, dp(pts) if pts is not None else None,
                                         dp(rets) if rets is not None else None,
                                         recs.ctypes.data_as(C.POINTER(_abi.SarSectionRecord)) if recs is not None else None,
                                         C.byref(stats) if stats is not None else None)
        return status, lib.sar_last_error().decode()

    def bad_surface(k, v):
        s = plane.copy()
        s[k] = v
        return s

    zero_but_s0 = np.zeros(10)
    zero_but_s0[0] = 3.0
    for fields, text in ((dict(surface=bad_surface(0, math.nan)), "surface[0] is not finite"), (dict(surface=bad_surface(8, math.inf)), "surface[8] is not finite"),
                         (dict(surface=bad_surface(3, -math.inf)), "surface[3] is not finite"), (dict(surface=np.zeros(10)), "all zero"),
                         (dict(surface=zero_but_s0), "all zero"),
                         (dict(dt=0.0), "dt must be finite and positive"), (dict(dt=-0.01), "dt must be finite and positive"),
                         (dict(dt=math.nan), "dt must be finite and positive"), (dict(dt=math.inf), "dt must be finite and positive"),
                         (dict(bound=0.0), "bound must be finite and positive"), (dict(bound=-1.0), "bound must be finite and positive"),
                         (dict(bound=math.inf), "bound must be finite and positive"), (dict(bound=math.nan), "bound must be finite and positive"),
                         (dict(direction=2), "direction must be +1, -1 or 0"), (dict(direction=-2), "direction must be +1, -1 or 0"),
                         (dict(plot=2), "plot must be 0 or 1"), (dict(plot=-1), "plot must be 0 or 1"),
                         (dict(samples=0), "samples must be 1 to 2^20"), (dict(samples=(1 << 20) + 1), "samples must be 1 to 2^20"),
                         (dict(max_steps=0), "max_steps must be at least 1"),
                         (dict(chunk_jobs=(1 << 24) + 1), "at most 2^24"), (dict(chunk_steps=(1 << 24) + 1), "at most 2^24")):
        status, msg = call(**fields)
        assert status == _abi.SAR_ERR_INVALID and text in msg, (fields, status, msg)
    assert call(cfg_=None)[0] == _abi.SAR_ERR_INVALID
    assert call(cfg_=cfg.replace(width=0))[0] == _abi.SAR_ERR_INVALID
    status, msg = call(jobs_=0)
    assert status == _abi.SAR_ERR_INVALID and "n_jobs must be at least 1" in msg
    status, msg = call(jobs_=17, samples=1 << 20)                            # 17 * 2^20 > 2^24: refused before any pointer is read
    assert status == _abi.SAR_ERR_INVALID and "n_jobs * samples must be at most 2^24" in msg
    big = np.full((16, 3), 0.1)
    status, msg = call(jobs_=16, s=big, samples=1 << 20, max_steps=(1 << 32) - 1)   # exactly 2^24, the largest max_steps: on to the runtime
    assert status == _abi.SAR_ERR_INVALID and "NULL" in msg
    for bad in (math.nan, math.inf, -math.inf):
        s2 = starts.copy()
        s2[2, 1] = bad
        status, msg = call(s=s2)
        assert status == _abi.SAR_ERR_INVALID and "start point 2 is not finite" in msg
    for kw in (dict(), dict(s=None), dict(pts=None), dict(rets=None), dict(recs=None), dict(stats=None), dict(params=False)):
        status, msg = call(**kw)                                              # everything right but the runtime / one pointer
        assert status == _abi.SAR_ERR_INVALID and "NULL" in msg, kw
    assert lib.sar_section_params_default(None) == _abi.SAR_ERR_INVALID
    xyz = np.zeros(3)
    good = sar.section_params(surface=plane)
    assert lib.sar_section_step(None, C.byref(good), dp(xyz), None, None, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_section_step(C.byref(cfg.c), None, dp(xyz), None, None, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_section_step(C.byref(cfg.c), C.byref(good), None, None, None, None) == _abi.SAR_ERR_INVALID
    for fields in (dict(dt=0.0), dict(bound=math.nan), dict(direction=3), dict(surface=np.zeros(10)), dict(surface=bad_surface(2, math.nan))):
        p = sar.section_params(**{"surface": plane, **fields})
        assert lib.sar_section_step(C.byref(cfg.c), C.byref(p), dp(xyz), None, None, None) == _abi.SAR_ERR_INVALID, fields
    assert lib.sar_section_step(C.byref(cfg.c), C.byref(good), dp(xyz), None, None, None) == _abi.SAR_OK and xyz[0] == 0.0   # Lorenz's origin
    with pytest.raises(AttributeError):
        sar.section_params(tolerance=1e-6)
    with pytest.raises(ValueError):
        sar.section_params(samples=-1)
    with pytest.raises(ValueError):
        sar.flow_section(cfg, None, plane, jobs=4, starts=np.zeros((3, 3)))


# ---- (b) sar_section_step is the restatement's step -------------------------------------------------------------------------------
def _same_step(sar, cfg, view, surface, p, **kw):
    got_p, got_kind, got_q, got_dt = sar.section_step(cfg, surface, p, **kw)
    want_p, want_kind, want_q, want_dt = P.section_step(view, surface, p, **kw)
    assert got_kind == want_kind and np.array_equal(_bits(got_p), _bits(want_p)), (p, got_kind, want_kind)
    if want_kind > 0:
        assert np.array_equal(_bits(got_q), _bits(want_q)) and _bits(got_dt)[0] == _bits(want_dt)[0], (p, got_q, want_q, got_dt, want_dt)
    else:
        assert got_q is None and got_dt is None
    return want_kind


@pytest.mark.parametrize("name", ("lorenz", "rossler", "sprott_m"))
def test_section_step_equals_the_restatement(sar, name):
    cfg = _config(sar, sar.flow_coefficients(name))
    view = R.view_of(cfg.c)
    rng = np.random.default_rng(31 + len(name))
    quadric = rng.uniform(-1.0, 1.0, size=10)                                # all ten coefficients non-zero
    p, pts = np.array([0.1, 0.1, 0.1]), []
    for t in range(1300):                                                    # 40 time units of a trajectory behind a transient:
        p = sar.flow_step(cfg, p, dt=0.05)                                   # it crosses each surface many times, both ways
        if t >= 500:
            pts.append(p)
    x_mid = float(np.median([q[0] for q in pts]))
    for surface in (P.plane((1.0, 0.0, 0.0), x_mid), np.array(cfg.coeff_x, dtype=np.float64), quadric):
        for direction in (1, -1, 0):
            kinds = [_same_step(sar, cfg, view, surface, q, dt=0.05, bound=1e6, direction=direction) for q in pts]
            assert kinds.count(1) + kinds.count(2) >= (2 if direction == 0 else 1) and kinds.count(0) >= 3, (name, direction, kinds.count(0))
    assert _same_step(sar, cfg, view, quadric, (9e5, 9e5, 9e5), dt=0.01, bound=1e6) == -1      # escaped
    assert _same_step(sar, cfg, view, quadric, (30.0, 1.0, 2.0), dt=0.01, bound=10.0) == -1


def test_section_step_on_the_surface_itself_and_on_a_nan(sar):
    cfg = _config(sar, sar.flow_coefficients("lorenz"))
    view = R.view_of(cfg.c)
    plane = P.plane((0.0, 0.0, 1.0), 27.0)
    rising, falling = (10.0, 10.0, 27.0), (1.0, 1.0, 27.0)                   # z' = x y - 8/3 z = 28 and -71 on the plane
    assert P.g(plane, *(np.float64(v) for v in rising)) == 0.0
    assert _same_step(sar, cfg, view, plane, rising, direction=1) == 0       # side(p0) is true: no up-crossing
    assert _same_step(sar, cfg, view, plane, rising, direction=-1) == 0
    assert _same_step(sar, cfg, view, plane, falling, direction=1) == 0
    assert _same_step(sar, cfg, view, plane, falling, direction=-1) == 1     # a down-crossing with D = -g0 = 0: q is p0, dt is 0
    _, _, q, dt = sar.section_step(cfg, plane, falling, direction=-1)
    assert np.array_equal(q, falling) and dt == 0.0
    nan_surface = np.zeros(10)
    nan_surface[2], nan_surface[6] = 1e308, -1e308                           # inf - inf
    with np.errstate(all="ignore"):
        assert np.isnan(P.g(nan_surface, np.float64(10.0), np.float64(10.0), np.float64(27.0)))
    for direction in (1, -1, 0):
        assert _same_step(sar, cfg, view, nan_surface, (10.0, 10.0, 27.0), direction=direction) == 0


def test_section_step_rough(sar):
    """The grazing plane of the oscillator: the steps along its trajectory, each through both; some are rough."""
    cfg = _config(sar, OSCILLATOR)
    view = R.view_of(cfg.c)
    surface = P.plane((0.0, 1.0, 0.0), math.cos(0.005))
    p, kinds = np.array([1.0, 0.0, 0.0]), []
    for _ in range(4000):
        kinds.append(_same_step(sar, cfg, view, surface, p, dt=0.01, direction=0))
        p = sar.section_step(cfg, surface, p, dt=0.01, direction=0)[0]
    assert kinds.count(2) >= 1 and kinds.count(1) >= 1 and kinds.count(-1) == 0


# ---- (c) the restatement against facts from elsewhere -----------------------------------------------------------------------------
@pytest.mark.parametrize("h", (0.01, 0.02))
def test_harmonic_oscillator_period_and_radius(h):
    """x' = y, y' = -x from (1, 0, 0): the section y = 0, downwards, is met once per turn at x = r0 = 1. RK4's leading phase error
    makes the period 2 pi (1 + h^4 / 120) (measured 1.0007 of that excess at both h); its amplitude error over 40 time units is
    2.6e-11 and 8.4e-10. Linear interpolation alone would miss the radius by h^2 / 8, about 1e-5."""
    points, ret, records, stats = P.run(OSCILLATOR, Y_PLANE, [[1.0, 0.0, 0.0]], dt=h, transient=0, direction=-1, samples=64,
                                        max_steps=int(round(40.0 / h)))
    k = int(records["found"][0])
    assert k == 6 and records["status"][0] == P.SHORT and records["clock_step"][0] == 0 and stats["rough"] == 0
    assert np.abs(ret[0, :k] - 2.0 * math.pi).max() <= 1.5 * 2.0 * math.pi * h ** 4 / 120.0
    assert (np.abs(np.abs(points[0, :k, 0]) - 1.0) / 1.0).max() <= 1e-9
    assert np.isnan(ret[0, k:]).all() and np.isnan(points[0, k:]).all()
    assert stats["ret_min"] == ret[0, :k].min() and stats["ret_max"] == ret[0, :k].max() and stats["crossings"] == k


def test_rossler_period_doubling(sar):
    """a = b = 0.2 on the half-plane y = 0, upwards: period 1, 2 and 4 at c = 2.5, 3.5 and 4.0 (one pass: a field per job)."""
    fields = np.stack([sar.flow_coefficients("rossler", a=0.2, b=0.2, c=c) for c in (2.5, 3.5, 4.0)], axis=2)
    points, ret, records, stats = P.run(fields, Y_PLANE, [[1.0, 1.0, 1.0]] * 3, dt=0.01, transient=30000, direction=1, samples=64, max_steps=8000)
    assert stats["rough"] == 0 and (records["found"] >= 12).all()
    xs = [np.unique(np.round(points[j, :records["found"][j], 0], 5)) for j in range(3)]
    rs = [np.unique(np.round(ret[j, :records["found"][j]], 6)) for j in range(3)]
    assert [len(x) for x in xs] == [1, 2, 4] and [len(r) for r in rs] == [1, 2, 4]
    assert list(rs[0]) == [5.748991] and list(rs[1]) == [5.363839, 6.181379]
    assert (points[:, :12, 0] > 0.0).all()                                   # y' = x + a y > 0 on y = 0: the half-plane x > 0


@pytest.fixture(scope="module")
def lorenz_maxima(sar):
    lorenz = sar.flow_coefficients("lorenz")
    starts = sar.start_points(0, 0, 32)
    return {h: P.run(lorenz, sar.section_extremum(lorenz, 2), starts, dt=h, transient=1000, direction=-1, samples=256, max_steps=8000)
            for h in (0.01, 0.005)}


def test_lorenz_cusp_map_of_successive_maxima(lorenz_maxima):
    points, ret, records, stats = lorenz_maxima[0.01]
    assert stats["rough"] == 0 and stats["full"] == 0 and stats["short_jobs"] == 32 and stats["clocked"] == 32
    found = records["found"]
    z = np.concatenate([points[j, :found[j], 2] for j in range(32)])
    assert len(z) >= 3000 and 29.0 <= z.min() and z.max() <= 48.5, (z.min(), z.max())
    zk = np.concatenate([points[j, :found[j] - 1, 2] for j in range(32)])
    zn = np.concatenate([points[j, 1:found[j], 2] for j in range(32)])
    assert 38.0 <= zk[np.argmax(zn)] <= 39.2, zk[np.argmax(zn)]
    order = np.argsort(zk)
    zs, rise = zk[order], np.diff(zn[order]) >= 0.0
    right, left = zs[:-1] > 39.2, zs[1:] < 38.0
    assert right.sum() >= 500 and left.sum() >= 500
    assert rise[right].sum() <= 0.01 * right.sum(), (rise[right].sum(), right.sum())          # falling to the right of the cusp
    assert (~rise[left]).sum() <= 0.10 * left.sum(), ((~rise[left]).sum(), left.sum())        # rising to its left: a thin fractal, no curve
    # every maximum is one: z' changes sign from + to -, so z'' < 0 there and the neighbours on the trajectory lie lower
    assert stats["extent"][4] == z.min() and stats["extent"][5] == z.max()


def test_lorenz_residual_falls_with_the_step(lorenz_maxima):
    """The surface z' = 0 is a quadric: one Henon step leaves O(D^5)."""
    coarse, fine = lorenz_maxima[0.01][3], lorenz_maxima[0.005][3]
    assert fine["rough"] == 0 and 0.0 < fine["residual_max"] and coarse["residual_max"] > 8.0 * fine["residual_max"], (coarse["residual_max"], fine["residual_max"])


def test_a_surface_the_trajectory_never_leaves(sar):
    """The origin of Lorenz is a fixed point on the plane z = 0: g is 0 throughout, side stays true."""
    points, ret, records, stats = P.run(sar.flow_coefficients("lorenz"), P.plane((0.0, 0.0, 1.0)), np.zeros((3, 3)), transient=10, direction=0,
                                        samples=4, max_steps=200)
    assert (records["status"] == P.SHORT).all() and (records["clock_step"] == P.NONE).all() and (records["found"] == 0).all()
    assert (records["steps"] == 200).all() and stats["clocked"] == 0 and stats["crossings"] == 0 and stats["short_jobs"] == 3
    assert np.isnan(points).all() and np.isnan(ret).all() and stats["residual_max"] == 0.0
    assert np.array_equal(stats["extent"], [np.inf, -np.inf] * 3) and stats["ret_min"] == np.inf and stats["ret_max"] == -np.inf


def test_a_grazing_plane_gives_rough_crossings():
    """The oscillator's circle of radius 1 and the plane y = cos 0.005 = 1 - 1.25e-5: the trajectory dips through it for 0.01 time
    units per turn, one step long. Near the tangency gdot is almost 0 and Henon's step overshoots: those crossings are rough."""
    _, _, records, stats = P.run(OSCILLATOR, P.plane((0.0, 1.0, 0.0), math.cos(0.005)), [[1.0, 0.0, 0.0]], dt=0.01, transient=0, direction=0,
                                 samples=64, max_steps=4000)
    assert records["rough"][0] >= 1 and records["found"][0] - records["rough"][0] >= 1, records
    assert stats["rough"] == records["rough"][0]


def test_both_directions_are_the_sum_of_each(sar):
    starts = sar.start_points(0, 0, 8)
    total = {}
    for direction in (0, 1, -1):
        _, _, records, stats = P.run(sar.flow_coefficients("lorenz"), P.plane((0.0, 0.0, 1.0), 27.0), starts, dt=0.01, transient=1000,
                                     direction=direction, samples=256, max_steps=3000)
        assert stats["full"] == 0 and stats["clocked"] == 8                   # samples never filled
        total[direction] = stats["crossings"] + stats["clocked"]
    assert total[0] == total[1] + total[-1] and total[1] >= 200 and total[-1] >= 200, total
