"""GPU: the orbit diagrams (sar_runtime_orbit, include/sar.h) — count, max and every column statistic against the numpy restatement
bit for bit on the logistic line (with closed-form columns checked independently of it), on a line with late deaths and on the 3-D
line between the two presets; independence of the launch shape; the limits and every refusal; no side effect on the runtime's
buffers; and the way up: colorize through Runtime.load + auto exposure, and lambda_1 per column."""
import ctypes as C
import math

import numpy as np
import pytest

import orbit_restatement as O
from orbit_cases import REFUSED, logistic as _logistic, refused_params

pytestmark = pytest.mark.gpu

HEIGHT, JOBS = 64, 70          # 70 jobs: a partial second wave
LINE = dict(width=5, height=HEIGHT, jobs=JOBS, transient=1000, steps=400, v_range=(0.0, 1.0))


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    yield r
    r.close()


def _restate(sar, a, b, seed=0, proj=(1.0, 0.0, 0.0), **kw):
    return O.diagram(a, b, kw["width"], kw["height"], sar.start_points(seed, 0, kw["jobs"]), kw["transient"], kw["steps"], kw["v_range"], proj)


def _same(d, want):
    assert d.count.dtype == np.uint32 and d.count.shape == want["count"].shape
    assert np.array_equal(d.count, want["count"])
    assert d.max == want["max"]
    for f in O.COLUMN_FIELDS:
        if f in ("vmin", "vmax"):                   # by value: -0.0 == 0.0
            assert np.array_equal(d.stats[f], want["stats"][f]), f
        else:
            assert np.array_equal(d.stats[f].astype(np.int64), want["stats"][f].astype(np.int64)), f
    assert not d.stats["_pad"].any()


@pytest.fixture(scope="module")
def line_reference(sar):
    """The restatement of test 1's diagram, computed once and left unchanged."""
    return _restate(sar, *_logistic(), **LINE)


@pytest.fixture(scope="module")
def line_diagram(sar, rt):
    return sar.orbit_diagram(rt, *_logistic(), **LINE)


def test_logistic_line_equals_the_restatement_and_the_closed_forms(sar, line_diagram, line_reference):
    d = line_diagram
    _same(d, line_reference)
    assert d.v_range == (0.0, 1.0)
    s, jobs, steps = d.stats, JOBS, LINE["steps"]
    # independently of the restatement: r = 2.8 sits on its fixed point, r = 3.2 on its 2-cycle, r = 3.6 is chaotic, r = 4.4 escapes
    r = np.array([d.coeffs(c)[0, 1] for c in range(5)])
    assert np.allclose(r, [2.8, 3.2, 3.6, 4.0, 4.4], rtol=0, atol=1e-15)
    assert np.array_equal(np.nonzero(d.count[:, 0])[0], [HEIGHT - 1 - int(HEIGHT * (1 - 1 / r[0]))])
    assert d.count[:, 0].sum() == jobs * steps == s["hits"][0] and s["occupied"][0] == 1
    root = math.sqrt((r[1] - 3) * (r[1] + 1))
    rows = sorted(HEIGHT - 1 - int(HEIGHT * (r[1] + 1 + sgn * root) / (2 * r[1])) for sgn in (1, -1))
    assert np.array_equal(np.nonzero(d.count[:, 1])[0], rows) and np.all(d.count[rows, 1] == jobs * steps // 2)
    assert s["occupied"][2] > 8
    assert s["dead_transient"][4] == jobs and not d.count[:, 4].any()
    assert s["vmin"][4] == math.inf and s["vmax"][4] == -math.inf
    assert np.array_equal(s["dead_transient"] + s["dead_late"] + s["alive"], [jobs] * 5)


def test_late_deaths(sar, rt):
    a, b = _logistic()
    kw = dict(LINE, transient=8)
    want = _restate(sar, a, b, **kw)
    late = want["stats"]["dead_late"]
    assert np.any((late > 0) & (late < JOBS)), late       # a column that loses some of its jobs after the transient, not before
    d = sar.orbit_diagram(rt, a, b, **kw)
    _same(d, want)
    assert np.array_equal(d.stats["hits"], d.count.sum(0, dtype=np.uint64))
    dying = int(np.argmax(late))
    assert d.stats["misses"][dying] > 0 and d.stats["alive"][dying] < JOBS


def test_a_line_between_the_presets_in_3d(sar, rt):
    pa, ss = sar.Config.poisson_saturne(), sar.Config.solar_sail()
    kw = dict(width=9, height=128, jobs=64, transient=200, steps=300)
    proj = (0.6, -0.3, 0.7)
    probe = _restate(sar, pa_coeffs(pa), pa_coeffs(ss), proj=proj, v_range=(-1.0, 1.0), **kw)["stats"]
    seen = probe["hits"] + probe["misses"] > 0
    v_range = (float(probe["vmin"][seen].min()), float(probe["vmax"][seen].max()))
    want = _restate(sar, pa_coeffs(pa), pa_coeffs(ss), proj=proj, v_range=v_range, **kw)
    s = want["stats"]
    assert np.any((s["misses"] > 0) | (s["dead_transient"] + s["dead_late"] > 0)) and np.count_nonzero(s["hits"]) >= 3
    d = sar.orbit_diagram(rt, pa, ss, proj=proj, v_range=v_range, **kw)
    _same(d, want)
    assert np.array_equal(d.coeffs(0), np.stack([pa.coeff_x, pa.coeff_y, pa.coeff_z]))


def pa_coeffs(cfg):
    return np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])


def test_results_do_not_depend_on_the_launch_shape(sar, rt, line_diagram, line_reference):
    a, b = _logistic()
    by_jobs = {1: [], 1024: []}                        # one lane of one wave; sixteen full waves
    try:
        for chunk, launches in ((1, 5), (2, 3), (0, 1)):
            rt.set_option("orbit_chunk", chunk)
            rt.enable_timing(True)
            d = sar.orbit_diagram(rt, a, b, **LINE)
            t = rt.last_timing()
            rt.enable_timing(False)
            assert t.iterate_launches == launches and t.iterate_ms > 0, chunk      # k_orbit's spans
            assert np.array_equal(d.count, line_diagram.count) and d.max == line_diagram.max, chunk
            assert d.stats.tobytes() == line_diagram.stats.tobytes(), chunk
            for jobs in by_jobs:
                by_jobs[jobs].append(sar.orbit_diagram(rt, a, b, **dict(LINE, jobs=jobs, steps=64)))
    finally:
        rt.set_option("orbit_chunk", 0)
        rt.enable_timing(False)
    for jobs, ds in by_jobs.items():
        _same(ds[0], _restate(sar, a, b, **dict(LINE, jobs=jobs, steps=64)))
        for d in ds[1:]:
            assert np.array_equal(d.count, ds[0].count) and d.stats.tobytes() == ds[0].stats.tobytes() and d.max == ds[0].max, jobs
    with pytest.raises(sar.SarError):
        rt.set_option("orbit_chunk", 65537)


def test_explicit_starts_and_the_seed(sar, rt):
    a, b = _logistic()
    kw = dict(LINE, jobs=33, steps=50)
    starts = sar.start_points(5, 0, 33)
    by_seed = sar.orbit_diagram(rt, a, b, seed=5, **kw)
    given = sar.orbit_diagram(rt, a, b, starts=starts, **kw)
    assert np.array_equal(by_seed.count, given.count) and by_seed.stats.tobytes() == given.stats.tobytes()
    _same(given, O.diagram(a, b, 5, HEIGHT, starts, 1000, 50, (0.0, 1.0)))
    assert not np.array_equal(by_seed.count, sar.orbit_diagram(rt, a, b, seed=6, **kw).count)
    with pytest.raises(ValueError):
        sar.orbit_diagram(rt, a, b, starts=starts[:-1], **kw)


def test_the_tallest_column(sar, rt):
    a, _ = _logistic(3.6, 3.6)
    kw = dict(width=1, height=32768, jobs=64, transient=100, steps=200, v_range=(0.0, 1.0))
    d = sar.orbit_diagram(rt, a, a, **kw)
    assert d.count.shape == (32768, 1)
    assert d.count.sum(dtype=np.uint64) == d.stats["hits"][0] == 64 * 200 and d.stats["misses"][0] == 0
    _same(d, _restate(sar, a, a, **kw))


@pytest.mark.parametrize("change,text", REFUSED)
def test_refusals_with_a_runtime(sar, rt, change, text):
    p = refused_params(sar, change)
    count = np.zeros(8, dtype=np.uint32)                 # (refused before anything is written)
    lib = sar.load_library()
    assert lib.sar_runtime_orbit(rt.handle, C.byref(p), None, count.ctypes.data_as(C.POINTER(C.c_uint32)), None, None) == 1
    assert text in lib.sar_last_error().decode()
    assert not count.any()


def test_the_runtime_is_only_lent(sar, rt):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    sar.orbit_diagram(rt, *_logistic(), **LINE)
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    lib = sar.load_library()
    p = refused_params(sar, {})
    assert lib.sar_runtime_orbit(rt.handle, C.byref(p), None, None, None, None) == 1     # no count buffer
    rt.reset()


def test_auto_range_costs_a_second_run_and_frames_every_visit(sar, rt, line_reference):
    a, b = _logistic()
    kw = {k: v for k, v in LINE.items() if k != "v_range"}
    d = sar.orbit_diagram(rt, a, b, **kw)
    s = line_reference["stats"]
    seen = s["hits"] + s["misses"] > 0
    lo, hi = s["vmin"][seen].min(), s["vmax"][seen].max()
    assert d.v_range == (lo - 0.02 * (hi - lo), hi + 0.02 * (hi - lo))
    assert not d.stats["misses"].any() and np.array_equal(d.stats["hits"], s["hits"])
    _same(d, _restate(sar, a, b, **dict(kw, v_range=d.v_range)))


def test_colorize_is_load_auto_exposure_colorize(sar, gpu, line_diagram):
    d = line_diagram
    cfg = sar.Config.solar_sail()
    hue = np.linspace(0.0, 0.9, 5)
    for h, expo in ((None, {}), (hue, dict(q_white=0.9))):
        img = d.colorize(cfg, hue=h, exposure=expo)
        sized = cfg.replace(width=5, height=HEIGHT, render_kind=sar.SAR_RENDER_GAS)
        other = sar.Runtime(sized, device=0)
        steps = np.zeros((HEIGHT, 5)) if h is None else np.repeat(hue[None, :], HEIGHT, axis=0)
        other.load(d.count, steps, np.zeros((HEIGHT, 5), dtype=np.float32), d.max)
        want = sar.colorize(sar.auto_exposure(sized, other, **expo), other)
        loaded = sar.Runtime(sized, device=0)
        d.load(loaded, h)
        assert np.array_equal(loaded.count(), d.count) and loaded.max() == d.max and np.array_equal(loaded.steps(), steps)
        other.close()
        loaded.close()
        assert img.shape == (HEIGHT, 5, 4) and img.dtype == np.uint16 and np.array_equal(img, want)
        assert img[..., :3].any()
    with pytest.raises(ValueError):
        wrong = sar.Runtime(cfg.replace(width=6, height=HEIGHT), device=0)
        try:
            d.load(wrong)
        finally:
            wrong.close()


def test_lyapunov_per_column(sar, rt, line_diagram):
    lam = line_diagram.lyapunov(rt, steps=4000)
    assert lam.shape == (5,)
    assert lam[0] < 0 and lam[1] < 0 and lam[2] > 0 and math.isnan(lam[4])
    assert abs(lam[0] - math.log(0.8)) < 1e-9          # the fixed point's multiplier is 2 - r
    # a generic 3-D line goes through the search alone: lambda_1 of the first column is the preset's
    pa = sar.Config.poisson_saturne()
    d = sar.orbit_diagram(rt, pa, sar.Config.solar_sail(), width=3, height=8, jobs=4, transient=10, steps=10, v_range=(-2.0, 2.0))
    lam3 = d.lyapunov(rt, steps=2000)
    recs, _ = sar.search_attractors(rt, 1, coeffs=pa_coeffs(pa)[None, :], steps=2000, keep_rejected=1)
    assert recs.size == 1 and lam3[0] == recs["lyapunov"][0, 0] and lam3[0] > 0
