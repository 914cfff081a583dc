"""GPU: the recurrence analysis (sar_runtime_recurrence, sar_runtime_recurrence_plot, sar_runtime_rqa, include/sar.h) — every count
against the numpy restatement bit for bit: random sets at every trajectory length where the kernels take another path, with
several jobs and sets, Theiler windows and bin counts; the planted sets and closed forms; the pairs family on the device at a bin
edge; six maps in one call with their records and points; independence of the chunk with the launch counts it implies; no side effect
on the runtime or on a held basin picture; one runtime through several lengths; the recurrence plot and its windows;
OrbitDiagram.recurrence; the refusals behind a runtime."""
import math

import numpy as np
import pytest

import basin_restatement as B
import rqa_cases as K
import rqa_restatement as R
import spectrum_cases as SK
from basin_cases import PITCHFORK_MU, PITCHFORK_WINDOW
from orbit_cases import logistic

pytestmark = pytest.mark.gpu

MAPS_SHAPE = dict(jobs=3, samples=300, transient=2000, theiler=1, line_bins=64)


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    yield r
    r.close()


def _same_counts(rec, want, what):
    assert {k: int(rec[k]) for k in R.COUNTS} == want, what


def _same_set(got, want, what):
    diag, vert, rec = got
    assert diag.dtype == np.uint64 and vert.dtype == np.uint64
    assert np.array_equal(diag, want[0]), (what, "diag", np.argwhere(diag != want[0])[:4].tolist())
    assert np.array_equal(vert, want[1]), (what, "vert", np.argwhere(vert != want[1])[:4].tolist())
    _same_counts(rec, want[2], what)


@pytest.mark.parametrize("t,jobs,sets,w,bins", K.SHAPES)
def test_sets_equal_the_restatement(sar, rt, t, jobs, sets, w, bins):
    pts = K.noisy_cycle(t, jobs, sets)
    diag, vert, recs = sar.recurrence_lines(rt, pts, eps2=K.EPS2, samples=t, theiler=w, line_bins=bins, records=True)
    assert diag.shape == vert.shape == (sets, bins + 1) and recs.shape == (sets,)
    for s in range(sets):
        _same_set((diag[s], vert[s], recs[s]), R.lines(pts[s], K.EPS2, t, w, bins), (t, s))
    one = sar.recurrence_lines(rt, pts[0], eps2=K.EPS2, samples=t, theiler=w, line_bins=bins)      # (n, 3): one set
    assert one[0].tobytes() == diag[0].tobytes() and one[1].tobytes() == vert[0].tobytes()


def test_a_set_as_one_trajectory_and_a_series(sar, rt):
    pts = K.noisy_cycle(100, 3, 1)[0]
    got = sar.recurrence_lines(rt, pts, eps2=K.EPS2, theiler=2, line_bins=16, records=True)      # samples left out: T = 300
    _same_set(got, R.lines(pts, K.EPS2, None, 2, 16), "one trajectory")
    by_eps = sar.recurrence_lines(rt, pts, 0.03, theiler=2, line_bins=16)
    assert by_eps[0].tobytes() == got[0].tobytes() and by_eps[1].tobytes() == got[1].tobytes()      # eps2 = eps * eps
    series = pts[:, 1]
    alone = np.zeros((300, 3))
    alone[:, 0] = series
    got = sar.recurrence_lines(rt, series, eps2=1e-4, line_bins=16, records=True)
    _same_set(got, R.lines(alone, 1e-4, None, 0, 16), "a series")
    assert got[2]["recurrences"] > 0


@pytest.mark.parametrize("t,w,bins", [(9, 0, 256), (9, 3, 4), (300, 0, 256), (300, 7, 2), (257, 255, 4), (600, 1, 256)])
def test_a_constant_set(sar, rt, t, w, bins):
    pts = np.full((t, 3), 0.375)
    _same_set(sar.recurrence_lines(rt, pts, eps2=1e-9, theiler=w, line_bins=bins, records=True), K.constant_lines(t, w, bins), (t, w))


@pytest.mark.parametrize("t,p,w,bins", [(30, 7, 0, 256), (300, 7, 6, 256), (515, 2, 0, 256), (515, 2, 1, 4), (701, 3, 1, 256)])
def test_tiled_points(sar, rt, t, p, w, bins):
    got = sar.recurrence_lines(rt, K.tiled_points(t, p), eps2=0.25, theiler=w, line_bins=bins, records=True)
    _same_set(got, K.tiled_lines(t, p, w, bins), (t, p, w))
    m = sar.rqa_measures(*got)
    rec = int(got[2]["recurrences"])
    assert m["det"] == (1.0 if t % p != 1 else (rec - 1) / rec)      # (the last line, at the largest multiple of p below T, may have length 1)
    assert m["lam"] == 0.0 and m["l_max"] == t - p and m["v_max"] == 1


@pytest.mark.parametrize("name", list(K.planted_sets()))
def test_planted_sets(sar, rt, name):
    pts, kw = K.planted_sets()[name]
    got = sar.recurrence_lines(rt, pts, records=True, **kw)
    _same_set(got, R.lines(pts, kw["eps2"], None, 0, kw["line_bins"]), name)
    plot = sar.recurrence_plot(rt, pts, eps2=kw["eps2"])
    assert np.array_equal(plot, R.matrix(pts, kw["eps2"])), name
    if name == "lattice, eps2 = 1":
        assert got[2]["recurrences"] == 1                             # the point met twice; distance exactly 1 is not below 1
    if name == "lattice, eps2 = 1 + ulp":
        assert got[2]["recurrences"] == 1 + 7 + 5                     # and the seven steps, and 0-5, 0-7, 1-6, 2-7, 4-7
    if name == "minus zero":
        assert got[2]["recurrences"] == 15
    if name == "infinities":
        assert got[2]["recurrences"] == 10 and not plot[1].any() and not plot[:, 3].any()      # the five all-zero points


@pytest.mark.parametrize("t,jobs,w,e", [(300, 1, 0, -10), (257, 1, 3, -8), (513, 1, 5, -12)])
def test_recurrences_are_the_pair_histograms_cumulative_count(sar, rt, t, jobs, w, e):
    pts = K.noisy_cycle(t, jobs, 1, seed=31)[0]
    _, _, rec = sar.recurrence_lines(rt, pts, eps2=2.0 ** e, samples=t, theiler=w, records=True)
    hist, cnt = sar.pair_histogram(rt, pts, samples=t, theiler=w, counts=True, sub_bits=0, e_min=-64, e_max=8)
    assert rec["recurrences"] > 0 and rec["recurrences"] == hist[:e + 64 + 1].sum()      # through the bin whose upper edge is 2^e
    assert rec["pairs"] == cnt["counted"]


@pytest.fixture(scope="module")
def maps_reference():
    """The restatement of the six maps at MAPS_SHAPE, computed once and left unchanged."""
    kw = {k: v for k, v in MAPS_SHAPE.items() if k != "jobs"}
    return [R.rqa(c, SK.unit_starts(MAPS_SHAPE["jobs"]), **kw) for c in SK.six_maps()]


@pytest.fixture(scope="module")
def maps_result(sar, rt):
    return sar.recurrence_analysis(rt, SK.six_maps(), starts=SK.unit_starts(MAPS_SHAPE["jobs"]), points=True, **MAPS_SHAPE)


def _same_record(rec, want, what):
    assert (int(rec["status"]), int(rec["fail_job"]), int(rec["fail_step"])) == (want["status"], want["fail_job"], want["fail_step"]), what
    assert np.array_equal(rec["extent"], want["extent"]), what      # by value: -0.0 == 0.0
    assert np.float64(rec["eps2"]).tobytes() == np.float64(want["eps2"]).tobytes(), (what, rec["eps2"], want["eps2"])
    _same_counts(rec["counts"], want["counts"], what)


def test_maps_equal_the_restatement(sar, rt, maps_result, maps_reference):
    res = maps_result
    assert res.diag.shape == res.vert.shape == (6, 65) and res.points.shape == (6, 900, 3)
    assert [w["status"] for w in maps_reference] == [R.BOUNDED] * 5 + [R.DIVERGED]
    for k, want in enumerate(maps_reference):
        assert np.array_equal(res.diag[k], want["diag"]) and np.array_equal(res.vert[k], want["vert"]), k
        _same_record(res.records[k], want, k)
        assert np.array_equal(res.points[k].view(np.uint64), want["points"].view(np.uint64)), k
    assert not res.diag[5].any() and not res.vert[5].any() and not res.points[5].any()      # DIVERGED: all zero
    assert res.records["eps2"][5] == 0.0 and res.records["fail_step"][5] > 0 and not any(res.records["counts"][5].tolist())
    assert np.array_equal(res.status, [0, 0, 0, 0, 0, sar.SAR_SEARCH_DIVERGED])
    # the returned points through sar_runtime_recurrence with the record's eps2: the same bytes
    for k in range(5):
        diag, vert, rec = sar.recurrence_lines(rt, res.points[k], eps2=float(res.records["eps2"][k]), samples=300, theiler=1, line_bins=64,
                                               records=True)
        assert diag.tobytes() == res.diag[k].tobytes() and vert.tobytes() == res.vert[k].tobytes(), k
        assert rec.tobytes() == res.records["counts"][k].tobytes(), k
    # what the measures say: the cycles are all lines, chaos is not; the shortcuts are measures(2, 2)
    m = res.measures()
    assert np.all(m["det"][[1, 2]] == 1.0) and m["det"][3] < 1.0 and m["l_max"][1] == 298 and math.isnan(m["rr"][5])
    assert np.array_equal(res.det[:5], m["det"][:5]) and np.array_equal(res.l_max, m["l_max"]) and np.array_equal(res.v_max, m["v_max"])
    for name in ("rr", "l_mean", "entr", "lam", "v_max"):
        assert getattr(res, name).shape == (6,)
    plot = res.plot(rt, 3, job=2)
    assert np.array_equal(plot, R.matrix(maps_reference[3]["points"][600:], maps_reference[3]["eps2"], 1))
    assert not res.plot(rt, 5).any() and res.plot(rt, 5).shape == (300, 300)


def test_a_fixed_point_and_an_explicit_threshold(sar, rt):
    fixed = np.zeros(30)                                              # x' = y' = z' = 0: every recorded point is the origin
    starts = SK.unit_starts(2)
    res = sar.recurrence_analysis(rt, np.stack([fixed, SK.henon()]), starts=starts, jobs=2, samples=65, transient=50, line_bins=8)
    want = [R.rqa(c, starts, 65, transient=50, line_bins=8) for c in (fixed, SK.henon())]
    assert want[0]["status"] == R.BOUNDED and want[0]["eps2"] == 0.0 and want[1]["eps2"] > 0.0
    for k in range(2):
        assert np.array_equal(res.diag[k], want[k]["diag"]) and np.array_equal(res.vert[k], want[k]["vert"]), k
        _same_record(res.records[k], want[k], k)
    assert not res.diag[0].any() and not res.vert[0].any() and not any(res.records["counts"][0].tolist()) and res.records["eps2"][0] == 0.0
    # an explicit eps2 overrides the fraction, for the fixed point too: all its pairs recur
    res = sar.recurrence_analysis(rt, np.stack([fixed, SK.henon()]), starts=starts, jobs=2, samples=65, transient=50, line_bins=8, eps2=0.01,
                                  eps_fraction=0.5)
    want = [R.rqa(c, starts, 65, transient=50, line_bins=8, eps2=0.01, eps_fraction=0.5) for c in (fixed, SK.henon())]
    for k in range(2):
        assert np.array_equal(res.diag[k], want[k]["diag"]) and np.array_equal(res.vert[k], want[k]["vert"]), k
        _same_record(res.records[k], want[k], k)
    assert np.all(res.records["eps2"] == 0.01) and res.records["counts"]["recurrences"][0] == res.records["counts"]["pairs"][0] == 2 * 64 * 65 // 2
    assert res.points is None


def test_results_do_not_depend_on_the_chunk(sar, rt, maps_result):
    pts = K.noisy_cycle(700, 3, 3)
    base = sar.recurrence_lines(rt, pts, eps2=K.EPS2, samples=700, theiler=1, line_bins=32, records=True)
    try:
        # 698 diagonals are 3 bands, 2 folded: 3 sets x 3 jobs x 2 = 18 workgroups; 300 samples, theiler 1: 298 diagonals, 2 bands,
        # 1 folded: 6 maps x 3 jobs = 18
        for chunk, launches in ((1, 18), (3, 6), (5, 4), (0, 1)):
            rt.enable_timing(True)
            got = sar.recurrence_lines(rt, pts, eps2=K.EPS2, samples=700, theiler=1, line_bins=32, chunk=chunk, records=True)
            t = rt.last_timing()
            assert t.iterate_launches == launches and t.iterate_ms > 0 and t.resolve_ms > 0, chunk
            assert all(g.tobytes() == b.tobytes() for g, b in zip(got, base)), chunk
            res = sar.recurrence_analysis(rt, SK.six_maps(), starts=SK.unit_starts(3), points=True, chunk=chunk, **MAPS_SHAPE)
            t = rt.last_timing()
            rt.enable_timing(False)
            assert t.iterate_launches == launches and t.warmup_ms > 0 and t.iterate_ms > 0 and t.resolve_ms > 0, chunk
            assert res.diag.tobytes() == maps_result.diag.tobytes() and res.vert.tobytes() == maps_result.vert.tobytes(), chunk
            assert res.records.tobytes() == maps_result.records.tobytes(), chunk
    finally:
        rt.enable_timing(False)
    one = sar.recurrence_analysis(rt, SK.six_maps()[3], starts=SK.unit_starts(3), **MAPS_SHAPE)      # one map per call
    assert one.diag[0].tobytes() == maps_result.diag[3].tobytes() and one.records[0].tobytes() == maps_result.records[3].tobytes()


def test_the_runtime_is_only_lent(sar, rt):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    basin = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), width=33, height=17, transient=300, steps=32, grid=8, **PITCHFORK_WINDOW)
    held = basin.colorize(cfg)
    sar.recurrence_analysis(rt, SK.six_maps(), jobs=3, samples=100, transient=100)
    sar.recurrence_lines(rt, K.noisy_cycle(100, 2, 2), eps2=K.EPS2, samples=100)
    sar.recurrence_plot(rt, K.noisy_cycle(100, 1, 1)[0], eps2=K.EPS2)
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    assert np.array_equal(basin.colorize(cfg), held)          # the basin's records are still the runtime's
    rt.reset()


def test_one_runtime_through_several_lengths(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    try:
        for t, jobs, sets, bins in ((64, 2, 1, 8), (700, 1, 2, 256), (3, 3, 3, 2), (513, 2, 1, 1024), (65, 1, 1, 4096), (700, 1, 2, 256)):
            pts = K.noisy_cycle(t, jobs, sets, seed=t)
            diag, vert, recs = sar.recurrence_lines(r, pts, eps2=K.EPS2, samples=t, line_bins=bins, records=True)
            for s in range(sets):
                _same_set((diag[s], vert[s], recs[s]), R.lines(pts[s], K.EPS2, t, 0, bins), (t, s))
    finally:
        r.close()


def test_recurrence_plot(sar, rt):
    pts = K.noisy_cycle(65, 2, 1)[0]
    for job in (0, 1):
        want = R.matrix(pts[job * 65:(job + 1) * 65], K.EPS2, 3)
        full = sar.recurrence_plot(rt, pts, eps2=K.EPS2, samples=65, theiler=3, job=job)
        assert full.dtype == bool and full.shape == (65, 65) and np.array_equal(full, want) and want.any()
        assert not np.diagonal(full, 3).any() and np.array_equal(full, full.T)
        # across the Theiler band, touching the last row and column, a row, a column, one entry
        for i0, j0, h, w in ((10, 8, 20, 30), (40, 50, 25, 15), (64, 0, 1, 65), (0, 64, 65, 1), (64, 64, 1, 1), (13, 26, 1, 1), (0, 13, 1, 1)):
            got = sar.recurrence_plot(rt, pts, eps2=K.EPS2, samples=65, theiler=3, job=job, window=(i0, j0, h, w))
            assert got.shape == (h, w) and np.array_equal(got, want[i0:i0 + h, j0:j0 + w]), (i0, j0, h, w)
    with pytest.raises(sar.SarError):
        sar.recurrence_plot(rt, pts, eps2=K.EPS2, samples=65, window=(1, 0, 65, 65))
    assert "leaves the trajectory" in sar.load_library().sar_last_error().decode()


def test_an_orbit_diagram_has_a_recurrence_analysis(sar, rt):
    a, b = logistic(2.9, 3.9)
    d = sar.orbit_diagram(rt, a, b, width=9, height=32, jobs=4, transient=200, steps=64, v_range=(0.0, 1.0))
    kw = dict(jobs=2, samples=200, transient=1500, theiler=1, line_bins=32, starts=SK.unit_starts(2))
    res = d.recurrence(rt, **kw)
    cs = np.stack([d.coeffs(c).reshape(30) for c in range(9)])
    direct = sar.recurrence_analysis(rt, cs, **kw)
    assert res.diag.shape == (9, 33) and res.diag.tobytes() == direct.diag.tobytes() and res.vert.tobytes() == direct.vert.tobytes()
    assert res.records.tobytes() == direct.records.tobytes() and np.array_equal(res.coeffs, cs)
    for c in (3, 8):
        want = R.rqa(cs[c], SK.unit_starts(2), 200, transient=1500, theiler=1, line_bins=32)
        assert np.array_equal(res.diag[c], want["diag"]) and np.array_equal(res.vert[c], want["vert"]), c
        _same_record(res.records[c], want, c)
    assert res.det[4] == 1.0 and res.det[8] < 1.0      # r = 3.4 is a period-2 cycle, r = 3.9 chaos


@pytest.mark.parametrize("change,text", K.RECURRENCE_REFUSED)
def test_recurrence_refusals_with_a_runtime(sar, rt, change, text):
    kw = dict(n=12, samples=0, theiler=0, line_bins=4, chunk=0, eps2=1.0)
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.recurrence_lines(rt, np.zeros((kw.pop("n"), 3)), **kw)
    assert text in sar.load_library().sar_last_error().decode()


@pytest.mark.parametrize("change,text", K.PLOT_REFUSED)
def test_plot_refusals_with_a_runtime(sar, rt, change, text):
    kw = dict(job=0, window=(0, 0, 6, 6))
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.recurrence_plot(rt, np.zeros((12, 3)), eps2=1.0, samples=6, **kw)
    assert text in sar.load_library().sar_last_error().decode()


@pytest.mark.parametrize("change,text", K.RQA_REFUSED)
def test_rqa_refusals_with_a_runtime(sar, rt, change, text):
    kw = dict(jobs=2, samples=8, stride=1, transient=10, bound=1e6)
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.recurrence_analysis(rt, SK.henon(), **kw)
    assert text in sar.load_library().sar_last_error().decode()


def test_what_is_not_a_number_is_refused_with_a_runtime(sar, rt):
    pts = K.noisy_cycle(16, 1, 2)
    pts[1, 3, 1] = math.nan
    with pytest.raises(sar.SarError):
        sar.recurrence_lines(rt, pts, eps2=1.0)
    assert "is NaN" in sar.load_library().sar_last_error().decode()
    c = SK.henon()
    c[4] = math.nan
    with pytest.raises(sar.SarError):
        sar.recurrence_analysis(rt, c, jobs=2, samples=8)
    assert "coefficients must be finite" in sar.load_library().sar_last_error().decode()
    diag, vert = sar.recurrence_lines(rt, np.zeros((0, 16, 3)), eps2=1.0, line_bins=4)      # no sets, no maps: nothing happens
    assert diag.shape == vert.shape == (0, 5)
    assert sar.recurrence_analysis(rt, np.zeros((0, 30)), jobs=2, samples=8, line_bins=4).diag.shape == (0, 5)
