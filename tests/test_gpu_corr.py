"""GPU: the correlation dimension (sar_runtime_pairs, sar_runtime_corrdim, include/sar.h) — pair histograms against the numpy
restatement bit for bit at every tile and wave boundary with planted edge cases, the line lattice against its closed form, maps
against the restatement (histograms, records, extents, points), independence of the launch, no side effect on the runtime, the Henon
map's D2 against the published interval, and the way up from search records."""
import math

import numpy as np
import pytest

import corr_cases as K
import corr_restatement as X
from orbit_cases import logistic

pytestmark = pytest.mark.gpu

MAPS_SHAPE = dict(jobs=70, samples=8, stride=3, transient=200)     # 70 jobs: a partial second wave


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    yield r
    r.close()


def _coeffs(cfg):
    return np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])


@pytest.fixture(scope="module")
def four_maps(sar):
    """The two presets (solar-sail loses some of these start points to infinity: DIVERGED, with a failing job that is not the first),
    Henon, and the logistic map at r = 4.4, which leaves for infinity from every start point."""
    return np.stack([_coeffs(sar.Config.poisson_saturne()), _coeffs(sar.Config.solar_sail()), K.henon(), logistic(4.4, 4.4)[0]])


@pytest.fixture(scope="module")
def maps_reference(sar, four_maps):
    """The restatement of the four maps at MAPS_SHAPE, computed once and left unchanged."""
    starts = sar.start_points(0, 0, MAPS_SHAPE["jobs"])
    return [X.corrdim(c, starts, MAPS_SHAPE["samples"], MAPS_SHAPE["stride"], MAPS_SHAPE["transient"], theiler=2) for c in four_maps]


@pytest.fixture(scope="module")
def maps_result(sar, rt, four_maps):
    return sar.correlation_dimension(rt, four_maps, points=True, theiler=2, **MAPS_SHAPE)


# 1 and 2: no pair, one pair; 63 / 64 / 65: the wave; 255 / 256 / 257: the 256-point tile; 700: three tiles, the last one partial
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 700])
def test_pairs_equal_the_restatement(sar, rt, n):
    pts = K.planted_sets(n)
    shapes = [(n, 0), (n, 5)]
    if n % 7 == 0:
        shapes += [(n // 7, 0), (n // 7, 5)]
    for samples, theiler in shapes:
        hist, cnt = sar.pair_histogram(rt, pts, samples=samples, theiler=theiler, counts=True)
        assert hist.shape == (3, 290) and hist.dtype == np.uint64
        for s in range(3):
            want, counted, skipped = X.pair_hist(pts[s], samples, theiler)
            assert np.array_equal(hist[s], want), (samples, theiler, s)
            assert (int(cnt["counted"][s]), int(cnt["skipped"][s])) == (counted, skipped)
            assert counted + skipped == n * (n - 1) // 2
    if n >= 6:
        hist = sar.pair_histogram(rt, pts)
        assert hist[0, 0] >= 1 and hist[1, 0] >= 1 and hist[1, 289] >= 1 and hist[2, 0] >= 2     # the planted pairs are where they belong


def test_other_binnings_and_infinite_coordinates(sar, rt):
    pts = K.planted_sets(65)[0]
    pts[7] = (math.inf, 0.0, 1.0)
    pts[9] = (math.inf, -math.inf, 0.0)                        # r^2 = NaN against point 7: the overflow bin
    for kw in (dict(sub_bits=0, e_min=-30, e_max=4), dict(sub_bits=4, e_min=-50, e_max=10), dict(sub_bits=3, e_min=-1022, e_max=-1000)):
        hist = sar.pair_histogram(rt, pts, **kw)
        assert np.array_equal(hist, X.pair_hist(pts, **kw)[0]), kw


def test_line_lattice_against_its_closed_form(sar, rt):
    n = 300
    hist, cnt = sar.pair_histogram(rt, K.line_lattice(n), counts=True)
    cum = np.cumsum(hist.astype(np.int64))
    for b in range(289):                                       # C_b = pairs with d^2 2^-20 < r2_b = (1 + m / 4) 2^(e - 64), in integers
        e, m = divmod(b, 4)
        q = math.ldexp(1.0 + m / 4.0, e - 64 + 20)
        D = math.isqrt(math.ceil(q) - 1) if q >= 1 else 0      # the largest d with d^2 < q
        assert cum[b] == K.line_cumulative(n, D), b
    assert int(cnt["counted"]) == n * (n - 1) // 2 == cum[-1]
    _, cnt = sar.pair_histogram(rt, K.line_lattice(n), samples=100, theiler=3, counts=True)
    assert int(cnt["skipped"]) == 3 * (99 + 98 + 97)


def _same_record(rec, want):
    assert int(rec["status"]) == want["status"]
    assert (int(rec["fail_job"]), int(rec["fail_step"])) == (want["fail_job"], want["fail_step"])
    assert (int(rec["counted"]), int(rec["skipped"])) == (want["counted"], want["skipped"])
    assert np.array_equal(rec["extent"], want["extent"])       # by value: -0.0 == 0.0
    line, wl = rec["line"], want["line"]
    assert (int(line["status"]), int(line["first_bin"]), int(line["last_bin"]), int(line["used"])) == \
        (wl["status"], wl["first_bin"], wl["last_bin"], wl["used"])
    if want["status"] == X.DIVERGED:
        assert math.isnan(rec["r_hi"]) and math.isnan(line["slope"])
        return
    assert rec["r_hi"] == want["r_hi"]
    for f in ("slope", "intercept", "rms"):
        if math.isnan(wl[f]):
            assert math.isnan(line[f])
        else:
            assert abs(line[f] - wl[f]) <= 1e-9 * max(abs(wl[f]), 1.0), f     # (the fit's conditioning: tests/test_corr_host.py)


def test_maps_equal_the_restatement(sar, rt, maps_result, maps_reference):
    res = maps_result
    assert res.hist.shape == (4, 290) and res.points.shape == (4, 560, 3) and res.edges.shape == (290,)
    assert [w["status"] for w in maps_reference] == [X.BOUNDED, X.DIVERGED, X.BOUNDED, X.DIVERGED]
    assert maps_reference[1]["fail_job"] > 0 and maps_reference[3]["fail_job"] == 0
    for k, want in enumerate(maps_reference):
        assert np.array_equal(res.hist[k], want["hist"]), k
        _same_record(res.records[k], want)
        assert np.array_equal(res.points[k].view(np.uint64), want["points"].view(np.uint64)), k
    assert not res.hist[3].any() and res.records["fail_step"][3] > 0 and res.records["counted"][3] == 0
    assert np.array_equal(res.status, [0, sar.SAR_SEARCH_DIVERGED, 0, sar.SAR_SEARCH_DIVERGED]) and math.isnan(res.d2[3])
    assert not res.hist[1].any() and not res.points[1].any() and not res.points[3].any()
    # the returned points through sar_runtime_pairs: the same histograms
    again = sar.pair_histogram(rt, res.points[[0, 2]], samples=MAPS_SHAPE["samples"], theiler=2)
    assert np.array_equal(again, res.hist[[0, 2]])
    # .fit refits on the host: the call's own window gives the records' lines, another window another line
    lines = res.fit()
    for f in sar.CORRDIM_LINE_DTYPE.names:
        assert np.array_equal(lines[f], res.records["line"][f], equal_nan=True), f
    wide = res.fit(c_lo=10.0, r_hi=math.inf)
    assert wide["used"][2] > lines["used"][2] and wide["status"][3] == sar.SAR_CORRDIM_NO_WINDOW


def test_results_do_not_depend_on_the_launch(sar, rt, four_maps, maps_result):
    pts = K.planted_sets(700)
    base = sar.pair_histogram(rt, pts, samples=100, theiler=5)
    lib = sar.load_library()
    try:
        for chunk, pair_launches in ((1, 4 * 6), (3, 4 * 2), (0, 1)):     # 700 points: 3 tiles, 6 cells of the folded triangle per set
            rt.set_option("corr_chunk", chunk)
            rt.enable_timing(True)
            hist = sar.pair_histogram(rt, pts, samples=100, theiler=5)
            t = rt.last_timing()
            if chunk:
                assert t.iterate_launches == 3 * 6 // chunk, chunk
            else:
                assert t.iterate_launches == 1
            assert t.iterate_ms > 0
            assert np.array_equal(hist, base), chunk
            res = sar.correlation_dimension(rt, four_maps, points=True, theiler=2, **MAPS_SHAPE)
            t = rt.last_timing()
            rt.enable_timing(False)
            assert t.warmup_ms > 0 and t.iterate_ms > 0 and t.iterate_launches == pair_launches, chunk     # 560 points: 3 tiles again
            assert np.array_equal(res.hist, maps_result.hist) and res.records.tobytes() == maps_result.records.tobytes(), chunk
            assert np.array_equal(res.points.view(np.uint64), maps_result.points.view(np.uint64)), chunk
        if hasattr(lib, "sar_runtime_set_test_option"):            # the copies of the LDS histogram change no count
            for copies in (1, 8):
                assert lib.sar_runtime_set_test_option(rt.handle, b"corr_replicas", copies) == 0
                assert np.array_equal(sar.pair_histogram(rt, pts, samples=100, theiler=5), base), copies
    finally:
        rt.set_option("corr_chunk", 0)
        rt.enable_timing(False)
        if hasattr(lib, "sar_runtime_set_test_option"):
            lib.sar_runtime_set_test_option(rt.handle, b"corr_replicas", 0)
    # one map per call
    for k in range(4):
        one = sar.correlation_dimension(rt, four_maps[k], points=True, theiler=2, **MAPS_SHAPE)
        assert np.array_equal(one.hist[0], maps_result.hist[k]) and one.records[0].tobytes() == maps_result.records[k].tobytes(), k
        assert np.array_equal(one.points[0].view(np.uint64), maps_result.points[k].view(np.uint64))
    # the caller's start points are the seed's
    given = sar.correlation_dimension(rt, four_maps, starts=sar.start_points(0, 0, 70), theiler=2, **MAPS_SHAPE)
    assert np.array_equal(given.hist, maps_result.hist) and given.points is None
    with pytest.raises(sar.SarError):
        rt.set_option("corr_chunk", 2 ** 30 + 1)


def test_the_runtime_is_only_lent(sar, rt, four_maps):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    rt.seed(9)
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    sar.correlation_dimension(rt, four_maps, **MAPS_SHAPE)
    sar.pair_histogram(rt, K.planted_sets(65))
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    # the start-point stream: the next render draws what a runtime seeded alike and left alone draws
    other = sar.Runtime(cfg, device=0)
    other.seed(9)
    sar.render_jobs(cfg, other, sar.start_points(3, 0, 64))
    other.reset()
    rt.reset()
    sar.render_jobs(cfg, rt)
    sar.render_jobs(cfg, other)
    assert np.array_equal(rt.count(), other.count()) and rt.max() == other.max()
    other.close()
    rt.reset()


def test_henon_d2_lies_in_the_published_interval(sar, rt):
    """x' = 1 - 1.4 x^2 + y, y' = 0.3 x (z' = 0.5 z): published D2 = 1.21 +- 0.01 (Grassberger & Procaccia 1983) and 1.220 +- 0.036
    (Sprott's tables); [1.184, 1.256] are the ends of the wider. The restatement gives 1.2116 at this shape with these start points."""
    res = sar.correlation_dimension(rt, K.henon(), jobs=64, samples=128, stride=4)
    rec = res.records[0]
    print("henon d2", res.d2[0], "window", rec["line"]["first_bin"], rec["line"]["last_bin"], "rms", rec["line"]["rms"])
    assert rec["status"] == sar.SAR_SEARCH_BOUNDED and rec["counted"] == 8192 * 8191 // 2
    assert 1.184 <= res.d2[0] <= 1.256


def test_search_records_go_in_as_they_are(sar, rt):
    recs, _ = sar.search_attractors(rt, 4096, seed=1, transient=1000, steps=4000, keep_rejected=1)
    bounded = recs[recs["status"] == sar.SAR_SEARCH_BOUNDED][:24]
    assert bounded.size >= 8
    # one job from the search's start point: the first 1000 + 1024 steps of the very trajectory the search followed
    res = sar.correlation_dimension(rt, bounded, search_seed=1, jobs=1, samples=1024, stride=1, transient=1000, theiler=4,
                                    starts=np.full((1, 3), 0.05))
    assert np.array_equal(res.coeffs[0], sar.search_candidate(1, int(bounded["candidate"][0])).reshape(30))
    assert np.all(res.status == sar.SAR_SEARCH_BOUNDED)
    has_window = res.records["line"]["status"] == sar.SAR_CORRDIM_FIT_OK
    assert has_window.any() and np.all(np.isfinite(res.d2[has_window])) and np.all(np.isnan(res.d2[~has_window]))
    for k in range(bounded.size):                              # the extent of 1024 of the search's 4000 points lies inside the search's
        e, s = res.records["extent"][k], bounded["extent"][k]
        assert np.all(e[0::2] >= s[0::2]) and np.all(e[1::2] <= s[1::2]), k
