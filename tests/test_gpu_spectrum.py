"""GPU: the power spectra (sar_runtime_spectra, sar_runtime_spectrum, include/sar.h) — every output double against the numpy
restatement bit for bit: random sets at every transform size where the kernel takes another path, with tails, odd hops, several
jobs and sets, both windows and two projections; the planted series; six maps in one call with their records and points;
independence of the chunk with the launch counts it implies; no side effect on the runtime or on a held basin picture; one runtime
through several sizes; OrbitDiagram.spectrum and the colours; the refusals behind a runtime. A value that is not finite is compared
by class: the same infinity, or NaN on both sides."""
import math

import numpy as np
import pytest

import basin_restatement as B
import spectrum_cases as K
import spectrum_restatement as S
from basin_cases import PITCHFORK_MU, PITCHFORK_WINDOW
from orbit_cases import logistic

pytestmark = pytest.mark.gpu

KINDS = dict(rect=S.RECT, hann=S.HANN)
MAPS_SHAPE = dict(jobs=8, segments=7, n=256, hop=128, transient=2000)
AXIS, SKEW = (1.0, 0.0, 0.0), (0.5, -2.0, 0.25)

# (n, hop, samples, jobs, sets, window, proj): N = 8 has fewer butterflies than lanes, 256 half a butterfly per lane and 512 one;
# 1024, 2048 and 4096 are the kernel's instances of 2, 4 and 8 per lane, and 4096 fills the LDS; hop 1, N / 2, N and odd;
# samples = N is one segment, the others leave a tail
SETS = [
    (8, 1, 12, 3, 3, "hann", AXIS),
    (8, 8, 8, 1, 1, "rect", SKEW),
    (8, 4, 19, 3, 1, "rect", AXIS),
    (16, 8, 37, 3, 3, "hann", SKEW),
    (16, 5, 16, 1, 3, "rect", AXIS),
    (256, 128, 529, 3, 1, "hann", AXIS),
    (256, 256, 256, 1, 3, "rect", SKEW),
    (512, 77, 700, 1, 3, "hann", SKEW),
    (512, 256, 1030, 3, 1, "rect", AXIS),
    (1024, 512, 2053, 3, 1, "hann", SKEW),
    (2048, 683, 3000, 1, 3, "rect", AXIS),
    (4096, 2048, 8197, 3, 1, "hann", SKEW),
    (4096, 4096, 4096, 1, 3, "rect", AXIS),
    (4096, 1365, 5500, 1, 1, "hann", AXIS),
]


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    yield r
    r.close()


def _same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got[np.isinf(want)], want[np.isinf(want)]), what
    g, w = got[fin].view(np.uint64), want[fin].view(np.uint64)
    assert np.array_equal(g, w), (what, int(np.sum(g != w)), np.argwhere(g != w)[:4].tolist())


@pytest.mark.parametrize("n,hop,samples,jobs,sets,window,proj", SETS)
def test_sets_equal_the_restatement(sar, rt, n, hop, samples, jobs, sets, window, proj):
    pts = K.random_sets(jobs * samples, sets)
    power, recs = sar.power_spectra(rt, pts, n=n, hop=hop, window=window, samples=samples, proj=proj, records=True)
    want_p, want_e, want_jobs, want_segs = S.spectra(pts, n, hop, KINDS[window], samples, proj)
    assert power.shape == (sets, n // 2 + 1) and (want_jobs, want_segs) == (jobs, (samples - n) // hop + 1)
    _same(power, want_p, "power")
    _same(recs["energy"], want_e, "energy")
    assert np.all(recs["jobs"] == jobs) and np.all(recs["segments"] == want_segs)
    assert np.all(power >= 0.0) and np.all(np.isfinite(power))
    one = sar.power_spectra(rt, pts[0], n=n, hop=hop, window=window, samples=samples, proj=proj)      # (n_points, 3): one set
    assert one.shape == (n // 2 + 1,) and one.tobytes() == power[0].tobytes()


def test_a_series_goes_into_x(sar, rt):
    pts = K.random_sets(100, 1)[0]
    assert sar.power_spectra(rt, pts[:, 0], n=16, hop=None).tobytes() == sar.power_spectra(rt, pts, n=16, hop=8).tobytes()
    assert sar.power_spectra(rt, pts[:, 1], n=16).tobytes() == sar.power_spectra(rt, pts, n=16, proj=(0.0, 1.0, 0.0)).tobytes()


@pytest.mark.parametrize("name", list(K.planted_series()))
def test_planted_series(sar, rt, name):
    series, kw = K.planted_series()[name]
    power, rec = sar.power_spectra(rt, series, records=True, **kw)
    pts = np.zeros((series.size, 3))
    pts[:, 0] = series
    want_p, want_e, _, want_segs = S.spectra(pts, kw["n"], kw["hop"], KINDS[kw["window"]])
    _same(power, want_p, name)
    _same(rec["energy"], want_e, name)
    assert rec["segments"] == want_segs and rec["jobs"] == 1
    if name in ("constant", "minus zero"):
        assert not power.view(np.uint64).any() and rec["energy"].tobytes() == bytes(8)      # all +0.0
    if name == "alternating":
        assert power.tolist() == [0.0, 0.0, 0.0, 0.0, 128.0] and rec["energy"] == 16.0
    if name == "1e200":
        assert np.isinf(power).any() and not np.isnan(power).any() and rec["energy"] == math.inf
    if name == "1.7e308":
        assert np.isnan(power).all()


@pytest.fixture(scope="module")
def maps_reference():
    """The restatement of the six maps at MAPS_SHAPE, computed once and left unchanged."""
    kw = {k: v for k, v in MAPS_SHAPE.items() if k != "jobs"}
    return [S.spectrum(c, K.unit_starts(MAPS_SHAPE["jobs"]), **kw) for c in K.six_maps()]


@pytest.fixture(scope="module")
def maps_result(sar, rt):
    return sar.power_spectrum(rt, K.six_maps(), starts=K.unit_starts(MAPS_SHAPE["jobs"]), points=True, **MAPS_SHAPE)


def _same_record(rec, want):
    assert (int(rec["status"]), int(rec["fail_job"]), int(rec["fail_step"]), int(rec["segments"])) == \
        (want["status"], want["fail_job"], want["fail_step"], want["segments"])
    assert np.array_equal(rec["extent"], want["extent"]) and rec["_pad"] == 0      # by value: -0.0 == 0.0
    _same(rec["energy"], want["energy"], "energy")


def test_maps_equal_the_restatement(sar, rt, maps_result, maps_reference):
    res = maps_result
    assert res.power.shape == (6, 129) and res.samples == 1024 and res.points.shape == (6, 8 * 1024, 3)
    assert [w["status"] for w in maps_reference] == [S.BOUNDED] * 5 + [S.DIVERGED]
    for k, want in enumerate(maps_reference):
        _same(res.power[k], want["power"], k)
        _same_record(res.records[k], want)
        assert np.array_equal(res.points[k].view(np.uint64), want["points"].view(np.uint64)), k
    assert not res.power[5].view(np.uint64).any() and not res.points[5].any()      # DIVERGED: all +0.0
    assert res.records["energy"][5].tobytes() == bytes(8) and res.records["fail_step"][5] > 0
    assert np.array_equal(res.status, [0, 0, 0, 0, 0, sar.SAR_SEARCH_DIVERGED])
    # the returned points through sar_runtime_spectra: the same power and energy
    again, recs = sar.power_spectra(rt, res.points[:5], n=256, hop=128, samples=res.samples, records=True)
    assert again.tobytes() == res.power[:5].tobytes() and recs["energy"].tobytes() == res.records["energy"][:5].tobytes()
    assert np.all(recs["jobs"] == 8) and np.all(recs["segments"] == 7)
    # what the spectra say: the rotation's line, the period-2 and period-4 lines, chaos without one
    assert res.peaks(4, 1)[0] == K.ROTATION_BIN and res.peaks(1, 1)[0] == 128 and set(res.peaks(2, 2)) >= {128}
    assert np.all(res.flatness[[1, 2, 4]] <= 1e-3) and np.all(res.flatness[[0, 3]] >= 0.5) and res.flatness[5] == 0.0
    assert res.freq[0] == 0.0 and res.freq[128] == 0.5 and res.psd.shape == res.power.shape
    assert np.all(res.db()[5] == -120.0) and res.db()[4, K.ROTATION_BIN] == 0.0 and res.db().max() == 0.0
    assert res.autocorrelation(0)[0] == 1.0 and 1 <= res.decorrelation(0) <= 8 and res.decorrelation(3) >= 1


def test_another_projection_and_stride(sar, rt):
    kw = dict(segments=3, n=16, hop=5, stride=3, transient=100, window="rect", proj=SKEW)
    starts = K.unit_starts(3, seed=9)
    res = sar.power_spectrum(rt, K.henon(), starts=starts, jobs=3, **kw)
    want = S.spectrum(K.henon(), starts, segments=3, n=16, hop=5, kind=S.RECT, stride=3, transient=100, proj=SKEW)
    _same(res.power[0], want["power"], "power")
    _same_record(res.records[0], want)
    assert res.points is None and res.freq[8] == 0.5 / 3


def test_results_do_not_depend_on_the_chunk(sar, rt, maps_result):
    pts = K.random_sets(3 * 37, 3)
    base = sar.power_spectra(rt, pts, n=16, hop=8, samples=37)
    try:
        for chunk, launches_sets, launches_maps in ((1, 9, 48), (3, 3, 16), (0, 1, 1)):
            rt.enable_timing(True)
            got = sar.power_spectra(rt, pts, n=16, hop=8, samples=37, chunk=chunk)
            t = rt.last_timing()
            assert t.iterate_launches == launches_sets and t.iterate_ms > 0 and t.resolve_ms > 0, chunk
            assert got.tobytes() == base.tobytes(), chunk
            res = sar.power_spectrum(rt, K.six_maps(), starts=K.unit_starts(8), points=True, chunk=chunk, **MAPS_SHAPE)
            t = rt.last_timing()
            rt.enable_timing(False)
            assert t.iterate_launches == launches_maps and t.warmup_ms > 0 and t.iterate_ms > 0 and t.resolve_ms > 0, chunk
            assert res.power.tobytes() == maps_result.power.tobytes() and res.records.tobytes() == maps_result.records.tobytes(), chunk
            assert np.array_equal(res.points.view(np.uint64), maps_result.points.view(np.uint64)), chunk
    finally:
        rt.enable_timing(False)
    one = sar.power_spectrum(rt, K.six_maps()[4], starts=K.unit_starts(8), **MAPS_SHAPE)      # one map per call
    assert one.power[0].tobytes() == maps_result.power[4].tobytes() and one.records[0].tobytes() == maps_result.records[4].tobytes()


def test_the_runtime_is_only_lent(sar, rt):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    basin = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), width=33, height=17, transient=300, steps=32, grid=8, **PITCHFORK_WINDOW)
    held = basin.colorize(cfg)
    sar.power_spectrum(rt, K.six_maps(), jobs=3, segments=2, n=64, transient=100)
    sar.power_spectra(rt, K.random_sets(100, 2), n=32)
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    assert np.array_equal(basin.colorize(cfg), held)          # the basin's records are still the runtime's
    rt.reset()


def test_one_runtime_through_several_sizes(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    try:
        for n, hop, samples, jobs in ((4096, 2048, 6144, 2), (8, 3, 20, 3), (1024, 512, 2048, 2), (4096, 2048, 6144, 2)):
            pts = K.random_sets(jobs * samples, 2, seed=n)
            got, recs = sar.power_spectra(r, pts, n=n, hop=hop, samples=samples, records=True)
            want_p, want_e, _, _ = S.spectra(pts, n, hop, S.HANN, samples)
            _same(got, want_p, n)
            _same(recs["energy"], want_e, n)
    finally:
        r.close()


def test_an_orbit_diagram_has_a_spectrum(sar, rt):
    a, b = logistic(2.9, 3.9)
    d = sar.orbit_diagram(rt, a, b, width=9, height=32, jobs=4, transient=200, steps=64, v_range=(0.0, 1.0))
    kw = dict(jobs=4, segments=3, n=64, hop=32, transient=1500, window="rect", starts=K.unit_starts(4))
    sp = d.spectrum(rt, **kw)
    cs = np.stack([d.coeffs(c).reshape(30) for c in range(9)])
    direct = sar.power_spectrum(rt, cs, **kw)
    assert sp.power.shape == (9, 33) and sp.power.tobytes() == direct.power.tobytes() and sp.records.tobytes() == direct.records.tobytes()
    assert np.array_equal(sp.coeffs, cs) and list(sp.params.proj) == list(d.params.proj)
    want = S.spectrum(cs[3], K.unit_starts(4), segments=3, n=64, hop=32, kind=S.RECT, transient=1500)
    _same(sp.power[3], want["power"], "column 3")
    assert sp.flatness.shape == (9,) and sp.flatness[-1] > sp.flatness[4]      # r = 3.9 is broadband, r = 3.4 a period-2 line
    count, top = sp.counts()
    k, m = np.unravel_index(np.argmax(sp.power.T), sp.power.T.shape)
    assert count.shape == (33, 9) and count.dtype == np.uint32 and top == 2 ** 32 - 2 and count[32 - k, m] == top
    img = sp.colorize(sar.Config.solar_sail())
    assert img.shape == (33, 9, 4) and img.dtype == np.uint16
    light = img[..., :3].astype(np.int64).sum(axis=2)
    assert light[32 - k, m] == light.max() and light.max() > light.min()      # the brightest pixel is the largest bin
    assert sp.colorize(sar.Config.solar_sail(), hue=sp.flatness).shape == (33, 9, 4)
    again = d.colorize(sar.Config.solar_sail(), hue=sp.flatness)      # the flatness is a hue for the diagram itself
    assert again.shape == (32, 9, 4)


@pytest.mark.parametrize("change,text", K.SPECTRA_REFUSED)
def test_spectra_refusals_with_a_runtime(sar, rt, change, text):
    kw = dict(n=8, hop=4, window="hann", samples=None, chunk=0, proj=(1.0, 0.0, 0.0), n_points=16)
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.power_spectra(rt, np.zeros((kw.pop("n_points"), 3)), **kw)
    assert text in sar.load_library().sar_last_error().decode()


@pytest.mark.parametrize("change,text", K.SPECTRUM_REFUSED)
def test_spectrum_refusals_with_a_runtime(sar, rt, change, text):
    kw = dict(jobs=2, segments=3, n=8, hop=4, stride=1, transient=10, bound=1e6)
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.power_spectrum(rt, K.henon(), **kw)
    assert text in sar.load_library().sar_last_error().decode()


def test_what_is_not_finite_is_refused_with_a_runtime(sar, rt):
    pts = K.random_sets(16, 2)
    pts[1, 3, 1] = math.inf
    with pytest.raises(sar.SarError):
        sar.power_spectra(rt, pts, n=8)
    assert "not finite" in sar.load_library().sar_last_error().decode()
    c = K.henon()
    c[4] = math.nan
    with pytest.raises(sar.SarError):
        sar.power_spectrum(rt, c, jobs=2, segments=1, n=8)
    assert "coefficients must be finite" in sar.load_library().sar_last_error().decode()
    assert sar.power_spectra(rt, np.zeros((0, 16, 3)), n=8).shape == (0, 5)      # no sets, no maps: nothing happens
    assert sar.power_spectrum(rt, np.zeros((0, 30)), jobs=2, segments=1, n=8).power.shape == (0, 5)
