"""GPU: the period planes (sar_runtime_period, include/sar.h) — every field of the records, `residual` included, against the numpy
restatement bit for bit on two Hénon planes and a plane around poisson-saturne; the known periods of tests/period_cases.py through
the list form; the sweep form against the list form; independence of the launch shape; no side effect on the image buffers; the
colours against their restatement (and through a PNG); and the periods of an orbit diagram's columns."""
import ctypes as C
import math
import os
import tempfile

import numpy as np
import pytest

import image_decode as D
import period_cases as K
import period_restatement as Q

pytestmark = pytest.mark.gpu

INT_FIELDS = ("status", "period", "transient_done", "steps_done")
BIG, SMALL = K.HENON_PLANES
SATURNE = dict(axes=(0, 13), d=0.08, width=48, height=40, params=dict(transient=1000, max_period=128))


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=64, height=64), device=0)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(records, want):
    for f in INT_FIELDS:
        assert np.array_equal(records[f].astype(np.int64), want[f].astype(np.int64)), f
    nan = np.isnan(want["residual"])
    assert np.array_equal(np.isnan(records["residual"]), nan)
    assert np.array_equal(_bits(records["residual"][~nan]), _bits(want["residual"][~nan]))


def _henon(sar, rt, case, **kw):
    w, h, params = case[:3]
    return sar.period_plane(rt, K.HENON_PLANE["base"], K.HENON_PLANE["axes"], K.HENON_PLANE["x_range"], K.HENON_PLANE["y_range"], w, h,
                            **params, **kw)


@pytest.fixture(scope="module")
def henon_references():
    """The restatements of the two Hénon planes, computed once and left unchanged."""
    return {(c[0], c[1]): Q.period_plane(width=c[0], height=c[1], **K.HENON_PLANE, **c[2]) for c in K.HENON_PLANES}


@pytest.fixture(scope="module")
def small_bytes(sar, rt):
    """The 37 x 21 plane's record bytes at the default launch shape."""
    return _henon(sar, rt, SMALL).records.tobytes()


# ---- 1. parity --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", K.HENON_PLANES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_henon_plane_equals_the_restatement(sar, rt, henon_references, case):
    w, h, _, diverged, zero, counts, _ = case
    pl = _henon(sar, rt, case)
    want = henon_references[(w, h)]
    assert pl.records.shape == (h, w)
    _same(pl.records, want)
    assert pl.stats == Q.stats(want)
    hist = pl.histogram()
    assert hist[0] == zero and [int(hist[p]) for p in counts] == list(counts.values())
    assert pl.stats["diverged_transient"] + pl.stats["diverged_late"] == diverged and hist.sum() == w * h - diverged
    assert len(hist) == pl.stats["max_period_found"] + 1


def test_plane_around_poisson_saturne_equals_the_restatement(sar, rt):
    cfg = sar.Config.poisson_saturne()
    base = np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    axes, d, w, h = SATURNE["axes"], SATURNE["d"], SATURNE["width"], SATURNE["height"]
    xr, yr = [(base[a] - d, base[a] + d) for a in axes]
    pl = sar.period_plane(rt, cfg, axes, xr, yr, w, h, **SATURNE["params"])
    want = Q.period_plane(base, axes, xr, yr, w, h, **SATURNE["params"])
    _same(pl.records, want)
    assert pl.stats == Q.stats(want) and pl.stats["pixels"] == w * h
    assert np.array_equal(_bits(pl.coeffs(5, 7)), _bits(Q.coeffs(base, axes, xr, yr, w, h)[7 * w + 5].reshape(3, 10)))


# ---- 2. known answers, through the list form ---------------------------------------------------------------------------------
def _listed(sar, rt, cs, **params):
    cs = np.asarray(cs)
    pl = sar.period_plane(rt, width=cs.shape[0], height=1, coeffs=cs, **params)
    return pl.records[0]


def test_logistic_periods(sar, rt):
    r = _listed(sar, rt, np.stack([K.logistic(v) for v, _, _ in K.LOGISTIC]), **K.LOGISTIC_PARAMS)
    assert [(int(s), int(p)) for s, p in zip(r["status"], r["period"])] == [(s, p) for _, s, p in K.LOGISTIC]
    last = r[-1]
    assert (int(last["transient_done"]), int(last["steps_done"])) == (K.LOGISTIC_DIVERGED_AT, 0) and math.isnan(last["residual"])
    assert np.all(r["transient_done"][:-1] == K.LOGISTIC_PARAMS["transient"])
    chaotic = r[(r["status"] == K.BOUNDED) & (r["period"] == 0)]
    assert np.all(chaotic["steps_done"] == K.LOGISTIC_PARAMS["max_period"]) and np.all(np.isnan(chaotic["residual"]))
    found = r[r["period"] != 0]
    assert np.all(found["steps_done"] == found["period"]) and np.all(found["residual"] <= K.LOGISTIC_PARAMS["eps"])


def test_henon_periods(sar, rt):
    r = _listed(sar, rt, np.stack([K.henon(a) for a, _ in K.HENON]), **K.HENON_PARAMS)
    assert np.all(r["status"] == K.BOUNDED) and [int(p) for p in r["period"]] == [p for _, p in K.HENON]


def test_exact_cycles(sar, rt):
    cs = np.stack([K.linear(m) for _, m, _ in K.CYCLES])
    r = _listed(sar, rt, cs, **K.CYCLE_PARAMS)
    assert [int(p) for p in r["period"]] == [p for _, _, p in K.CYCLES] == [int(s) for s in r["steps_done"]]
    assert np.all(r["status"] == K.BOUNDED) and np.array_equal(_bits(r["residual"]), _bits(np.zeros(len(K.CYCLES))))
    short = _listed(sar, rt, cs, **{**K.CYCLE_PARAMS, "max_period": 5})
    assert [int(p) for p in short["period"]] == [1, 2, 3, 4, 0] and int(short["steps_done"][-1]) == 5
    assert short["status"][-1] == K.BOUNDED and math.isnan(short["residual"][-1])
    assert np.array_equal(_bits(short["residual"][:-1]), _bits(np.zeros(4)))


# ---- 3. the sweep form equals the list form ------------------------------------------------------------------------------------
def test_sweep_form_equals_list_form(sar, rt, small_bytes):
    from strange_attractor_renderer_amd import _abi
    w, h, params = SMALL[:3]
    cs = Q.coeffs(width=w, height=h, **K.HENON_PLANE)
    listed = sar.period_plane(rt, width=w, height=h, coeffs=cs, **params)
    assert listed.records.tobytes() == small_bytes
    assert np.array_equal(_bits(listed.coeffs(3, 2)), _bits(cs[2 * w + 3].reshape(3, 10)))
    # base, axes and ranges are ignored with a list: absurd ones change nothing
    p = sar.period_params(np.full(30, math.nan), (7, 7), (math.inf, 0.0), (0.0, math.nan), w, h, **params)
    rec = np.empty(w * h, dtype=sar.PERIOD_RECORD_DTYPE)
    st = sar.load_library().sar_runtime_period(rt.handle, C.byref(p), cs.ctypes.data_as(C.POINTER(C.c_double)),
                                               rec.ctypes.data_as(C.POINTER(_abi.SarPeriodRecord)), None)
    assert st == 0 and rec.tobytes() == small_bytes


# ---- 4. the launch shape ---------------------------------------------------------------------------------------------------------
def test_launch_shape_does_not_matter(sar, rt, henon_references, small_bytes):
    w, h, params = SMALL[:3]                     # tiles_x = 5: a tile row is 320 pixels; the last tiles are partial
    _same(np.frombuffer(small_bytes, dtype=sar.PERIOD_RECORD_DTYPE).reshape(h, w), henon_references[(w, h)])
    try:
        for chunk in (0, 64, 100, 128, 320, 1000, 1 << 22):
            rt.set_option("period_chunk", chunk)
            assert _henon(sar, rt, SMALL).records.tobytes() == small_bytes, chunk
        assert _henon(sar, rt, SMALL).records.tobytes() == small_bytes      # two calls in a row
        with pytest.raises(sar.SarError) as e:
            rt.set_option("period_chunk", (1 << 30) + 1)
        assert e.value.status == 1
        assert _henon(sar, rt, SMALL).records.tobytes() == small_bytes      # the refused value changed nothing
    finally:
        rt.set_option("period_chunk", 0)
    for ww, hh in ((1, 11), (13, 1)):            # a plane of one column / one row
        got = sar.period_plane(rt, K.HENON_PLANE["base"], K.HENON_PLANE["axes"], K.HENON_PLANE["x_range"], K.HENON_PLANE["y_range"],
                               ww, hh, **params)
        _same(got.records, Q.period_plane(width=ww, height=hh, **K.HENON_PLANE, **params))


# ---- 5. no side effects ------------------------------------------------------------------------------------------------------------
def test_no_side_effect_on_the_image_buffers_and_timing(sar, gpu):
    cfg = sar.Config.poisson_saturne(iterations=1024 * 200, width=64, height=64, jobs_total=1024, seed=5)
    r = sar.Runtime(cfg, device=0)
    try:
        sar.render(cfg, r)
        before = (r.count(), r.steps(), r.zbuf(), r.max())
        r.enable_timing(True)
        r.set_option("period_chunk", 256)
        pl = sar.period_plane(r, cfg, (0, 1), (-0.5, 0.5), (-0.5, 0.5), 40, 24, transient=200, max_period=32)
        t = r.last_timing()
        after = (r.count(), r.steps(), r.zbuf(), r.max())
        assert np.array_equal(before[0], after[0]) and before[3] == after[3]
        assert np.array_equal(before[1].view(np.uint64), after[1].view(np.uint64))
        assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32))
        assert t.iterate_ms > 0 and t.iterate_launches == 4   # 5 x 3 tiles, 4 per launch of 256 pixels
        assert pl.records.shape == (24, 40)
    finally:
        r.close()


# ---- 6. colorize ---------------------------------------------------------------------------------------------------------------------
def test_colorize_matches_the_restatement(sar, rt):
    pl = _henon(sar, rt, BIG)
    cfg = sar.Config.poisson_saturne()
    pal = cfg.palette_rgb[:cfg.palette_len]
    img = pl.colorize(cfg)
    assert img.shape == (BIG[1], BIG[0], 4) and img.dtype == np.uint16
    assert np.array_equal(img, Q.colorize(pl.status, pl.period, pal))
    assert np.array_equal(pl.colorize(cfg, colours=5), Q.colorize(pl.status, pl.period, pal, colours=5))
    assert np.all(img[pl.status == K.DIVERGED] == 0) and np.all(img[(pl.status == K.BOUNDED) & (pl.period == 0)] == (0, 0, 0, 65535))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "period.png")
        sar.write_image(img, path)
        assert np.array_equal(D.decode_png(path), img)
    out = np.empty(img.size, dtype=np.uint16)
    zero = sar.period_colors(0)
    assert sar.load_library().sar_runtime_period_colorize(C.byref(cfg.c), rt.handle, C.byref(zero), out.ctypes.data_as(C.POINTER(C.c_uint16))) == 1
    other = _henon(sar, rt, SMALL)
    with pytest.raises(ValueError):
        pl.colorize(cfg)                         # stale: the runtime holds `other`'s records
    assert other.colorize(cfg).shape == (SMALL[1], SMALL[0], 4)


def test_colorize_without_a_period_plane_is_refused(sar, gpu):
    cfg = sar.Config.solar_sail(width=16, height=16)
    r = sar.Runtime(cfg, device=0)
    try:
        out = np.empty(16 * 16 * 4, dtype=np.uint16)
        st = sar.load_library().sar_runtime_period_colorize(C.byref(cfg.c), r.handle, None, out.ctypes.data_as(C.POINTER(C.c_uint16)))
        assert st == 1
    finally:
        r.close()


# ---- 7. the orbit diagram's columns ------------------------------------------------------------------------------------------------
def test_orbit_diagram_periods_along_the_logistic_line(sar, rt):
    from orbit_cases import logistic
    line = K.LOGISTIC_LINE
    d = sar.orbit_diagram(rt, *logistic(*line["r_range"]), width=line["width"], height=32, jobs=64, transient=200, steps=64,
                          v_range=(0.0, 1.0))
    per = d.period(rt, start=line["start"])
    assert per.shape == (line["width"],) and per.dtype == np.int64
    cs = np.stack([d.coeffs(c).reshape(30) for c in range(line["width"])])
    want = Q.period_list(cs, start=line["start"])
    assert np.array_equal(per, np.where(want["status"] == K.BOUNDED, want["period"].astype(np.int64), -1))
    assert {1, 2, 4, 8} <= set(per.tolist()) and np.all(per >= 0)
    assert np.count_nonzero(per == 0) <= line["max_zero_columns"]    # slow convergence at the three bifurcation points
    assert np.all(np.diff(per[per != 0]) >= 0)
    # a column that leaves the bound box reads -1
    wide = sar.orbit_diagram(rt, *logistic(3.9, 4.4), width=3, height=8, jobs=64, transient=50, steps=16, v_range=(0.0, 1.0))
    assert wide.period(rt, start=line["start"], transient=500).tolist()[-1] == -1
