"""Host: the correlation dimension without a device (include/sar.h: sar_pairs_*, sar_corrdim_*) — the restatement against closed-form
lattice counts at every bin edge, sar_pairs_edges and sar_corrdim_fit against the restatement, the defaults, the "no window" case and
every refusal that needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

import corr_cases as K
import corr_restatement as X


def test_line_lattice_equals_the_closed_form_at_every_edge():
    n = 300
    hist, counted, skipped = X.pair_hist(K.line_lattice(n))
    assert counted == n * (n - 1) // 2 and skipped == 0
    cum = np.cumsum(hist.astype(np.int64))
    r2 = X.edges_r2()
    for b in range(len(r2)):                                   # C_b = pairs with r2 < r2_b: d^2 2^-20 < r2_b, in integers
        q = r2[b] * 2.0 ** 20                                  # exact: a power of two times m / 4
        D = math.isqrt(math.ceil(q) - 1) if q >= 1 else 0      # the largest d with d^2 < q
        assert cum[b] == K.line_cumulative(n, D), b
    assert cum[-1] == counted
    _, counted, skipped = X.pair_hist(K.line_lattice(n), samples=100, theiler=3)
    assert skipped == 3 * (99 + 98 + 97) and counted + skipped == n * (n - 1) // 2


def test_plane_lattice_equals_the_closed_form_at_every_edge():
    m = 16
    hist, counted, _ = X.pair_hist(K.plane_lattice(m))
    cum = np.cumsum(hist.astype(np.int64))
    r2 = X.edges_r2()
    for b in range(len(r2)):
        q = r2[b] * 2.0 ** 12                                  # r2 = (a^2 + b^2) 2^-12
        assert cum[b] == K.plane_cumulative(m, math.ceil(q)), b
    assert counted == m * m * (m * m - 1) // 2


def test_bins_of_the_edge_cases():
    assert X.n_bins() == 290
    r2 = np.array([0.0, 5e-324, 2.0 ** -1022, 2.0 ** -65, 2.0 ** -64, 1.25 * 2.0 ** -64, 1.0, 1.75, 2.0 ** 8 * (1 - 2.0 ** -53), 2.0 ** 8,
                   np.inf, np.nan, -np.nan])
    assert list(X.bin_of(r2)) == [0, 0, 0, 0, 1, 2, 257, 260, 288, 289, 289, 289, 289]


def test_defaults_and_edges(sar):
    p = sar.pairs_params()
    assert (p.samples, p.theiler, p.sub_bits, p.e_min, p.e_max) == (0, 0, 2, -64, 8)
    q = sar.corrdim_params()
    assert (q.jobs, q.samples, q.stride, q.transient, q.theiler, q.sub_bits, q.e_min, q.e_max) == (256, 128, 4, 1000, 0, 2, -64, 8)
    assert (q.seed, q.bound, q.c_lo, q.r_hi_fraction) == (0, 1e6, 100.0, 2.0 ** -4)
    e = sar.pair_edges()
    assert e.shape == (290,) and e[-1] == math.inf
    assert np.array_equal(e[:-1], np.sqrt(X.edges_r2()))
    assert e[0] == 2.0 ** -32 and e[288] == 16.0
    for kw in (dict(sub_bits=0, e_min=-10, e_max=3), dict(sub_bits=4, e_min=-1022, e_max=-1000), dict(sub_bits=3, e_min=1000, e_max=1023)):
        e = sar.pair_edges(sar.pairs_params(**kw))
        assert e.size == X.n_bins(**kw) and np.array_equal(e[:-1], np.sqrt(X.edges_r2(**kw)))
    assert "corr_chunk" in sar.api._abi.STABLE_OPTIONS
    with pytest.raises(ValueError):
        sar.pairs_params(theiler=-1)
    with pytest.raises(AttributeError):
        sar.corrdim_params(width=3)


def _same_line(got, want):
    assert (int(got["status"]), int(got["first_bin"]), int(got["last_bin"]), int(got["used"])) == \
        (want["status"], want["first_bin"], want["last_bin"], want["used"])
    for f in ("slope", "intercept", "rms"):
        if math.isnan(want[f]):
            assert math.isnan(got[f]), f
        else:
            # 1e-9 relative: libm and summation differences over at most 1024 terms of order 1 — the fit's conditioning
            assert abs(got[f] - want[f]) <= 1e-9 * max(abs(want[f]), 1.0), (f, got[f], want[f])


def test_fit_equals_the_restatement(sar):
    rng = np.random.default_rng(5)
    hist = rng.integers(0, 1000, size=290).astype(np.uint64)
    hist[:40] = 0
    for c_lo, r_hi in ((100.0, math.inf), (1.0, 2.0 ** -3), (5000.0, 1.0), (100.0, 2.0 ** -20)):
        _same_line(sar.corrdim_fit(hist, None, c_lo, r_hi), X.fit(hist, c_lo, r_hi))
    kw = dict(sub_bits=4, e_min=-40, e_max=2)
    h2 = rng.integers(0, 50, size=X.n_bins(**kw)).astype(np.uint64)
    _same_line(sar.corrdim_fit(h2, sar.pairs_params(**kw), 10.0, 0.75), X.fit(h2, 10.0, 0.75, **kw))


def test_fit_recovers_a_power_law(sar):
    r = sar.pair_edges()
    c = np.rint(1e4 * (r[:-1] / r[120]) ** 1.5)               # C_b = r_b^1.5 up to a factor, rounded to integers
    c[:120] = 0                                                # ... from 10^4 upwards
    hist = np.zeros(290, dtype=np.uint64)
    hist[:-1] = np.diff(np.concatenate([[0.0], c])).astype(np.uint64)
    line = sar.corrdim_fit(hist, None, 1e4, math.inf)
    assert line["status"] == sar.SAR_CORRDIM_FIT_OK and line["first_bin"] == 120 and line["last_bin"] == 288
    assert abs(line["slope"] - 1.5) < 1e-3 and line["rms"] < 1e-3
    assert abs(X.fit(hist, 1e4)["slope"] - 1.5) < 1e-3


def test_no_window(sar):
    hist = np.zeros(290, dtype=np.uint64)
    for h in (hist, np.where(np.arange(290) == 100, 5, 0).astype(np.uint64)):
        line = sar.corrdim_fit(h)
        assert line["status"] == sar.SAR_CORRDIM_NO_WINDOW and line["used"] == 0 and math.isnan(line["slope"]) and math.isnan(line["rms"])
    hist[100:102] = 500                                        # two bins below r_hi: still fewer than three
    line = sar.corrdim_fit(hist, None, 100.0, float(sar.pair_edges()[101]))
    assert line["status"] == sar.SAR_CORRDIM_NO_WINDOW
    _same_line(line, X.fit(hist, 100.0, float(sar.pair_edges()[101])))
    line = sar.corrdim_fit(hist, None, 100.0, float(sar.pair_edges()[102]))
    assert line["status"] == sar.SAR_CORRDIM_FIT_OK and line["used"] == 3 and line["first_bin"] == 100


def test_fit_refusals(sar):
    hist = np.ones(290, dtype=np.uint64)
    for c_lo, r_hi, text in ((0.5, 1.0, "c_lo"), (math.nan, 1.0, "c_lo"), (100.0, 0.0, "r_hi"), (100.0, math.nan, "r_hi"), (100.0, -1.0, "r_hi")):
        with pytest.raises(sar.SarError):
            sar.corrdim_fit(hist, None, c_lo, r_hi)
        assert text in sar.load_library().sar_last_error().decode()
    with pytest.raises(ValueError):
        sar.corrdim_fit(hist[:-1])
    with pytest.raises(sar.SarError):
        sar.pair_edges(sar.pairs_params(sub_bits=5))


@pytest.mark.parametrize("change,text", K.PAIRS_REFUSED)
def test_pairs_refusals_need_no_device(sar, change, text):
    change = dict(change)
    n = change.pop("n", 10)
    p = sar.pairs_params(**change)
    pts = np.zeros((min(max(n, 1), 16), 3))                    # (refused before the points are read)
    hist = np.zeros(1024, dtype=np.uint64)
    lib = sar.load_library()
    assert lib.sar_runtime_pairs(None, C.byref(p), 1, n, pts.ctypes.data_as(C.POINTER(C.c_double)),
                                 hist.ctypes.data_as(C.POINTER(C.c_uint64)), None) == 1
    assert text in lib.sar_last_error().decode()
    assert not hist.any()


def test_a_nan_coordinate_is_refused_without_a_device(sar):
    pts = np.zeros((2, 5, 3))
    pts[1, 3, 2] = math.nan
    hist = np.zeros((2, 290), dtype=np.uint64)
    lib = sar.load_library()
    assert lib.sar_runtime_pairs(None, None, 2, 5, pts.ctypes.data_as(C.POINTER(C.c_double)), hist.ctypes.data_as(C.POINTER(C.c_uint64)), None) == 1
    assert "coordinate 2 of point 3 of set 1 is NaN" in lib.sar_last_error().decode()


@pytest.mark.parametrize("change,text", K.CORRDIM_REFUSED)
def test_corrdim_refusals_need_no_device(sar, change, text):
    p = sar.corrdim_params(**dict(dict(jobs=4, samples=4, stride=1, transient=10), **change))
    lib = sar.load_library()
    hist = np.zeros(1024, dtype=np.uint64)
    rec = np.zeros(1, dtype=sar.CORRDIM_RECORD_DTYPE)
    co = K.henon()
    assert lib.sar_runtime_corrdim(None, C.byref(p), 1, co.ctypes.data_as(C.POINTER(C.c_double)), None, hist.ctypes.data_as(C.POINTER(C.c_uint64)),
                                   rec.ctypes.data_as(C.POINTER(sar.api._abi.SarCorrdimRecord)), None) == 1
    assert text in lib.sar_last_error().decode()


def test_corrdim_refuses_coefficients_and_starts_that_are_not_finite(sar):
    p = sar.corrdim_params(jobs=2, samples=2, stride=1, transient=1)
    lib = sar.load_library()
    hist = np.zeros(290, dtype=np.uint64)
    rec = np.zeros(1, dtype=sar.CORRDIM_RECORD_DTYPE)
    args = (hist.ctypes.data_as(C.POINTER(C.c_uint64)), rec.ctypes.data_as(C.POINTER(sar.api._abi.SarCorrdimRecord)), None)
    co = K.henon()
    co[7] = math.inf
    assert lib.sar_runtime_corrdim(None, C.byref(p), 1, co.ctypes.data_as(C.POINTER(C.c_double)), None, *args) == 1
    assert "coefficients must be finite (map 0, entry 7)" in lib.sar_last_error().decode()
    st = np.zeros((2, 3))
    st[1, 0] = math.nan
    co = K.henon()
    assert lib.sar_runtime_corrdim(None, C.byref(p), 1, co.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_double)), *args) == 1
    assert "start points must be finite (job 1)" in lib.sar_last_error().decode()
