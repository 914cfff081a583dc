"""Host: the power spectra without a device (include/sar.h: sar_spectra_*, sar_spectrum_*) — the library's twiddle and window tables
against the restatement's bit for bit, the defaults, sar_spectra_segments and every refusal with a piece of its text; then the
restatement itself: against np.fft.rfft, against Parseval's identity, on maps whose spectra are known (a rotation, the logistic
map's cycles, chaos) and on the planted series."""
import ctypes as C
import math

import numpy as np
import pytest

import spectrum_cases as K
import spectrum_restatement as S

SIZES = [2 ** k for k in range(3, 13)]
LINES_SHAPE = dict(segments=7, n=256, hop=128, transient=2000)      # 8 jobs
BROAD_SHAPE = dict(segments=15, n=256, hop=128, transient=2000)     # 16 jobs


def _error(sar) -> str:
    return sar.load_library().sar_last_error().decode()


def test_tables_equal_the_restatement(sar):
    for n in SIZES:
        assert sar.spectrum_twiddles(n).tobytes() == S.twiddles(n).tobytes(), n
        for name, kind in (("rect", S.RECT), ("hann", S.HANN)):
            assert sar.spectrum_window(name, n).tobytes() == S.window(kind, n).tobytes(), (n, name)
    tw = sar.spectrum_twiddles(8)
    assert tw[0].tolist() == [1.0, 0.0] and math.copysign(1.0, tw[0, 1]) == -1.0      # -sin(0) is -0.0
    assert np.all(sar.spectrum_window("rect", 16) == 1.0) and sar.spectrum_window("hann", 16)[0] == 0.0
    assert sar.spectrum_window("hann", 16)[8] == 1.0
    for bad in (0, 4, 12, 8192):
        with pytest.raises(sar.SarError):
            sar.spectrum_twiddles(bad)
        assert "power of two" in _error(sar)
        with pytest.raises(sar.SarError):
            sar.spectrum_window("hann", bad)
    with pytest.raises(sar.SarError):
        sar.spectrum_window(2, 8)
    assert "window" in _error(sar)
    with pytest.raises(ValueError):
        sar.spectrum_window("welch", 8)
    lib = sar.load_library()
    assert lib.sar_spectrum_twiddles(8, None) == 1 and lib.sar_spectrum_window(0, 8, None) == 1


def test_defaults(sar):
    p = sar.spectra_params()
    assert (p.n, p.hop, p.window, p.samples, p.chunk, list(p.proj)) == (1024, 512, sar.SAR_WINDOW_HANN, 0, 0, [1.0, 0.0, 0.0])
    q = sar.spectrum_params()
    assert (q.jobs, q.segments, q.n, q.hop, q.window, q.stride, q.transient, q.chunk, q.seed, q.bound, list(q.proj)) == \
        (16, 15, 1024, 512, sar.SAR_WINDOW_HANN, 1, 1000, 0, 0, 1e6, [1.0, 0.0, 0.0])
    assert sar.spectra_params(n=64, hop=None).hop == 32 and sar.spectrum_params(n=8, hop=None, window="rect").window == sar.SAR_WINDOW_RECT
    assert C.sizeof(type(p)) == 48 and C.sizeof(type(q)) == 72
    assert sar.SPECTRA_RECORD_DTYPE.itemsize == 16 and sar.SPECTRUM_RECORD_DTYPE.itemsize == 80
    lib = sar.load_library()
    assert lib.sar_spectra_params_default(None) == 1 and lib.sar_spectrum_params_default(None) == 1


def test_segments(sar):
    assert sar.spectra_segments(1024) == (1, 1) and sar.spectra_segments(8192) == (1, 15)
    assert sar.spectra_segments(16, n=8, hop=4) == (1, 3) and sar.spectra_segments(19, n=8, hop=4) == (1, 3)      # a tail of 3
    assert sar.spectra_segments(48, n=8, hop=1, samples=12) == (4, 5) and sar.spectra_segments(48, n=8, hop=8, samples=8) == (6, 1)
    assert sar.spectra_segments(45, n=8, hop=3, samples=15) == (3, 3)
    assert sar.spectra_segments(2 ** 20, n=4096, hop=4096, samples=2 ** 16) == (16, 16)
    for samples, n, hop in ((8, 8, 8), (100, 16, 5), (4096, 64, 1), (37, 32, 32)):
        assert sar.spectra_segments(samples, n=n, hop=hop)[1] == S.n_segments(samples, n, hop)
    lib = sar.load_library()
    jobs = C.c_uint32()
    assert lib.sar_spectra_segments(None, 2048, C.byref(jobs), None) == 0 and jobs.value == 1      # NULL: the defaults


@pytest.mark.parametrize("change,text", K.SPECTRA_REFUSED)
def test_spectra_refusals(sar, change, text):
    kw = dict(n=8, hop=4, window="hann", samples=0, chunk=0, proj=(1.0, 0.0, 0.0), n_points=16)
    kw.update(change)
    n_points = kw.pop("n_points")
    with pytest.raises(sar.SarError):
        sar.spectra_segments(n_points, **kw)
    assert text in _error(sar), _error(sar)
    # the same from sar_runtime_spectra, before it looks at the runtime or the points
    p = sar.spectra_params(**kw)
    assert sar.load_library().sar_runtime_spectra(None, C.byref(p), 1, n_points, None, None, None) == 1
    assert text in _error(sar), _error(sar)


def test_spectra_refuse_what_is_not_finite_and_take_nothing(sar):
    lib = sar.load_library()
    p = sar.spectra_params(n=8, hop=4)
    power = np.full((2, 5), 7.0)
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    for bad in (math.nan, math.inf, -math.inf):
        pts = np.zeros((2, 16, 3))
        pts[1, 9, 2] = bad
        assert lib.sar_runtime_spectra(None, C.byref(p), 2, 16, ptr(pts), ptr(power), None) == 1
        assert "not finite" in _error(sar) and "point 9 of set 1" in _error(sar)
    assert lib.sar_runtime_spectra(None, C.byref(p), 0, 16, None, None, None) == 0      # no sets: nothing to do, no runtime needed
    assert lib.sar_runtime_spectra(None, C.byref(p), 1, 16, None, ptr(power), None) == 1 and "NULL" in _error(sar)
    assert lib.sar_runtime_spectra(None, C.byref(p), 1, 16, ptr(np.zeros((16, 3))), ptr(power), None) == 1 and "runtime" in _error(sar)
    assert np.all(power == 7.0)


def _spectrum_call(sar, p, coeffs, starts=None):
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))
    from strange_attractor_renderer_amd import _abi
    power = np.zeros((1, 4097))
    recs = np.zeros(1, dtype=sar.SPECTRUM_RECORD_DTYPE)
    return sar.load_library().sar_runtime_spectrum(None, C.byref(p), 1, ptr(coeffs), ptr(starts), ptr(power),
                                                   recs.ctypes.data_as(C.POINTER(_abi.SarSpectrumRecord)), None)


@pytest.mark.parametrize("change,text", K.SPECTRUM_REFUSED)
def test_spectrum_refusals(sar, change, text):
    kw = dict(jobs=2, segments=3, n=8, hop=4, stride=1, transient=10, bound=1e6)
    kw.update(change)
    assert _spectrum_call(sar, sar.spectrum_params(**kw), K.henon()) == 1
    assert text in _error(sar), _error(sar)


def test_spectrum_refuses_what_is_not_finite_and_takes_nothing(sar):
    p = sar.spectrum_params(jobs=2, segments=3, n=8, hop=4, transient=10)
    for bad in (math.nan, math.inf):
        c = K.henon()
        c[17] = bad
        assert _spectrum_call(sar, p, c) == 1 and "coefficients must be finite" in _error(sar)
        starts = np.full((2, 3), 0.1)
        starts[1, 0] = bad
        assert _spectrum_call(sar, p, K.henon(), starts) == 1 and "start points must be finite" in _error(sar)
    lib = sar.load_library()
    assert lib.sar_runtime_spectrum(None, C.byref(p), 0, None, None, None, None, None) == 0      # no maps: nothing to do
    assert lib.sar_runtime_spectrum(None, None, 1, None, None, None, None, None) == 1 and "parameters" in _error(sar)
    assert lib.sar_runtime_spectrum(None, C.byref(p), 1, None, None, None, None, None) == 1 and "NULL" in _error(sar)
    assert _spectrum_call(sar, p, K.henon()) == 1 and "runtime" in _error(sar)


# ---- the restatement itself ---------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def henon_series():
    """One Henon trajectory of 4096 + 2048 recorded x values."""
    status, _, _, pts = S.CR.record_points(K.henon(), K.unit_starts(1), 6144, 1, 1000)
    assert status == S.BOUNDED
    return pts[:, 0].copy()


def _bound(n):
    return 32.0 * math.log2(n) * 2.0 ** -53


@pytest.mark.parametrize("kind", [S.RECT, S.HANN])
@pytest.mark.parametrize("n", SIZES)
def test_restatement_against_rfft(henon_series, n, kind):
    """The radix-2 error bound is about 6 log2(N) eps for the amplitudes, twice that for a square, plus the tree sums; measured
    5e-16 of the largest bin at most."""
    v = henon_series[:n]
    pts = np.zeros((n, 3))
    pts[:, 0] = v
    power, energy, jobs, segs = S.spectra(pts, n=n, hop=n, kind=kind)
    assert (jobs, segs) == (1, 1) and power.shape == (n // 2 + 1,)
    a = (v - np.mean(v)) * S.window(kind, n)
    want = np.abs(np.fft.rfft(a)) ** 2
    err = float(np.max(np.abs(power - want)) / np.max(want))
    print("rfft", n, kind, err)
    assert err <= _bound(n)
    assert abs(energy - float(np.sum(a * a))) <= _bound(n) * energy


@pytest.mark.parametrize("kind", [S.RECT, S.HANN])
@pytest.mark.parametrize("n", [8, 64, 1024, 4096])
def test_parseval(henon_series, n, kind):
    pts = np.zeros((henon_series.size, 3))
    pts[:, 0] = henon_series
    power, energy, _, segs = S.spectra(pts, n=n, hop=n // 2, kind=kind)
    assert segs == (6144 - n) // (n // 2) + 1
    c = np.full(n // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    gap = abs(float(np.sum(c * power)) / (n * energy) - 1.0)
    print("parseval", n, kind, gap)
    assert gap <= _bound(n)


@pytest.fixture(scope="module")
def line_spectra():
    """(map name, window) -> power of the periodic maps at LINES_SHAPE with 8 jobs."""
    starts = K.unit_starts(8)
    maps = dict(rotation=K.rotation(), l32=K.logistic_map(3.2), l35=K.logistic_map(3.5))
    out = {}
    for name, c in maps.items():
        for kind in (S.RECT, S.HANN):
            r = S.spectrum(c, starts, kind=kind, **LINES_SHAPE)
            assert r["status"] == S.BOUNDED and r["segments"] == 7
            out[name, kind] = r["power"]
    return out


def _share(power, bins):
    return float(np.sum(power[list(bins)]) / np.sum(power))


def test_a_rotation_is_one_line(line_spectra):
    for kind, bins in ((S.RECT, [37]), (S.HANN, [36, 37, 38])):
        p = line_spectra["rotation", kind]
        assert int(np.argmax(p)) == K.ROTATION_BIN and _share(p, bins) >= 0.999, kind


def test_the_logistic_cycles_are_subharmonic_lines(line_spectra):
    assert _share(line_spectra["l32", S.RECT], [128]) >= 0.999
    assert _share(line_spectra["l35", S.RECT], [64, 128]) >= 0.999
    assert _share(line_spectra["l35", S.HANN], [63, 64, 65, 127, 128]) >= 0.999
    assert line_spectra["l35", S.RECT][64] > 0.0 and line_spectra["l32", S.RECT][64] <= 1e-20 * line_spectra["l32", S.RECT][128]
    for name in ("rotation", "l32", "l35"):
        assert S.flatness(line_spectra[name, S.RECT]) <= 1e-6, name


def test_chaos_is_broadband():
    starts = K.unit_starts(16)
    for c in (K.henon(), K.logistic_map(3.9)):
        r = S.spectrum(c, starts, **BROAD_SHAPE)
        assert r["status"] == S.BOUNDED
        p = r["power"]
        print("broadband", float(np.max(p) / np.sum(p)), S.flatness(p))
        assert np.max(p) <= 0.1 * np.sum(p) and S.flatness(p) >= 0.5


def test_a_map_that_leaves_has_no_spectrum():
    r = S.spectrum(K.logistic_map(4.5), K.unit_starts(4), segments=3, n=8, hop=4, transient=50)
    assert r["status"] == S.DIVERGED and r["segments"] == 0 and r["energy"] == 0.0 and r["fail_step"] > 0
    assert not r["power"].view(np.uint64).any()


def _planted(name):
    series, kw = K.planted_series()[name]
    pts = np.zeros((series.size, 3))
    pts[:, 0] = series
    return S.spectra(pts, n=kw["n"], hop=kw["hop"], kind=dict(rect=S.RECT, hann=S.HANN)[kw["window"]])


def test_planted_series():
    power, energy, jobs, segs = _planted("constant")
    assert (jobs, segs) == (1, 4) and not power.view(np.uint64).any() and energy == 0.0 and not math.copysign(1.0, energy) < 0
    power, energy, _, segs = _planted("alternating")
    assert segs == 2 and power.tolist() == [0.0, 0.0, 0.0, 0.0, 128.0] and energy == 16.0
    power, energy, _, segs = _planted("subnormals")
    assert segs == 3 and np.all(np.isfinite(power)) and np.all(power >= 0.0) and energy >= 0.0
    power, energy, _, _ = _planted("minus zero")
    assert not power.view(np.uint64).any() and energy == 0.0
    power, energy, _, _ = _planted("1e200")
    assert np.isinf(power).any() and not np.isnan(power).any() and energy == math.inf
    power, energy, _, _ = _planted("1.7e308")
    assert np.isnan(power).all() and energy == math.inf      # the mean is infinite: every a_t is -inf
