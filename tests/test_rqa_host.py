"""Host: the recurrence analysis without a device (include/sar.h: sar_recurrence_*, sar_rqa_*) — the restatement held to closed forms
(a constant set, tiled points, two alternating points), to the identities between its counts and to corr_restatement's cumulative
pair count at a bin edge; sar_rqa_measures through ctypes against the restatement's; the defaults and every refusal that needs no
device, with a piece of its text; and the conditions that keep the GPU cases honest, asserted on the restatement alone."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import corr_restatement as CR
import rqa_cases as K
import rqa_restatement as R

NO_RUNTIME = types.SimpleNamespace(handle=None, device=0)      # every refusal below comes before the runtime is looked at


def _error(sar) -> str:
    return sar.load_library().sar_last_error().decode()


def _same_lines(got, want, what):
    assert np.array_equal(got[0], want[0]), (what, "diag", got[0].tolist(), want[0].tolist())
    assert np.array_equal(got[1], want[1]), (what, "vert", got[1].tolist(), want[1].tolist())
    assert got[2] == want[2], (what, got[2], want[2])


@pytest.mark.parametrize("t,w,bins", [(1, 0, 4), (2, 0, 4), (9, 0, 256), (9, 3, 256), (9, 8, 4), (9, 20, 4), (40, 1, 8), (40, 5, 2)])
def test_a_constant_set(t, w, bins):
    pts = np.full((t, 3), 0.375)
    _same_lines(R.lines(pts, 1e-9, theiler=w, line_bins=bins), K.constant_lines(t, w, bins), (t, w, bins))
    diag, vert, c = R.lines(pts, 1e-9, theiler=w, line_bins=bins)
    assert diag[0] == 0 and vert[0] == 0 and c["recurrences"] == c["pairs"]      # everything outside the band recurs
    if t > w + 1:
        assert c["diag_longest"] == t - w - 1 == c["vert_longest"] and R.measures(diag, vert, c, 1, 1)["rr"] == 1.0


@pytest.mark.parametrize("t,p,w,bins", [(30, 7, 0, 256), (30, 7, 6, 256), (23, 5, 2, 8), (50, 3, 1, 256), (15, 2, 0, 256), (17, 2, 1, 4)])
def test_tiled_points(t, p, w, bins):
    assert t % p                                               # T is no multiple of p
    got = R.lines(K.tiled_points(t, p), 0.25, theiler=w, line_bins=bins)
    _same_lines(got, K.tiled_lines(t, p, w, bins), (t, p, w, bins))
    diag, vert, c = got
    assert vert[1] == c["vert_lines"] == 2 * c["recurrences"] and c["vert_longest"] == 1      # all vertical lines have length 1
    m = R.measures(diag, vert, c)
    # DET = 1 unless the last line, on the largest multiple of p below T, has length 1
    assert m["det"] == (1.0 if t % p != 1 else (c["recurrences"] - 1) / c["recurrences"])
    assert m["lam"] == 0.0 and m["l_max"] == t - p and math.isnan(m["tt"])


def test_two_alternating_points():
    pts = K.tiled_points(11, 2)
    diag, vert, c = R.lines(pts, 0.25, line_bins=16)
    assert [int(v) for v in np.nonzero(diag)[0]] == [1, 3, 5, 7, 9] and diag.sum() == 5      # k = 2, 4, .., 10: lengths 9, 7, .., 1
    assert c == dict(recurrences=25, pairs=55, diag_lines=5, vert_lines=50, diag_longest=9, vert_longest=1)
    assert not R.matrix(pts, 0.25)[0, 1] and R.matrix(pts, 0.25)[0, 2] and not R.matrix(pts, 0.25, theiler=2)[0, 2]


def test_the_matrix_at_its_edges():
    infs, kw = K.planted_sets()["infinities"]
    r = R.matrix(infs, kw["eps2"])
    assert not r[1].any() and not r[:, 4].any() and not r[3].any() and r[0, 2] and np.array_equal(r, r.T)
    sub, _ = K.planted_sets()["subnormals"]
    r = R.matrix(sub, 5e-324)
    assert r[0, 1] and r[0, 2] and r[2, 3] and r[0, 4] and not r[6, 7] and not r[0, 0]      # r2 underflows to 0: recurrent
    assert not r[0, 5] and not r[4, 5] and R.matrix(sub, 1e-320)[4, 5]                 # r2 = 5e-324, the smallest double, is not below it
    lattice, _ = K.planted_sets()["lattice, eps2 = 1"]
    assert R.matrix(lattice, 1.0).sum() == 2 and R.matrix(lattice, 1.0)[0, 6]                     # only the point met twice
    assert R.matrix(lattice, math.nextafter(1.0, 2.0))[0, 1] and not R.matrix(lattice, math.nextafter(1.0, 2.0))[0, 2]
    zeros, _ = K.planted_sets()["minus zero"]
    assert R.matrix(zeros, 1e-300).sum() == 30


@pytest.fixture(scope="module")
def random_reference():
    """The restatement of the random sets at every shape, first set only, computed once and left unchanged."""
    out = []
    for t, jobs, sets, w, bins in K.SHAPES:
        pts = K.noisy_cycle(t, jobs, sets)[0]
        out.append((pts, R.lines(pts, K.EPS2, t, w, bins)))
    return out


def test_identities(random_reference):
    for (t, jobs, sets, w, bins), (pts, (diag, vert, c)) in zip(K.SHAPES, random_reference):
        l = np.arange(bins + 1, dtype=np.uint64)
        assert diag[0] == 0 and vert[0] == 0 and diag.sum() == c["diag_lines"] and vert.sum() == c["vert_lines"]
        if c["diag_longest"] <= bins:                             # nothing clamps
            assert int((l * diag).sum()) == c["recurrences"], (t, w)
        else:
            assert int((l * diag).sum()) < c["recurrences"] and diag[bins] > 0
        if c["vert_longest"] <= bins:
            assert int((l * vert).sum()) == 2 * c["recurrences"], (t, w)
        assert c["pairs"] == jobs * sum(t - k for k in range(w + 1, t)) and c["recurrences"] <= c["pairs"]
        if t <= w + 1:
            assert not diag.any() and not vert.any() and not any(c.values())


@pytest.mark.parametrize("t,jobs,w,e", [(120, 1, 0, -10), (120, 1, 3, -8), (60, 3, 0, -10), (40, 3, 2, -6)])
def test_recurrences_are_the_cumulative_pair_count_at_a_bin_edge(t, jobs, w, e):
    """eps2 = 2^e is the upper edge of bin e - e_min at sub_bits 0, and a bin holds r2 below its upper edge: the pairs of one
    trajectory closer than eps are the histogram's cumulative count through that bin; with several trajectories the histogram also
    counts the pairs between them."""
    pts = K.noisy_cycle(t, jobs, 1, seed=31)[0]
    eps2 = 2.0 ** e
    _, _, c = R.lines(pts, eps2, t, w, 256)
    hist, counted, _ = CR.pair_hist(pts, t, w, sub_bits=0, e_min=-64, e_max=8)
    traj = np.arange(jobs * t) // t
    d = pts[None, :, :] - pts[:, None, :]
    r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    across = int(np.triu((r2 < eps2) & (traj[:, None] != traj[None, :]), 1).sum())
    assert c["recurrences"] > 0 and (jobs == 1) == (across == 0)
    assert c["recurrences"] + across == int(hist[:e + 64 + 1].sum())
    assert c["pairs"] + jobs * (jobs - 1) // 2 * t * t == counted


def test_the_gpu_cases_are_honest(random_reference):
    """What the random sets must hold for the GPU comparison to mean something. RR is asked of the shapes with at least 63 points
    whose Theiler window leaves pairs: below that a trajectory has at most three pairs and RR is 0, 1/3, .. or undefined."""
    clamps = ends = 0
    for (t, jobs, sets, w, bins), (pts, (diag, vert, c)) in zip(K.SHAPES, random_reference):
        if t < 63 or t <= w + 1:
            continue
        rr = c["recurrences"] / c["pairs"]
        assert 0.01 <= rr <= 0.5, (t, w, rr)
        clamps += c["diag_longest"] > bins
        ends += R.ends_at_the_end(pts, K.EPS2, t, w)
        if bins == 256:
            assert np.count_nonzero(diag) >= 5 and np.count_nonzero(vert) >= 3, (t, w, np.count_nonzero(diag), np.count_nonzero(vert))
    assert clamps >= 1 and ends >= 1


def _measures(sar, diag, vert, c, l_min, v_min):
    rec = np.zeros((), dtype=sar.RECURRENCE_RECORD_DTYPE)
    for k in R.COUNTS:
        rec[k] = c[k]
    return sar.rqa_measures(diag, vert, rec, l_min, v_min)


def test_measures_equal_the_restatement(sar, random_reference):
    seen = 0
    for (t, jobs, sets, w, bins), (_, (diag, vert, c)) in zip(K.SHAPES, random_reference):
        for l_min, v_min in ((1, 1), (2, 2), (2, bins), (bins, 1)):
            got, want = _measures(sar, diag, vert, c, l_min, v_min), R.measures(diag, vert, c, l_min, v_min)
            for k in ("rr", "det", "l_mean", "div", "lam", "tt"):
                assert np.float64(got[k]).tobytes() == np.float64(want[k]).tobytes() or (math.isnan(got[k]) and math.isnan(want[k])), (t, k)
            assert (int(got["l_max"]), int(got["v_max"])) == (want["l_max"], want["v_max"])
            # the C library's and numpy's log may differ in the last place; p log p <= 1 / e per class
            assert (math.isnan(got["entr"]) and math.isnan(want["entr"])) or abs(got["entr"] - want["entr"]) <= 1e-12, (t, got["entr"])
            seen += not math.isnan(want["entr"]) and want["entr"] > 0.0
    assert seen >= 10
    diag, vert, c = K.constant_lines(9, 0, 16)
    m = _measures(sar, diag, vert, c, 2, 2)
    assert m["rr"] == 1.0 and m["det"] == 35.0 / 36.0 and m["l_mean"] == 5.0 and m["l_max"] == 8 and m["div"] == 0.125
    assert abs(m["entr"] - math.log(7.0)) <= 1e-12 and m["lam"] == 70.0 / 72.0 and m["v_max"] == 8
    empty = _measures(sar, np.zeros(5, dtype=np.uint64), np.zeros(5, dtype=np.uint64), dict.fromkeys(R.COUNTS, 0), 2, 2)
    assert all(math.isnan(empty[k]) for k in ("rr", "det", "l_mean", "div", "entr", "lam", "tt")) and empty["l_max"] == 0


def test_measures_refusals(sar):
    diag, vert, c = K.constant_lines(9, 0, 4)
    for l_min, v_min in ((0, 2), (2, 0), (5, 2), (2, 5)):
        with pytest.raises(sar.SarError):
            _measures(sar, diag, vert, c, l_min, v_min)
        assert "l_min and v_min" in _error(sar)
    with pytest.raises(sar.SarError):
        _measures(sar, diag[:2], vert[:2], c, 1, 1)                  # line_bins = 1
    assert "line_bins" in _error(sar)
    lib = sar.load_library()
    assert lib.sar_rqa_measures(None, None, None, 4, 1, 1, None) == 1 and "NULL" in _error(sar)


def test_defaults(sar):
    p = sar.recurrence_params()
    assert (p.samples, p.theiler, p.line_bins, p.chunk, p.eps2) == (0, 0, 256, 0, 0.0)
    q = sar.rqa_params()
    assert (q.jobs, q.samples, q.stride, q.transient, q.seed, q.bound, q.theiler, q.line_bins, q.chunk, q.eps2, q.eps_fraction) == \
        (16, 1024, 1, 1000, 0, 1e6, 0, 256, 0, 0.0, 0.05)
    assert C.sizeof(type(p)) == 24 and C.sizeof(type(q)) == 64
    assert sar.RECURRENCE_RECORD_DTYPE.itemsize == 48 and sar.RQA_RECORD_DTYPE.itemsize == 120 and sar.RQA_MEASURES_DTYPE.itemsize == 72
    lib = sar.load_library()
    assert lib.sar_recurrence_params_default(None) == 1 and lib.sar_rqa_params_default(None) == 1
    with pytest.raises(ValueError):
        sar.recurrence_lines(NO_RUNTIME, np.zeros((4, 3)))           # neither eps nor eps2
    with pytest.raises(ValueError):
        sar.recurrence_lines(NO_RUNTIME, np.zeros((4, 3)), 0.1, eps2=0.01)


@pytest.mark.parametrize("change,text", K.RECURRENCE_REFUSED)
def test_recurrence_refusals(sar, change, text):
    kw = dict(n=12, samples=0, theiler=0, line_bins=4, chunk=0, eps2=1.0)
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.recurrence_lines(NO_RUNTIME, np.zeros((kw.pop("n"), 3)), **kw)
    assert text in _error(sar), _error(sar)


@pytest.mark.parametrize("change,text", K.PLOT_REFUSED)
def test_plot_refusals(sar, change, text):
    kw = dict(job=0, window=(0, 0, 6, 6))
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.recurrence_plot(NO_RUNTIME, np.zeros((12, 3)), eps2=1.0, samples=6, **kw)
    assert text in _error(sar), _error(sar)


@pytest.mark.parametrize("change,text", K.RQA_REFUSED)
def test_rqa_refusals(sar, change, text):
    from corr_cases import henon
    kw = dict(jobs=2, samples=8, stride=1, transient=10, bound=1e6)
    kw.update(change)
    with pytest.raises(sar.SarError):
        sar.recurrence_analysis(NO_RUNTIME, henon(), **kw)
    assert text in _error(sar), _error(sar)


def test_what_needs_no_device(sar):
    pts = np.zeros((2, 12, 3))
    pts[1, 5, 2] = math.nan
    with pytest.raises(sar.SarError):
        sar.recurrence_lines(NO_RUNTIME, pts, eps2=1.0)
    assert "is NaN" in _error(sar)
    with pytest.raises(sar.SarError):
        sar.recurrence_plot(NO_RUNTIME, pts[1], eps2=1.0)
    assert "is NaN" in _error(sar)
    pts[1, 5, 2] = math.inf                                          # infinities are taken: only the runtime is missing
    with pytest.raises(sar.SarError):
        sar.recurrence_lines(NO_RUNTIME, pts, eps2=1.0, theiler=2 ** 32 - 1)
    assert "runtime is NULL" in _error(sar)
    from corr_cases import henon
    c = henon()
    c[3] = math.inf
    with pytest.raises(sar.SarError):
        sar.recurrence_analysis(NO_RUNTIME, c, jobs=2, samples=8)
    assert "coefficients must be finite" in _error(sar)
    diag, vert = sar.recurrence_lines(NO_RUNTIME, np.zeros((0, 12, 3)), eps2=1.0, line_bins=4)      # no sets, no maps: nothing happens
    assert diag.shape == vert.shape == (0, 5)
    assert sar.recurrence_analysis(NO_RUNTIME, np.zeros((0, 30)), jobs=2, samples=8, line_bins=4).diag.shape == (0, 5)
