"""GPU: the basin probes (sar_runtime_basin_fates, sar_runtime_basin_uncertainty, include/sar.h) — every field of the fates, the
levels, the base fates and the masks against the numpy restatement bit for bit: fates at the sizes that run partial waves and
workgroup edges, the identity (a pixel's own start point has the pixel's fate), ladders at every group shape, independence of
`chunk`, the closed form, the solar-sail window, a grid = 1 picture, no side effect on the runtime or the picture, a reused runtime,
basin stability, and the refusals behind a runtime. tests/test_fate_host.py shows on the restatement that these inputs hold several
classes and few UNKNOWN probes."""
import ctypes as C

import numpy as np
import pytest

import basin_restatement as B
import fate_cases as K
import fate_restatement as F
from basin_cases import PITCHFORK, PITCHFORK_MU, PITCHFORK_WINDOW, preset_coeffs

pytestmark = pytest.mark.gpu


def _runtime(sar):
    return sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = _runtime(sar)
    yield r
    r.close()


def _held(sar, runtime, coeffs, box=None, **kw):
    """A basin picture on `runtime` and its restated held picture, from the device's own labels (tests/test_gpu_basin.py holds those
    to the restatement)."""
    b = sar.basin_map(runtime, coeffs, box=box, **kw)
    pic = F.picture(coeffs, box=(tuple(b.params.box_lo), tuple(b.params.box_hi)), status=b.status, label=b.label, **kw)
    return b, pic


@pytest.fixture(scope="module")
def held1(sar, gpu):
    """A runtime of its own that keeps holding the 33 x 17 pitchfork picture: the tests that use it compute no other picture on it."""
    r = _runtime(sar)
    b, pic = _held(sar, r, B.pitchfork(PITCHFORK_MU), **K.pitchfork_kw(1))
    yield r, b, pic
    r.close()


@pytest.fixture(scope="module")
def ladder1(held1):
    """The sweep's ladder restated once, at all 65 base points and 31 levels."""
    _, _, pic = held1
    base = K.window_points(PITCHFORK_WINDOW, K.LADDER["n"], K.LADDER["seed"])
    return base, F.ladder(pic, base, K.LADDER["dir"], K.LADDER["eps0"], K.LADDER["levels"])


def _same_fates(got, want):
    assert got.shape == want.shape
    for f in F.FATE_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (f, np.flatnonzero(got[f] != want[f])[:4], got[f][got[f] != want[f]][:4], want[f][got[f] != want[f]][:4])


def _same_ladder(u, want):
    assert u.levels.shape == want["levels"].shape
    assert np.array_equal(u.levels["eps"].view(np.uint64), want["levels"]["eps"].view(np.uint64))
    for f in ("tested", "uncertain", "unknown"):
        assert np.array_equal(u.levels[f], want["levels"][f]), (f, u.levels[f], want["levels"][f])
    _same_fates(u.fate0, want["fate0"])
    for f in F.MASK_DTYPE.names:
        assert np.array_equal(u.masks[f], want["masks"][f]), (f, np.flatnonzero(u.masks[f] != want["masks"][f])[:4])


@pytest.mark.parametrize("n", K.FATE_NS)
def test_fates_at_every_size(sar, held1, n):
    _, b, pic = held1
    pts = K.window_points(PITCHFORK_WINDOW, max(K.FATE_NS), 3)[:n]
    got = b.fates(pts)
    assert got.dtype == sar.BASIN_FATE_DTYPE and got.shape == (n,)
    _same_fates(got, F.fates(pic, pts))


@pytest.mark.parametrize("case", range(len(PITCHFORK)))
def test_identity_a_pixels_own_start_point_has_the_pixels_fate(sar, rt, case):
    kw = K.pitchfork_kw(case)
    b = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), **kw)
    starts = np.stack([b.start(x, y) for y in range(kw["height"]) for x in range(kw["width"])])
    f = b.fates(starts)
    pix = b.pixels.reshape(-1)
    for field in ("status", "escape_step", "label"):
        assert np.array_equal(f[field], pix[field]), field
    assert not f["hit"].any() and (f["status"] == sar.SAR_SEARCH_DIVERGED).sum() == PITCHFORK[case][3]
    assert np.all(f["label"][f["status"] == sar.SAR_SEARCH_DIVERGED] == sar.BASIN_NONE)


def _ladder_kw(levels=None, chunk=0):
    return dict(dir=K.LADDER["dir"], eps0=K.LADDER["eps0"], levels=K.LADDER["levels"] if levels is None else levels, chunk=chunk)


@pytest.mark.parametrize("levels", K.LADDER_KS)
def test_ladders_at_every_group_shape(sar, held1, ladder1, levels):
    r, _, pic = held1
    base, full = ladder1
    u = sar.basin_uncertainty(r, base, **_ladder_kw(levels))
    assert u.levels.dtype == sar.BASIN_LEVEL_DTYPE and u.masks.dtype == sar.BASIN_LADDER_MASK_DTYPE and len(u.levels) == levels
    _same_ladder(u, F.ladder(pic, base, K.LADDER["dir"], K.LADDER["eps0"], levels))
    # a shorter ladder is a prefix of the full one
    assert np.array_equal(u.levels["uncertain"], full["levels"]["uncertain"][:levels])
    assert np.array_equal(u.masks["uncertain_bits"], full["masks"]["uncertain_bits"] & np.uint32((1 << levels) - 1))
    if levels == K.LADDER["levels"]:
        assert list(u.levels["uncertain"]) == K.LADDER_UNCERTAIN


@pytest.mark.parametrize("n", K.LADDER_NS)
def test_ladders_at_every_count_of_base_points(sar, held1, ladder1, n):
    r, _, pic = held1
    base, _ = ladder1
    u = sar.basin_uncertainty(r, base[:n], **_ladder_kw(10))
    _same_ladder(u, F.ladder(pic, base[:n], K.LADDER["dir"], K.LADDER["eps0"], 10))
    assert np.all(u.levels["tested"] + u.levels["unknown"] == n)


def test_results_do_not_depend_on_the_chunk(sar, held1, ladder1):
    r, b, _ = held1
    base, full = ladder1
    r.enable_timing(True)
    try:
        got = {}
        for chunk, launches in ((1, 65), (3, 22), (0, 1), (64, 2), (2 ** 32 - 1, 1)):
            u = sar.basin_uncertainty(r, base, **_ladder_kw(10, chunk))
            t = r.last_timing()
            assert t.iterate_launches == launches and t.iterate_ms > 0, chunk          # k_basin_ladder's spans
            got[chunk] = (u.levels.tobytes(), u.fate0.tobytes(), u.masks.tobytes())
        assert all(v == got[0] for v in got.values())
        b.fates(base)
        t = r.last_timing()
        assert t.iterate_launches == 1 and t.iterate_ms > 0                            # k_basin_fate's span
    finally:
        r.enable_timing(False)
    u = sar.basin_uncertainty(r, base, **_ladder_kw(10))
    assert np.array_equal(u.levels["uncertain"], full["levels"]["uncertain"][:10])


def test_closed_form(sar, rt):
    b, pic = _held(sar, rt, K.closed_map(), box=K.CLOSED_BOX, **K.CLOSED_KW)
    u = b.uncertainty(points=K.closed_base(), direction=K.CLOSED["dir"], eps0=K.CLOSED["eps0"], levels=K.CLOSED["levels"])
    _same_ladder(u, F.ladder(pic, K.closed_base(), K.CLOSED["dir"], K.CLOSED["eps0"], K.CLOSED["levels"]))
    assert list(u.levels["uncertain"]) == K.CLOSED_UNCERTAIN and not u.levels["unknown"].any() and np.all(u.levels["tested"] == 1024)
    fit = u.fit(min_uncertain=1, f_max=1.0)
    assert abs(fit.alpha - 1.0) < 1e-12 and list(fit.levels) == list(range(1, 11)) and abs(u.boundary_dimension(1, min_uncertain=1, f_max=1.0)) < 1e-12


def test_solar_sail_window(sar, rt):
    b, pic = _held(sar, rt, preset_coeffs(sar, "solar_sail"), **K.SOLAR_KW)
    base = K.window_points(K.SOLAR_KW, K.SOLAR["n"], K.SOLAR["seed"])
    u = sar.basin_uncertainty(rt, base, dir=K.SOLAR["dir"], eps0=K.SOLAR["eps0"], levels=K.SOLAR["levels"])
    _same_ladder(u, F.ladder(pic, base, K.SOLAR["dir"], K.SOLAR["eps0"], K.SOLAR["levels"]))
    pts = K.window_points(K.SOLAR_KW, 257, 5)
    pts[:, 2] += np.linspace(-0.2, 0.2, 257)                                        # off the plane
    _same_fates(b.fates(pts), F.fates(pic, pts))
    # the defaults of BasinMap.uncertainty: du normalised, |du| / 8, 24 levels, base points of default_rng(seed) on the plane
    d = b.uncertainty(n=33, seed=4)
    assert (list(d.params.dir), d.params.eps0, d.params.levels) == ([1.0, 0.0, 0.0], 0.125, 24)
    assert np.array_equal(d.base, K.window_points(K.SOLAR_KW, 33, 4))
    _same_ladder(d, F.ladder(pic, d.base, (1.0, 0.0, 0.0), 0.125, 24))


def test_a_grid_1_picture(sar, rt):
    b, pic = _held(sar, rt, B.pitchfork(PITCHFORK_MU), box=B.UNIT_BOX, **K.GRID1_KW)
    base = K.window_points(PITCHFORK_WINDOW, K.GRID1["n"], K.GRID1["seed"])
    u = sar.basin_uncertainty(rt, base, dir=K.GRID1["dir"], eps0=K.GRID1["eps0"], levels=K.GRID1["levels"])
    _same_ladder(u, F.ladder(pic, base, K.GRID1["dir"], K.GRID1["eps0"], K.GRID1["levels"]))
    f = b.fates(base)
    bounded = f["status"] == sar.SAR_SEARCH_BOUNDED
    assert bounded.any() and (~bounded).any() and not f["label"][bounded].any() and not f["hit"].any()   # escape versus stay


def test_the_runtime_and_the_picture_are_only_lent(sar, rt):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    b = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), **K.pitchfork_kw(1))
    img = b.colorize(cfg)
    pts = K.window_points(PITCHFORK_WINDOW, 300, 7)
    first = b.fates(pts)
    b.uncertainty(n=40, levels=10)
    b.stability(n=100)
    assert np.array_equal(b.colorize(cfg), img)                                      # the picture's records and labels are untouched
    assert b.fates(pts).tobytes() == first.tobytes()
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    rt.reset()


def test_one_runtime_through_two_pictures(sar, gpu):
    r = _runtime(sar)
    try:
        c = B.pitchfork(PITCHFORK_MU)
        a, pic_a = _held(sar, r, c, **K.pitchfork_kw(1))
        pts = K.window_points(PITCHFORK_WINDOW, 700, 11)
        _same_fates(a.fates(pts), F.fates(pic_a, pts))
        _same_ladder(a.uncertainty(points=pts[:22], levels=10), F.ladder(pic_a, pts[:22], (1.0, 0.0, 0.0), 0.5, 10))
        b, pic_b = _held(sar, r, c, **K.pitchfork_kw(0))                             # another size and grid: the table is uploaded anew
        assert (b.params.grid, a.params.grid) == (16, 8)
        _same_fates(b.fates(pts[:3]), F.fates(pic_b, pts[:3]))
        _same_fates(b.fates(pts[:257]), F.fates(pic_b, pts[:257]))
        _same_ladder(b.uncertainty(points=pts[:65], levels=21), F.ladder(pic_b, pts[:65], (1.0, 0.0, 0.0), 0.5, 21))
        with pytest.raises(ValueError):
            a.fates(pts[:3])                                                         # the runtime holds b's picture now
    finally:
        r.close()


def test_stability_counts(sar, held1):
    _, b, pic = held1
    for box in (None, ((-1.5, -0.25, -0.5), (1.5, 1.0, 0.5))):
        s = b.stability(n=500, box=box, seed=9)
        assert s.points.shape == (500, 3)
        if box is None:
            assert np.array_equal(s.points, K.window_points(PITCHFORK_WINDOW, 500, 9))
        else:
            assert np.all(s.points >= np.array(box[0])) and np.all(s.points < np.array(box[1])) and np.ptp(s.points[:, 2]) > 0.5
        want = F.fates(pic, s.points)
        _same_fates(s.fates, want)
        cls = F.classes(want)
        counts = [int((cls == k).sum()) for k in range(b.n_attractors)] + [int((cls == F.NONE).sum()), int((cls == F.UNKNOWN).sum())]
        assert list(s.counts) == counts and sum(counts) == 500 and (s.escaped, s.unknown) == (counts[-2], counts[-1])
        assert np.allclose(s.share, np.array(counts) / 500.0, rtol=0, atol=1e-15)
        assert np.allclose(s.stderr, np.sqrt(s.share * (1.0 - s.share) / 500.0), rtol=0, atol=1e-15)
        assert counts[0] > 0 and counts[1] > 0 and counts[-2] > 0
    # the counts the entry itself returns
    cnt = sar._abi.SarBasinFateCounts()
    pts = np.ascontiguousarray(s.points)
    out = np.empty(500, dtype=sar.BASIN_FATE_DTYPE)
    assert sar.load_library().sar_runtime_basin_fates(held1[0].handle, 500, pts.ctypes.data_as(C.POINTER(C.c_double)),
                                                      out.ctypes.data_as(C.POINTER(sar._abi.SarBasinFate)), C.byref(cnt)) == 0
    assert (cnt.points, cnt.diverged, cnt.unknown, cnt.labelled) == (500, counts[-2], counts[-1], sum(counts[:-2]))


def test_refusals_with_a_runtime(sar, gpu):
    lib = sar.load_library()
    r = _runtime(sar)
    try:
        pts = K.window_points(PITCHFORK_WINDOW, 8, 1)
        for call in (lambda: sar.basin_fates(r, pts), lambda: sar.basin_uncertainty(r, pts)):      # no picture yet
            with pytest.raises(sar.SarError):
                call()
            assert "holds no basin picture" in lib.sar_last_error().decode()
        c = B.pitchfork(PITCHFORK_MU)
        old = sar.basin_map(r, c, **K.pitchfork_kw(1))
        assert len(old.fates(pts)) == 8
        box = (tuple(old.params.box_lo), tuple(old.params.box_hi))
        with pytest.raises(sar.SarError):
            sar.basin_map(r, c, box=box, **dict(K.pitchfork_kw(1), grid=0))                        # a basin call that fails
        for call in (lambda: sar.basin_fates(r, pts), lambda: sar.basin_uncertainty(r, pts)):
            with pytest.raises(sar.SarError):
                call()
            assert "holds no basin picture" in lib.sar_last_error().decode()
        with pytest.raises(ValueError):
            old.fates(pts)                                                                          # and the object knows it is stale
        new = sar.basin_map(r, c, **K.pitchfork_kw(1))
        assert new.fates(pts).tobytes() == sar.basin_fates(r, pts).tobytes()
        for stale in (old.fates, lambda p: old.uncertainty(points=p), lambda p: old.stability(n=4)):
            with pytest.raises(ValueError):
                stale(pts)
        # refused arguments behind a runtime leave the picture held
        bad = pts.copy()
        bad[5, 2] = np.nan
        with pytest.raises(sar.SarError):
            new.fates(bad)
        assert "must be finite (point 5)" in lib.sar_last_error().decode()
        with pytest.raises(sar.SarError):
            new.uncertainty(points=pts, levels=32)
        with pytest.raises(sar.SarError):
            new.uncertainty(points=pts, eps0=0.0)
        assert len(new.fates(pts)) == 8
    finally:
        r.close()
