"""GPU: the Lyapunov planes (sar_runtime_plane, include/sar.h) — the records against the numpy restatement bit for bit in both
modes, the spectrum mode against sar_runtime_search on the same maps, an analytic diagonal plane, determinism across calls, launch
chunks and partial tiles, no side effect on the image buffers, the colours against a numpy restatement (and through a PNG), and
the path from a plane's hottest pixel to a framed render."""
import ctypes as C
import math
import os
import tempfile

import numpy as np
import pytest

import image_decode as D
import lyapunov_reference as L
import plane_restatement as P

pytestmark = pytest.mark.gpu

NOLIMIT = dict(min_lyapunov=-math.inf, min_ky_dim=-math.inf, keep_rejected=1)
RAW = ("status", "transient_done", "steps_done", "log2_exp", "mant")


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=64, height=64), device=0)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_raw(got, want):
    for f in RAW:
        g, w = got[f], want[f]
        if f == "mant":
            assert np.array_equal(_bits(g), _bits(w)), f
        else:
            assert np.array_equal(g.astype(np.int64), w.astype(np.int64)), f


def _base(sar, preset):
    cfg = getattr(sar.Config, preset)()
    return np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])


def _around(base, axes, d):
    return [(base[a] - d, base[a] + d) for a in axes]


@pytest.mark.parametrize("preset,axes,d", [("poisson_saturne", (0, 13), 0.08), ("solar_sail", (5, 22), 0.1)])
def test_l1_parity_with_the_restatement(sar, rt, preset, axes, d):
    base = _base(sar, preset)
    xr, yr = _around(base, axes, d)
    w, h, tr, steps = 48, 40, 1000, 2000
    pl = sar.lyapunov_plane(rt, base, axes, xr, yr, w, h, "l1", transient=tr, steps=steps)
    want = P.plane(base, axes, xr, yr, w, h, "l1", transient_steps=tr, steps=steps)
    _same_raw(pl.records, want)
    assert np.array_equal(_bits(pl.lyapunov), _bits(want["lyapunov"][..., 0]))
    assert np.all(np.isnan(pl.records["lyapunov"][..., 1:])) and np.all(np.isnan(pl.records["ky_dim"]))
    st = pl.stats
    assert st["pixels"] == w * h == st["bounded"] + st["degenerate"] + st["diverged_late"] + st["diverged_transient"]
    assert st["bounded"] == np.count_nonzero(want["status"] == P.BOUNDED) > 0
    assert st["diverged_transient"] == np.count_nonzero((want["status"] == P.DIVERGED) & (want["steps_done"] == 0))


def test_spectrum_equals_the_search(sar, rt):
    base = _base(sar, "poisson_saturne")
    axes = (3, 27)
    xr, yr = _around(base, axes, 0.15)
    w, h, tr, steps = 24, 20, 1000, 2000
    spec = sar.lyapunov_plane(rt, base, axes, xr, yr, w, h, "spectrum", transient=tr, steps=steps)
    cs = P.coeffs(base, axes, xr, yr, w, h).reshape(-1, 30)
    recs, stats = sar.search_attractors(rt, w * h, coeffs=cs, transient=tr, steps=steps, **NOLIMIT)
    flat = spec.records.reshape(-1)
    got = flat[recs["candidate"]]
    for f in ("status", "steps_done", "log2_exp"):
        assert np.array_equal(got[f].astype(np.int64), recs[f].astype(np.int64)), f
    for f in ("mant", "lyapunov", "ky_dim"):
        assert np.array_equal(_bits(got[f]), _bits(recs[f])), f
    dropped = np.setdiff1d(np.arange(w * h), recs["candidate"])
    assert dropped.size == stats["diverged_transient"] and recs.size > 0
    assert np.all(flat[dropped]["status"] == sar.SAR_SEARCH_DIVERGED) and np.all(flat[dropped]["steps_done"] == 0)
    assert np.all(flat[recs["candidate"]]["transient_done"] == tr)
    l1 = sar.lyapunov_plane(rt, base, axes, xr, yr, w, h, "l1", transient=tr, steps=steps).records.reshape(-1)
    b = recs[recs["status"] == sar.SAR_SEARCH_BOUNDED]
    assert b.size > 0
    assert np.array_equal(_bits(l1[b["candidate"]]["mant"][:, 0]), _bits(b["mant"][:, 0]))
    assert np.array_equal(l1[b["candidate"]]["log2_exp"][:, 0], b["log2_exp"][:, 0])


def test_analytic_diagonal_plane(sar, rt):
    a_, b_, c_ = 0.5, 0.7, 0.3
    base = L.affine_coeffs([[a_, 0, 0], [0, b_, 0], [0, 0, c_]], (0.01, 0.02, 0.03))
    axes, xr, yr = (1, 15), (-1.5, 1.5), (-0.9, 0.8)
    w, h, tr, steps, bound = 9, 6, 100, 500, 1e3
    kw = dict(transient=tr, steps=steps, bound=bound)
    spec = sar.lyapunov_plane(rt, base, axes, xr, yr, w, h, "spectrum", **kw)
    l1 = sar.lyapunov_plane(rt, base, axes, xr, yr, w, h, "l1", **kw)
    a = P.sweep(*xr, w)
    b = P.sweep(*yr, h)[::-1]
    assert a[w // 2] == 0.0 and np.any(np.abs(a) > 1)
    for pl in (spec, l1):
        assert np.all(pl.status[:, w // 2] == sar.SAR_SEARCH_DEGENERATE) and np.all(pl.records["steps_done"][:, w // 2] == 1)
        for xi in np.nonzero(np.abs(a) > 1)[0]:
            c = list(P.coeffs(base, axes, xr, yr, w, h)[0, xi])
            p, step = [0.05] * 3, None
            for t in range(tr):
                p = L.next_point(c, *p)
                if not all(abs(v) <= bound for v in p):
                    step = t + 1
                    break
            assert step is not None
            col = pl.records[:, xi]
            assert np.all(col["status"] == sar.SAR_SEARCH_DIVERGED) and np.all(col["steps_done"] == 0)
            assert np.all(col["transient_done"] == step)
    for yi in range(h):
        for xi in range(w):
            if not (0 < abs(a[xi]) < 1 and b[yi] != 0):
                continue
            assert spec.status[yi, xi] == sar.SAR_SEARCH_BOUNDED
            want = sorted((math.log(abs(a[xi])), math.log(abs(b[yi])), math.log(c_)), reverse=True)
            assert np.max(np.abs(spec.lyapunov[yi, xi] - want)) <= 1e-12, (xi, yi)
            assert abs(l1.lyapunov[yi, xi] - math.log(abs(a[xi]))) <= 1e-12, (xi, yi)


def test_determinism_across_calls_chunks_and_partial_tiles(sar, rt):
    base = _base(sar, "solar_sail")
    axes = (8, 19)
    xr, yr = _around(base, axes, 0.12)
    w, h, kw = 37, 21, dict(transient=300, steps=400)     # tiles_x = 5: a tile row is 320 pixels; the last tiles are partial
    want = P.plane(base, axes, xr, yr, w, h, "l1", transient_steps=300, steps=400)
    runs = []
    try:
        for chunk in (0, 0, 64, 100, 128, 320, 1000, 1 << 22):
            rt.set_option("plane_chunk", chunk)
            for mode in ("l1", "spectrum"):
                runs.append((mode, sar.lyapunov_plane(rt, base, axes, xr, yr, w, h, mode, **kw).records.copy()))
    finally:
        rt.set_option("plane_chunk", 0)
    _same_raw(runs[0][1], want)
    for mode in ("l1", "spectrum"):
        first = [r for m, r in runs if m == mode]
        for r in first[1:]:
            assert r.tobytes() == first[0].tobytes(), mode
    # a plane of one row / one column
    for (ww, hh) in ((1, 11), (13, 1)):
        got = sar.lyapunov_plane(rt, base, axes, xr, yr, ww, hh, "l1", **kw).records
        _same_raw(got, P.plane(base, axes, xr, yr, ww, hh, "l1", transient_steps=300, steps=400))


def test_no_side_effect_on_the_image_buffers_and_timing(sar, gpu):
    cfg = sar.Config.poisson_saturne(iterations=1024 * 200, width=64, height=64, jobs_total=1024, seed=5)
    r = sar.Runtime(cfg, device=0)
    try:
        sar.render(cfg, r)
        before = (r.count(), r.steps(), r.zbuf(), r.max())
        r.enable_timing(True)
        r.set_option("plane_chunk", 256)
        pl = sar.lyapunov_plane(r, cfg, (0, 1), (-0.5, 0.5), (-0.5, 0.5), 40, 24, transient=200, steps=300)
        t = r.last_timing()
        after = (r.count(), r.steps(), r.zbuf(), r.max())
        assert np.array_equal(before[0], after[0]) and before[3] == after[3]
        assert np.array_equal(before[1].view(np.uint64), after[1].view(np.uint64))
        assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32))
        assert t.iterate_ms > 0 and t.iterate_launches == 4   # 5 x 3 tiles, 4 per launch of 256 pixels
        assert pl.records.shape == (24, 40)
    finally:
        r.close()


def test_colorize_without_a_plane_is_refused(sar, gpu):
    cfg = sar.Config.solar_sail(width=16, height=16)
    r = sar.Runtime(cfg, device=0)
    try:
        out = np.empty(16 * 16 * 4, dtype=np.uint16)
        st = sar.load_library().sar_runtime_plane_colorize(C.byref(cfg.c), r.handle, None, out.ctypes.data_as(C.POINTER(C.c_uint16)))
        assert st == 1
    finally:
        r.close()


@pytest.mark.parametrize("mode,colors", [("l1", {}), ("spectrum", dict(threshold=0.05, chaos_scale=0.1, order_scale=0.5))])
def test_colorize_matches_the_restatement(sar, rt, mode, colors):
    base = _base(sar, "poisson_saturne")
    axes = (0, 13)
    xr, yr = _around(base, axes, 0.3)
    pl = sar.lyapunov_plane(rt, base, axes, xr, yr, 40, 32, mode, transient=500, steps=800)
    cfg = sar.Config.poisson_saturne()
    img = pl.colorize(cfg, **colors)
    lam1 = pl.records["lyapunov"][..., 0]
    want = P.colorize(pl.status, pl.records["steps_done"], lam1, cfg.palette_rgb[:cfg.palette_len], **colors)
    bounded = pl.status == sar.SAR_SEARCH_BOUNDED
    assert np.array_equal(img[~bounded], want[~bounded])
    assert np.max(np.abs(img[bounded].astype(np.int64) - want[bounded].astype(np.int64))) <= 1
    assert np.any(bounded)
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "plane.png")
        sar.write_image(img, path)
        assert np.array_equal(D.decode_png(path), img)
    other = sar.lyapunov_plane(rt, base, axes, xr, yr, 8, 8, mode, transient=10, steps=10)
    with pytest.raises(ValueError):
        pl.colorize(cfg)
    assert other.colorize(cfg).shape == (8, 8, 4)


def test_hottest_pixel_is_a_found_map_that_renders(sar, rt):
    import search_restatement as R
    base = R.candidates(1, 545, 1)[0]            # a map the search accepts (tests/test_lyapunov_reference.py)
    axes = (2, 24)
    xr, yr = _around(base, axes, 0.02)
    pl = sar.lyapunov_plane(rt, base, axes, xr, yr, 32, 32, "l1", transient=1000, steps=4000)
    lam = np.where(pl.status == sar.SAR_SEARCH_BOUNDED, pl.lyapunov, -np.inf)
    y, x = np.unravel_index(np.argmax(lam), lam.shape)
    assert lam[y, x] > 0.005
    c = pl.coeffs(x, y)
    recs, stats = sar.search_attractors(rt, 1, coeffs=c.reshape(1, 30), transient=1000, steps=4000)
    assert stats["accepted"] == 1
    assert recs[0]["mant"][0] == pl.records[y, x]["mant"][0] and recs[0]["log2_exp"][0] == pl.records[y, x]["log2_exp"][0]
    assert recs[0]["lyapunov"][0] == lam[y, x]    # e1's growth is the largest column's: the same finish of the same fields
    w = h = 256
    jobs = 4096
    cfg = sar.Config.from_coefficients(c).replace(width=w, height=h, iterations=10_000_000, jobs_total=jobs, seed=11)
    cfg = sar.frame_view(cfg, rt, 1024, 2000, margin=0.05)
    img_rt = sar.Runtime(cfg, device=0)
    try:
        sar.render_jobs(cfg, img_rt)
        count = img_rt.count()
    finally:
        img_rt.close()
    assert np.count_nonzero(count) >= 0.005 * w * h
