"""GPU: the FTLE maps (sar_runtime_ftle, include/sar.h) — every field of the records and every statistic against the numpy
restatement bit for bit on the Henon plane, the degenerate shapes, the pitchfork and both presets; independence of the chunk; the
fates against basin_map's; BasinMap.ftle; no side effect on the runtime's buffers or on a held basin picture; one runtime through
several sizes; the colours; the refusals; and the timing spans."""
import ctypes as C

import numpy as np
import pytest

import basin_restatement as B
import ftle_restatement as F
from basin_cases import PITCHFORK_MU, PITCHFORK_WINDOW
from ftle_cases import FTLE_STEPS, HENON_SMALL, REFUSED, maps, refused_params

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(m, want):
    for f in F.RECORD_FIELDS:
        got = m.records[f]
        assert got.shape == want[f].shape, f
        if got.dtype == np.float64:
            assert np.array_equal(_bits(got), _bits(want[f])), (f, np.argwhere(_bits(got) != _bits(want[f]))[:4])
        else:
            assert got.dtype == want[f].dtype and np.array_equal(got, want[f]), (f, np.argwhere(got != want[f])[:4])
    assert not m.records["_pad"].any()
    for f in F.STATS_FIELDS:
        assert m.stats[f] == want["stats"][f] and type(m.stats[f]) is type(want["stats"][f]), f
    for f, prop in (("status", m.status), ("escape_step", m.escape_step), ("flags", m.flags), ("end", m.end), ("stretch2", m.stretch2), ("ftle", m.ftle)):
        assert prop.tobytes() == np.ascontiguousarray(m.records[f]).tobytes(), f
    assert m.gram.shape == m.status.shape + (3,) and np.array_equal(_bits(m.gram[..., 1]), _bits(m.records["g12"]))


@pytest.fixture(scope="module")
def pictures(sar):
    """(name, coeffs, kw) of every picture and its restatement, computed once and left unchanged."""
    return {name: (c, kw, F.ftle(c, **kw)) for name, c, kw in maps(sar)}


NAMES = ["henon_small", "degenerate_1x29", "degenerate_37x1", "degenerate_1x1", "pitchfork_48x40", "pitchfork_33x17", "poisson_saturne", "solar_sail"]


def test_the_names_are_the_cases(sar):
    assert [name for name, _, _ in maps(sar)] == NAMES


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_restatement(sar, rt, pictures, name):
    c, kw, want = pictures[name]
    m = sar.ftle_map(rt, c, **kw)
    _same(m, want)
    assert np.array_equal(_bits(m.start(kw["width"] - 1, 0)), _bits(F.start(kw["origin"], kw["du"], kw["dv"], kw["width"], kw["height"])[0, -1]))
    if name in ("henon_small", "pitchfork_48x40", "poisson_saturne", "solar_sail"):     # both fates, and a finite field to look at
        assert m.stats["bounded"] and m.stats["escaped"] and m.stats["edge"] and np.isfinite(m.ftle).any()


def test_results_do_not_depend_on_the_chunk(sar, rt, pictures):
    c, kw, want = pictures["henon_small"]
    tiles = 5 * 4                                            # 37 x 29 in 8 x 8 tiles
    full = sar.ftle_map(rt, c, **kw)
    try:
        for chunk, launches in ((64, tiles), (192, 7), (0, 1)):
            rt.enable_timing(True)
            m = sar.ftle_map(rt, c, chunk=chunk, **kw)
            t = rt.last_timing()
            rt.enable_timing(False)
            assert t.iterate_launches == launches and t.iterate_ms > 0 and t.resolve_ms > 0, chunk   # k_ftle_flow's bands, k_ftle_gram
            assert m.records.tobytes() == full.records.tobytes() and m.stats == full.stats, chunk
    finally:
        rt.enable_timing(False)
    _same(m, want)


def test_fates_are_the_basins(sar, rt, pictures):
    for name in ("henon_small", "pitchfork_33x17", "solar_sail"):
        c, kw, _ = pictures[name]
        geo = {k: v for k, v in kw.items() if k != "steps"}
        m = sar.ftle_map(rt, c, **kw)
        b = sar.basin_map(rt, c, box=B.UNIT_BOX, transient=0, steps=kw["steps"], grid=1, **geo)
        assert np.array_equal(m.status, b.status) and np.array_equal(m.escape_step, b.escape_step), name
        # BasinMap.ftle: the basin's own map and plane
        again = b.ftle(rt, steps=kw["steps"])
        assert again.records.tobytes() == m.records.tobytes() and again.stats == m.stats, name
        assert bytes(again.params) == bytes(m.params)
        assert b.ftle(rt, steps=kw["steps"], chunk=64, bound=1e6).records.tobytes() == m.records.tobytes()


def test_the_runtime_is_only_lent(sar, rt, pictures):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    basin = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), width=33, height=17, transient=300, steps=32, grid=8, **PITCHFORK_WINDOW)
    held = basin.colorize(cfg)
    c, kw, _ = pictures["henon_small"]
    m = sar.ftle_map(rt, c, **kw)
    m.colorize(cfg)
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    assert np.array_equal(basin.colorize(cfg), held)          # the basin's records are still the runtime's
    rt.reset()


def test_one_runtime_through_several_sizes(sar, rt, pictures):
    order = ["henon_small", "degenerate_1x1", "pitchfork_48x40", "henon_small"]
    got = []
    for name in order:
        c, kw, want = pictures[name]
        got.append(sar.ftle_map(rt, c, **kw))
        _same(got[-1], want)
    assert got[-1].records.tobytes() == got[0].records.tobytes() and got[-1].stats == got[0].stats


def _palette(cfg):
    return cfg.palette_rgb[:cfg.palette_len]


def test_colours(sar, rt, pictures):
    cfg = sar.Config.solar_sail()
    for name in ("henon_small", "poisson_saturne", "degenerate_1x1"):
        c, kw, _ = pictures[name]
        m = sar.ftle_map(rt, c, **kw)
        lo, hi = m.window()
        assert (lo, hi) == F.window(m.ftle) and lo < hi
        for window, fade in ((None, None), ((-0.1, 0.35), 3.5)):
            img = m.colorize(cfg, **({} if window is None else dict(window=window, fade=fade)))
            want = F.colorize(m.status, m.escape_step, m.flags, m.ftle, _palette(cfg), *((lo, hi) if window is None else window),
                              fade=32.0 if fade is None else fade)
            assert img.shape == want.shape == m.status.shape + (4,) and img.dtype == np.uint16
            exact = (m.status == sar.SAR_SEARCH_DIVERGED) | ((m.flags & sar.SAR_FTLE_EDGE) != 0) | ~np.isfinite(m.ftle)
            assert np.array_equal(img[exact], want[exact]), np.argwhere((img != want).any(-1) & exact)[:4]
            diff = np.abs(img.astype(np.int64) - want.astype(np.int64))
            print(name, window, "largest channel difference", int(diff.max()), "pixels that differ", int((diff > 0).any(-1).sum()))
            assert diff.max() <= 1               # the device's log against the host's: include/sar.h
            assert np.all(img[..., 3] == 65535)
        if name == "henon_small":
            edge = (m.flags & sar.SAR_FTLE_EDGE) != 0
            esc = m.status == sar.SAR_SEARCH_DIVERGED
            assert edge.any() and np.all(img[edge] == 65535) and np.all(img[esc][:, 0] < 32768) and img[~esc & ~edge][:, :3].any()
    with pytest.raises(sar.SarError):
        m.colorize(cfg, window=(0.5, 0.5))
    with pytest.raises(sar.SarError):
        m.colorize(cfg, fade=0.0)
    earlier = m
    c, kw, _ = pictures["degenerate_37x1"]
    later = sar.ftle_map(rt, c, **kw)
    with pytest.raises(ValueError):
        earlier.colorize(cfg)                    # another map has been computed since
    assert later.colorize(cfg).shape == (1, 37, 4)


def test_colorize_without_a_map_is_refused(sar, gpu):
    cfg = sar.Config.solar_sail(width=16, height=16)
    r = sar.Runtime(cfg, device=0)
    try:
        out = np.zeros(16 * 16 * 4, dtype=np.uint16)
        lib = sar.load_library()
        assert lib.sar_runtime_ftle_colorize(C.byref(cfg.c), r.handle, None, out.ctypes.data_as(C.POINTER(C.c_uint16))) == 1
        assert lib.sar_last_error().decode() == "sar_runtime_ftle_colorize: the runtime has no FTLE map (sar_runtime_ftle first)"
        assert not out.any()
    finally:
        r.close()


@pytest.mark.parametrize("change,text", REFUSED[::4], ids=[str(k) for k in range(0, len(REFUSED), 4)])
def test_refusals_with_a_runtime(sar, rt, change, text):
    p = refused_params(sar, change)
    pix = np.zeros(64, dtype=sar.FTLE_PIXEL_DTYPE)          # (refused before anything is written)
    lib = sar.load_library()
    assert lib.sar_runtime_ftle(rt.handle, C.byref(p), pix.ctypes.data_as(C.POINTER(sar._abi.SarFtlePixel)), None) == 1
    assert lib.sar_last_error().decode() == text
    assert not pix.view(np.uint8).any()


def test_steps_beyond_one_checked_run(sar, rt):
    """N = 1, 16, 17 and 33: below, at and across the runs of 16 steps between two tests for a wave that is done."""
    c = F.henon()
    geo = {k: v for k, v in HENON_SMALL.items() if k != "steps"}
    assert FTLE_STEPS < 16
    for steps in (1, 16, 17, 33):
        _same(sar.ftle_map(rt, c, steps=steps, **geo), F.ftle(c, steps=steps, **geo))
