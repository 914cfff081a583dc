"""GPU: the basins of attraction (sar_runtime_basin, include/sar.h) — every field of the pixel records, the table and the statistics
against the numpy restatement bit for bit on the pitchfork fixture and on both presets; the pitchfork's mirror symmetry, which needs
no restatement; independence of the chunk and of the order of the pixels; no side effect on the runtime's buffers; the start points
of a basin against k_orbit; and the colours."""
import ctypes as C
import os

import numpy as np
import pytest

import basin_restatement as B
import image_decode as D
from basin_cases import (PITCHFORK, PITCHFORK_MU, PITCHFORK_WINDOW, PRESET_COUNTS, PRESET_SHAPE, PRESET_STEPS, PRESET_WINDOW, REFUSED,
                         preset_coeffs, refused_params)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    yield r
    r.close()


def _palette(cfg):
    return cfg.palette_rgb[:cfg.palette_len]


def _same(b, want):
    for f in ("status", "escape_step", "root", "label"):
        got = getattr(b, f)
        assert got.shape == want[f].shape and got.dtype == want[f].dtype, f
        assert np.array_equal(got, want[f]), (f, np.argwhere(got != want[f])[:4])
    assert b.n_attractors == want["stats"]["attractors"] == len(b.attractors)
    for f in B.ATTRACTOR_FIELDS:
        assert np.array_equal(b.attractors[f], want["attractors"][f]), f
    for f in B.STATS_FIELDS:
        assert b.stats[f] == want["stats"][f], f
    assert np.array_equal(b.stats["extent"].view(np.uint64), want["extent"].view(np.uint64)), (b.stats["extent"], want["extent"])


def _pitchfork_kw(case):
    shape, steps, _, _ = PITCHFORK[case]
    return dict(PITCHFORK_WINDOW, **shape, **steps)


@pytest.fixture(scope="module")
def pitchfork_references():
    """The restatements of the two pitchfork pictures, computed once and left unchanged."""
    c = B.pitchfork(PITCHFORK_MU)
    return [B.basin_auto(c, **_pitchfork_kw(k)) for k in range(len(PITCHFORK))]


@pytest.fixture(scope="module")
def pitchfork_basins(sar, rt):
    c = B.pitchfork(PITCHFORK_MU)
    return [sar.basin_map(rt, c, **_pitchfork_kw(k)) for k in range(len(PITCHFORK))]


@pytest.mark.parametrize("case", range(len(PITCHFORK)))
def test_pitchfork_equals_the_restatement(pitchfork_basins, pitchfork_references, case):
    b, want = pitchfork_basins[case], pitchfork_references[case]
    assert (tuple(b.params.box_lo), tuple(b.params.box_hi)) == want["box"]          # the learned box, then everything in it
    _same(b, want)
    _, _, sizes, escaped = PITCHFORK[case]
    assert list(b.attractors["pixels"]) == sizes and b.stats["escaped_transient"] + b.stats["escaped_tail"] == escaped
    assert abs(b.share(0) - sizes[0] / b.label.size) < 1e-15 and b.share(0) + b.share(1) + b.share(2) == pytest.approx(b.stats["bounded"] / b.label.size)


@pytest.fixture(scope="module")
def preset_basins(sar, rt):
    return {name: sar.basin_map(rt, preset_coeffs(sar, name), **PRESET_WINDOW, **PRESET_SHAPE, **PRESET_STEPS) for name in sorted(PRESET_COUNTS)}


@pytest.mark.parametrize("name", sorted(PRESET_COUNTS))
def test_presets_equal_the_restatement(sar, preset_basins, name):
    want = B.basin_auto(preset_coeffs(sar, name), **PRESET_WINDOW, **PRESET_SHAPE, **PRESET_STEPS)
    b = preset_basins[name]
    assert (tuple(b.params.box_lo), tuple(b.params.box_hi)) == want["box"]
    _same(b, want)
    assert (b.stats["escaped_transient"] + b.stats["escaped_tail"], b.stats["bounded"]) == PRESET_COUNTS[name]


@pytest.mark.parametrize("width,height", [(1, 1), (1, 7)])
def test_the_smallest_planes(sar, rt, width, height):
    c = B.pitchfork(PITCHFORK_MU)
    kw = dict(origin=(0.3, -0.5, 0.05), du=(0.0, 0.0, 0.0), dv=(0.0, 3.0, 0.0), width=width, height=height, transient=300, steps=32, grid=8)
    want = B.basin_auto(c, **kw)
    b = sar.basin_map(rt, c, **kw)
    _same(b, want)
    assert np.array_equal(b.start(0, height - 1), [0.3, -0.5, 0.05])
    assert b.stats["bounded"] == b.stats["pixels"] == width * height and b.n_attractors >= 1


def test_grid_1_puts_every_bounded_pixel_on_root_0(sar, rt, pitchfork_references):
    c = B.pitchfork(PITCHFORK_MU)
    kw = dict(_pitchfork_kw(1), grid=1)
    b = sar.basin_map(rt, c, box=B.UNIT_BOX, **kw)
    _same(b, B.basin(c, box=B.UNIT_BOX, **kw))
    bounded = b.status == sar.SAR_SEARCH_BOUNDED
    assert bounded.any() and not b.root[bounded].any() and not b.label[bounded].any() and b.n_attractors == 1
    assert list(b.attractors[0]["cell_lo"]) == list(b.attractors[0]["cell_hi"]) == [0, 0, 0] and b.attractors[0]["cells"] == 1
    # the cheap first pass: its extent is the one the full picture was framed on
    assert np.array_equal(b.stats["extent"].view(np.uint64), pitchfork_references[1]["extent"].view(np.uint64))
    assert np.array_equal(b.status, pitchfork_references[1]["status"])


def test_a_window_where_everything_escapes(sar, rt):
    c = B.pitchfork(PITCHFORK_MU)
    kw = dict(origin=(3.0, 3.0, 0.05), du=(1.0, 0.0, 0.0), dv=(0.0, 1.0, 0.0), width=9, height=5, transient=100, steps=16, grid=8)
    b = sar.basin_map(rt, c, **kw)
    _same(b, B.basin_auto(c, **kw))
    assert b.n_attractors == 0 and len(b.attractors) == 0 and b.stats["bounded"] == 0 and b.stats["cells"] == 0
    assert np.all(b.status == sar.SAR_SEARCH_DIVERGED) and np.all(b.label == sar.BASIN_NONE) and np.all(b.root == sar.BASIN_NONE)
    assert list(b.stats["extent"]) == [np.inf, -np.inf] * 3
    assert (tuple(b.params.box_lo), tuple(b.params.box_hi)) == ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))      # the unit box
    n = C.c_uint32(7)
    pix = np.empty(45, dtype=sar.BASIN_PIXEL_DTYPE)
    assert sar.load_library().sar_runtime_basin(rt.handle, C.byref(b.params), pix.ctypes.data_as(C.POINTER(sar._abi.SarBasinPixel)), None, 0,
                                                C.byref(n), None) == 0 and n.value == 0
    img = b.colorize(sar.Config.solar_sail())                                                     # no attractor to divide by: all grey
    assert np.array_equal(img, B.colorize(b.status, b.escape_step, b.label, 0, _palette(sar.Config.solar_sail())))


def test_cap_1_of_three_attractors(sar, rt, pitchfork_basins):
    full = pitchfork_basins[1]
    b = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), box=(tuple(full.params.box_lo), tuple(full.params.box_hi)), cap=1, **_pitchfork_kw(1))
    assert b.n_attractors == 3 and len(b.attractors) == 1 and b.attractors.tobytes() == full.attractors[:1].tobytes()
    assert b.pixels.tobytes() == full.pixels.tobytes()                                # labels unchanged
    # through the ABI: one record written, the rest of the caller's buffer untouched
    table = np.full(3, 0xAB, dtype=np.uint8).repeat(sar.BASIN_ATTRACTOR_DTYPE.itemsize).view(sar.BASIN_ATTRACTOR_DTYPE)
    n = C.c_uint32()
    pix = np.empty(full.label.size, dtype=sar.BASIN_PIXEL_DTYPE)
    assert sar.load_library().sar_runtime_basin(rt.handle, C.byref(b.params), pix.ctypes.data_as(C.POINTER(sar._abi.SarBasinPixel)),
                                                table.ctypes.data_as(C.POINTER(sar._abi.SarBasinAttractor)), 1, C.byref(n), None) == 0
    assert n.value == 3 and table[:1].tobytes() == full.attractors[:1].tobytes() and np.all(table[1:].view(np.uint8) == 0xAB)


def test_pitchfork_symmetry(sar, rt):
    """x -> -x maps the pitchfork onto itself: with a window and a box symmetric in x, fates mirror and the two large basins swap."""
    c = B.pitchfork(PITCHFORK_MU)
    for case in range(len(PITCHFORK)):
        b = sar.basin_map(rt, c, box=((-1.0, -0.25, -1.0), (1.0, 0.75, 1.0)), **_pitchfork_kw(case))
        assert np.array_equal(b.status, b.status[:, ::-1]) and np.array_equal(b.escape_step, b.escape_step[:, ::-1])
        a = b.attractors
        assert b.n_attractors == 3 and a["pixels"][0] == a["pixels"][1] > a["pixels"][2] and a["cells"][0] == a["cells"][1]
        assert np.array_equal(b.label == 0, (b.label == 1)[:, ::-1]) and np.array_equal(b.label == 2, (b.label == 2)[:, ::-1])
        G = b.params.grid
        assert list(a["cell_lo"][0]) == [G - 1 - a["cell_hi"][1][0], a["cell_lo"][1][1], a["cell_lo"][1][2]]


def test_results_do_not_depend_on_the_chunk(sar, rt, pitchfork_basins, preset_basins):
    c = B.pitchfork(PITCHFORK_MU)
    full = pitchfork_basins[0]
    box = (tuple(full.params.box_lo), tuple(full.params.box_hi))
    tiles = 6 * 5                                           # 48 x 40 in 8 x 8 tiles
    ss = preset_basins["solar_sail"]
    try:
        for chunk, launches in ((64, tiles), (100, tiles), (4096, 1), (640, 3), (0, 1)):
            rt.set_option("basin_chunk", chunk)
            rt.enable_timing(True)
            b = sar.basin_map(rt, c, box=box, **_pitchfork_kw(0))
            t = rt.last_timing()
            rt.enable_timing(False)
            assert t.iterate_launches == launches and t.iterate_ms > 0 and t.warmup_ms > 0, chunk      # k_basin_mark's / k_basin_screen's spans
            assert b.pixels.tobytes() == full.pixels.tobytes() and b.attractors.tobytes() == full.attractors.tobytes(), chunk
            assert b.stats["extent"].tobytes() == full.stats["extent"].tobytes() and b.stats["cells"] == full.stats["cells"], chunk
            s = sar.basin_map(rt, preset_coeffs(sar, "solar_sail"), box=(tuple(ss.params.box_lo), tuple(ss.params.box_hi)), **PRESET_WINDOW,
                              **PRESET_SHAPE, **PRESET_STEPS)
            assert s.pixels.tobytes() == ss.pixels.tobytes() and s.attractors.tobytes() == ss.attractors.tobytes(), chunk
    finally:
        rt.set_option("basin_chunk", 0)
        rt.enable_timing(False)
    with pytest.raises(sar.SarError):
        rt.set_option("basin_chunk", 2 ** 30 + 1)


def test_results_do_not_depend_on_the_order(sar, rt, pitchfork_basins, preset_basins):
    for full, c, kw in ((pitchfork_basins[1], B.pitchfork(PITCHFORK_MU), _pitchfork_kw(1)),
                        (preset_basins["poisson_saturne"], preset_coeffs(sar, "poisson_saturne"), dict(PRESET_WINDOW, **PRESET_SHAPE, **PRESET_STEPS))):
        box = (tuple(full.params.box_lo), tuple(full.params.box_hi))
        again = sar.basin_map(rt, c, box=box, **kw)
        assert again.pixels.tobytes() == full.pixels.tobytes() and again.attractors.tobytes() == full.attractors.tobytes()
        assert again.stats["extent"].tobytes() == full.stats["extent"].tobytes()
    # the pitchfork plane flipped in both axes (32 and 16 steps of du = 4 and dv = 3: every start point is the same double)
    full, kw = pitchfork_basins[1], _pitchfork_kw(1)
    o, du, dv = (np.array(kw[k]) for k in ("origin", "du", "dv"))
    flipped = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), box=(tuple(full.params.box_lo), tuple(full.params.box_hi)),
                            **dict(kw, origin=(o + du) + dv, du=-du, dv=-dv))
    assert np.array_equal(flipped.start(0, 0), full.start(32, 16)) and np.array_equal(flipped.start(5, 3), full.start(27, 13))
    assert np.array_equal(flipped.status, full.status[::-1, ::-1]) and np.array_equal(flipped.escape_step, full.escape_step[::-1, ::-1])
    assert np.array_equal(flipped.root, full.root[::-1, ::-1])

    def key(b):
        return sorted(zip(b.attractors["root"].tolist(), b.attractors["pixels"].tolist(), b.attractors["cells"].tolist()))
    assert key(flipped) == key(full)


def test_the_runtime_is_only_lent(sar, rt):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    b = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), **_pitchfork_kw(1))
    b.colorize(cfg)
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    rt.reset()


@pytest.mark.parametrize("change,text", REFUSED)
def test_refusals_with_a_runtime(sar, rt, change, text):
    p = refused_params(sar, change)
    pix = np.zeros(64, dtype=sar.BASIN_PIXEL_DTYPE)          # (refused before anything is written)
    lib = sar.load_library()
    assert lib.sar_runtime_basin(rt.handle, C.byref(p), pix.ctypes.data_as(C.POINTER(sar._abi.SarBasinPixel)), None, 0, None, None) == 1
    assert text in lib.sar_last_error().decode()
    assert not pix.view(np.uint8).any()


def test_starts_of_a_basin_stay_and_escaped_starts_leave(sar, rt, preset_basins):
    """Against k_orbit: one column of the preset's own map, the same transient, bound and steps."""
    for name, b in preset_basins.items():
        c = preset_coeffs(sar, name)
        kw = dict(width=1, height=1, jobs=64, transient=PRESET_STEPS["transient"], steps=PRESET_STEPS["steps"], bound=b.params.bound,
                  v_range=(-1.0, 1.0))
        stay = b.starts(0, 64)
        assert stay.shape == (64, 3) and stay.dtype == np.float64
        idx = np.flatnonzero(b.label.reshape(-1) == 0)
        pick = idx[(np.arange(64) * idx.size) // 64]
        assert np.array_equal(stay, np.stack([b.start(int(i % 48), int(i // 48)) for i in pick]))
        d = sar.orbit_diagram(rt, c, c, starts=stay, **kw)
        assert d.stats["dead_transient"][0] == d.stats["dead_late"][0] == 0 and d.stats["alive"][0] == 64
        gone = np.flatnonzero(b.status.reshape(-1) == sar.SAR_SEARCH_DIVERGED)[:64]
        leave = np.stack([b.start(int(i % 48), int(i // 48)) for i in gone])
        d = sar.orbit_diagram(rt, c, c, starts=leave, **kw)
        assert d.stats["dead_transient"][0] + d.stats["dead_late"][0] == 64 and d.stats["alive"][0] == 0
    earlier = preset_basins["solar_sail"]
    third = sar.basin_map(rt, B.pitchfork(PITCHFORK_MU), **_pitchfork_kw(1))
    rep = third.starts(2, 40)                                 # 17 pixels asked for 40 points: they repeat, in order
    assert rep.shape == (40, 3) and np.unique(rep, axis=0).shape[0] == 17 and np.all(rep[:, 0] == 0.0)
    with pytest.raises(ValueError):
        third.starts(3, 4)
    with pytest.raises(ValueError):
        earlier.colorize(sar.Config.solar_sail())                 # another picture has been computed since


def test_colours(sar, rt, tmp_path):
    cfg = sar.Config.solar_sail()
    for c, kw in ((B.pitchfork(PITCHFORK_MU), _pitchfork_kw(0)), (preset_coeffs(sar, "solar_sail"), dict(PRESET_WINDOW, **PRESET_SHAPE, **PRESET_STEPS))):
        b = sar.basin_map(rt, c, **kw)
        for fade in (None, 3.5):
            img = b.colorize(cfg, **({} if fade is None else dict(fade=fade)))
            want = B.colorize(b.status, b.escape_step, b.label, b.n_attractors, _palette(cfg), 32.0 if fade is None else fade)
            assert img.shape == want.shape == b.status.shape + (4,) and img.dtype == np.uint16
            assert np.array_equal(img, want), np.argwhere(img != want)[:4]
        esc = b.status == sar.SAR_SEARCH_DIVERGED
        assert esc.any() and np.all(img[..., 3] == 65535)
        assert np.all(img[esc][:, 0] == img[esc][:, 1]) and np.all(img[esc][:, 1] == img[esc][:, 2])
        assert np.all(img[esc][:, 0] < 32768) and img[~esc][:, :3].any()
    path = str(tmp_path / "basin.png")
    sar.write_image(img, path)
    assert np.array_equal(D.decode_png(path), img)
    with pytest.raises(sar.SarError):
        b.colorize(cfg, fade=0.0)
    assert os.path.getsize(path) > 0
