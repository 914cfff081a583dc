"""GPU: shaded rendering (sar_shade, sar_shade_device, k_shade) against the numpy restatement (tests/shade_restatement.py), bit for
bit: the RGBA16 image and every statistic on the states of tests/shade_cases.py loaded into a runtime — with the statistics, without
them (the path that never waits) and into a device buffer —, the buffers it must leave alone, a rendered frame before and after the
density filter, a runtime of a frame group, a Gas colorize on either side of it, and the refusals that need a runtime."""
import ctypes as C

import numpy as np
import pytest

import shade_cases as K
import shade_restatement as S

pytestmark = pytest.mark.gpu

ALL_CASES = pytest.mark.parametrize("name", K.NAMES)


def _diff(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return f"{len(bad)} differ, first at {bad[:4].tolist()}: got {[got[tuple(i)].tolist() for i in bad[:4]]}, " \
           f"want {[want[tuple(i)].tolist() for i in bad[:4]]}"


def _cfg(sar, k):
    return sar.Config.solar_sail(**k.cfg)


def _window(sar, k):
    w = k.window
    return None if w is None else sar.ColorRange(w["lo"], w["hi"], w["pos_lo"], w["pos_hi"], 0, bool(w["applied"]))


@pytest.fixture(scope="module")
def runtimes(sar, gpu):
    """One runtime per frame size, shared by the loaded-state tests (each test loads what it needs)."""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = sar.Runtime(sar.Config.solar_sail(width=w, height=h))
        return made[(w, h)]

    yield get
    for rt in made.values():
        rt.close()


def _state(rt):
    return rt.count(), rt.steps().view(np.uint64), rt.zbuf().view(np.uint32), rt.max()


def _assert_untouched(rt, before, what):
    """`before`: _state(rt) read before the calls (the load itself stores a depth of -0.0 as +0.0: the state is what the runtime holds)."""
    count, steps, zbuf, mx = _state(rt)
    assert np.array_equal(count, before[0]), f"{what}: count changed"
    assert np.array_equal(steps, before[1]), f"{what}: steps changed"
    assert np.array_equal(zbuf, before[2]), f"{what}: zbuf changed"
    assert mx == before[3], f"{what}: max changed"


def _device_image(sar, cfg, rt, **kw):
    import torch
    h, w = cfg.c.height, cfg.c.width
    dev = torch.zeros(w * h * 4, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    sar.shade_device(cfg, rt, dev.data_ptr(), **kw)
    rt.synchronize()
    return dev.cpu().numpy().view(np.uint16).reshape(h, w, 4)


@ALL_CASES
def test_loaded_state_matches_the_restatement(sar, runtimes, name):
    k, ref = K.case(name), K.reference(name)
    cfg, win = _cfg(sar, k), _window(sar, k)
    rt = runtimes(k.width, k.height)
    rt.load(k.count, k.steps, k.zbuf, k.max)
    before = _state(rt)
    assert np.array_equal(before[0], k.count) and np.array_equal(before[1], k.steps.view(np.uint64)) and before[3] == k.max
    img, stats = rt.shade(cfg, stats=True, window=win, **k.params)
    assert stats == ref.stats, f"{name}: stats {stats} vs {ref.stats}"
    assert img.dtype == np.uint16 and img.shape == (k.height, k.width, 4)
    assert np.array_equal(img, ref.rgba), f"{name}: {_diff(img, ref.rgba)}"
    _assert_untouched(rt, before, name)
    quiet = sar.shade(cfg, rt, window=win, **k.params)                  # no statistics: the call never waits for them
    assert np.array_equal(quiet, ref.rgba), f"{name}: without statistics: {_diff(quiet, ref.rgba)}"
    dev = _device_image(sar, cfg, rt, window=win, **k.params)
    assert np.array_equal(dev, ref.rgba), f"{name}: shade_device: {_diff(dev, ref.rgba)}"
    _assert_untouched(rt, before, f"{name}: after three calls")


def test_defaults_and_null_params(sar, runtimes):
    k = K.case("random-70x40-R8-s1")
    cfg = _cfg(sar, k)
    rt = runtimes(k.width, k.height)
    rt.load(k.count, k.steps, k.zbuf, k.max)
    want, want_stats = K.shade(k._replace(params={}))
    img, stats = rt.shade(cfg, stats=True)
    assert stats == want_stats and np.array_equal(img, want), _diff(img, want)
    lib, out = sar.load_library(), np.zeros((k.height, k.width, 4), dtype=np.uint16)
    from strange_attractor_renderer_amd import _abi
    st = _abi.SarShadeStats()
    assert lib.sar_shade(C.byref(cfg.c), rt.handle, None, C.byref(st), out.ctypes.data_as(C.POINTER(C.c_uint16))) == 0
    assert np.array_equal(out, want) and (st.surface, st.background, st.isolated, st.occluded, st.smoothed) == tuple(
        want_stats[f] for f in ("surface", "background", "isolated", "occluded", "smoothed"))


def test_refusals_that_need_a_runtime(sar, runtimes):
    k = K.case("random-70x40-R8-s1")
    cfg = _cfg(sar, k)
    rt = runtimes(k.width, k.height)
    rt.load(k.count, k.steps, k.zbuf, k.max)
    before = _state(rt)
    lib, p = sar.load_library(), sar.shade_params()
    out = np.zeros((k.height, k.width, 4), dtype=np.uint16)
    ptr = out.ctypes.data_as(C.POINTER(C.c_uint16))
    other = cfg.replace(width=k.width + 1)
    assert lib.sar_shade(C.byref(other.c), rt.handle, C.byref(p), None, ptr) == 2                  # SAR_ERR_DIM_MISMATCH, as colorize
    assert lib.sar_colorize(C.byref(other.c), rt.handle, ptr) == 2
    assert lib.sar_shade_device(C.byref(other.c), rt.handle, C.byref(p), None, C.c_void_p(8)) == 2
    assert lib.sar_shade(C.byref(cfg.c), rt.handle, C.byref(p), None, None) == 1 and "output" in lib.sar_last_error().decode()
    assert lib.sar_shade_device(C.byref(cfg.c), rt.handle, C.byref(p), None, None) == 1
    with pytest.raises(sar.SarError):
        rt.shade(cfg, ao_radius=9)
    with pytest.raises(sar.SarError):
        rt.shade(cfg.replace(scale=0.0))
    assert not out.any()
    _assert_untouched(rt, before, "after the refusals")


def test_timing_books_the_kernel_as_colorize(sar, runtimes):
    k = K.case("random-96x80-R8-s1")
    cfg = _cfg(sar, k)
    rt = runtimes(k.width, k.height)
    rt.load(k.count, k.steps, k.zbuf, k.max)
    rt.enable_timing(True)
    try:
        rt.shade(cfg, **k.params)
        assert rt.last_timing().colorize_ms > 0.0
    finally:
        rt.enable_timing(False)


# ---- a rendered frame ----------------------------------------------------------------------------------------------------------
def _palette(cfg):
    return [[cfg.c.palette_rgb[i][ch] for ch in range(3)] for i in range(cfg.c.palette_len)]


def _restated(cfg, rt, **params):
    return S.shade(rt.count(), rt.steps(), rt.zbuf(), cfg.c.width, cfg.c.scale, _palette(cfg), cfg.c.transparent, S.params(**params))


def test_rendered_frame_before_and_after_the_density_filter(sar, gpu):
    jobs = 400
    cfg = sar.Config.solar_sail(width=200, height=160, iterations=jobs * 700, jobs_total=jobs, transparent=0)
    rt = sar.Runtime(cfg)
    try:
        sar.render_jobs(cfg, rt, sar.start_points(11, 0, jobs))
        gas = sar.colorize(cfg, rt)
        want, want_stats = _restated(cfg, rt)
        assert 0 < want_stats["surface"] < 200 * 160 and want_stats["occluded"] > 0 and want_stats["smoothed"] > 0
        img, stats = sar.shade(cfg, rt, stats=True)
        assert stats == want_stats and np.array_equal(img, want), _diff(img, want)
        assert np.array_equal(sar.colorize(cfg, rt), gas), "a Gas colorize gives other bytes after a shade call"
        rt.density_filter()
        want2, want_stats2 = _restated(cfg, rt, min_count=2)
        img2, stats2 = sar.shade(cfg, rt, stats=True, min_count=2)
        assert stats2 == want_stats2 and np.array_equal(img2, want2), _diff(img2, want2)
        assert not np.array_equal(img2, img)
    finally:
        rt.close()


def test_exposure_and_colour_range_modes_do_not_apply(sar, gpu):
    k, ref = K.case("random-70x40-R3-s1"), K.reference("random-70x40-R3-s1")
    cfg = _cfg(sar, k)
    rt = sar.Runtime(cfg)
    try:
        rt.load(k.count, k.steps, k.zbuf, k.max)
        rt.set_exposure()
        rt.set_color_range()
        assert np.array_equal(rt.shade(cfg, **k.params), ref.rgba)
        rt.hold_color_range(sar.ColorRange(0.2, 0.4))
        assert np.array_equal(rt.shade(cfg, **k.params), ref.rgba)
    finally:
        rt.close()


def test_group_runtime_gives_the_same_image(sar, gpu):
    k, ref = K.case("random-96x80-R8-s1"), K.reference("random-96x80-R8-s1")
    cfg = _cfg(sar, k)
    grp = sar.Runtime.group(cfg, 3)
    try:
        for rt in grp:
            rt.load(k.count, k.steps, k.zbuf, k.max)
        devs = [_device_image(sar, cfg, rt, **k.params) for rt in grp]
        for i, (rt, dev) in enumerate(zip(grp, devs)):
            assert np.array_equal(dev, ref.rgba), f"group runtime {i}: shade_device"
            img, stats = rt.shade(cfg, stats=True, **k.params)
            assert stats == ref.stats and np.array_equal(img, ref.rgba), f"group runtime {i}"
    finally:
        for rt in reversed(grp):
            rt.close()
