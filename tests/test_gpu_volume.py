"""GPU: volume rendering (sar_runtime_volume*, include/sar.h) — the volume, its statistics, the sections, the marched images and the
march statistics against the numpy restatement bit for bit on the cases of tests/volume_cases.py (the two presets at 64 x 48, 33 x 17
and 200 x 3, D = 1, 5, 8 and 33, a 1 x 1 image, a clipped range, 262 144 visits of one voxel, and the depth cases' +-inf, NaN,
subnormal and constant depths); the two identities that tie the volume to render, on the device's OWN render of the same jobs;
independence of "volume_chunk" and "volume_steps"; add = 1; the refusals that need a runtime; no side effect on the runtime's frame;
load_section; the timing fields."""
import numpy as np
import pytest

import volume_cases as K
import volume_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=64, height=48), device=0)
    yield r
    r.close()


def _volume(sar, rt, k, learned=False, **kw):
    rt.set_width_height(k.width, k.height)
    return sar.volume(rt, k.config(sar), jobs=k.jobs, iterations=k.iterations, slabs=k.slabs, z_range=None if learned else k.z_range,
                      starts=k.starts, **kw)


def _same_stats(got, want):
    for f in R.STATS:
        assert got[f] == want[f], (f, got, want)      # (z_min / z_max by value: of -0.0 and +0.0 either may be reported)


def _same_volume(v, k):
    _same_stats(v.stats, k.stats)
    vol = v.slabs()
    assert vol.dtype == np.uint32 and vol.shape == k.vol.shape
    assert np.array_equal(vol, k.vol), (int((vol != k.vol).sum()), np.argwhere(vol != k.vol)[:4].tolist())


# ---- 1. parity, case by case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.NAMES)
def test_case_equals_the_restatement(sar, rt, name):
    k = K.case(name)
    learned = name in K.LEARNED
    v = _volume(sar, rt, k, learned=learned)
    if learned:
        assert v.z_range == tuple(k.z_range)          # the range volume(z_range=None) learns is the restatement's
    _same_volume(v, k)
    windows = [(0, None)] + ([(2, k.slabs - 1), (k.slabs - 1, k.slabs), (0, 1)] if k.slabs > 3 else [])
    for k0, k1 in windows:
        count, nearest = v.section(k0, k1)
        want = R.section(k.vol, k0, k1)
        assert count.dtype == np.uint32 and nearest.dtype == np.int32
        assert np.array_equal(count, want[0]) and np.array_equal(nearest, want[1]), (k0, k1)
        assert np.array_equal(v.slabs(k0, k1), k.vol[k0:k1])
    for which in (K.MARCHES if name in K.MARCHED else ("default",)):
        if which == "window" and k.slabs <= 3:
            continue
        for transparent in (0, 1):
            img, st = v.march(config=k.config(sar, transparent=transparent), stats=True, **k.march_params(which))
            want_img, want_st = k.march(which, transparent)
            assert img.dtype == np.uint16 and img.shape == want_img.shape
            assert np.array_equal(img, want_img), (which, transparent, int((img != want_img).any(axis=-1).sum()),
                                                   np.argwhere((img != want_img).any(axis=-1))[:4].tolist())
            assert st == want_st, (which, transparent)
            assert np.array_equal(v.march(config=k.config(sar, transparent=transparent), **k.march_params(which)), want_img)


# ---- 2. the volume against the device's own render of the same jobs ---------------------------------------------------------------
@pytest.mark.parametrize("name", ("ps_small", "ss_small", "odd_ss", "wide_ps", "clipped", "alt_inf_wide", "overflow_mid_wide", "shrink_alt_tiny",
                                  "const_pos_wide", "falling_sentinel_wide", "falling_sentinel_tiny"))
def test_identities_against_the_devices_own_render(sar, rt, name):
    k = K.case(name)
    cfg = k.config(sar)
    v = _volume(sar, rt, k)
    rt.reset()
    sar.render_job_range(cfg, rt, k.iterations, k.starts)
    count, zbuf = rt.count().astype(np.int64), rt.zbuf()
    ray = v.slabs().astype(np.int64).sum(axis=0)
    s = v.stats
    assert (ray <= count).all()
    assert int(count.sum()) - int(ray.sum()) == s["below"] + s["above"] + s["nan"] and int(count.sum()) == s["visits"]
    if s["below"] + s["above"] + s["nan"] == 0:
        assert np.array_equal(ray, count)
        assert np.array_equal(v.section()[0], rt.count())
    nearest = v.section()[1]
    kz = R.slab(zbuf, k.slabs, *k.z_range)              # (sar_volume_slab is held to it in tests/test_volume_host.py)
    at = (count > 0) & (zbuf != np.float32(-1.0)) & (kz >= 0)
    assert np.array_equal(nearest[at], kz[at])
    if name in ("ps_small", "ss_small", "shrink_alt_tiny", "const_pos_wide"):
        assert at.sum() >= 100


# ---- 3. the launch shape, add -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ps_small", "ss_small", "overflow_mid_wide"))
def test_chunk_and_steps_change_no_bit(sar, rt, name):
    k = K.case(name)
    try:
        for chunk, steps in ((7, 100), (64, 1), (0, 255)):
            rt.set_option("volume_chunk", chunk)
            rt.set_option("volume_steps", steps)
            _same_volume(_volume(sar, rt, k), k)
        for option in ("volume_chunk", "volume_steps"):
            with pytest.raises(sar.SarError, match=f"{option} must be at most 2\\^24"):
                rt.set_option(option, (1 << 24) + 1)
    finally:
        rt.set_option("volume_chunk", 0)
        rt.set_option("volume_steps", 0)


@pytest.mark.parametrize("name", ("ps_small", "ss_small", "shrink_alt_tiny"))
def test_two_adds_over_the_job_halves_equal_one_call(sar, rt, name):
    k = K.case(name)
    half = k.jobs // 2
    rt.set_width_height(k.width, k.height)
    v = sar.volume(rt, k.config(sar), jobs=half, iterations=k.iterations, slabs=k.slabs, z_range=k.z_range, starts=k.starts[:half])
    first = R.volume(k.view, k.starts[:half], k.iterations, k.slabs, *k.z_range)
    _same_stats(v.stats, first[1])
    _same_stats(v.add(k.starts[half:]), k.stats)
    _same_volume(v, k)


def test_add_on_another_shape_is_refused_and_the_volume_stays(sar, rt):
    from strange_attractor_renderer_amd import _abi
    import ctypes as C
    k = K.case("ps_small")
    v = _volume(sar, rt, k)
    lib, st = sar.load_library(), _abi.SarVolumeStats()
    sp = k.starts.ctypes.data_as(C.POINTER(C.c_double))
    lo, hi = k.z_range
    for fields in (dict(slabs=k.slabs + 1), dict(z_lo=np.nextafter(lo, -1.0)), dict(z_hi=np.nextafter(hi, 1.0))):
        p = sar.volume_params(**{**dict(slabs=k.slabs, z_lo=lo, z_hi=hi, add=1), **fields})
        assert lib.sar_runtime_volume(C.byref(k.config(sar).c), rt.handle, C.byref(p), k.jobs, k.iterations, sp, C.byref(st)) == _abi.SAR_ERR_INVALID
        assert "add needs a held volume" in lib.sar_last_error().decode()
    # other refusals with a runtime: a config of another size, a window outside the volume
    p = sar.volume_params(slabs=k.slabs, z_lo=lo, z_hi=hi)
    other = k.config(sar, width=k.width + 1)
    assert lib.sar_runtime_volume(C.byref(other.c), rt.handle, C.byref(p), k.jobs, k.iterations, sp, C.byref(st)) == _abi.SAR_ERR_DIM_MISMATCH
    for k0, k1 in ((0, k.slabs + 1), (3, 3), (5, 2)):
        with pytest.raises(sar.SarError, match="the window must satisfy"):
            v.section(k0, k1)
        with pytest.raises(sar.SarError, match="the window must satisfy"):
            v.slabs(k0, k1)
        with pytest.raises(sar.SarError, match="the window must satisfy"):
            v.march(k0=k0, k1=k1)
    with pytest.raises(sar.SarError) as e:
        v.march(config=other)
    assert e.value.status == _abi.SAR_ERR_DIM_MISMATCH
    _same_volume(v, k)                                 # the held volume is as it was
    assert np.array_equal(v.march(), k.march("default", 1)[0])


def test_without_a_volume_the_readers_refuse(sar, rt):
    k = K.case("ps_small")
    v = _volume(sar, rt, k)
    rt.set_width_height(k.width + 3, k.height)         # drops the held volume
    for call in (v.section, v.slabs, v.march):
        with pytest.raises(sar.SarError, match="holds no volume|the runtime holds"):
            call()
    rt.set_width_height(k.width, k.height)
    with pytest.raises(sar.SarError, match="holds no volume"):
        v.section()
    with pytest.raises(sar.SarError, match="add needs a held volume"):
        v.add(k.starts)
    v2 = _volume(sar, rt, k)
    with pytest.raises(ValueError):                    # the Python object of the volume that went
        v.section()
    v2.close()
    with pytest.raises(ValueError):
        v2.section()
    v2.close()                                         # (twice: nothing to do)
    _same_volume(_volume(sar, rt, k), k)               # the runtime is usable


# ---- 4. the runtime is lent --------------------------------------------------------------------------------------------------------
def test_the_frame_keeps_its_bits_and_a_section_loads_into_it(sar, gpu):
    k = K.case("ps_small")
    cfg = k.config(sar, seed=5)
    r = sar.Runtime(cfg, device=0)
    try:
        sar.render_jobs(cfg, r)
        before = (r.count().tobytes(), r.steps().tobytes(), r.zbuf().tobytes(), r.max(), sar.colorize(cfg, r).tobytes())
        v = sar.volume(r, cfg, jobs=k.jobs, iterations=k.iterations, slabs=k.slabs, z_range=k.z_range, starts=k.starts)
        v.section()
        v.slabs(1, 3)
        v.march(stats=True, t_min=0.25)
        v.add(k.starts[:8])
        after = (r.count().tobytes(), r.steps().tobytes(), r.zbuf().tobytes(), r.max(), sar.colorize(cfg, r).tobytes())
        assert before == after
        # the start-point stream too: the next drawn render is the one a fresh runtime's second render gives
        sar.render_jobs(cfg, r)
        fresh = sar.Runtime(cfg, device=0)
        try:
            sar.render_jobs(cfg, fresh)
            sar.render_jobs(cfg, fresh)
            assert r.count().tobytes() == fresh.count().tobytes() and r.zbuf().tobytes() == fresh.zbuf().tobytes()
        finally:
            fresh.close()
        # load_section(0, D): the frame's count is the plain render's count of the same jobs (no visit of ps_small lacks a slab)
        v = sar.volume(r, cfg, jobs=k.jobs, iterations=k.iterations, slabs=k.slabs, z_range=k.z_range, starts=k.starts)
        count, nearest = v.load_section()
        loaded = r.count()
        gas = sar.colorize(cfg.replace(render_kind=sar.SAR_RENDER_GAS), r)
        r.reset()
        sar.render_job_range(cfg, r, k.iterations, k.starts)
        assert loaded.tobytes() == r.count().tobytes() == count.tobytes() and int(count.max()) == r.max()
        plain = sar.colorize(cfg.replace(render_kind=sar.SAR_RENDER_GAS), r)
        assert np.array_equal(gas[..., 3], plain[..., 3])      # Gas alpha is the count-derived brightness; the hue is the slab's
        assert np.array_equal(nearest >= 0, count > 0)
        # a slab section goes through the same chain
        part, _ = v.load_section(2, 5)
        assert np.array_equal(r.count(), R.section(k.vol, 2, 5)[0]) and r.max() == int(part.max())
        assert sar.colorize(cfg, r).shape == (k.height, k.width, 4)
        shaded = r.shade(cfg)
        assert shaded.shape == (k.height, k.width, 4)
    finally:
        r.close()


def test_timing_fields(sar, rt):
    k = K.case("ps_small")
    rt.enable_timing(True)
    try:
        rt.set_option("volume_steps", 100)
        v = _volume(sar, rt, k)
        t = rt.last_timing()
        assert t.iterate_launches == 3 and t.iterate_ms > 0 and t.warmup_ms > 0
        v.march()
        assert rt.last_timing().colorize_ms > 0
        v.section()
        assert rt.last_timing().colorize_ms > 0
    finally:
        rt.set_option("volume_steps", 0)
        rt.enable_timing(False)
