"""GPU: the kernels that READ a volume, and add = 1, on the volumes of tests/volume_edge_cases.py against the numpy restatement bit for
bit. The volumes go in through the hooks build's sar_runtime_debug_volume_load (Runtime.debug_load_volume), as frames go in through
sar_runtime_load: 1024 and 257 slabs (k_volume_march's slab-colour loop beyond one trip, every row of its LDS table, windows beyond
slab 255), a transmittance down in the subnormals, opacities of exactly 1 and of nothing, a ray that stops at its first slab, counts of
2^31 and 2^32 - 1, an empty volume, palette positions outside [0, 1], palettes of 1 and 15 rows, four workgroups with a ragged last
one, a section that wraps to 0 under a nearest slab, a reduction beyond one trip of its grid, sar_runtime_volume_march_device, add = 1
across a voxel's wrap under two launch shapes, the accumulate at 1024 slabs, refused loads and a reused runtime."""
import ctypes as C
import math

import numpy as np
import pytest

import volume_cases as K
import volume_edge_cases as E
import volume_restatement as R

pytestmark = pytest.mark.gpu

MARCHED = tuple(n for n in E.NAMES if n != "big_reduce")
SECTIONED = tuple(n for n in E.NAMES if n not in ("big_reduce", "positions", "palettes"))
U32 = 1 << 32


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=E.SMALL[0], height=E.SMALL[1]), device=0)
    yield r
    r.close()


def _load(sar, rt, k, **kw):
    """The case's volume loaded into rt, resized to the case first."""
    rt.set_width_height(k.width, k.height)
    return rt.debug_load_volume(k.config(sar), k.vol, E.Z_RANGE, **kw)


def _same_stats(got, want):
    for f in R.STATS:
        assert got[f] == want[f], (f, got, want)


def _same_image(img, want, what):
    assert img.dtype == np.uint16 and img.shape == want.shape, what
    bad = (img != want).any(axis=-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), img[bad][:2].tolist(), want[bad][:2].tolist())


def _device_march(rt, v, cfg, stats, **p):
    """v.march_device into a torch tensor: (image, statistics or None)."""
    import torch
    dev = torch.zeros(cfg.c.width * cfg.c.height * 4, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    st = v.march_device(dev.data_ptr(), config=cfg, stats=stats, **p)
    rt.synchronize()
    return dev.cpu().numpy().view(np.uint16).reshape(cfg.c.height, cfg.c.width, 4), st


def _frame(rt):
    return rt.count().tobytes(), rt.zbuf().tobytes(), rt.steps().tobytes(), rt.max()


# ---- 1. a loaded volume reads back; its statistics are the device's reduction --------------------------------------------------------
@pytest.mark.parametrize("name", E.NAMES)
def test_loaded_volume_reads_back_with_its_statistics(sar, rt, name):
    k = E.case(name)
    v = _load(sar, rt, k)
    assert v.depth == k.slabs and v.z_range == E.Z_RANGE
    _same_stats(v.stats, k.stats)                      # nonempty and vmax: k_volume_reduce; visits = stored: the voxels' 64-bit sum
    vol = v.slabs()
    assert vol.dtype == np.uint32 and np.array_equal(vol, k.vol)
    if k.slabs > 2:
        assert np.array_equal(v.slabs(k.slabs - 2, k.slabs), k.vol[-2:]) and np.array_equal(v.slabs(0, 1), k.vol[:1])


# ---- 2. the marches -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", MARCHED)
def test_march_equals_the_restatement(sar, rt, name):
    k = E.case(name)
    v = _load(sar, rt, k)
    for label, _, p in k.marches:
        for transparent in (0, 1):
            what = (name, label, transparent)
            cfg = k.config(sar, label, transparent)
            want_img, want_st = k.march(label, transparent)
            img, st = v.march(config=cfg, stats=True, **p)
            _same_image(img, want_img, what)
            assert st == want_st, (what, st, want_st)
            dev, dev_st = _device_march(rt, v, cfg, True, **p)
            _same_image(dev, want_img, (what, "march_device"))
            assert dev_st == want_st, (what, "march_device", dev_st, want_st)
            quiet, none = _device_march(rt, v, cfg, False, **p)          # without statistics: the call never waits
            assert none is None
            _same_image(quiet, want_img, (what, "march_device without statistics"))
    assert np.array_equal(v.slabs(), k.vol)            # a march reads


# ---- 3. the sections ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SECTIONED)
def test_section_equals_the_restatement(sar, rt, name):
    k = E.case(name)
    v = _load(sar, rt, k)
    for k0, k1 in k.windows:
        count, nearest = v.section(k0, k1)
        want = k.section(k0, k1)
        assert count.dtype == np.uint32 and nearest.dtype == np.int32
        assert np.array_equal(count, want[0]) and np.array_equal(nearest, want[1]), (name, k0, k1)


@pytest.mark.parametrize("name", ("wrap_to_zero", "max_counts"))
def test_a_wrapped_section_loads_into_the_frame(sar, rt, name):
    """Volume.load_section's docstring in numpy, on sections whose count wrapped — to 0 under a nearest slab, or to 2^32 - 7."""
    k = E.case(name)
    v = _load(sar, rt, k)
    lo, hi = E.Z_RANGE
    for k0, k1 in k.windows:
        count, nearest = k.section(k0, k1)
        got = v.load_section(k0, k1)
        assert np.array_equal(got[0], count) and np.array_equal(got[1], nearest)
        centre = (lo + (nearest.astype(np.float64) + 0.5) * ((hi - lo) / k.slabs)).astype(np.float32)
        zbuf = np.where(nearest >= 0, centre, np.float32(-1.0)).astype(np.float32)
        steps = np.where(nearest >= 0, (nearest.astype(np.float64) + 0.5) / k.slabs, 0.0)
        assert np.array_equal(rt.count(), count) and rt.max() == int(count.max())
        assert rt.zbuf().tobytes() == zbuf.tobytes() and rt.steps().tobytes() == steps.tobytes(), (name, k0, k1)
    if name == "wrap_to_zero":
        count, nearest = k.section()
        assert ((count == 0) & (nearest == 2)).sum() >= k.height * k.width // 2       # the frame holds a depth where it counts nothing
    assert np.array_equal(v.slabs(), k.vol)


# ---- 4. add = 1 across a voxel's wrap ---------------------------------------------------------------------------------------------------
_ADDS = {}


def _wrap_case(first):
    """(hot, loaded volume, its statistics, the hot voxel, the other voxel, R.volume of hot's jobs into it): the hot voxel holds `first`."""
    if first not in _ADDS:
        hot = K.case("hot")
        at = np.unravel_index(int(np.argmax(hot.vol)), hot.vol.shape)
        other = (0, 0, 0) if at != (0, 0, 0) else (1, 0, 0)
        loaded = np.zeros(hot.vol.shape, dtype=np.uint32)
        loaded[at], loaded[other] = first, U32 - 1
        stats = E.stats_of(loaded)
        _ADDS[first] = (hot, loaded, stats, at, other, R.volume(hot.view, hot.starts, hot.iterations, hot.slabs, *hot.z_range, into=(loaded, stats)))
    return _ADDS[first]


@pytest.mark.parametrize("shape", ((0, 0), (7, 100)), ids=("default_launches", "chunk7_steps100"))
@pytest.mark.parametrize("first", (U32 - 100, U32 - 262144), ids=("past_zero", "to_zero"))
def test_add_across_a_wrap(sar, rt, first, shape):
    hot, loaded, stats, at, other, (want_vol, want) = _wrap_case(first)
    n = K.HOT_JOBS * K.HOT_ITERS
    assert n == 262144 and int(hot.vol[at]) == n and int(want_vol[at]) == (first + n) % U32 == (262044 if first == U32 - 100 else 0)
    assert want["vmax"] == U32 - 1 and want["stored"] == first + (U32 - 1) + n and want["nonempty"] == (2 if first == U32 - 100 else 1)
    rt.set_width_height(hot.width, hot.height)
    cfg = hot.config(sar)
    try:
        rt.set_option("volume_chunk", shape[0])
        rt.set_option("volume_steps", shape[1])
        v = rt.debug_load_volume(cfg, loaded, hot.z_range, iterations=hot.iterations)
        _same_stats(v.stats, stats)
        _same_stats(v.add(hot.starts), want)
    finally:
        rt.set_option("volume_chunk", 0)
        rt.set_option("volume_steps", 0)
    assert np.array_equal(v.slabs(), want_vol), np.argwhere(v.slabs() != want_vol)[:4].tolist()
    for transparent in (0, 1):                          # a voxel back at 0 is an empty one
        img, st = v.march(config=hot.config(sar, transparent=transparent), stats=True)
        want_img, want_st = R.march(want_vol, want["vmax"], hot.palette, transparent)
        _same_image(img, want_img, (first, shape, transparent))
        assert st == want_st and st["slabs_seen"] == want["nonempty"]
    count, nearest = v.section()
    assert np.array_equal(count, R.section(want_vol)[0]) and np.array_equal(nearest, R.section(want_vol)[1])


# ---- 5. the accumulate at the largest D -------------------------------------------------------------------------------------------------
def test_accumulate_into_1024_slabs(sar, rt):
    k = K.case("odd_ps")
    want_vol, want = R.volume(k.view, k.starts, k.iterations, 1024, *k.z_range)
    assert np.count_nonzero(want_vol.reshape(1024, -1).any(axis=1)) >= 256 and want_vol[768:].any()     # slabs used all along the index
    rt.set_width_height(k.width, k.height)
    v = sar.volume(rt, k.config(sar), jobs=k.jobs, iterations=k.iterations, slabs=1024, z_range=k.z_range, starts=k.starts)
    _same_stats(v.stats, want)
    assert np.array_equal(v.slabs(), want_vol)
    for transparent in (0, 1):
        img, st = v.march(config=k.config(sar, transparent=transparent), stats=True)
        want_img, want_st = R.march(want_vol, want["vmax"], k.palette, transparent)
        _same_image(img, want_img, ("odd_ps at 1024 slabs", transparent))
        assert st == want_st


# ---- 6. refused loads, a reused runtime ---------------------------------------------------------------------------------------------------
def test_a_refused_load_changes_nothing(sar, rt):
    from strange_attractor_renderer_amd import _abi
    k = E.case("d257")
    v = _load(sar, rt, k)
    cfg = k.config(sar)
    shape = (k.height, k.width)
    lib = sar.load_library()
    for slabs in (0, 1025):
        with pytest.raises(sar.SarError, match="slabs must be 1 to 1024"):
            rt.debug_load_volume(cfg, np.zeros((slabs, *shape), dtype=np.uint32), E.Z_RANGE)
    for z_range in ((1.0, 1.0), (2.0, 1.0), (math.nan, 1.0), (0.0, math.inf), (-math.inf, 0.0), (0.0, 5e-324)):
        with pytest.raises(sar.SarError, match="z_lo and z_hi must be finite"):
            rt.debug_load_volume(cfg, np.ones((8, *shape), dtype=np.uint32), z_range)
    for bad in ((8, k.height, k.width + 1), (8, k.height + 1, k.width), (8, k.height * k.width), (k.height, k.width)):
        with pytest.raises(ValueError):                # the wrapper: no buffer of another size reaches the copy
            rt.debug_load_volume(cfg, np.ones(bad, dtype=np.uint32), E.Z_RANGE)
    with pytest.raises(ValueError):
        rt.debug_load_volume(cfg.replace(width=k.width + 1), np.ones((8, k.height, k.width + 1), dtype=np.uint32), E.Z_RANGE)
    one = np.ones((1, *shape), dtype=np.uint32)
    ptr = one.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.sar_runtime_debug_volume_load(None, 1, -1.0, 1.0, ptr) == _abi.SAR_ERR_INVALID and "NULL" in lib.sar_last_error().decode()
    assert lib.sar_runtime_debug_volume_load(rt.handle, 1, -1.0, 1.0, None) == _abi.SAR_ERR_INVALID and "NULL" in lib.sar_last_error().decode()
    assert lib.sar_runtime_debug_volume_stats(rt.handle, None) == _abi.SAR_ERR_INVALID
    # the held volume is as it was: its bits, its statistics, its march
    assert np.array_equal(v.slabs(), k.vol)
    st = _abi.SarVolumeStats()
    assert lib.sar_runtime_debug_volume_stats(rt.handle, C.byref(st)) == _abi.SAR_OK and (st.nonempty, st.vmax) == (k.stats["nonempty"], k.stats["vmax"])
    label, _, p = k.marches[0]
    _same_image(v.march(config=k.config(sar, label, 1), **p), k.march(label, 1)[0], "after the refusals")
    # more than 2^30 voxels: refused by the count alone, before anything is read (the runtime's size drops the held volume)
    rt.set_width_height(1025, 1024)
    assert lib.sar_runtime_debug_volume_load(rt.handle, 1024, -1.0, 1.0, ptr) == _abi.SAR_ERR_INVALID and "2^30 voxels" in lib.sar_last_error().decode()
    assert lib.sar_runtime_debug_volume_stats(rt.handle, C.byref(st)) == _abi.SAR_ERR_INVALID and "holds no volume" in lib.sar_last_error().decode()
    with pytest.raises((sar.SarError, ValueError)):
        v.section()
    rt.set_width_height(k.width, k.height)


def test_loads_on_a_reused_runtime_leave_the_frame_alone(sar, rt):
    first, second, small = E.case("sparse_1024_wide"), E.case("d257"), K.case("odd_ps")
    v = _load(sar, rt, first)                           # the largest allocation first: the next load reuses it
    _same_image(v.march(config=first.config(sar, "default", 1)), first.march("default", 1)[0], "first load")
    rt.set_width_height(second.width, second.height)    # drops the held volume
    with pytest.raises((sar.SarError, ValueError)):
        v.section()
    rng = np.random.default_rng(2817)
    shape = (second.height, second.width)
    count = rng.integers(0, U32, size=shape, dtype=np.uint64).astype(np.uint32)
    rt.load(count, rng.random(shape), rng.standard_normal(shape).astype(np.float32), int(count.max()))
    before = _frame(rt)
    v = rt.debug_load_volume(second.config(sar), second.vol, E.Z_RANGE)
    _same_stats(v.stats, second.stats)
    for label, _, p in second.marches:
        cfg = second.config(sar, label, 0)
        _same_image(v.march(config=cfg, **p), second.march(label, 0)[0], ("second load", label))
        _same_image(_device_march(rt, v, cfg, True, **p)[0], second.march(label, 0)[0], ("second load, march_device", label))
    assert np.array_equal(v.section(255, 257)[0], second.section(255, 257)[0]) and np.array_equal(v.slabs(), second.vol)
    v2 = rt.debug_load_volume(second.config(sar), E.case("positions").vol[::-1], E.Z_RANGE)      # a load over a loaded volume
    assert np.array_equal(v2.slabs(), second.vol[::-1]) and v2.stats["nonempty"] == second.stats["nonempty"]
    with pytest.raises(ValueError):                    # the Python object of the volume that went
        v.section()
    assert _frame(rt) == before                        # loads, marches and sections lend the frame nothing
    rt.set_width_height(small.width, small.height)
    got = sar.volume(rt, small.config(sar), jobs=small.jobs, iterations=small.iterations, slabs=small.slabs, z_range=small.z_range,
                     starts=small.starts)
    _same_stats(got.stats, small.stats)
    assert np.array_equal(got.slabs(), small.vol)
    _same_image(got.march(), small.march("default", 1)[0], "the runtime's own volume after the loads")
