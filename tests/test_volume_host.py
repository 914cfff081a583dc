"""CPU: volume rendering without a device (include/sar.h: sar_runtime_volume*) — the cases of tests/volume_cases.py still reach what
they were built for; the numpy restatement against the ORACLE's render of the same jobs (the volume summed along the ray is render's
count less the visits without a slab, the nearest non-empty slab is the slab of render's zbuf); sar_volume_slab against the
restatement at slab edges, +-inf, NaN, -0.0 and subnormals; every refusal that needs no device; the mirrors of the ABI."""
import ctypes as C
import math

import numpy as np
import pytest

import volume_cases as K
import volume_restatement as R


@pytest.mark.parametrize("name", K.NAMES)
def test_case_reaches_what_it_was_built_for(oracle, name):
    K.check_condition(name)


def test_figures_of_the_small_cases(oracle):
    ps, ss = K.case("ps_small"), K.case("ss_small")
    assert ps.stats["vmax"] == 111 and ps.stats["visits"] == ps.stats["stored"] == 64 * 256
    assert ss.stats["nan"] == 4864
    clipped = K.case("clipped")
    assert clipped.stats["visits"] == 64 * 256 and clipped.stats["nan"] == 0
    assert K.case("one_slab").stats["nonempty"] == int(np.count_nonzero(R.section(K.case("one_slab").vol)[0]))
    one = K.case("one_pixel")
    assert one.vol.shape == (8, 1, 1) and one.stats["nonempty"] == 8


@pytest.mark.parametrize("name", K.NAMES)
def test_restatement_against_the_oracle(oracle, name):
    k = K.case(name)
    ort = oracle.Runtime(k.width, k.height)
    oracle.render_jobs(k.oracle_config, ort, k.starts, k.iterations)
    count, zbuf = ort.count.astype(np.int64), ort.zbuf
    ray = k.vol.astype(np.int64).sum(axis=0)
    s = k.stats
    assert (ray <= count).all()
    assert int(count.sum()) - int(ray.sum()) == s["below"] + s["above"] + s["nan"]
    assert int(count.sum()) == s["visits"]
    if s["below"] + s["above"] + s["nan"] == 0:
        assert np.array_equal(ray, count)
    _, nearest = R.section(k.vol)
    kz = R.slab(zbuf, k.slabs, *k.z_range)
    at = (count > 0) & (zbuf != np.float32(-1.0)) & (kz >= 0)
    assert np.array_equal(nearest[at], kz[at])
    if name in ("ps_small", "ss_small", "shrink_alt_tiny", "const_pos_wide"):
        assert at.sum() >= 100                 # the identity binds
    # (where it binds everywhere: the covered pixels are the pixels with a slab)
    if s["below"] + s["above"] + s["nan"] == 0 and not (zbuf[count > 0] == np.float32(-1.0)).any():
        assert np.array_equal(nearest >= 0, count > 0)


def _slab(sar, zf, slabs, z_lo, z_hi):
    return sar.volume_slab(zf, slabs=slabs, z_range=(z_lo, z_hi))


def test_slab_of_a_depth_is_the_restatement(sar):
    tiny = float(np.finfo(np.float32).tiny)
    sub = float(np.float32(1e-45))
    ranges = [(8, -8.0, 8.0), (7, -1e-23, 1e-23), (1, -1.0, 1.0), (1024, -0.37166813435032964, 0.37520987214520574), (5, 0.0, 2.5),
              (33, -3e38, 3e38), (3, -sub, sub)]
    for slabs, z_lo, z_hi in ranges:
        edges = [z_lo + (z_hi - z_lo) * e / slabs for e in range(slabs + 1)] if slabs <= 33 else [z_lo, z_hi, 0.0]
        zs = [np.float32(v) for e in edges for v in (e, np.nextafter(np.float32(e), np.float32(np.inf)), np.nextafter(np.float32(e), np.float32(-np.inf)))]
        zs += [np.float32(v) for v in (0.0, -0.0, sub, -sub, tiny, -tiny, 5e-24, -5e-24, 0.25, -1.0, math.inf, -math.inf, math.nan,
                                       3.4028235e38, -3.4028235e38)]
        want = R.slab(np.array(zs, dtype=np.float32), slabs, z_lo, z_hi)
        got = [_slab(sar, z, slabs, z_lo, z_hi) for z in zs]
        assert got == want.tolist(), (slabs, z_lo, z_hi)
    assert _slab(sar, math.inf, 8, -8.0, 8.0) == sar.VOLUME_ABOVE == -2 and _slab(sar, -math.inf, 8, -8.0, 8.0) == sar.VOLUME_BELOW == -1
    assert _slab(sar, math.nan, 8, -8.0, 8.0) == sar.VOLUME_NAN == -3
    assert _slab(sar, -0.0, 8, 0.0, 8.0) == 0 and _slab(sar, 8.0, 8, 0.0, 8.0) == sar.VOLUME_ABOVE and _slab(sar, 7.9999995, 8, 0.0, 8.0) == 7


def test_defaults_and_layouts(sar):
    from strange_attractor_renderer_amd import _abi
    p = sar.volume_params()
    assert (p.z_lo, p.z_hi, p.slabs, p.add) == (-1.0, 1.0, 64, 0)
    m = sar.volume_march_params()
    assert (m.half_count, m.t_min, m.pos_lo, m.pos_hi, m.k0, m.k1, list(m.background)) == (0.0, 0.0, 0.0, 1.0, 0, 0, [0, 0, 0])
    assert C.sizeof(_abi.SarVolumeParams) == 24 and C.sizeof(_abi.SarVolumeStats) == 64
    assert C.sizeof(_abi.SarVolumeMarchParams) == 48 and C.sizeof(_abi.SarVolumeMarchStats) == 16
    assert _abi.SarVolumeStats.vmax.offset == 48 and _abi.SarVolumeStats.z_max.offset == 56
    assert _abi.SarVolumeMarchParams.background.offset == 40
    assert set(_abi.VOLUME_OPTIONS) == {"volume_chunk", "volume_steps"} and not set(_abi.VOLUME_OPTIONS) & set(_abi.STABLE_OPTIONS)
    assert R.learned_range(-1.0, 3.0) == sar.volume_learned_range(-1.0, 3.0) == (-1.0625, 3.0625)
    assert R.learned_range(0.25, 0.25) == sar.volume_learned_range(0.25, 0.25) == (-0.25, 0.75)
    assert R.learned_range(math.inf, -math.inf) == sar.volume_learned_range(math.inf, -math.inf) == (-1.0, 1.0)


def test_refusals_that_need_no_device(sar):
    from strange_attractor_renderer_amd import _abi
    lib = sar.load_library()
    cfg = sar.Config.solar_sail(width=64, height=48)
    starts = np.full((4, 3), 0.1)
    st = _abi.SarVolumeStats()
    sp = starts.ctypes.data_as(C.POINTER(C.c_double))

    def call(cfg_=cfg, jobs=4, iters=16, s=sp, **fields):
        p = sar.volume_params(**fields)
        status = lib.sar_runtime_volume(C.byref(cfg_.c) if cfg_ is not None else None, None, C.byref(p), jobs, iters, s, C.byref(st))
        return status, lib.sar_last_error().decode()

    for fields, text in ((dict(slabs=0), "slabs must be 1 to 1024"), (dict(slabs=1025), "slabs must be 1 to 1024"),
                         (dict(z_lo=math.nan), "z_lo and z_hi must be finite"), (dict(z_hi=math.inf), "z_lo and z_hi must be finite"),
                         (dict(z_lo=1.0, z_hi=1.0), "z_hi - z_lo positive"), (dict(z_lo=2.0, z_hi=1.0), "z_hi - z_lo positive"),
                         (dict(z_lo=0.0, z_hi=5e-324, slabs=1024), "finite"),
                         (dict(add=2), "add must be 0 or 1"), (dict(add=-1), "add must be 0 or 1")):
        status, msg = call(**fields)
        assert status == _abi.SAR_ERR_INVALID and text in msg, (fields, status, msg)
    assert call(cfg_=None)[0] == _abi.SAR_ERR_INVALID
    assert call(cfg_=sar.Config.solar_sail(width=0, height=48))[0] == _abi.SAR_ERR_INVALID
    status, msg = call(cfg_=sar.Config.solar_sail(width=2048, height=1024), slabs=1024)
    assert status == _abi.SAR_ERR_INVALID and "2^30 voxels" in msg
    for kw, text in ((dict(jobs=0), "n_jobs must be 1 to 2^24"), (dict(jobs=(1 << 24) + 1, s=None), "n_jobs must be 1 to 2^24"),
                     (dict(iters=0), "iters_per_job must be 1 to 2^40"), (dict(iters=(1 << 40) + 1), "iters_per_job must be 1 to 2^40")):
        status, msg = call(**kw)
        assert status == _abi.SAR_ERR_INVALID and text in msg, (kw, status, msg)
    for bad in (math.nan, math.inf, -math.inf):
        s2 = starts.copy()
        s2[2, 1] = bad
        status, msg = call(s=s2.ctypes.data_as(C.POINTER(C.c_double)))
        assert status == _abi.SAR_ERR_INVALID and "start point 2 is not finite" in msg
    status, msg = call()                      # everything right but the runtime
    assert status == _abi.SAR_ERR_INVALID and "NULL" in msg
    # the readers
    count = np.zeros((48, 64), dtype=np.uint32)
    cp = count.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.sar_runtime_volume_section(None, 0, 1, cp, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_runtime_volume_read(None, 0, 1, cp) == _abi.SAR_ERR_INVALID
    assert lib.sar_runtime_volume_free(None) == _abi.SAR_ERR_INVALID
    img = np.zeros((48, 64, 4), dtype=np.uint16)
    ip = img.ctypes.data_as(C.POINTER(C.c_uint16))
    for fields, text in ((dict(half_count=-1.0), "half_count"), (dict(half_count=math.inf), "half_count"), (dict(half_count=math.nan), "half_count"),
                         (dict(t_min=1.0), "t_min"), (dict(t_min=-0.5), "t_min"), (dict(t_min=math.nan), "t_min"),
                         (dict(pos_lo=math.inf), "pos_lo"), (dict(pos_hi=math.nan), "pos_lo")):
        p = sar.volume_march_params(**fields)
        for entry in (lib.sar_runtime_volume_march, lib.sar_runtime_volume_march_device):
            assert entry(C.byref(cfg.c), None, C.byref(p), None, ip) == _abi.SAR_ERR_INVALID
            assert text in lib.sar_last_error().decode(), fields
    p = sar.volume_march_params()
    assert lib.sar_runtime_volume_march(None, None, C.byref(p), None, ip) == _abi.SAR_ERR_INVALID
    assert lib.sar_runtime_volume_march(C.byref(cfg.c), None, C.byref(p), None, ip) == _abi.SAR_ERR_INVALID   # no runtime
    assert lib.sar_volume_params_default(None) == _abi.SAR_ERR_INVALID and lib.sar_volume_march_params_default(None) == _abi.SAR_ERR_INVALID
    k = C.c_int32()
    assert lib.sar_volume_slab(None, 0.0, C.byref(k)) == _abi.SAR_ERR_INVALID
    assert lib.sar_volume_slab(C.byref(sar.volume_params()), 0.0, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_volume_slab(C.byref(sar.volume_params(slabs=0)), 0.0, C.byref(k)) == _abi.SAR_ERR_INVALID
    with pytest.raises(ValueError):
        sar.volume_params(slabs=-1)
    with pytest.raises(AttributeError):
        sar.volume_march_params(opacity=1.0)


def test_march_restatement_is_a_compositing(oracle):
    """What the restatement itself must satisfy, whatever the device does: an opaque image over a black background never exceeds the
    transparent one's premultiplied value, alpha is 1 - T, an empty pixel is the background, and a window sees its own slabs only."""
    k = K.case("ps_small")
    img_t, st_t = k.march("default", 1)
    img_o, st_o = k.march("default", 0)
    assert st_t == st_o and st_t["covered"] == int(np.count_nonzero(k.vol.any(axis=0))) and st_t["slabs_seen"] == k.stats["nonempty"]
    empty = ~k.vol.any(axis=0)
    assert (img_t[empty] == 0).all() and (img_o[empty] == (0, 0, 0, 65535)).all() and (img_o[..., 3] == 65535).all()
    assert (img_t[~empty][:, 3] > 0).all()
    bg = k.march("coloured", 0)[0]
    assert (bg[empty] == (65535, 1000, 30000, 65535)).all()
    win, st_w = k.march("window", 1)
    assert st_w["slabs_seen"] == int(np.count_nonzero(k.vol[2:k.slabs - 1]))
