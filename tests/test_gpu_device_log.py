"""GPU: the device logarithm and everything coloured through it, held to exact sets (tests/log_brackets.py).

The probe (include/sar_test_hooks.h: sar_runtime_debug_device_log) runs the kernels' own log and ln_u32 on planted and random
arguments: every result must be one of the two doubles that enclose the true logarithm (or its class's one value), and host libm's
inside the table. The sites — the Gas colorize in its four forms, the exposure record and the image under it, the gallery's tile
colorize, the plane's and the FTLE map's colorize — must then give, per pixel or record, a member of the set their stated expression
takes over those brackets. The conditions of every case (class sizes, set sizes, the oracle's membership) are
tests/test_log_brackets_host.py's.

Measured on an MI355X (ROCm 7.2), the figures this file prints: see DESIGN.md section 3."""
import math

import numpy as np
import pytest

import color_range_restatement as CR
import device_log_cases as K
import ftle_restatement as F
import log_brackets as LB
from ftle_cases import maps
from test_gpu_exposure import QPAIRS, STATES, _loaded, _record, restate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.poisson_saturne(width=K.W, height=K.H), device=0)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _palette(cfg):
    return [tuple(float(v) for v in row) for row in cfg.palette_rgb[:cfg.palette_len]]


# ---- the probe ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe_reference():
    """(u32 arguments, f64 arguments, the nearest double to each true logarithm): computed once."""
    u, x = K.probe_u32(), K.probe_f64()
    return u, x, np.array([LB.nearest(float(c)) for c in u]), np.array([LB.nearest(float(v)) for v in x])


def _shares(got, args, near, where):
    libm = np.array([K._c_log(float(v)) for v in args])
    same = lambda a, b: (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))   # noqa: E731
    n = int(where.sum())
    is_near, is_libm = same(got, near)[where], same(got, libm)[where]
    return n, int(is_near.sum()), int(is_libm.sum()), int((~is_near).sum())


def test_ln_u32_is_the_table_inside_it_and_a_bracket_member_beyond(sar, rt, probe_reference):
    u, _, near, _ = probe_reference
    got = rt.debug_device_log(u)
    assert got.dtype == np.float64 and got.shape == u.shape
    table = (u >= 1) & (u <= K.TABLE)
    libm = np.array([math.log(float(c)) for c in u[table]])
    assert np.array_equal(_bits(got[table]), _bits(libm)), u[table][_bits(got[table]) != _bits(libm)][:8]
    assert _bits(got[0]) == _bits(math.log(float(K.TABLE - 1))) and _bits(got[1]) == _bits(math.log(float(K.TABLE)))
    assert np.all(np.isneginf(got[u == 0])) and (u == 0).sum() == 1                 # the u32 wrap of count + 1
    inside = LB.members(got, u.astype(np.float64))
    worst = max(LB.ulp_distance(g, float(c)) for g, c in zip(got, u))
    n, is_near, is_libm, other = _shares(got, u, near, u > K.TABLE)
    print(f"ln_u32 beyond the table, {n} arguments: {is_near} the nearest double, {is_libm} host libm's value, {other} the other neighbour; "
          f"largest distance outside a bracket {worst} doubles")
    assert inside.all(), [(int(c), float(g)) for c, g in zip(u[~inside][:8], got[~inside][:8])]


def test_log_is_a_bracket_member_on_mantissas_binades_subnormals_and_the_classes(sar, rt, probe_reference):
    _, x, _, near = probe_reference
    got = rt.debug_device_log(x)
    inside = LB.members(got, x)
    finite = np.isfinite(x) & (x > 0)
    worst = max(LB.ulp_distance(g, v) for g, v in zip(got[finite], x[finite]))
    n, is_near, is_libm, other = _shares(got, x, near, finite)
    print(f"log, {n} finite positive arguments: {is_near} the nearest double, {is_libm} host libm's value, {other} the other neighbour; "
          f"largest distance outside a bracket {worst} doubles")
    assert inside.all(), [(float(v), float(g)) for v, g in zip(x[~inside][:8], got[~inside][:8])]
    cls = dict(zip([repr(v) for v in K.PROBE_F64_CLASSES], got[-len(K.PROBE_F64_CLASSES):]))
    assert cls["0.0"] == cls["-0.0"] == -math.inf and cls["inf"] == math.inf and all(math.isnan(cls[k]) for k in ("-1.0", "-inf", "nan"))
    assert _bits(got[2]) == _bits(0.0)                                               # log(1.0) = +0.0
    assert got[np.nonzero(x == 5e-324)[0][0]] in LB.bracket(5e-324) and -745.0 < got[np.nonzero(x == 5e-324)[0][0]] < -744.0


def test_the_probe_refuses_what_its_header_says(sar, rt):
    import ctypes as C
    lib = sar.load_library()
    one, out = np.ones(1), np.zeros(1)
    p, o = one.ctypes.data, out.ctypes.data_as(C.POINTER(C.c_double))
    for args in ((None, 0, p, 1, o), (rt.handle, 0, None, 1, o), (rt.handle, 0, p, 1, None), (rt.handle, 0, p, 0, o), (rt.handle, 2, p, 1, o),
                 (rt.handle, 1, p, (1 << 20) + 1, o)):
        assert lib.sar_runtime_debug_device_log(*args) == sar._abi.SAR_ERR_INVALID and "sar_runtime_debug_device_log" in lib.sar_last_error().decode()
    assert not out.any()
    with pytest.raises(TypeError):
        rt.debug_device_log(np.ones(3, dtype=np.float32))
    full = rt.debug_device_log(np.full(1 << 20, 3, dtype=np.uint32))                 # the hook's limit itself: every block of the grid
    assert np.all(_bits(full) == _bits(math.log(3.0)))


# ---- the Gas colorize on loaded states --------------------------------------------------------------------------------------------------
def _oracle_image(oracle, cfg, count, pos, zbuf, mx):
    ort = oracle.Runtime(cfg.c.width, cfg.c.height)
    ort.count[:] = count; ort.steps[:] = pos; ort.zbuf[:] = zbuf; ort.set_max(mx)
    return oracle.colorize(cfg.c, ort)


class _DeviceBuffer:
    """nbytes of zeroed device memory from the HIP runtime the library brought in (no torch: its import alone takes ten seconds)."""

    def __init__(self, nbytes: int):
        import ctypes as C
        self.hip, self.nbytes, self.ptr = C.CDLL(None), int(nbytes), C.c_void_p()
        for name, args in (("hipMalloc", [C.POINTER(C.c_void_p), C.c_size_t]), ("hipMemset", [C.c_void_p, C.c_int, C.c_size_t]),
                           ("hipMemcpy", [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]), ("hipFree", [C.c_void_p])):
            getattr(self.hip, name).argtypes, getattr(self.hip, name).restype = args, C.c_int
        assert self.hip.hipMalloc(C.byref(self.ptr), self.nbytes) == 0 and self.hip.hipMemset(self.ptr, 0, self.nbytes) == 0
        assert self.hip.hipDeviceSynchronize() == 0                                     # (the zeros are there before any stream writes)

    def read_u16(self) -> np.ndarray:
        out = np.empty(self.nbytes // 2, dtype=np.uint16)
        assert self.hip.hipMemcpy(out.ctypes.data, self.ptr, self.nbytes, 2) == 0      # hipMemcpyDeviceToHost
        return out

    def free(self):
        if self.ptr:
            self.hip.hipFree(self.ptr)
            self.ptr = None


def _hold(label, img, sets, classes, ref, first=0):
    """img's pixels [first, first + n) are members of their sets; bit-equal to the oracle where both logarithms come from the table."""
    px = np.asarray(img).reshape(-1, 4)
    n = px.shape[0]
    inside = LB.image_in_sets(px, sets[first:first + n])
    want = ref.reshape(-1, 4)[first:first + n]
    differ = (px != want).any(-1)
    print(f"{label}: {int(differ.sum())} of {n} pixels differ from the oracle, {int((~inside).sum())} are no member of their set")
    assert inside.all(), (label, np.nonzero(~inside)[0][:8] + first)
    table = classes.ravel()[first:first + n] == 0
    assert np.array_equal(px[table], want[table]), label


@pytest.mark.parametrize("transparent", [0, 1])
def test_gas_colorize_in_every_form_gives_members_of_the_sets(sar, oracle, gpu, transparent):
    cfg = sar.Config.poisson_saturne(width=K.W, height=K.H, transparent=transparent)
    pal, bright = _palette(cfg), (cfg.brightness_offset, cfg.brightness_factor)
    states = [K.gas_state(name) for name in K.GAS_STATES]
    rts = sar.Runtime.group(cfg, 2, device=0)
    first, n = K.RANGE_SLICE
    part, outs = _DeviceBuffer(n * 8), [_DeviceBuffer(K.W * K.H * 8) for _ in rts]
    try:
        refs = []
        for name, r, (count, steps, zbuf, mx) in zip(K.GAS_STATES, rts, states):
            r.load(count, steps, zbuf, mx)
            sets = LB.gas_image_sets(steps, count, mx, pal, bright, bool(transparent))
            classes, ref = LB.gas_class(count, mx), _oracle_image(oracle, cfg, count, steps, zbuf, mx)
            refs.append((sets, classes, ref))
            _hold(f"{name} colorize", sar.colorize(cfg, r), sets, classes, ref)
            # a slice, with the max the runtime's scalars hold
            sar.colorize_range_device(cfg, r, first, n, part.ptr.value)
            r.synchronize()
            _hold(f"{name} colorize_range_device", part.read_u16(), sets, classes, ref, first)
            # the window kernel: an applied colour range, the record the device's own
            r.set_color_range()
            w = sar.color_range(cfg, r)
            want = CR.window(count, steps)
            assert w.applied and (w.lo, w.hi, w.pos_lo, w.pos_hi, w.covered) == (want.lo, want.hi, want.pos_lo, want.pos_hi, want.covered)
            pos = CR.positions(steps, want)
            _hold(f"{name} colorize under a colour range", sar.colorize(cfg, r), LB.gas_image_sets(pos, count, mx, pal, bright, bool(transparent)),
                  classes, _oracle_image(oracle, cfg, count, pos, zbuf, mx))
            r.set_color_range(None)
        sar.colorize_device_batch([cfg, cfg], rts, [o.ptr.value for o in outs])
        rts[0].synchronize()
        for name, o, (sets, classes, ref) in zip(K.GAS_STATES, outs, refs):
            _hold(f"{name} colorize_device_batch", o.read_u16(), sets, classes, ref)
    finally:
        for r in rts:
            r.close()
        for b in [part] + outs:
            b.free()


# ---- exposure ------------------------------------------------------------------------------------------------------------------------------
EXPOSURE_STATES = {"big_61x17": STATES["big_61x17"], "ties_three_passes": STATES["ties_three_passes"], "max_alone_beyond": K.exposure_inside_state()}


@pytest.mark.parametrize("name", sorted(EXPOSURE_STATES))
def test_exposure_records_and_the_images_under_them_are_members(sar, gpu, name):
    count = EXPOSURE_STATES[name]
    M = int(count.max())
    assert M + 1 > K.TABLE
    cfg, r = _loaded(sar, count, M)
    try:
        kw = dict(cfg_offset=cfg.brightness_offset, cfg_factor=cfg.brightness_factor)
        libm = 0
        for qb, qw in QPAIRS:
            got = _record(sar.exposure(cfg, r, q_black=qb, q_white=qw))
            records, exact = LB.exposure_set(restate, count, M, q_black=qb, q_white=qw, **kw)
            assert got[2:6] == exact, (qb, qw, got)                                   # the counts and `covered` are exact as before
            assert (LB.float_bits(got[0]), LB.float_bits(got[1]), got[6]) in records, (qb, qw, got, len(records))
            want = restate(count, M, qb, qw, **kw)
            libm += int(LB.float_bits(got[0]) == LB.float_bits(want[0]) and LB.float_bits(got[1]) == LB.float_bits(want[1]))
        print(f"{name}: {libm} of {len(QPAIRS)} records equal host libm's restatement bit for bit")
        # the image under the mode, with the record the device returned
        r.set_exposure()
        e = sar.exposure(cfg, r)
        assert e.applied
        img = sar.colorize(cfg, r)
        sets = LB.gas_image_sets(r.steps(), count, M, _palette(cfg), (e.offset, e.factor), bool(cfg.c.transparent))
        inside = LB.image_in_sets(img, sets)
        many = sum(len(s) > 1 for s in sets)
        print(f"{name}: image under the mode, {int((~inside).sum())} of {inside.size} pixels no member of their set, {many} sets of more than one tuple")
        assert inside.all(), np.nonzero(~inside)[0][:8]
    finally:
        r.close()


# ---- the gallery's tile colorize -----------------------------------------------------------------------------------------------------------
def test_a_gallery_tile_of_two_piled_pixels_beyond_the_table(sar, rt):
    base = sar.Config.poisson_saturne(transparent=1, render_kind=sar.SAR_RENDER_GAS, **K.gallery_view())
    items = sar.gallery_items(K.IDENTITY.reshape(1, 30), [((0.0, 0.0, 0.0), 1.0)], base=base)
    g = sar.gallery(rt, base, items, tile=(2, 1), cols=1, jobs=K.GALLERY_JOBS, iterations=K.GALLERY_JOBS * K.GALLERY_ITERATIONS,
                    starts=K.gallery_starts(), raw=True)
    count = g.count[0]
    assert tuple(int(v) for v in count.ravel()) == K.GALLERY_COUNTS and int(g.stats[0]["max"]) == max(K.GALLERY_COUNTS)
    sets = LB.gas_image_sets(g.steps[0], count, max(K.GALLERY_COUNTS), _palette(base), (base.brightness_offset, base.brightness_factor), True)
    tile = g.tile(0)
    assert tile.shape == (1, 2, 4) and LB.image_in_sets(tile, sets).all(), (tile.tolist(), sets)
    assert tile[0, 0, 3] < 65535 == tile[0, 1, 3] and tile[..., :3].any()            # the fuller pixel is the max: factor 1; the other is not


# ---- the plane's and the FTLE map's colorize ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(K.PLANES))
def test_plane_colorize_gives_members_of_the_sets(sar, rt, name):
    import plane_restatement as P
    p = K.PLANES[name]
    cfg = getattr(sar.Config, p["preset"])()
    base = np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    xr, yr = [(base[a] - p["d"], base[a] + p["d"]) for a in p["axes"]]
    pl = sar.lyapunov_plane(rt, base, p["axes"], xr, yr, p["width"], p["height"], p["mode"], transient=p["transient"], steps=p["steps"])
    img = pl.colorize(cfg, **p["colors"])
    k = 3 if p["mode"] == "spectrum" else 1
    rec = pl.records
    stack = LB.plane_candidates(pl.status, rec["steps_done"], rec["log2_exp"], rec["mant"], k, _palette(cfg), **p["colors"])
    inside = LB.stack_member(img, stack)
    want = P.colorize(pl.status, rec["steps_done"], rec["lyapunov"][..., 0], _palette(cfg), **p["colors"])
    bounded = pl.status == sar.SAR_SEARCH_BOUNDED
    print(f"{name}: {int((img != want).any(-1).sum())} of {img.shape[0] * img.shape[1]} pixels differ from the restatement with host libm, "
          f"{int((~inside).sum())} are no member of their set, {int((LB.stack_sizes(stack) > 1).sum())} sets of more than one colour")
    assert inside.all(), np.argwhere(~inside)[:8]
    assert bounded.sum() >= 100 and np.array_equal(img[~bounded], want[~bounded])       # the pixels include/sar.h states exactly


@pytest.fixture(scope="module")
def ftle_cases(sar):
    return {name: (c, kw) for name, c, kw in maps(sar) if name in K.FTLE_MAPS}


@pytest.mark.parametrize("name", K.FTLE_MAPS)
def test_ftle_colorize_gives_members_of_the_sets(sar, rt, ftle_cases, name):
    c, kw = ftle_cases[name]
    cfg = sar.Config.solar_sail()
    m = sar.ftle_map(rt, c, **kw)
    for window, fade in K.FTLE_WINDOWS:
        img = m.colorize(cfg, **({} if window is None else dict(window=window, fade=fade)))
        lo, hi = m.window() if window is None else window
        fade_ = 32.0 if fade is None else fade
        stack = LB.ftle_candidates(m.status, m.escape_step, m.flags, m.stretch2, kw["steps"], _palette(cfg), lo, hi, fade_)
        inside = LB.stack_member(img, stack)
        want = F.colorize(m.status, m.escape_step, m.flags, m.ftle, _palette(cfg), lo, hi, fade=fade_)
        print(f"{name} {window}: {int((img != want).any(-1).sum())} of {inside.size} pixels differ from the restatement with host libm, "
              f"{int((~inside).sum())} are no member of their set, {int((LB.stack_sizes(stack) > 1).sum())} sets of more than one colour")
        assert inside.all(), np.argwhere(~inside)[:8]
        exact = (m.status == sar.SAR_SEARCH_DIVERGED) | ((m.flags & sar.SAR_FTLE_EDGE) != 0) | ~np.isfinite(m.ftle)
        assert np.array_equal(img[exact], want[exact]) and np.all(img[..., 3] == 65535)   # the pixels include/sar.h states exactly
