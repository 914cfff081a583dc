"""Host: tests/log_brackets.py — the reference of the device logarithm — held to facts from elsewhere, its candidate functions to the
restatements they are built on, the conditions of every case of tests/test_gpu_device_log.py computed from the reference alone, and
what the sets do and do not tell of a wrong logarithm."""
import math

import numpy as np
import pytest

import color_range_restatement as CR
import device_log_cases as K
import ftle_restatement as F
import log_brackets as LB
import plane_restatement as P
from log_brackets import S2
from test_gpu_exposure import QPAIRS, STATES, restate

EXPOSURE_STATES = {"big_61x17": STATES["big_61x17"], "ties_three_passes": STATES["ties_three_passes"], "max_alone_beyond": K.exposure_inside_state()}
PALETTE, BRIGHTNESS = S2.DEFAULT_PALETTE, S2.BRIGHTNESS


def _finite_arguments():
    x = K.probe_f64()
    x = x[np.isfinite(x) & (x > 0)]
    u = K.probe_u32().astype(np.float64)
    return np.concatenate([x, u[u > 0]])


# ---- bracket against facts from elsewhere ----------------------------------------------------------------------------------------------
def test_host_libm_lies_in_every_bracket():
    for x in _finite_arguments():
        assert LB.member(math.log(x), x), x


def test_a_200_bit_logarithm_rounds_into_every_bracket():
    mpmath = pytest.importorskip("mpmath")
    with mpmath.workprec(200):
        for x in _finite_arguments():
            y = float(mpmath.log(mpmath.mpf(float(x))))           # rounded to nearest
            assert LB.member(y, x) and y == LB.nearest(x), x


def test_bracket_of_one_and_the_classes():
    assert LB.bracket(1.0) == (0.0, 0.0) and math.copysign(1.0, LB.bracket(1.0)[0]) == 1.0
    assert LB.bracket(0.0) == LB.bracket(-0.0) == (-math.inf, -math.inf)
    assert LB.bracket(math.inf) == (math.inf, math.inf)
    for x in (-1.0, -5e-324, -math.inf, math.nan):
        assert all(v != v for v in LB.bracket(x)), x
    assert LB.member(math.nan, -1.0) and LB.member(math.nan, math.nan) and not LB.member(0.0, -1.0) and not LB.member(math.nan, 2.0)
    assert LB.member(-math.inf, 0.0) and not LB.member(math.inf, 0.0) and not LB.member(-0.0, 1.0)
    lo, hi = LB.bracket(5e-324)                                    # a subnormal argument brackets like any other
    assert lo < hi == math.nextafter(lo, math.inf) and lo <= math.log(5e-324) <= hi and abs(lo + 744.4400719213812) < 1e-12
    lo, hi = LB.bracket(2.0)
    assert (lo, hi) == (0.6931471805599453, math.nextafter(0.6931471805599453, 1.0))   # ln 2 = 0.693147180559945309417...
    assert LB.ulp_distance(lo, 2.0) == 0 and LB.ulp_distance(math.nextafter(lo, 0.0), 2.0) == 1 and LB.ulp_distance(math.nextafter(hi, 1.0), 2.0) == 1


def test_brackets_are_monotone_over_neighbouring_doubles():
    rng = np.random.default_rng(60)
    starts = [0.5, 1.0, math.nextafter(1.0, 0.0), 5e-324, 2.0 ** -1022, 1e308, float(K.TABLE)] + list(np.ldexp(1.0 + rng.random(40), rng.integers(-1022, 1023, size=40).astype(np.int32)))
    for x in starts:
        prev = LB.bracket(x)
        for _ in range(8):
            x = math.nextafter(x, math.inf)
            cur = LB.bracket(x)
            assert cur[0] >= prev[0] and cur[1] >= prev[1] and cur[0] <= cur[1], x
            prev = cur


def test_ln_u32_set_is_the_table_the_bracket_or_the_wrap():
    assert LB.ln_u32_set(0) == (-math.inf,)
    assert LB.ln_u32_set(1) == (0.0,)
    assert LB.ln_u32_set(K.TABLE) == (math.log(float(K.TABLE)),) and LB.ln_u32_set(K.TABLE - 1) == (math.log(float(K.TABLE - 1)),)
    assert LB.ln_u32_set(K.TABLE + 1) == LB.bracket(float(K.TABLE + 1)) and len(set(LB.ln_u32_set(K.TABLE + 1))) == 2
    assert LB.ln_u32_set(LB.M32) == LB.bracket(4294967295.0)


def test_the_probes_arguments_are_the_stated_ones():
    u, x = K.probe_u32(), K.probe_f64()
    assert u.dtype == np.uint32 and u.size == 4 + 33 + 3 + 4096 + 256 and x.size == 4 + 2048 + 2048 + 2 + len(K.PROBE_F64_CLASSES)
    assert list(u[:4]) == [K.TABLE - 1, K.TABLE, K.TABLE + 1, K.TABLE + 2] and {0, 1, LB.M32, 1 << 31, (1 << 31) + 1} <= set(int(v) for v in u)
    assert (u[40:40 + 4096] > K.TABLE).all() and (u[40 + 4096:] <= K.TABLE).all() and (u[40 + 4096:] >= 1).all()
    m, w = x[4:4 + 2048], x[4 + 2048:4 + 4096]
    assert (m >= 0.5).all() and (m < 1.0).all() and w.min() < 2.0 ** -900 and w.max() > 2.0 ** 900 and (w >= 2.0 ** -1022).all() and np.isfinite(w).all()
    assert len(set(np.frexp(w)[1])) > 1200                           # the binades from 2^-1022 to 2^1023


# ---- the candidate functions restate the same expressions -----------------------------------------------------------------------------------
def _libm_only(c):
    return (-math.inf,) if c == 0 else (math.log(float(c)),)


def _s2_runtime(count, steps, mx):
    rt = S2.Runtime(count.shape[1], count.shape[0])
    rt.count, rt.steps, rt.max = [int(v) for v in count.ravel()], [float(v) for v in steps.ravel()], int(mx)
    return rt


def _oracle_image(sar, oracle, count, steps, zbuf, mx, transparent, brightness=None):
    h, w = count.shape
    cfg = sar.Config.poisson_saturne(width=w, height=h, transparent=transparent)
    if brightness is not None:
        cfg = cfg.replace(brightness_offset=brightness[0], brightness_factor=brightness[1])
    assert [tuple(float(v) for v in r) for r in cfg.palette_rgb[:cfg.palette_len]] == PALETTE
    assert brightness is not None or (cfg.brightness_offset, cfg.brightness_factor) == BRIGHTNESS
    ort = oracle.Runtime(w, h)
    ort.count[:] = count; ort.steps[:] = steps; ort.zbuf[:] = zbuf; ort.set_max(mx)
    return oracle.colorize(cfg.c, ort)


@pytest.mark.parametrize("window", [False, True])
@pytest.mark.parametrize("transparent", [0, 1])
@pytest.mark.parametrize("name", K.GAS_STATES)
def test_gas_sets_fed_libm_are_the_restatement_and_the_oracle(sar, oracle, name, transparent, window):
    count, steps, zbuf, mx = K.gas_state(name)
    w = CR.window(count, steps)
    assert w.applied
    pos = CR.positions(steps, w) if window else steps
    sets = LB.gas_image_sets(pos, count, mx, PALETTE, BRIGHTNESS, bool(transparent), sets=_libm_only)
    assert all(len(s) == 1 for s in sets)
    mine = np.array([next(iter(s)) for s in sets], dtype=np.uint16).reshape(count.shape + (4,))
    nan = np.isnan(pos)                             # (the restatement's math.floor refuses them: those pixels are the oracle's below)
    restated = np.array(S2.colorize_gas(_s2_runtime(count, np.where(nan, 0.0, pos), mx), PALETTE, BRIGHTNESS, bool(transparent)),
                        dtype=np.uint16).reshape(mine.shape)
    wrapped = count == LB.M32                       # the restatement's counts are Python ints: count + 1 does not wrap there
    assert wrapped.sum() == 3 and 1 <= nan.sum() <= 8 and np.array_equal(mine[~wrapped & ~nan], restated[~wrapped & ~nan])
    assert np.array_equal(mine, _oracle_image(sar, oracle, count, pos, zbuf, mx, transparent))


def test_exposure_sets_fed_libm_are_the_restatement():
    for name, count in EXPOSURE_STATES.items():
        M = int(count.max())
        for qb, qw in QPAIRS:
            want = restate(count, M, qb, qw)
            got, exact = LB.exposure_set(restate, count, M, sets=_libm_only, q_black=qb, q_white=qw)
            assert got == {(LB.float_bits(want[0]), LB.float_bits(want[1]), want[6])} and exact == want[2:6], (name, qb, qw)


@pytest.fixture(scope="module")
def planes():
    """name -> (parameters, the restatement's plane)."""
    base = np.array(S2.POISSON["x"] + S2.POISSON["y"] + S2.POISSON["z"])
    out = {}
    for name, p in K.PLANES.items():
        xr, yr = [(base[a] - p["d"], base[a] + p["d"]) for a in p["axes"]]
        out[name] = (p, P.plane(base, p["axes"], xr, yr, p["width"], p["height"], p["mode"], transient_steps=p["transient"], steps=p["steps"]))
    return out


def _libm_logs(x):
    with np.errstate(all="ignore"):
        return np.array([K._c_log(float(v)) for v in np.ravel(x)]).reshape(np.shape(x))


@pytest.mark.parametrize("name", sorted(K.PLANES))
def test_plane_image_fed_libm_is_the_restatement(planes, name):
    p, pl = planes[name]
    k = 3 if p["mode"] == "spectrum" else 1
    mine = LB.plane_image(pl["status"], pl["steps_done"], pl["log2_exp"], _libm_logs(pl["mant"]), k, PALETTE, **p["colors"])
    assert np.array_equal(mine, P.colorize(pl["status"], pl["steps_done"], pl["lyapunov"][..., 0], PALETTE, **p["colors"]))
    bounded = pl["status"] == P.BOUNDED
    assert bounded.sum() >= 100 and mine[bounded][:, :3].any()
    stack = LB.plane_candidates(pl["status"], pl["steps_done"], pl["log2_exp"], pl["mant"], k, PALETTE, **p["colors"])
    many = LB.stack_sizes(stack) > 1
    print(name, "pixels with more than one candidate colour:", int(many.sum()), "of", many.size)
    assert stack.shape[0] == 2 ** k and LB.stack_member(mine, stack).all() and many.mean() <= 0.01


@pytest.fixture(scope="module")
def ftle_pictures(sar):
    from ftle_cases import maps
    return {name: (kw, F.ftle(c, **kw)) for name, c, kw in maps(sar) if name in K.FTLE_MAPS}


@pytest.mark.parametrize("name", K.FTLE_MAPS)
def test_ftle_image_fed_libm_is_the_restatement(ftle_pictures, name):
    kw, m = ftle_pictures[name]
    for window, fade in K.FTLE_WINDOWS:
        lo, hi = F.window(m["ftle"]) if window is None else window
        fade = 32.0 if fade is None else fade
        mine = LB.ftle_image(m["status"], m["escape_step"], m["flags"], _libm_logs(m["stretch2"]), kw["steps"], PALETTE, lo, hi, fade)
        assert np.array_equal(mine, F.colorize(m["status"], m["escape_step"], m["flags"], m["ftle"], PALETTE, lo, hi, fade=fade))
        stack = LB.ftle_candidates(m["status"], m["escape_step"], m["flags"], m["stretch2"], kw["steps"], PALETTE, lo, hi, fade)
        many = LB.stack_sizes(stack) > 1
        print(name, window, "pixels with more than one candidate colour:", int(many.sum()), "of", many.size)
        assert LB.stack_member(mine, stack).all() and many.mean() <= 0.01


# ---- the conditions of the GPU cases ------------------------------------------------------------------------------------------------------
def test_gas_cases_hold_their_conditions(sar, oracle):
    classes = np.zeros(4, dtype=np.int64)
    for name in K.GAS_STATES:
        count, steps, zbuf, mx = K.gas_state(name)
        assert count.shape == (K.H, K.W) and ((mx + 1 <= K.TABLE) == (name == "max_in_table"))
        classes += np.bincount(LB.gas_class(count, mx).ravel(), minlength=4)
        for c in (K.TABLE - 2, K.TABLE - 1, K.TABLE, LB.M32):
            assert (count == c).sum() >= 3, (name, c)
        short = (count == 0) & ~np.isnan(steps)
        assert short.sum() >= 400 and ((count == 0) & np.isnan(steps)).sum() >= 1 and np.isnan(steps[count != 0]).any()
        assert (steps[count != 0] < 0).any() and (steps[count != 0] >= 1).any() and np.isinf(steps).any()
        for transparent in (0, 1):
            for window in (False, True):
                pos = CR.positions(steps, CR.window(count, steps)) if window else steps
                sets = LB.gas_image_sets(pos, count, mx, PALETTE, BRIGHTNESS, bool(transparent))
                many = np.array([len(s) > 1 for s in sets])
                inside = LB.image_in_sets(_oracle_image(sar, oracle, count, pos, zbuf, mx, transparent), sets)
                print(name, "transparent", transparent, "window", window, "pixels with more than one candidate tuple:", int(many.sum()), "of", many.size)
                assert many.mean() <= 0.01 and inside.all()
    print("pixels per class (in/in, beyond/in, in/beyond, beyond/beyond):", classes.tolist())
    assert (classes >= 100).all()


def test_exposure_cases_hold_their_conditions():
    for name, count in EXPOSURE_STATES.items():
        M = int(count.max())
        assert M + 1 > K.TABLE, name
        sizes = []
        for qb, qw in QPAIRS:
            got, exact = LB.exposure_set(restate, count, M, q_black=qb, q_white=qw)
            want = restate(count, M, qb, qw)
            assert (LB.float_bits(want[0]), LB.float_bits(want[1]), want[6]) in got and 1 <= len(got) <= 8
            sizes.append(len(got))
        print(name, "candidate records per quantile pair:", sizes)
    plain = restate(EXPOSURE_STATES["max_alone_beyond"], K.EXPOSURE_INSIDE_MAX)
    assert plain[2] + 1 <= K.TABLE and plain[3] + 1 <= K.TABLE and plain[5] == K.EXPOSURE_INSIDE_MAX and plain[6] == 1


def test_the_gallery_tile_piles_two_unequal_counts_beyond_the_table(sar, oracle):
    cfg = sar.Config.poisson_saturne(width=2, height=1, iterations=K.GALLERY_JOBS * K.GALLERY_ITERATIONS, jobs_total=K.GALLERY_JOBS, transparent=1, render_kind=sar.SAR_RENDER_GAS,
                                     coeff_x=K.IDENTITY[:10], coeff_y=K.IDENTITY[10:20], coeff_z=K.IDENTITY[20:], **K.gallery_view())
    ort = oracle.Runtime(2, 1)
    oracle.render_jobs(cfg.c, ort, K.gallery_starts(), K.GALLERY_ITERATIONS)
    assert tuple(int(v) for v in ort.count.ravel()) == K.GALLERY_COUNTS and ort.max == max(K.GALLERY_COUNTS)
    assert K.GALLERY_COUNTS[0] != K.GALLERY_COUNTS[1] and min(K.GALLERY_COUNTS) + 1 > K.TABLE
    sets = LB.gas_image_sets(ort.steps, ort.count, int(ort.max), PALETTE, BRIGHTNESS, True)
    assert LB.image_in_sets(oracle.colorize(cfg.c, ort), sets).all() and len(sets[0] | sets[1]) > 1


# ---- sensitivity: what a wrong logarithm does to the probe's membership test and to the sets ------------------------------------------------------
def _device_like(log):
    """ln_u32 with `log` in the device's place: the table stays host libm's."""
    return lambda c: math.log(float(c)) if 0 < c <= K.TABLE else log(float(c))


@pytest.mark.parametrize("stand_in", sorted(K.STAND_INS))
def test_what_rejects_a_wrong_logarithm(stand_in):
    log = K.STAND_INS[stand_in]
    ln = _device_like(log)
    # the probe's membership test
    x = K.probe_f64()
    u = K.probe_u32()
    bad = sum(not LB.member(log(float(v)), float(v)) for v in x) + sum(not LB.member(ln(int(c)), float(c)) for c in u if c > K.TABLE)
    print(stand_in, "probe results outside their bracket:", bad, "of", x.size + int((u > K.TABLE).sum()))
    assert bad > 0
    # the exposure sets
    rejected = total = 0
    for name, count in EXPOSURE_STATES.items():
        M = int(count.max())
        for qb, qw in QPAIRS:
            r = LB.restate_with(restate, ln, count, M, qb, qw)
            got, _ = LB.exposure_set(restate, count, M, q_black=qb, q_white=qw)
            total += 1
            rejected += (LB.float_bits(r[0]), LB.float_bits(r[1]), r[6]) not in got
    print(stand_in, "exposure records outside their set:", rejected, "of", total)
    assert rejected > 0
    # the image sets: the second line
    pixels = outside = 0
    for name in K.GAS_STATES:
        count, steps, zbuf, mx = K.gas_state(name)
        sets = LB.gas_image_sets(steps, count, mx, PALETTE, BRIGHTNESS, True)
        img = [LB.gas_pixel(float(s), ln((int(c) + 1) & LB.M32), ln((mx + 1) & LB.M32), PALETTE, BRIGHTNESS, True) for s, c in zip(steps.ravel(), count.ravel())]
        outside += int((~LB.image_in_sets(np.array(img), sets)).sum())
        pixels += count.size
    print(stand_in, "Gas pixels outside their set:", outside, "of", pixels)
    if stand_in == "float32":
        assert outside > 0          # 2^-24 relative moves a 16-bit channel in many pixels
    else:
        assert outside <= pixels // 100   # a few ulps reach a channel only where it sits on an integer's edge: the images cannot tell


def test_the_probe_is_in_the_hooks_build_alone(sar):
    """The product exports no sar_runtime_debug_device_log and include/sar.h does not name it; the hooks build has it, and without a
    runtime it refuses before any device call."""
    import ctypes as C
    import os
    from strange_attractor_renderer_amd import _abi
    hook = "sar_runtime_debug_device_log"
    product, hooks = C.CDLL(_abi.LIB_PATH), C.CDLL(_abi.HOOKS_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sar.h")).read()
    assert not hasattr(product, hook) and hasattr(hooks, hook) and hook not in header
    assert hook in _abi.OPTIONAL_PROTOTYPES and hook not in _abi.PROTOTYPES and callable(sar.Runtime.debug_device_log)
    one, out = np.ones(1), np.zeros(1)
    lib = sar.load_library()
    assert lib.sar_runtime_debug_device_log(None, 0, one.ctypes.data, 1, out.ctypes.data_as(C.POINTER(C.c_double))) == _abi.SAR_ERR_INVALID
    assert "NULL" in lib.sar_last_error().decode() and not out.any()
