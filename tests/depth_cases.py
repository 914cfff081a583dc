"""What the depth-case tests share (tests/test_depth_cases_host.py, tests/test_gpu_depth_cases.py): maps built so that a render
itself reaches the depth states the presets never show — every visit a depth candidate, depths outside (-1, 1) and outside any
range a warm-up measured, exact ties between jobs on every pixel, +-inf, depths at and below the -1 sentinel, subnormals, -0.0,
frames whose depths are all negative or all equal.

The carrier is Hénon in (x, y); z is decoupled and linear, z' = b + a z. The view is the identity (rotation_angle 0 and angle 0:
sin 0 is exactly 0), so the pixel comes from (x, y) alone and the depth is exactly -(z + cy), cy = center_camera[1]. Colours are
solar-sail's AdjustedVelocity. Every case runs JOBS jobs of n iterations at both SIZES; 256 x 64 has a power-of-two width and a
height that is a multiple of eight, so 16-bit depth hints live in 8 x 8 tiles there.

`check_condition` asserts, on the ORACLE's result only, that a case still reaches the state it was built for (a change to the
start-point stream, say, must not quietly take a case's point away); the figures measured when the cases were made are in the
table's comments as 96 x 64 / 256 x 64. Coefficient order within a row: 1, x, x^2, xy, xz, y, y^2, yz, z, z^2."""
from __future__ import annotations

import math

import numpy as np

import oracle_lib

SEED, JOBS = 7, 320
SIZES = ((96, 64), (256, 64))
SCALE = 0.35
D = 2.0 ** -10
HENON_X = (1.0, 0.0, -1.4, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0)
HENON_Y = (0.0, 0.3, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
AV_OFFSET, AV_FACTOR = 0.8, -0.2

# name -> a, b, cy, starts ("nat": the stream of SEED; "tied": every z = 2^-5; "sentinel": z = 2^-6 on odd jobs, 0.2 z on even
# ones), n
CASES = {
    # each job's depth rises by d a step: every visit beats all earlier ones of its job. set = covered = 367 / 1169, depths 1.36-2.44
    "rising": dict(a=1.0, b=-D, cy=0.0, starts="nat", n=1500),
    # depths 5.36-6.44: beyond the default quantiser's [-1, 3) and beyond any range a warm-up saw
    "rising_far": dict(a=1.0, b=-D, cy=-4.0, starts="nat", n=1500),
    # all jobs share one depth per step: order-dependent 116 / 136
    "rising_tied": dict(a=1.0, b=-D, cy=0.0, starts="tied", n=1500),
    # depth falls through -1: visited but unset 16 / 266, set 348 / 898, every depth negative (max -0.978); odd jobs hit exactly
    # -1.0f at counted iteration 8; Depth image max 1411 / 1465 (the fold's 0.0 seed in effect)
    "falling_sentinel": dict(a=1.0, b=D, cy=0.0, starts="sentinel", n=400),
    # the sign alternates, |depth| passes f32::MAX during the counted iterations: +inf 364 / 1164, finite 1 / 3, order-dependent 363 / 1154
    "alt_inf": dict(a=-1.05, b=0.0, cy=0.0, starts="nat", n=1500),
    # +-inf already in the warm-up (the measured hint range has an infinite span): every set pixel +inf, 365 / 1166
    "alt_inf_warm": dict(a=-1.1, b=0.0, cy=0.0, starts="nat", n=1200),
    # ~365 counted iterations at +-inf depth, then z^2 overflows, x is NaN and the rest land on pixel (0, 0): 75 025 of 192 000;
    # steps = -inf on 3 / 12 pixels
    "overflow_mid": dict(a=-1.3, b=0.0, cy=0.0, starts="nat", n=600),
    # depth rises to -0.0 through the f32 subnormals: subnormal 276 / 1068, -0.0 on 90 / 96
    "shrink_neg": dict(a=0.95, b=0.0, cy=0.0, starts="nat", n=900),
    # both signs, |depth| <= 5e-24; the Depth image has 365 / 1148 distinct levels
    "shrink_alt": dict(a=-0.95, b=0.0, cy=0.0, starts="nat", n=900),
    # one depth everywhere: every pixel a tie, order-dependent 364 / 1162; Depth image all zero (0 / 0, and (z - min) = 0 under the seed)
    "const_pos": dict(a=0.0, b=-0.25, cy=0.0, starts="nat", n=600),
    "const_neg": dict(a=0.0, b=0.25, cy=0.0, starts="nat", n=600),
}
NAMES = tuple(CASES)
NAT = tuple(c for c in NAMES if CASES[c]["starts"] == "nat")        # the cases whose start points are the plain stream
START_SETS = ("nat", "tied", "sentinel")


def coeff_z(case) -> list:
    z = [0.0] * 10
    z[0], z[8] = CASES[case]["b"], CASES[case]["a"]
    return z


def _fields(case, size, jobs, n, kw) -> dict:
    f = dict(coeff_x=HENON_X, coeff_y=HENON_Y, coeff_z=coeff_z(case), rotation_axis=(0.0, 0.0, 1.0), rotation_angle=0.0, angle=0.0,
             center_camera=(0.0, CASES[case]["cy"], 0.0), scale=SCALE, color_transform=oracle_lib.SAR_CT_ADJUSTED_VELOCITY,
             ct_offset=AV_OFFSET, ct_factor=AV_FACTOR, width=size[0], height=size[1], iterations=jobs * n, jobs_total=jobs, seed=SEED)
    f.update(kw)
    return f


def config(mod, case, size, jobs=JOBS, n=None, **kw):
    """The case's config at `size` for `jobs` jobs of `n` (default the case's) iterations each: a Config of the product package
    (through Config.replace alone), or the oracle's config structure when `mod` is oracle_lib. `kw` replaces further fields."""
    f = _fields(case, size, jobs, CASES[case]["n"] if n is None else n, kw)
    if hasattr(mod, "Config"):
        return mod.Config.solar_sail().replace(**f)
    c = mod.solar_sail()
    for k, v in f.items():
        if isinstance(v, (tuple, list)):
            for i, x in enumerate(v):
                getattr(c, k)[i] = x
        else:
            setattr(c, k, v)
    return c


def preset(case) -> dict:
    """The case as tests/golden/second_restatement.py takes a map."""
    return dict(x=list(HENON_X), y=list(HENON_Y), z=coeff_z(case), center_camera=(0.0, CASES[case]["cy"], 0.0), axis=(0.0, 0.0, 1.0),
                rotation=0.0, scale=SCALE, transform=("adjusted_velocity", AV_OFFSET, AV_FACTOR))


def start_set(name) -> np.ndarray:
    st = oracle_lib.start_points(SEED, 0, JOBS)
    if name == "tied":
        st[:, 2] = 2.0 ** -5
    elif name == "sentinel":
        st[1::2, 2] = 2.0 ** -6
        st[0::2, 2] *= 0.2
    else:
        assert name == "nat", name
    return st


def starts(case) -> np.ndarray:
    return start_set(CASES[case]["starts"])


class State:
    """What a render left, frozen: count, max, zbuf, steps and the three images the tests compare."""

    def __init__(self, oracle, cfg, ort):
        self.count, self.max, self.zbuf, self.steps = ort.count.copy(), ort.max, ort.zbuf.copy(), ort.steps.copy()
        c = oracle.copy_config(cfg)
        c.render_kind = oracle.SAR_RENDER_DEPTH
        self.depth = oracle.colorize(c, ort)
        c.render_kind = oracle.SAR_RENDER_GAS
        self.gas = []
        for transparent in (0, 1):
            c.transparent = transparent
            self.gas.append(oracle.colorize(c, ort))
        for a in (self.count, self.zbuf, self.steps, self.depth, *self.gas):
            a.setflags(write=False)

    def image(self, kind, transparent=1):
        return self.depth if kind == oracle_lib.SAR_RENDER_DEPTH else self.gas[transparent]


_CACHE = {}


def oracle_runtime(oracle, case, size, lo=0, hi=JOBS, start_name=None, n=None, reverse=False):
    """A fresh oracle runtime with jobs [lo, hi) of the case (of start set `start_name`, default the case's own; `n` iterations,
    default the case's) rendered in order — or in reverse order. Not cached: the caller may merge into it."""
    st = start_set(start_name or CASES[case]["starts"])[lo:hi]
    n = CASES[case]["n"] if n is None else n
    ort = oracle.Runtime(*size)
    oracle.render_jobs(config(oracle, case, size, jobs=hi - lo, n=n), ort, st[::-1] if reverse else st, n)
    return ort


def freeze(oracle, case, size, ort) -> State:
    return State(oracle, config(oracle, case, size), ort)


def reference(oracle, case, size, lo=0, hi=JOBS, start_name=None, n=None, reverse=False) -> State:
    """The oracle's sequential render of jobs [lo, hi), once per argument set and module run; read-only."""
    key = (case, tuple(size), lo, hi, start_name or CASES[case]["starts"], CASES[case]["n"] if n is None else n, reverse)
    if key not in _CACHE:
        _CACHE[key] = freeze(oracle, case, size, oracle_runtime(oracle, case, size, lo, hi, start_name, n, reverse))
    return _CACHE[key]


def bits(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def order_dependent(oracle, case, size) -> int:
    """Pixels whose `steps` change when the jobs are rendered in reverse order: the pixels a tie between jobs decides."""
    return int(np.count_nonzero(bits(reference(oracle, case, size).steps) != bits(reference(oracle, case, size, reverse=True).steps)))


def figures(oracle, case, size) -> dict:
    """The numbers the conditions are about, from the oracle's render."""
    ref = reference(oracle, case, size)
    covered, is_set = ref.count > 0, ref.zbuf != np.float32(-1.0)
    z = ref.zbuf[is_set]
    tiny = np.finfo(np.float32).tiny
    return dict(covered=int(covered.sum()), set=int(is_set.sum()), unset_visited=int((covered & ~is_set).sum()),
                set_unvisited=int((is_set & ~covered).sum()), distinct=len(np.unique(z)), zmin=float(z.min()), zmax=float(z.max()),
                pos_inf=int(np.isposinf(z).sum()), finite=int(np.isfinite(z).sum()),
                subnormal=int(((z != 0) & (np.abs(z) < tiny)).sum()), neg_zero=int((bits(z) == 0x80000000).sum()),
                steps_neg_inf=int(np.isneginf(ref.steps).sum()), count00=int(ref.count[0, 0]),
                depth_max=int(ref.depth[..., 0].max()), depth_distinct=len(np.unique(ref.depth[..., 0])),
                order_dependent=order_dependent(oracle, case, size))


_CHECKED = {}


def check_condition(oracle, case, size) -> dict:
    """Asserts that the oracle's render of the case still reaches what the case is for; returns the figures."""
    if (case, tuple(size)) in _CHECKED:
        return _CHECKED[case, tuple(size)]
    f = figures(oracle, case, size)
    what = f"{case} {size[0]}x{size[1]}: {f}"
    assert f["set_unvisited"] == 0, what
    if case == "rising":
        assert f["set"] == f["covered"] > 0 and f["distinct"] >= 0.9 * f["covered"], what
    elif case == "rising_far":
        assert f["set"] > 0 and f["zmin"] > 3.0, what
    elif case == "rising_tied":
        assert f["order_dependent"] >= 50, what
    elif case == "falling_sentinel":
        assert f["unset_visited"] >= 8 and f["set"] >= 100 and f["zmax"] < 0.0 and 0 < f["depth_max"] < 65535, what
        cfg = config(oracle, case, size)
        for p0 in starts(case)[1::2]:
            assert oracle.iterate(cfg, p0, 1008)[2] == 1.0, what      # depth exactly -1.0f: the sentinel itself, never stored
    elif case == "alt_inf":
        assert f["pos_inf"] >= 300 and f["finite"] >= 1 and f["order_dependent"] >= 300, what
    elif case == "alt_inf_warm":
        assert f["pos_inf"] == f["set"] >= 300, what
    elif case == "overflow_mid":
        assert 0.25 < f["count00"] / (JOBS * CASES[case]["n"]) < 0.6 and f["pos_inf"] >= 300 and f["steps_neg_inf"] >= 1, what
    elif case == "shrink_neg":
        assert f["subnormal"] >= 100 and f["neg_zero"] >= 30, what
    elif case == "shrink_alt":
        assert f["zmin"] < 0.0 < f["zmax"] and f["depth_distinct"] >= 200, what
    else:
        assert case in ("const_pos", "const_neg"), case
        assert f["distinct"] == 1 and f["order_dependent"] >= 300 and f["depth_max"] == 0, what
        assert math.copysign(0.25, -CASES[case]["b"]) == f["zmin"] == f["zmax"], what
    _CHECKED[case, tuple(size)] = f
    return f
