"""The reference of the device logarithm and of everything coloured through it (host only: the standard library and numpy).

bracket(x) is the pair of neighbouring doubles that enclose the true ln x, from `decimal` at 60 digits. A logarithm whose error is at
most one ulp returns one of the two, so a site that takes such a logarithm and then evaluates a stated expression has, per pixel or
per record, a small SET of possible results: the expression over the product of the brackets. The candidate functions below build
those sets. Each restates its site's expression through the suite's existing restatement, with the logarithm(s) as ARGUMENTS: none
of them calls a logarithm of its own (tests/test_log_brackets_host.py feeds them host libm's and gets the restatements back bit for
bit, and feeds them wrong logarithms to show what the sets reject)."""
from __future__ import annotations

import decimal
import functools
import itertools
import math
import os
import sys

import numpy as np

import ftle_restatement as F
import plane_restatement as P

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import second_restatement as S2   # noqa: E402

_CTX = decimal.Context(prec=60)
_D = decimal.Decimal
TABLE = 1 << 20          # ln_u32's host table: ln(k + 1), k < 2^20
M32 = 0xFFFFFFFF
INF, NAN = math.inf, math.nan


@functools.lru_cache(maxsize=None)
def _true_ln(x: float):
    return _D(x).ln(_CTX)           # Decimal(x) is x exactly; ln is correctly rounded to 60 digits


@functools.lru_cache(maxsize=None)
def _bracket(x: float) -> tuple:
    if x != x or x < 0.0:
        return (NAN, NAN)
    if x == 0.0:
        return (-INF, -INF)
    if x == INF:
        return (INF, INF)
    if x == 1.0:
        return (0.0, 0.0)           # the one argument whose logarithm is a double
    true = _true_ln(x)
    f = float(true)                 # the double nearest to it
    gap = _D(f) - true              # exact: a Decimal subtraction of a 17-digit-exponent double from 60 digits is done at full width
    # 60 digits decide the side unless ln x lies within 1e-58 of a double; no argument of this suite comes near (43 digits to spare)
    assert abs(gap) > abs(true) * _D("1e-57"), f"ln({x!r}) is too close to a double for 60 digits"
    return (f, math.nextafter(f, INF)) if gap < 0 else (math.nextafter(f, -INF), f)


def bracket(x) -> tuple:
    """(lo, hi): the neighbouring doubles with lo <= ln x <= hi for a finite x > 0 (lo == hi == 0 for x == 1). The classes of C's
    log: +-0 -> (-inf, -inf), x < 0 and NaN -> (nan, nan), +inf -> (inf, inf). A subnormal x brackets like any other."""
    return _bracket(float(x))


def nearest(x) -> float:
    """The member of bracket(x) nearer to the true logarithm (what a correctly rounded log returns)."""
    x = float(x)
    lo, hi = _bracket(x)
    if lo == hi or lo != lo:
        return lo
    true = _true_ln(x)
    return lo if true - _D(lo) < _D(hi) - true else hi


def member(y, x) -> bool:
    """Is y a result a logarithm within one ulp may give for x — a member of the bracket, or of the class's one value (bit for bit:
    -0.0 is no member of (0.0, 0.0))?"""
    lo, hi = bracket(x)
    y = float(y)
    if lo != lo:
        return y != y
    return any(y == v and math.copysign(1.0, y) == math.copysign(1.0, v) for v in (lo, hi))


def members(ys, xs) -> np.ndarray:
    return np.array([member(y, x) for y, x in zip(np.ravel(ys), np.ravel(xs))], dtype=bool).reshape(np.shape(ys))


def ulp_distance(y, x) -> float:
    """How far y lies outside bracket(x), in doubles (0 for a member; inf where the class differs): the figure to report if a
    logarithm ever leaves its bracket."""
    lo, hi = bracket(x)
    y = float(y)
    if member(y, x):
        return 0
    if lo != lo or y != y or math.isinf(lo) or math.isinf(y):
        return INF
    key = lambda v: (lambda b: b if b >= 0 else -(b & 0x7FFFFFFFFFFFFFFF))(int(np.float64(v).view(np.int64)))   # noqa: E731
    return max(key(lo) - key(y), key(y) - key(hi))


def brackets(xs) -> tuple:
    """(lo, hi) arrays of bracket() over an array."""
    flat = [bracket(v) for v in np.ravel(np.asarray(xs, dtype=np.float64))]
    shape = np.shape(xs)
    return np.array([b[0] for b in flat]).reshape(shape), np.array([b[1] for b in flat]).reshape(shape)


# ---- ln_u32 (csrc/sar_device.hpp) --------------------------------------------------------------------------------------------------
def _libm_table(c: int) -> float:
    return math.log(float(c))        # the table IS host libm's (csrc/sar_runtime.cpp: host_ln_lut), not a logarithm of this module's


def ln_u32_set(c: int, table=_libm_table) -> tuple:
    """The values ln_u32(c) may return for a u32 c: the ONE table value for c - 1 < 2^20, bracket(c) beyond it, -inf for c == 0 (the
    u32 wrap of count + 1: the index c - 1 is huge and the device takes log(0.0))."""
    c = int(c)
    assert 0 <= c <= M32
    if c == 0:
        return (-INF,)
    if c - 1 < TABLE:
        return (table(c),)
    lo, hi = bracket(float(c))
    return (lo, hi)


def _assignments(args, sets=ln_u32_set):
    """Every way to give each DISTINCT argument one member of its set (the device's logarithm is a function: equal arguments get equal
    values), as dicts argument -> value."""
    distinct = sorted(set(args))
    for choice in itertools.product(*[sets(a) for a in distinct]):
        yield dict(zip(distinct, choice))


# ---- the Gas pixel (csrc/sar_image.hip: colorize_gas_body; csrc/sar_gallery.hip's tile colorize) -------------------------------------
def gas_pixel(position, ln_count, ln_max, entries, brightness, transparent):
    """One pixel of second_restatement.colorize_gas with the two logarithms handed in. `position` is what Palette::interpolate gets:
    steps, or color_range_restatement.positions(steps, window) under an applied colour range."""
    one = S2.Runtime(1, 1)                       # one pixel with count 0 under max 1: colorize_gas asks for ln(1.0) and ln(2.0)
    nan = position != position
    one.count, one.max, one.steps = [0], 1, [0.0 if nan else position]
    libm, S2._ln = S2._ln, lambda v: ln_count if v == 1.0 else ln_max
    try:
        px = S2.colorize_gas(one, entries, brightness, transparent)[0]
    finally:
        S2._ln = libm
    # (the restatement's math.floor refuses a NaN position. Palette::interpolate makes a NaN colour of it, `as u16` makes 0 of every
    # such channel, and alpha knows no position: the oracle, which takes NaN, agrees in tests/test_log_brackets_host.py)
    return (0, 0, 0, px[3]) if nan else px


def gas_pixel_set(position, count: int, max_: int, entries, brightness, transparent, sets=ln_u32_set) -> set:
    """The (r, g, b, a) tuples a pixel may take: over ln_u32(count + 1) x ln_u32(max + 1), at most 4."""
    cn, cm = (int(count) + 1) & M32, (int(max_) + 1) & M32
    return {gas_pixel(position, a[cn], a[cm], entries, brightness, transparent) for a in _assignments((cn, cm), sets)}


def gas_image_sets(positions, count, max_: int, entries, brightness, transparent, sets=ln_u32_set) -> list:
    """gas_pixel_set of every pixel, row-major."""
    return [gas_pixel_set(float(p), int(c), max_, entries, brightness, transparent, sets)
            for p, c in zip(np.ravel(positions), np.ravel(count))]


def image_in_sets(img, sets) -> np.ndarray:
    """Per pixel (row-major): is the image's tuple a member of the pixel's set?"""
    px = np.asarray(img).reshape(-1, 4)
    return np.array([tuple(int(v) for v in p) in s for p, s in zip(px, sets)], dtype=bool)


def gas_class(count, max_: int) -> np.ndarray:
    """The class of each pixel: 0 numerator and denominator in the table, 1 numerator beyond, 2 denominator beyond, 3 both. (A wrapped
    argument, 0, is beyond the table: the device's log takes it.)"""
    beyond = lambda c: ((np.asarray(c, dtype=np.uint64) + 1) & M32).astype(np.int64) - 1   # noqa: E731
    num = (beyond(count) >= TABLE) | (beyond(count) < 0)
    den = bool(beyond(max_) >= TABLE or beyond(max_) < 0)
    return num.astype(np.int64) + 2 * int(den)


# ---- the exposure record (csrc/sar_select.hip: record) ---------------------------------------------------------------------------------
class _MathWith:
    """The math module with `log` replaced by a logarithm of u32 arguments handed in."""

    def __init__(self, ln):
        self._ln = ln

    def log(self, v):
        return self._ln(int(v))

    def __getattr__(self, name):
        return getattr(math, name)


def restate_with(restate, ln, count, max_, *args, **params):
    """`restate` (tests/test_gpu_exposure.py) with ln(c) for every u32 c > 0 it takes a logarithm of — its own expression, order and
    fallbacks; only the module's `math.log` is another while it runs. (c == 0 stays its -inf.)"""
    g = restate.__globals__
    libm, g["math"] = g["math"], _MathWith(ln)
    try:
        return restate(count, max_, *args, **params)
    finally:
        g["math"] = libm


def exposure_set(restate, count, max_, sets=ln_u32_set, **params) -> tuple:
    """(the set of (offset's bits, factor's bits, applied) the record may hold, its exact part (black, white, covered, M)): `restate`
    (tests/test_gpu_exposure.py) over the logarithms of black + 1, white + 1 and M + 1, at most 8 records."""
    plain = restate(count, max_, **params)
    args = [(int(v) + 1) & M32 for v in (plain[2], plain[3], plain[5])]
    out = set()
    for a in _assignments(args, sets):
        r = restate_with(restate, a.__getitem__, count, max_, **params)
        assert r[2:6] == plain[2:6]
        out.add((float_bits(r[0]), float_bits(r[1]), r[6]))
    return out, plain[2:6]


def float_bits(x) -> int:
    return int(np.float64(x).view(np.uint64))


# ---- the plane's pixel (csrc/sar_plane.hip: plane_lambda1, k_plane_colorize) ---------------------------------------------------------
def plane_lambda1(log2_exp, mant_logs, steps_done, k: int) -> np.ndarray:
    """plane_lambda1<K>: ((double)E * ln2 + log M) / steps_done per exponent, the largest by `lk > l ? lk : l`. mant_logs[..., j] is the
    logarithm of mant[..., j], handed in."""
    folded = np.asarray(steps_done).astype(np.float64)
    with np.errstate(all="ignore"):
        l = (np.asarray(log2_exp[..., 0], dtype=np.float64) * P.LN2 + mant_logs[..., 0]) / folded
        for j in range(1, k):
            lj = (np.asarray(log2_exp[..., j], dtype=np.float64) * P.LN2 + mant_logs[..., j]) / folded
            l = np.where(lj > l, lj, l)
    return l


def plane_image(status, steps_done, log2_exp, mant_logs, k: int, palette_rgb, **colors) -> np.ndarray:
    return P.colorize(status, steps_done, plane_lambda1(log2_exp, mant_logs, steps_done, k), palette_rgb, **colors)


def plane_candidates(status, steps_done, log2_exp, mant, k: int, palette_rgb, **colors) -> np.ndarray:
    """(2^k, H, W, 4): the image under every choice of bracket member per exponent (the same choice in every pixel; a pixel's set is
    its column of this stack)."""
    lo, hi = brackets(np.asarray(mant)[..., :k])
    both = np.stack([lo, hi])                                     # (2, H, W, k)
    out = []
    for choice in itertools.product((0, 1), repeat=k):
        logs = np.stack([both[c][..., j] for j, c in enumerate(choice)], axis=-1)
        out.append(plane_image(status, steps_done, log2_exp, logs, k, palette_rgb, **colors))
    return np.stack(out)


# ---- the FTLE pixel (csrc/sar_ftle.hip: k_ftle_colorize) ---------------------------------------------------------------------------------
def ftle_image(status, escape_step, flags, stretch2_logs, steps: int, palette_rgb, lo: float, hi: float, fade: float = 32.0) -> np.ndarray:
    """ftle = log(stretch2) / (2 steps) with the logarithm handed in, then ftle_restatement.colorize."""
    with np.errstate(all="ignore"):
        f = np.asarray(stretch2_logs, dtype=np.float64) / np.float64(2.0 * float(steps))
    return F.colorize(status, escape_step, flags, f, palette_rgb, lo, hi, fade=fade)


def ftle_candidates(status, escape_step, flags, stretch2, steps: int, palette_rgb, lo: float, hi: float, fade: float = 32.0) -> np.ndarray:
    """(2, H, W, 4): the image under either member of bracket(stretch2)."""
    return np.stack([ftle_image(status, escape_step, flags, logs, steps, palette_rgb, lo, hi, fade) for logs in brackets(stretch2)])


def stack_member(img, stack) -> np.ndarray:
    """(H, W): is the image's pixel one of the stack's pixels there?"""
    return (np.asarray(stack) == np.asarray(img)[None]).all(-1).any(0)


def stack_sizes(stack) -> np.ndarray:
    """(H, W): how many distinct pixels the stack holds there."""
    s = np.asarray(stack).astype(np.uint64)
    key = (s[..., 0] << np.uint64(48)) | (s[..., 1] << np.uint64(32)) | (s[..., 2] << np.uint64(16)) | s[..., 3]
    key = np.sort(key, axis=0)
    return 1 + (key[1:] != key[:-1]).sum(0)
