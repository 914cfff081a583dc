"""numpy restatement of the FTLE maps (include/sar.h: sar_ftle_start, sar_runtime_ftle, sar_runtime_ftle_colorize), vectorised over
the pixels: the definition applied literally in fp64 — basin_restatement's start points, search_restatement's map step, the same
subtractions, multiplies, adds and compares in the same order. The finish goes pixel by pixel through math.sqrt and math.log — the
host libm the library's finish calls —, so that every field of the records, stretch2 and ftle included, and every statistic is
bit-identical to the library's. The colours use the records' ftle: the device takes its own log, so they agree to within 1."""
from __future__ import annotations

import math

import numpy as np

import search_restatement as R
from basin_restatement import start
from plane_restatement import _as_u16

BOUNDED, DIVERGED = R.BOUNDED, R.DIVERGED
EDGE, ONE_SIDED_U, ONE_SIDED_V, NO_U, NO_V = 1, 2, 4, 8, 16
RECORD_FIELDS = ("status", "escape_step", "flags", "end", "g11", "g12", "g22", "stretch2", "ftle")
STATS_FIELDS = ("pixels", "escaped", "bounded", "edge", "one_sided", "isolated", "ftle_min", "ftle_max")


def henon(a: float = 1.4, b: float = 0.3) -> np.ndarray:
    """x' = 1 - a x^2 + y, y' = b x, z' = 0 as 30 coefficients."""
    c = np.zeros(30)
    c[0], c[2], c[5], c[10 + 1] = 1.0, -a, 1.0, b
    return c


def linear(A) -> np.ndarray:
    """p' = A p as 30 coefficients."""
    A = np.asarray(A, dtype=np.float64).reshape(3, 3)
    c = np.zeros(30)
    for r in range(3):
        c[10 * r + 1], c[10 * r + 5], c[10 * r + 8] = A[r]
    return c


def flow(coeffs, origin, du, dv, width: int, height: int, steps: int, bound: float = 1e6):
    """k_ftle_flow: (status, escape_step, end) as (height, width[, 3]) arrays; a DIVERGED pixel's end is 0."""
    cs = 0.0 + 1.0 * np.asarray(coeffs, dtype=np.float64).reshape(30)
    c = [[cs[10 * r + k] for k in range(10)] for r in range(3)]
    p0 = start(origin, du, dv, width, height).reshape(-1, 3)
    x, y, z = (p0[:, k].copy() for k in range(3))
    alive = np.ones(width * height, dtype=bool)
    esc = np.zeros(width * height, dtype=np.int64)
    with np.errstate(all="ignore"):
        for t in range(steps):
            if not alive.any():
                break
            x, y, z = R.next_point(c, x, y, z)
            ok = R._within(x, y, z, bound)
            esc = np.where(alive & ~ok, t + 1, esc)
            alive &= ok
    shape = (height, width)
    end = np.stack([np.where(alive, v, 0.0) for v in (x, y, z)], axis=-1).reshape(height, width, 3)
    return np.where(alive, BOUNDED, DIVERGED).astype(np.int32).reshape(shape), esc.astype(np.uint32).reshape(shape), end


def _shifted(a, dy: int, dx: int, fill):
    """out[y, x] = a[y + dy, x + dx] inside the picture, `fill` outside."""
    h, w = a.shape[:2]
    out = np.full_like(a, fill)
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    yd, xd = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
    out[ys, xs] = a[yd, xd]
    return out


def _axis(bounded, end, plus, minus, one_sided: int, none: int):
    """The difference along one axis (plus / minus: the (dy, dx) of the two neighbours) and the axis' flags."""
    inside = np.ones(bounded.shape, dtype=bool)
    in_p, in_m = _shifted(inside, *plus, False), _shifted(inside, *minus, False)
    up, um = _shifted(bounded, *plus, False), _shifted(bounded, *minus, False)
    hi = np.where(up[..., None], _shifted(end, *plus, 0.0), end)
    lo = np.where(um[..., None], _shifted(end, *minus, 0.0), end)
    diff = hi - lo
    d = np.where((up & um)[..., None], diff * 0.5, diff)
    flags = np.where((in_p & ~up) | (in_m & ~um), EDGE, 0) | np.where(up != um, one_sided, 0) | np.where(~up & ~um, none, 0)
    return d, flags


def gram(status, end):
    """k_ftle_gram: (flags, g11, g12, g22); zero for a DIVERGED pixel."""
    bounded = status == BOUNDED
    with np.errstate(all="ignore"):
        a, fu = _axis(bounded, end, (0, 1), (0, -1), ONE_SIDED_U, NO_U)
        b, fv = _axis(bounded, end, (-1, 0), (1, 0), ONE_SIDED_V, NO_V)     # row 0 is the high end of tv: (x, y - 1) is the plus side
        g11 = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
        g12 = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
        g22 = (b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1]) + b[..., 2] * b[..., 2]
    flags = np.where(bounded, fu | fv, 0).astype(np.uint32)
    return flags, np.where(bounded, g11, 0.0), np.where(bounded, g12, 0.0), np.where(bounded, g22, 0.0)


def metric(du, dv, width: int, height: int):
    """(m11, m12, m22, A) of hu = du / (width - 1), hv = dv / (height - 1); an axis of one pixel has hu or hv = 0."""
    hu = [float(v) / float(width - 1) if width > 1 else 0.0 for v in du]
    hv = [float(v) / float(height - 1) if height > 1 else 0.0 for v in dv]
    m11 = (hu[0] * hu[0] + hu[1] * hu[1]) + hu[2] * hu[2]
    m12 = (hu[0] * hv[0] + hu[1] * hv[1]) + hu[2] * hv[2]
    m22 = (hv[0] * hv[0] + hv[1] * hv[1]) + hv[2] * hv[2]
    return m11, m12, m22, m11 * m22 - m12 * m12


def _div(a: float, b: float) -> float:
    """IEEE a / b for b != 0 or not (Python raises on a zero divisor)."""
    return float(np.float64(a) / np.float64(b))


def _log(s: float) -> float:
    """C's log: -inf at 0, NaN below it and for NaN."""
    if s != s or s < 0.0:
        return math.nan
    return -math.inf if s == 0.0 else math.log(s)


def finish_pixel(status: int, flags: int, g11: float, g12: float, g22: float, m, steps: int):
    """(stretch2, ftle) of one record: include/sar.h's host finish in its order of operations."""
    m11, m12, m22, A = m
    no_u, no_v = bool(flags & NO_U), bool(flags & NO_V)
    s = math.nan
    with np.errstate(all="ignore"):
        if status == BOUNDED and not no_u and not no_v:
            B = (g11 * m22 + g22 * m11) - 2.0 * (g12 * m12)
            Cc = g11 * g22 - g12 * g12
            disc = B * B - 4.0 * (A * Cc)
            disc = disc if disc > 0.0 else 0.0
            s = _div(B + math.sqrt(disc), 2.0 * A)
        elif status == BOUNDED and not no_u:
            s = _div(g11, m11)
        elif status == BOUNDED and not no_v:
            s = _div(g22, m22)
        return s, _div(_log(s), 2.0 * float(steps))


def ftle(coeffs, origin, du, dv, width: int, height: int, steps: int, bound: float = 1e6) -> dict:
    """The whole of sar_runtime_ftle on the host: the RECORD_FIELDS as (height, width[, 3]) arrays and "stats"."""
    status, esc, end = flow(coeffs, origin, du, dv, width, height, steps, bound)
    flags, g11, g12, g22 = gram(status, end)
    m = metric(du, dv, width, height)
    s2, f = np.empty((height, width)), np.empty((height, width))
    for y in range(height):
        for x in range(width):
            s2[y, x], f[y, x] = finish_pixel(int(status[y, x]), int(flags[y, x]), float(g11[y, x]), float(g12[y, x]), float(g22[y, x]), m, steps)
    fin = f[np.isfinite(f)]
    bounded = int((status == BOUNDED).sum())
    stats = {"pixels": width * height, "escaped": width * height - bounded, "bounded": bounded, "edge": int(((flags & EDGE) != 0).sum()),
             "one_sided": int(((flags & (ONE_SIDED_U | ONE_SIDED_V)) != 0).sum()),
             "isolated": int((((flags & NO_U) != 0) & ((flags & NO_V) != 0)).sum()),
             "ftle_min": float(fin.min()) if fin.size else math.inf, "ftle_max": float(fin.max()) if fin.size else -math.inf}
    return {"status": status, "escape_step": esc, "flags": flags, "end": end, "g11": g11, "g12": g12, "g22": g22, "stretch2": s2, "ftle": f,
            "stats": stats}


def window(f) -> tuple:
    """FtleMap.window(): the 1 % and 99 % quantiles of the finite ftle."""
    fin = f[np.isfinite(f)]
    if fin.size == 0:
        return 0.0, 1.0
    lo, hi = (float(v) for v in np.quantile(fin, (0.01, 0.99)))
    return (lo, hi) if lo < hi else (lo - 0.5, hi + 0.5)


def colorize(status, escape_step, flags, f, palette_rgb, lo: float, hi: float, fade: float = 32.0) -> np.ndarray:
    """(H, W, 4) RGBA16 of sar_runtime_ftle_colorize from the records' ftle."""
    pal = np.asarray(palette_rgb, dtype=np.float64)
    pal = np.concatenate([pal, pal[-1:]])          # Palette::new duplicates the last entry
    length = pal.shape[0] - 1
    h, w = status.shape
    out = np.zeros((h, w, 4), dtype=np.uint16)
    out[..., 3] = 65535
    escaped = status != BOUNDED
    edge = ~escaped & ((flags & EDGE) != 0)
    hot = ~escaped & ~edge & np.isfinite(f)
    with np.errstate(all="ignore"):
        e = escape_step.astype(np.float64)
        grey = _as_u16((0.5 * (e / (e + np.float64(fade)))) * 65535.0)
        v = (f - np.float64(lo)) / (np.float64(hi) - np.float64(lo))
        v = np.where(v < 0.0, 0.0, np.where(v >= 1.0, 0.999999, v))
        v = v * float(length)
        fl = np.floor(v)
        n = np.clip(np.where(np.isnan(fl), 0, fl).astype(np.int64), 0, length - 1)
        t = v - fl
        t1 = 1.0 - t
        for ch in range(3):
            col = _as_u16(np.sqrt(pal[n + 1, ch] * t + pal[n, ch] * t1) * 65535.0)
            out[..., ch] = np.where(escaped, grey, np.where(edge, 65535, np.where(hot, col, 0)))
    return out
