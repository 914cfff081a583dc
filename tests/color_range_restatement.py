"""include/sar.h's colour range (sar_color_range_params / sar_color_range) restated in numpy: the population, the order by the
sortable 64-bit key, the exact order statistics, the fallback and the palette position — the same IEEE operations in the same
order, so that the GPU's records and images are held to it bit for bit."""
import math
from collections import namedtuple

import numpy as np

Window = namedtuple("Window", "lo hi pos_lo pos_hi covered applied")
SIGN = np.uint64(1 << 63)


def sortable(values) -> np.ndarray:
    """The uint64 key of each double: its bits, all flipped when the sign bit is set, the sign bit set otherwise."""
    b = np.ascontiguousarray(values, dtype=np.float64).view(np.uint64)
    return np.where(b & SIGN != 0, ~b, b | SIGN)


def unsortable(keys) -> np.ndarray:
    k = np.ascontiguousarray(keys, dtype=np.uint64)
    return np.where(k & SIGN != 0, k ^ SIGN, ~k).view(np.float64)


def window(count, steps, q_lo=0.01, q_hi=0.99, pos_lo=0.0, pos_hi=1.0) -> Window:
    c = np.asarray(count).ravel()
    s = np.asarray(steps, dtype=np.float64).ravel()
    member = (c != 0) & ~np.isnan(s)
    keys = np.sort(sortable(s[member]))
    n = int(keys.size)
    if n == 0:
        return Window(0.0, 0.0, float(pos_lo), float(pos_hi), 0, 0)
    ks = [min(math.floor(float(q) * float(n)), n - 1) for q in (q_lo, q_hi)]
    lo, hi = (float(v) for v in unsortable(keys[ks]))
    with np.errstate(all="ignore"):
        span = float(np.float64(hi) - np.float64(lo))
    applied = math.isfinite(lo) and math.isfinite(hi) and span > 0.0 and math.isfinite(span)
    return Window(lo, hi, float(pos_lo), float(pos_hi), n, int(applied))


def positions(steps, w: Window) -> np.ndarray:
    """What colorize hands to Palette::interpolate in the place of steps: pos_lo + ((steps - lo) / span) * (pos_hi - pos_lo), or
    steps themselves under a window that is not applied."""
    s = np.asarray(steps, dtype=np.float64)
    if not w.applied:
        return s.copy()
    with np.errstate(all="ignore"):
        span = np.float64(w.hi) - np.float64(w.lo)
        return np.float64(w.pos_lo) + ((s - np.float64(w.lo)) / span) * (np.float64(w.pos_hi) - np.float64(w.pos_lo))


def clamped(pos) -> np.ndarray:
    """Palette::interpolate's clamp (src/lib.rs:442-472): below 0 -> 0, from 1 on -> 0.999999."""
    p = np.array(pos, dtype=np.float64)
    return np.where(p < 0.0, 0.0, np.where(p >= 1.0, 0.999999, p))


def segments(pos, palette_len: int) -> np.ndarray:
    """The palette segment floor(clamped * len) of each (non-NaN) position."""
    return np.floor(clamped(pos) * float(palette_len)).astype(np.int64)
