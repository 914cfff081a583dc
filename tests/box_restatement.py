"""numpy restatement of box counting (include/sar.h: sar_runtime_boxes, sar_runtime_boxdim, sar_boxdim_fit, sar_box_log2_q32), written
from the contract alone: the cell of a point, the occupied cells of every level through np.unique on the shifted triples, the four
sums with lg32 in Python integers, a map's cube from its extent (corr_restatement's orbit), and the three least-squares lines. The
rows, statuses, cubes and points are bit-identical to the device's; the lines agree with the library's to the conditioning of the fit."""
from __future__ import annotations

import math

import numpy as np

import corr_restatement as X

BOUNDED, DIVERGED = X.BOUNDED, X.DIVERGED
FIT_OK, NO_WINDOW = 0, 1
LEVEL_DTYPE = np.dtype([("cells", "<u8"), ("singles", "<u8"), ("sum_sq", "<u8"), ("n_log_n", "<u8")])


def lg32(n: int) -> int:
    """log2(n) with 32 fraction bits, truncated: the top bit, then 32 squarings of the mantissa in [2^63, 2^64)."""
    assert n >= 1
    e = n.bit_length() - 1
    y = n << (63 - e)
    frac = 0
    for _ in range(32):
        y = (y * y) >> 63
        bit = y >> 64                                          # the square reached 2^64
        if bit:
            y >>= 1
        frac = (frac << 1) | bit
    return (e << 32) | frac


def cells(points, origin=(0.0, 0.0, 0.0), size=1.0, levels=16) -> np.ndarray:
    """(n, 3) int64: c_k = !(u >= 0) ? 0 : (u >= 2^L ? 2^L - 1 : trunc(u)), u = (p - origin_k) * scale, scale = 2^L / size."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    scale = float(1 << levels) / float(size)
    with np.errstate(all="ignore"):
        u = (p - np.asarray(origin, dtype=np.float64)[None, :]) * scale
    top = float(1 << levels)
    c = np.zeros(u.shape, dtype=np.int64)                      # !(u >= 0), NaN included
    high = u >= top
    c[high] = (1 << levels) - 1
    mid = (u >= 0.0) & ~high
    c[mid] = u[mid].astype(np.int64)                           # truncation
    return c


def level_rows(points, origin=(0.0, 0.0, 0.0), size=1.0, levels=16) -> np.ndarray:
    """(levels + 1,) LEVEL_DTYPE of one set: the cell of a point at level l is its finest cell >> (L - l)."""
    c = cells(points, origin, size, levels)
    rows = np.zeros(levels + 1, dtype=LEVEL_DTYPE)
    logs = {}
    for l in range(levels + 1):
        _, occ = np.unique(c >> (levels - l), axis=0, return_counts=True)
        occ = [int(v) for v in occ]
        assert sum(occ) == c.shape[0]
        for v in set(occ) - set(logs):
            logs[v] = lg32(v)
        rows[l] = (len(occ), sum(v == 1 for v in occ), sum(v * v for v in occ), sum(v * logs[v] for v in occ))
    return rows


def cube(extent):
    """origin = the three minima, size = the largest span, 1.0 where that is 0."""
    e = np.asarray(extent, dtype=np.float64)
    size = 0.0
    for k in range(3):
        span = float(e[2 * k + 1] - e[2 * k])
        size = span if span > size else size
    return e[0::2].copy(), (size if size > 0.0 else 1.0)


def _line(xs, ys) -> dict:
    k = len(xs)
    mx, my = sum(xs) / k, sum(ys) / k
    sxx = sum((x - mx) * (x - mx) for x in xs)
    sxy = sum((x - mx) * (y - my) for x, y in zip(xs, ys))
    slope = sxy / sxx
    icpt = my - slope * mx
    rms = math.sqrt(sum((y - (icpt + slope * x)) ** 2 for x, y in zip(xs, ys)) / k)
    return dict(slope=slope, intercept=icpt, rms=rms)


def entropies(rows, n: int, l: int):
    """(y0, y1, y2) of level l: ln cells, ln n - (n_log_n / 2^32) ln 2 / n, 2 ln n - ln sum_sq."""
    r = rows[l]
    ln2 = math.log(2.0)
    return (math.log(float(int(r["cells"]))), math.log(float(n)) - (float(int(r["n_log_n"])) / 4294967296.0) * ln2 / float(n),
            2.0 * math.log(float(n)) - math.log(float(int(r["sum_sq"]))))


def fit(rows, n: int, l_min=3, min_occupancy=16.0) -> dict:
    """The three lines over the levels l >= l_min with n >= min_occupancy * cells_l, in level order."""
    L = len(rows) - 1
    used = [l for l in range(l_min, L + 1) if int(rows[l]["cells"]) and float(n) >= min_occupancy * float(int(rows[l]["cells"]))]
    nan = dict(slope=math.nan, intercept=math.nan, rms=math.nan)
    if len(used) < 3:
        return dict(d0=nan, d1=nan, d2=nan, first_level=0, last_level=0, used=0, status=NO_WINDOW)
    assert used == list(range(used[0], used[-1] + 1))          # contiguous: cells never shrinks with l
    xs = [float(l) * math.log(2.0) for l in used]
    ys = [entropies(rows, n, l) for l in used]
    return dict(d0=_line(xs, [y[0] for y in ys]), d1=_line(xs, [y[1] for y in ys]), d2=_line(xs, [y[2] for y in ys]),
                first_level=used[0], last_level=used[-1], used=len(used), status=FIT_OK)


def boxdim(coeffs, starts, samples, stride, transient, levels=16, l_min=3, min_occupancy=16.0, bound=1e6) -> dict:
    """sar_runtime_boxdim for one map on the host."""
    status, job, step, pts = X.record_points(coeffs, starts, samples, stride, transient, bound)
    if status == DIVERGED:
        return dict(status=status, fail_job=job, fail_step=step, levels=np.zeros(levels + 1, dtype=LEVEL_DTYPE), points=pts,
                    extent=np.array([np.inf, -np.inf] * 3), origin=np.full(3, np.nan), size=math.nan,
                    lines=fit(np.zeros(levels + 1, dtype=LEVEL_DTYPE), len(pts)))
    ext = X.extent(pts)
    origin, size = cube(ext)
    rows = level_rows(pts, origin, size, levels)
    return dict(status=status, fail_job=0, fail_step=0, levels=rows, points=pts, extent=ext, origin=origin, size=size,
                lines=fit(rows, len(pts), l_min, min_occupancy))
