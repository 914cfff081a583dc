"""numpy restatement of the orbit diagrams (include/sar.h: sar_orbit_coeffs, sar_runtime_orbit), vectorised over columns x jobs: the
definition applied literally in fp64 — search_restatement's map step, the same multiplies, adds and compares in the same order — so
that count, max and every field of the column statistics are bit-identical to the device's."""
from __future__ import annotations

import numpy as np

import search_restatement as R

COLUMN_FIELDS = ("dead_transient", "dead_late", "alive", "occupied", "max", "hits", "misses", "vmin", "vmax")


def coeffs(a, b, width: int) -> np.ndarray:
    """(width, 30): column c is a + (b - a) * t, t = c / (width - 1) (0 when width == 1), then 0. + 1. * c."""
    a = np.asarray(a, dtype=np.float64).reshape(30)
    b = np.asarray(b, dtype=np.float64).reshape(30)
    span = b - a
    c = np.arange(width, dtype=np.float64)
    t = c / np.float64(width - 1) if width > 1 else np.zeros(1)
    v = a[None, :] + span[None, :] * t[:, None]
    return 0.0 + 1.0 * v


def diagram(a, b, width: int, height: int, starts, transient: int, steps: int, v_range, proj=(1.0, 0.0, 0.0), bound: float = 1e6) -> dict:
    """The whole of sar_runtime_orbit on the host: {"count": (height, width) uint32, "max": int, "stats": dict of (width,) arrays}."""
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    jobs = starts.shape[0]
    cs = np.repeat(coeffs(a, b, width), jobs, axis=0)          # lane = column * jobs + job
    col = np.repeat(np.arange(width), jobs)
    c = R._rows(cs)
    x, y, z = (np.tile(starts[:, k], width) for k in range(3))
    p0, p1, p2 = (np.float64(v) for v in proj)
    v_lo = np.float64(v_range[0])
    scale = np.float64(height) / (np.float64(v_range[1]) - v_lo)
    hf = np.float64(height)
    n = width * jobs
    alive = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(transient):
            if not alive.any():
                break
            x, y, z = R.next_point(c, x, y, z)
            alive &= R._within(x, y, z, bound)
        survived = alive.copy()
        count = np.zeros((height, width), dtype=np.int64)
        hits = np.zeros(n, dtype=np.int64)
        misses = np.zeros(n, dtype=np.int64)
        vmin = np.full(n, np.inf)
        vmax = np.full(n, -np.inf)
        for _ in range(steps):
            if not alive.any():
                break
            x, y, z = R.next_point(c, x, y, z)
            alive &= R._within(x, y, z, bound)
            v = (p0 * x + p1 * y) + p2 * z
            u = (v - v_lo) * scale
            hit = alive & (u >= 0.0) & (u < hf)
            vmin = np.where(alive & (v < vmin), v, vmin)
            vmax = np.where(alive & (v > vmax), v, vmax)
            np.add.at(count, (height - 1 - u[hit].astype(np.int64), col[hit]), 1)
            hits += hit
            misses += alive & ~hit
    assert count.max() < 2 ** 32

    def per_column(v):
        return v.reshape(width, jobs)

    stats = {
        "dead_transient": per_column(~survived).sum(1),
        "dead_late": per_column(survived & ~alive).sum(1),
        "alive": per_column(alive).sum(1),
        "occupied": (count > 0).sum(0),
        "max": count.max(0),
        "hits": per_column(hits).sum(1),
        "misses": per_column(misses).sum(1),
        "vmin": per_column(vmin).min(1),
        "vmax": per_column(vmax).max(1),
    }
    return {"count": count.astype(np.uint32), "max": int(count.max()), "stats": stats}
