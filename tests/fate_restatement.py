"""numpy restatement of the basin probes (include/sar.h: sar_runtime_basin_fates, sar_runtime_basin_uncertainty), built on
basin_restatement and search_restatement: the held picture's cell-label table from a picture's own labels, the fate of any start
point — the same map step, bound test and node arithmetic in the same order — and the uncertainty ladder. Every field is
bit-identical to the device's."""
from __future__ import annotations

import numpy as np

import basin_restatement as B
import search_restatement as R

BOUNDED, DIVERGED = B.BOUNDED, B.DIVERGED
NONE = B.NONE                 # label of a DIVERGED probe; a table entry no tail visited
UNKNOWN = 0xFFFFFFFE          # label of a BOUNDED probe none of whose tail points lies in a labelled cell
FATE_DTYPE = np.dtype([("status", np.int32), ("escape_step", np.uint32), ("label", np.uint32), ("hit", np.uint32)])
LEVEL_DTYPE = np.dtype([("eps", np.float64), ("tested", np.uint64), ("uncertain", np.uint64), ("unknown", np.uint64)])
MASK_DTYPE = np.dtype([("uncertain_bits", np.uint32), ("unknown_bits", np.uint32)])


def _rows(coeffs):
    cs = 0.0 + 1.0 * np.asarray(coeffs, dtype=np.float64).reshape(30)
    return [[cs[10 * r + k] for k in range(10)] for r in range(3)]


def _cells(p, lo, hi, grid: int):
    """basin_cell (sar_basin.hpp) to the letter: !(u >= 0) ? 0 : u >= grid ? grid - 1 : trunc(u) — a NaN, which only a point that
    has left the bound box can hold, is cell 0."""
    scale = np.float64(grid) / (np.float64(hi) - np.float64(lo))
    u = (p - np.float64(lo)) * scale
    c = np.where(~(u >= 0.0), 0.0, np.where(u >= np.float64(grid), np.float64(grid - 1), np.trunc(u)))
    return c.astype(np.int64)


def _node(x, y, z, box, G: int):
    (xl, yl, zl), (xh, yh, zh) = box
    return (_cells(z, zl, zh, G) * G + _cells(y, yl, yh, G)) * G + _cells(x, xl, xh, G)


class Picture:
    """What a runtime holds of a basin picture for the probes: the map, transient, steps, bound, grid, box and `table` (grid^3,)
    uint32 — a cell's attractor label, NONE where no tail went."""

    def __init__(self, coeffs, transient: int, steps: int, grid: int, box, bound: float, table: np.ndarray):
        self.coeffs, self.transient, self.steps, self.grid, self.bound, self.table = np.asarray(coeffs, dtype=np.float64), transient, steps, grid, bound, table
        self.box = (tuple(float(v) for v in box[0]), tuple(float(v) for v in box[1]))


def picture(coeffs, origin, du, dv, width: int, height: int, transient: int, steps: int, grid: int, box, bound: float = 1e6,
            status=None, label=None) -> Picture:
    """The held picture of basin(...) with these parameters. `status` / `label`: the picture's own (height, width) arrays — the
    device's or basin_restatement's; computed with basin_restatement when absent. Every cell a bounded pixel's tail visits takes that
    pixel's label: all cells of one pixel lie in one component, and every visited cell lies on some bounded pixel's tail."""
    if status is None or label is None:
        r = B.basin(coeffs, origin, du, dv, width, height, transient, steps, grid, box, bound)
        status, label = r["status"], r["label"]
    c = _rows(coeffs)
    p0 = B.start(origin, du, dv, width, height).reshape(-1, 3)
    keep = np.asarray(status).reshape(-1) == BOUNDED
    lab = np.asarray(label).reshape(-1)[keep].astype(np.uint32)
    x, y, z = (p0[keep, k].copy() for k in range(3))
    box = (tuple(float(v) for v in box[0]), tuple(float(v) for v in box[1]))
    G = int(grid)
    table = np.full(G * G * G, NONE, dtype=np.uint32)

    def mark():
        node = _node(x, y, z, box, G)
        seen = table[node]
        assert np.all((seen == NONE) | (seen == lab)), "two attractors in one cell: the labels are not this picture's"
        table[node] = lab

    with np.errstate(all="ignore"):
        for _ in range(transient):
            x, y, z = R.next_point(c, x, y, z)
        mark()
        for _ in range(steps):
            x, y, z = R.next_point(c, x, y, z)
            mark()
    return Picture(coeffs, transient, steps, G, box, bound, table)


def fates(pic: Picture, points) -> np.ndarray:
    """The fates of the points (n, 3), as FATE_DTYPE."""
    pts = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = len(pts)
    c = _rows(pic.coeffs)
    x, y, z = (pts[:, k].copy() for k in range(3))
    alive = np.ones(n, dtype=bool)
    esc = np.zeros(n, dtype=np.int64)
    label = np.full(n, UNKNOWN, dtype=np.uint32)
    hit = np.full(n, pic.steps + 1, dtype=np.int64)

    def look(j: int, is_open):
        found = pic.table[_node(x, y, z, pic.box, pic.grid)]
        take = is_open & (found != NONE)
        label[take] = found[take]
        hit[take] = j
        return is_open & ~take

    with np.errstate(all="ignore"):
        for t in range(pic.transient):
            x, y, z = R.next_point(c, x, y, z)
            ok = R._within(x, y, z, pic.bound)
            esc = np.where(alive & ~ok, t + 1, esc)
            alive &= ok
        is_open = look(0, alive.copy())
        for t in range(pic.steps):
            x, y, z = R.next_point(c, x, y, z)
            ok = R._within(x, y, z, pic.bound)
            esc = np.where(alive & ~ok, pic.transient + t + 1, esc)
            alive &= ok
            is_open = look(t + 1, is_open & ok)
    out = np.zeros(n, dtype=FATE_DTYPE)
    out["status"] = np.where(alive, BOUNDED, DIVERGED)
    out["escape_step"] = np.where(alive, 0, esc)
    out["label"] = np.where(alive, label, NONE)
    out["hit"] = np.where(alive, hit, 0)
    return out


def classes(f: np.ndarray) -> np.ndarray:
    """DIVERGED ? NONE : label — all escapes are one class, UNKNOWN is a class of its own."""
    return np.where(f["status"] == BOUNDED, f["label"], NONE).astype(np.uint32)


def ladder(pic: Picture, base, direction, eps0: float, K: int) -> dict:
    """{"levels": LEVEL_DTYPE (K,), "fate0": FATE_DTYPE (n,), "masks": MASK_DTYPE (n,)} of the ladder e_k = ldexp(eps0, -(k - 1))."""
    b = np.asarray(base, dtype=np.float64).reshape(-1, 3)
    d = np.asarray(direction, dtype=np.float64).reshape(3)
    n = len(b)
    eps = np.ldexp(np.float64(eps0), -np.arange(K))
    step = d[None, None, :] * eps[None, :, None]                       # one multiply
    plus, minus = b[:, None, :] + step, b[:, None, :] - step           # one add / one subtract
    f0 = fates(pic, b)
    c0 = classes(f0)
    cp = classes(fates(pic, plus.reshape(-1, 3))).reshape(n, K)
    cm = classes(fates(pic, minus.reshape(-1, 3))).reshape(n, K)
    unknown = (c0 == UNKNOWN)[:, None] | (cp == UNKNOWN) | (cm == UNKNOWN)
    uncertain = ~unknown & ((cp != c0[:, None]) | (cm != c0[:, None]))
    levels = np.zeros(K, dtype=LEVEL_DTYPE)
    levels["eps"] = eps
    levels["unknown"] = unknown.sum(0)
    levels["uncertain"] = uncertain.sum(0)
    levels["tested"] = n - unknown.sum(0)
    bit = (np.uint64(1) << np.arange(K, dtype=np.uint64))[None, :]
    masks = np.zeros(n, dtype=MASK_DTYPE)
    masks["uncertain_bits"] = (uncertain * bit).sum(1).astype(np.uint32)
    masks["unknown_bits"] = (unknown * bit).sum(1).astype(np.uint32)
    return {"levels": levels, "fate0": f0, "masks": masks}


def fit(levels: np.ndarray, min_uncertain: int = 16, f_max: float = 0.5):
    """(alpha, the 1-based levels used): the least-squares slope of log2 f on log2 eps."""
    f = levels["uncertain"] / np.maximum(levels["tested"], 1).astype(np.float64)
    use = np.flatnonzero((levels["uncertain"] >= max(min_uncertain, 1)) & (f <= f_max))
    x, y = np.log2(levels["eps"][use]), np.log2(f[use])
    dx = x - x.mean()
    return float((dx * (y - y.mean())).sum() / (dx * dx).sum()), use + 1


def plane_points(origin, du, dv, n: int, seed: int) -> np.ndarray:
    """n points uniform on the plane origin + du * u + dv * v, (u, v) = default_rng(seed).random((n, 2)): BasinMap's drawing."""
    t = np.random.default_rng(seed).random((n, 2))
    o, u, v = (np.asarray(a, dtype=np.float64).reshape(3) for a in (origin, du, dv))
    return (o[None, :] + u[None, :] * t[:, :1]) + v[None, :] * t[:, 1:]
