"""numpy restatement of the basins of attraction (include/sar.h: sar_basin_start, sar_runtime_basin, sar_runtime_basin_colorize),
vectorised over the pixels: the definition applied literally in fp64 — search_restatement's map step, the same multiplies, adds and
compares in the same order —, the set of unique edges between the cells of consecutive tail points, and a plain union-find over
that set. Every field of the pixel records, the table, the statistics and the colours is bit-identical to the device's."""
from __future__ import annotations

import numpy as np

import search_restatement as R
from plane_restatement import _as_u16

BOUNDED, DIVERGED = R.BOUNDED, R.DIVERGED
NONE = 0xFFFFFFFF
ATTRACTOR_FIELDS = ("root", "pixels", "cells", "first_pixel", "cell_lo", "cell_hi")
STATS_FIELDS = ("pixels", "escaped_transient", "escaped_tail", "bounded", "attractors", "cells")


def pitchfork(mu: float) -> np.ndarray:
    """x' = mu x - x y, y' = x^2, z' = 0.5 z as 30 coefficients: for 1 < mu < 2 the fixed points (+-sqrt(mu - 1), mu - 1, 0) attract,
    the origin attracts only along x = 0, and |x0| large enough escapes."""
    c = np.zeros(30)
    c[1], c[3], c[10 + 2], c[20 + 8] = mu, -1.0, 1.0, 0.5
    return c


def start(origin, du, dv, width: int, height: int) -> np.ndarray:
    """(height, width, 3): (origin + du * tu) + dv * tv, tu = x / (width - 1), tv = (height - 1 - y) / (height - 1), 0 for a size of 1."""
    o, u, v = (np.asarray(a, dtype=np.float64).reshape(3) for a in (origin, du, dv))
    tu = np.arange(width, dtype=np.float64) / np.float64(width - 1) if width > 1 else np.zeros(1)
    tv = (np.float64(height - 1) - np.arange(height, dtype=np.float64)) / np.float64(height - 1) if height > 1 else np.zeros(1)
    return (o[None, None, :] + u[None, None, :] * tu[None, :, None]) + v[None, None, :] * tv[:, None, None]


def _cells(p, lo, hi, grid: int):
    scale = np.float64(grid) / (np.float64(hi) - np.float64(lo))
    u = (p - np.float64(lo)) * scale
    c = np.where(u < 0.0, 0.0, np.where(u >= np.float64(grid), np.float64(grid - 1), np.trunc(u)))
    return c.astype(np.int64)


def _find(parent: dict, v: int) -> int:
    while parent[v] != v:
        v = parent[v]
    return v


def basin(coeffs, origin, du, dv, width: int, height: int, transient: int, steps: int, grid: int, box, bound: float = 1e6) -> dict:
    """The whole of sar_runtime_basin on the host: {"status", "escape_step", "root", "label": (height, width) arrays, "attractors": a dict
    of arrays sorted as the table is, "stats": dict of ints, "extent": (6,) float64}."""
    cs = (0.0 + 1.0 * np.asarray(coeffs, dtype=np.float64).reshape(30))
    c = [[cs[10 * r + k] for k in range(10)] for r in range(3)]
    p0 = start(origin, du, dv, width, height).reshape(-1, 3)
    n = width * height
    x, y, z = (p0[:, k].copy() for k in range(3))
    alive = np.ones(n, dtype=bool)
    esc = np.zeros(n, dtype=np.int64)
    (xl, yl, zl), (xh, yh, zh) = box
    G = int(grid)

    def node():
        return (_cells(z, zl, zh, G) * G + _cells(y, yl, yh, G)) * G + _cells(x, xl, xh, G)

    with np.errstate(all="ignore"):
        for t in range(transient):
            x, y, z = R.next_point(c, x, y, z)
            ok = R._within(x, y, z, bound)
            esc = np.where(alive & ~ok, t + 1, esc)
            alive &= ok
        nodes = np.empty((steps + 1, n), dtype=np.int64)
        nodes[0] = node()
        lo = [v.copy() for v in (x, y, z)]
        hi = [v.copy() for v in (x, y, z)]
        for t in range(steps):
            x, y, z = R.next_point(c, x, y, z)
            ok = R._within(x, y, z, bound)
            esc = np.where(alive & ~ok, transient + t + 1, esc)
            alive &= ok
            nodes[t + 1] = node()
            for k, v in enumerate((x, y, z)):
                lo[k] = np.where(v < lo[k], v, lo[k])
                hi[k] = np.where(v > hi[k], v, hi[k])
    # only the pixels that stay bounded to the end have a tail
    tails = nodes[:, alive]
    a, b = tails[:-1].reshape(-1), tails[1:].reshape(-1)
    differ = a != b
    edges = np.unique(np.stack([a[differ], b[differ]], axis=1), axis=0) if differ.any() else np.zeros((0, 2), dtype=np.int64)
    visited = np.unique(tails)
    parent = {int(v): int(v) for v in visited}
    for u, v in edges:
        ru, rv = _find(parent, int(u)), _find(parent, int(v))
        if ru != rv:
            parent[max(ru, rv)] = min(ru, rv)      # (the smaller node stays the root: a component's root is its smallest node)
    root_of = {v: _find(parent, v) for v in parent}

    status = np.where(alive, BOUNDED, DIVERGED).astype(np.int32)
    root = np.full(n, NONE, dtype=np.uint32)
    root[alive] = [root_of[int(v)] for v in tails[-1]]
    roots = sorted(set(root_of.values()))
    table = []
    for r in roots:
        cells = np.array([v for v in visited if root_of[int(v)] == r], dtype=np.int64)
        xyz = np.stack([cells % G, cells // G % G, cells // G // G], axis=1)
        pix = np.flatnonzero(root == r)
        table.append((r, pix.size, cells.size, int(pix[0]) if pix.size else NONE, xyz.min(0), xyz.max(0)))
    table.sort(key=lambda a: (-a[1], a[0]))
    label = np.full(n, NONE, dtype=np.uint32)
    for k, a in enumerate(table):
        label[root == a[0]] = k
    attractors = {f: np.array([a[i] for a in table], dtype=np.uint32).reshape((len(table), 3) if f.startswith("cell_") else (len(table),))
                  for i, f in enumerate(ATTRACTOR_FIELDS)}
    bounded = int(alive.sum())
    stats = {"pixels": n, "escaped_transient": int((~alive & (esc <= transient)).sum()), "escaped_tail": int((~alive & (esc > transient)).sum()),
             "bounded": bounded, "attractors": len(table), "cells": int(visited.size)}
    extent = np.array([f(v[alive]) if bounded else s for l, h in zip(lo, hi) for f, v, s in ((np.min, l, np.inf), (np.max, h, -np.inf))])
    shape = (height, width)
    return {"status": status.reshape(shape), "escape_step": np.where(alive, 0, esc).astype(np.uint32).reshape(shape),
            "root": root.reshape(shape), "label": label.reshape(shape), "attractors": attractors, "stats": stats, "extent": extent}


def learned_box(extent, bounded: int):
    """basin_map's box=None: the extent widened by 2 % per side (0.5 for an axis without width), a unit box without a bounded pixel."""
    lo, hi = [], []
    for k in range(3):
        if not bounded:
            lo.append(0.0)
            hi.append(1.0)
            continue
        a, b = float(extent[2 * k]), float(extent[2 * k + 1])
        pad = 0.02 * (b - a) if b > a else 0.5
        lo.append(a - pad)
        hi.append(b + pad)
    return tuple(lo), tuple(hi)


UNIT_BOX = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def basin_auto(coeffs, origin, du, dv, width: int, height: int, transient: int, steps: int, grid: int, bound: float = 1e6) -> dict:
    """basin() in the box a grid = 1 first pass learns, as basin_map(box=None) does; the box is returned as "box"."""
    probe = basin(coeffs, origin, du, dv, width, height, transient, steps, 1, UNIT_BOX, bound)
    box = learned_box(probe["extent"], probe["stats"]["bounded"])
    out = basin(coeffs, origin, du, dv, width, height, transient, steps, grid, box, bound)
    out["box"] = box
    return out


def colorize(status, escape_step, label, attractors: int, palette_rgb, fade: float = 32.0) -> np.ndarray:
    """(H, W, 4) RGBA16 of sar_runtime_basin_colorize."""
    pal = np.asarray(palette_rgb, dtype=np.float64)
    pal = np.concatenate([pal, pal[-1:]])          # Palette::new duplicates the last entry
    length = pal.shape[0] - 1
    h, w = status.shape
    out = np.zeros((h, w, 4), dtype=np.uint16)
    out[..., 3] = 65535
    escaped = status != BOUNDED
    with np.errstate(all="ignore"):
        e = escape_step.astype(np.float64)
        g = 0.5 * (e / (e + np.float64(fade)))
        grey = _as_u16(g * 65535.0)
        v = (label.astype(np.float64) + 0.5) / np.float64(attractors)
        v = np.where(v < 0.0, 0.0, np.where(v >= 1.0, 0.999999, v))
        v = v * float(length)
        fl = np.floor(v)
        n = np.clip(np.where(np.isnan(fl), 0, fl).astype(np.int64), 0, length - 1)
        t = v - fl
        t1 = 1.0 - t
        for ch in range(3):
            col = np.sqrt(pal[n + 1, ch] * t + pal[n, ch] * t1)
            out[..., ch] = np.where(escaped, grey, _as_u16(col * 65535.0))
    return out
