"""The unstable-manifold family (include/sar.h: sar_runtime_manifold, sar_manifold_pixel) restated in numpy — test infrastructure.

Every floating-point operation is one numpy float64 operation (numpy never contracts a multiply and an add), in the order the header
gives; everything behind the fp64 steps is int64. The projection's constants are computed as tests/golden/second_restatement.py's
render computes them (its rotation_matrix, math.sin / math.cos of the angle, width * scale, 0.5 / scale, height / 2).

A `view` is a dict like second_restatement's presets: the rows "x", "y", "z" of the map's coefficients, "center_camera", "axis",
"rotation", "scale" — plus "angle", "width", "height"."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import second_restatement as G  # noqa: E402

OK, DOMAIN_ESCAPED = 0, 1
NONE = 0xFFFFFFFF
PLACED = 2.0 ** 30
DEFAULTS = dict(samples=4096, steps=32, max_span=16, bound=1e6)
BRANCH_DTYPE = np.dtype([("base", "<f8", 3), ("dir", "<f8", 3), ("delta", "<f8"), ("period", "<u4"), ("_pad", "<u4")])
RECORD_DTYPE = np.dtype([("status", "<i4"), ("first_long_step", "<u4"), ("alive_end", "<u4"), ("_pad", "<u4"), ("a", "<f8", 3), ("b", "<f8", 3),
                         ("n_drawn", "<u8"), ("n_dead", "<u8"), ("n_far", "<u8"), ("n_long", "<u8"), ("pixels", "<u8"), ("length_px", "<u8")])


def constants(view) -> dict:
    """What render hoists out of its loop (second_restatement.render), for this view."""
    scale, width, height = view["scale"], float(view["width"]), float(view["height"])
    return dict(m=G.rotation_matrix(view), sin_v=math.sin(view["angle"]), cos_v=math.cos(view["angle"]), cc=view["center_camera"],
                width_scaled=width * scale, scale_adjusted_mid=0.5 / scale, half_height=height / 2.0)


def coefficients(view) -> np.ndarray:
    """(3, 10) the map's coefficients, each through 0. + 1. * c."""
    return 0.0 + 1.0 * np.array([view["x"], view["y"], view["z"]], dtype=np.float64)


def next_point(c, x, y, z):
    """One step of the map on arrays (or scalars) of float64: each row's sum left to right, multiply then add."""
    terms = (x, x * x, x * y, x * z, y, y * y, y * z, z, z * z)
    out = []
    for r in range(3):
        s = c[r][0]
        for k, t in enumerate(terms):
            s = s + t * c[r][k + 1]
        out.append(s)
    return out[0], out[1], out[2]


def within(x, y, z, bound):
    return (np.abs(x) <= bound) & (np.abs(y) <= bound) & (np.abs(z) <= bound)


def project(k, x, y, z):
    """fi, fj of points in the view whose constants are k (render's lines :773-786)."""
    m, cc = k["m"], k["cc"]
    sx = m[0][0] * x + m[0][1] * y + m[0][2] * z
    sy = m[1][0] * x + m[1][1] * y + m[1][2] * z
    sz = m[2][0] * x + m[2][1] * y + m[2][2] * z
    ax, az = sx + cc[0], sz + cc[1]
    x2 = ax * k["cos_v"] + az * k["sin_v"]
    fi = (k["scale_adjusted_mid"] - x2) * k["width_scaled"]
    fj = k["half_height"] - (sy + cc[2]) * k["width_scaled"]
    return fi, fj


def pixel(view, xyz):
    """(fi, fj) of one point: what sar_manifold_pixel gives."""
    with np.errstate(all="ignore"):
        fi, fj = project(constants(view), np.float64(xyz[0]), np.float64(xyz[1]), np.float64(xyz[2]))
    return np.array([fi, fj], dtype=np.float64)


def place(fi, fj):
    """placed, X, Y: the signed pixel of every placed point (0 where it is not placed)."""
    placed = (fi >= -PLACED) & (fi < PLACED) & (fj >= -PLACED) & (fj < PLACED)
    X = np.where(placed, np.floor(np.where(placed, fi, 0.0)), 0.0).astype(np.int64)
    Y = np.where(placed, np.floor(np.where(placed, fj, 0.0)), 0.0).astype(np.int64)
    return placed, X, Y


def raster(X0, Y0, dX, dY):
    """The pixels of drawn segments from (X0, Y0) by (dX, dY), int64 arrays: (segment index, X, Y) of every plot, in no particular
    order. L = 0 plots (X0, Y0) once; L >= 1 plots k = 0 .. L - 1 at X0 + floor((2 k dX + L) / (2 L)), likewise Y (// floors)."""
    L = np.maximum(np.abs(dX), np.abs(dY))
    seg, xs, ys = [np.flatnonzero(L == 0)], [X0[L == 0]], [Y0[L == 0]]
    for k in range(int(L.max()) if L.size else 0):
        on = np.flatnonzero(L > k)
        l = L[on]
        seg.append(on)
        xs.append(X0[on] + (2 * k * dX[on] + l) // (2 * l))
        ys.append(Y0[on] + (2 * k * dY[on] + l) // (2 * l))
    return np.concatenate(seg), np.concatenate(xs), np.concatenate(ys)


def fundamental_domain(c, branch, bound):
    """a, b and whether every point on the way passed the bound test."""
    with np.errstate(all="ignore"):
        a = [np.float64(branch["base"][k]) + np.float64(branch["delta"]) * np.float64(branch["dir"][k]) for k in range(3)]
        v, ok = tuple(a), bool(within(*a, bound))
        for _ in range(int(branch["period"])):
            v = next_point(c, *v)
            ok = ok and bool(within(*v, bound))
    return np.array(a), np.array([np.float64(t) for t in v]), ok


def manifold(view, branches, samples=4096, steps=32, max_span=16, bound=1e6):
    """count (height, width) u32, first (height, width) u32, records (RECORD_DTYPE, one per branch)."""
    width, height = int(view["width"]), int(view["height"])
    c, k = coefficients(view), constants(view)
    count, first = np.zeros(width * height, dtype=np.int64), np.full(width * height, NONE, dtype=np.int64)
    records = np.zeros(len(branches), dtype=RECORD_DTYPE)
    records["first_long_step"] = NONE
    with np.errstate(all="ignore"):
        for bi, branch in enumerate(branches):
            rec = records[bi]
            a, b, ok = fundamental_domain(c, branch, bound)
            rec["a"], rec["b"] = a, b
            if not ok:
                rec["status"] = DOMAIN_ESCAPED
                continue
            d = b - a
            t = np.arange(samples, dtype=np.float64) / np.float64(samples - 1)
            x, y, z = a[0] + d[0] * t, a[1] + d[1] * t, a[2] + d[2] * t
            alive = np.ones(samples, dtype=bool)
            for n in range(steps + 1):
                alive &= within(x, y, z, bound)
                placed, X, Y = place(*project(k, x, y, z))
                both_alive, both_placed = alive[:-1] & alive[1:], placed[:-1] & placed[1:]
                dX, dY = X[1:] - X[:-1], Y[1:] - Y[:-1]
                L = np.maximum(np.abs(dX), np.abs(dY))
                dead = ~both_alive
                far = both_alive & ~both_placed
                long_ = both_alive & both_placed & (L > max_span)
                drawn = both_alive & both_placed & (L <= max_span)
                rec["n_dead"] += int(dead.sum())
                rec["n_far"] += int(far.sum())
                rec["n_long"] += int(long_.sum())
                rec["n_drawn"] += int(drawn.sum())
                rec["length_px"] += int(L[drawn].sum())
                if long_.any() and rec["first_long_step"] == NONE:
                    rec["first_long_step"] = n
                _, px, py = raster(X[:-1][drawn], Y[:-1][drawn], dX[drawn], dY[drawn])
                inside = (px >= 0) & (px < width) & (py >= 0) & (py < height)
                pix = py[inside] * width + px[inside]
                np.add.at(count, pix, 1)
                np.minimum.at(first, pix, n * 4096 + bi)
                rec["pixels"] += int(inside.sum())
                if n == steps:
                    rec["alive_end"] = int(alive.sum())
                else:
                    x, y, z = next_point(c, x, y, z)
    assert count.max(initial=0) < 2 ** 32
    return count.astype(np.uint32).reshape(height, width), first.astype(np.uint32).reshape(height, width), records


def branches_array(rows) -> np.ndarray:
    """BRANCH_DTYPE from rows (base3, dir3, delta, period)."""
    out = np.zeros(len(rows), dtype=BRANCH_DTYPE)
    for i, (base, direction, delta, period) in enumerate(rows):
        out[i] = (tuple(base), tuple(direction), delta, period, 0)
    return out
