"""numpy restatement of the cycles family (include/sar.h: sar_cycles_starts, sar_cycle_charpoly, sar_runtime_cycles), vectorised over
the starts of one map: the same multiplies, adds, subtractions, divisions and compares in the same order, so that every field of the
records and of the orbit slots is bit-identical to the device's. No square root, no logarithm; numpy never contracts a multiply and
an add."""
from __future__ import annotations

import numpy as np

from search_restatement import next_point

CONVERGED, ESCAPED, SINGULAR, NOT_CONVERGED = 0, 1, 2, 3
DEFAULTS = dict(period=1, jobs=512, grid=8, max_newton=64, cap=64, box_lo=(-2.0, -2.0, -2.0), box_hi=(2.0, 2.0, 2.0), tol=1e-12, bound=1e6,
                merge=1e-6, same=1e-9)
RECORD_FIELDS = ("converged", "escaped", "singular", "not_converged", "n_orbits", "orbits_lost", "hits_lost", "newton_iterations")
ORBIT_DTYPE = np.dtype([("rep", np.float64, 3), ("period", np.uint32), ("head", np.uint32), ("hits", np.uint32), ("newton", np.uint32),
                        ("residual", np.float64), ("M", np.float64, 9)])


def starts(grid: int = 8, box_lo=(-2.0, -2.0, -2.0), box_hi=(2.0, 2.0, 2.0)) -> np.ndarray:
    """(grid^3, 3): start j = (ix grid + iy) grid + iz at lo + ((double)i + 0.5) * step per axis, step = (hi - lo) / (double)grid."""
    lo, hi = np.asarray(box_lo, np.float64), np.asarray(box_hi, np.float64)
    step = (hi - lo) / np.float64(grid)
    i = np.arange(grid, dtype=np.float64)
    axis = [lo[k] + (i + 0.5) * step[k] for k in range(3)]
    ix, iy, iz = np.meshgrid(np.arange(grid), np.arange(grid), np.arange(grid), indexing="ij")
    return np.stack([axis[0][ix.ravel()], axis[1][iy.ravel()], axis[2][iz.ravel()]], axis=1)


def charpoly(M) -> np.ndarray:
    """(trace, the sum of the principal 2 x 2 minors, the determinant) of M[9] row-major, in sar_cycle_charpoly's order."""
    m = [np.float64(v) for v in np.asarray(M, np.float64).reshape(9)]
    with np.errstate(all="ignore"):
        tr = (m[0] + m[4]) + m[8]
        c00, c01, c02 = m[4] * m[8] - m[5] * m[7], m[5] * m[6] - m[3] * m[8], m[3] * m[7] - m[4] * m[6]
        minors = ((m[0] * m[4] - m[1] * m[3]) + (m[0] * m[8] - m[2] * m[6])) + c00
        det = (m[0] * c00 + m[1] * c01) + m[2] * c02
    return np.array([tr, minors, det])


def _rows(c30):
    c = 0.0 + 1.0 * np.asarray(c30, np.float64).reshape(30)
    return [[c[10 * r + k] for k in range(10)] for r in range(3)]


def _within(p, bound):
    return (np.abs(p[0]) <= bound) & (np.abs(p[1]) <= bound) & (np.abs(p[2]) <= bound)


def _max3(a, b, c):
    ab = np.where(a > b, a, b)
    return np.where(ab > c, ab, c)


def _tangent(c, p, m):
    """One step at p carrying the columns m[k] of the product: (F(p), J(p) m) — the Jacobian rows and V = J Q of tangent_eval."""
    x, y, z = p
    x2, y2, z2 = x + x, y + y, z + z
    J = [(((r[1] + x2 * r[2]) + y * r[3]) + z * r[4], ((x * r[3] + r[5]) + y2 * r[6]) + z * r[7], ((x * r[4] + y * r[7]) + r[8]) + z2 * r[9])
         for r in c]
    v = [[(J[a][0] * m[k][0] + J[a][1] * m[k][1]) + J[a][2] * m[k][2] for a in range(3)] for k in range(3)]
    return next_point(c, x, y, z), v


def _identity(n):
    one, zero = np.ones(n), np.zeros(n)
    return [[one.copy() if a == k else zero.copy() for a in range(3)] for k in range(3)]


def newton(c30, start_points, period, max_newton=64, tol=1e-12, bound=1e6):
    """The Newton solve of every start: (status, iterations, x) with x the converged point (whatever the lane held otherwise)."""
    c = _rows(c30)
    s = np.asarray(start_points, np.float64).reshape(-1, 3)
    n = s.shape[0]
    x = [s[:, k].copy() for k in range(3)]
    status = np.full(n, NOT_CONVERGED, dtype=np.int32)
    iters = np.zeros(n, dtype=np.uint32)
    running = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for it in range(max_newton + 1):
            if not running.any():
                break
            p, m, inb = [v.copy() for v in x], _identity(n), np.ones(n, dtype=bool)
            for _ in range(period):
                p, m = _tangent(c, p, m)
                inb &= _within(p, bound)
            r = [p[k] - x[k] for k in range(3)]
            res = _max3(np.abs(r[0]), np.abs(r[1]), np.abs(r[2]))
            # A = M - I, row-major a b c / d e f / g h i (m[k][a] is row a of column k)
            a, b, cc = m[0][0] - 1.0, m[1][0], m[2][0]
            d, e, f = m[0][1], m[1][1] - 1.0, m[2][1]
            g, h, i = m[0][2], m[1][2], m[2][2] - 1.0
            c00, c01, c02 = e * i - f * h, f * g - d * i, d * h - e * g
            c10, c11, c12 = cc * h - b * i, a * i - cc * g, b * g - a * h
            c20, c21, c22 = b * f - cc * e, cc * d - a * f, a * e - b * d
            det = (a * c00 + b * c01) + cc * c02
            n0 = (c00 * r[0] + c10 * r[1]) + c20 * r[2]
            n1 = (c01 * r[0] + c11 * r[1]) + c21 * r[2]
            n2 = (c02 * r[0] + c12 * r[1]) + c22 * r[2]
            esc = ~inb
            conv = inb & (res <= tol)
            last = np.full(n, it == max_newton)
            sing = (det == 0.0) | ~(np.abs(det) < np.inf)
            stop = esc | conv | last | sing
            code = np.where(esc, ESCAPED, np.where(conv, CONVERGED, np.where(last, NOT_CONVERGED, SINGULAR))).astype(np.int32)
            ended = running & stop
            status[ended] = code[ended]
            iters[ended] = it
            step = running & ~stop
            x = [np.where(step, x[k] - nk / det, x[k]) for k, nk in enumerate((n0, n1, n2))]
            running = step
    return status, iters, x


def finish(c30, x, period, same=1e-9):
    """Passes 1 and 2 for CONVERGED points x: (q, rep, M row-major (n, 9), residual)."""
    c = _rows(c30)
    n = x[0].shape[0]
    with np.errstate(all="ignore"):
        p = [v.copy() for v in x]
        rep = [v.copy() for v in x]
        q = np.full(n, period, dtype=np.uint32)
        found = np.zeros(n, dtype=bool)
        for k in range(1, period + 1):
            p = next_point(c, *p)
            d = _max3(np.abs(p[0] - x[0]), np.abs(p[1] - x[1]), np.abs(p[2] - x[2]))
            hit = ~found & (d <= same) if period % k == 0 else np.zeros(n, dtype=bool)
            q = np.where(hit, np.uint32(k), q)
            found |= hit
            less = (p[0] < rep[0]) | ((p[0] == rep[0]) & ((p[1] < rep[1]) | ((p[1] == rep[1]) & (p[2] < rep[2]))))
            take = ~found & less & (k < period)
            rep = [np.where(take, p[a], rep[a]) for a in range(3)]
        p, m = [v.copy() for v in rep], _identity(n)
        for k in range(period):
            np_, nm = _tangent(c, p, m)
            go = k < q
            p = [np.where(go, np_[a], p[a]) for a in range(3)]
            m = [[np.where(go, nm[j][a], m[j][a]) for a in range(3)] for j in range(3)]
        residual = _max3(np.abs(p[0] - rep[0]), np.abs(p[1] - rep[1]), np.abs(p[2] - rep[2]))
    M = np.stack([m[j][a] for a in range(3) for j in range(3)], axis=1)   # row a, column j
    return q, np.stack(rep, axis=1), M, residual


def merge_orbits(status, iters, q, rep, M, residual, merge=1e-6, cap=64):
    """The merge of one map's finds in start order: (record dict, orbit slots (cap,) of ORBIT_DTYPE)."""
    n = status.shape[0]
    conv = status == CONVERGED
    head = np.full(n, -1, dtype=np.int64)
    for j in np.nonzero(conv)[0]:
        d = _max3(np.abs(rep[:j + 1, 0] - rep[j, 0]), np.abs(rep[:j + 1, 1] - rep[j, 1]), np.abs(rep[:j + 1, 2] - rep[j, 2]))
        leader = int(np.nonzero(conv[:j + 1] & (q[:j + 1] == q[j]) & (d <= merge))[0][0])
        head[j] = j if leader == j else head[leader]
    heads = np.nonzero(head == np.arange(n))[0]
    hits = np.bincount(head[conv], minlength=n)
    orbits = np.zeros(cap, dtype=ORBIT_DTYPE)
    kept = heads[:cap]
    for slot, h in enumerate(kept):
        orbits[slot] = (rep[h], q[h], h, hits[h], iters[h], residual[h], M[h])
    rec = dict(converged=int(conv.sum()), escaped=int((status == ESCAPED).sum()), singular=int((status == SINGULAR).sum()),
               not_converged=int((status == NOT_CONVERGED).sum()), n_orbits=len(kept), orbits_lost=len(heads) - len(kept),
               hits_lost=int(hits[heads[cap:]].sum()), newton_iterations=int(iters.astype(np.int64).sum()))
    return rec, orbits


def cycles_one(c30, start_points, period=1, max_newton=64, tol=1e-12, bound=1e6, merge=1e-6, same=1e-9, cap=64):
    """sar_runtime_cycles for one map: (record dict, orbit slots)."""
    status, iters, x = newton(c30, start_points, period, max_newton, tol, bound)
    q, rep, M, residual = finish(c30, x, period, same)
    return merge_orbits(status, iters, q, rep, M, residual, merge, cap)


def cycles(coeffs, start_points=None, period=1, grid=8, box_lo=(-2.0, -2.0, -2.0), box_hi=(2.0, 2.0, 2.0), **params):
    """The whole call: (list of record dicts, (n_maps, cap) orbit slots). start_points None: the lattice."""
    cs = np.asarray(coeffs, np.float64).reshape(-1, 30)
    s = starts(grid, box_lo, box_hi) if start_points is None else np.asarray(start_points, np.float64).reshape(-1, 3)
    out = [cycles_one(c, s, period, **params) for c in cs]
    return [r for r, _ in out], np.stack([o for _, o in out])
