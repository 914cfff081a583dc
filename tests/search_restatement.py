"""numpy restatement of the chaotic-map search (include/sar.h: sar_search_candidate, sar_runtime_search), vectorised over the
candidates: the same multiplies, adds, divides, square roots and frexp in the same order, so that the raw fields of the
records (status, steps_done, log2_exp, mant, extent) are bit-identical to the device's; the finish uses math.log."""
from __future__ import annotations

import math

import numpy as np

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
BOUNDED, DIVERGED, DEGENERATE = 0, 1, 2


def mix64(z: np.ndarray) -> np.ndarray:
    z = np.asarray(z, dtype=np.uint64)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def candidates(seed: int, first: int, n: int, lo: float = -1.2, hi: float = 1.2) -> np.ndarray:
    """(n, 30) coefficients of candidates first .. first+n-1: draw 30c+j of SplitMix64(seed), lo + (hi - lo) * u."""
    idx = np.arange(first, first + n, dtype=np.uint64)[:, None] * np.uint64(30) + np.arange(30, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        d = mix64(np.uint64(seed) + (idx + np.uint64(1)) * GOLDEN)
    u = (d >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    c = np.float64(lo) + np.float64(hi - lo) * u
    return 0.0 + 1.0 * c


def next_point(c, x, y, z):
    """PolynomialSprott2Degree::next_point, c = (cx, cy, cz), each a list of 10 arrays (or scalars)."""
    xx, xy, xz, yy, yz, zz = x * x, x * y, x * z, y * y, y * z, z * z
    terms = (None, x, xx, xy, xz, y, yy, yz, z, zz)
    out = []
    for row in c:
        s = row[0]
        for k in range(1, 10):
            s = s + terms[k] * row[k]
        out.append(s)
    return out


def _rows(coeffs: np.ndarray):
    return [[coeffs[:, 10 * r + k] for k in range(10)] for r in range(3)]


def _within(x, y, z, bound):
    return (np.abs(x) <= bound) & (np.abs(y) <= bound) & (np.abs(z) <= bound)


def screen(coeffs: np.ndarray, start, transient: int, bound: float):
    """Phase 1: (alive mask, x, y, z) after `transient` steps."""
    c = _rows(coeffs)
    n = coeffs.shape[0]
    x, y, z = (np.full(n, float(v)) for v in start)
    alive = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for _ in range(transient):
            x, y, z = next_point(c, x, y, z)
            alive &= _within(x, y, z, bound)
    return alive, x, y, z


def _norm_status(n):
    return np.where(n == 0.0, DEGENERATE, np.where(n < np.inf, BOUNDED, DIVERGED))


def lyapunov(coeffs: np.ndarray, x, y, z, steps: int, bound: float) -> dict:
    """Phase 2 for the given survivors: raw fields as the device writes them."""
    c = _rows(coeffs)
    n = coeffs.shape[0]
    x, y, z = (np.array(v, dtype=np.float64) for v in (x, y, z))
    one, zero = np.ones(n), np.zeros(n)
    q = [[one.copy(), zero.copy(), zero.copy()], [zero.copy(), one.copy(), zero.copy()], [zero.copy(), zero.copy(), one.copy()]]
    m = [one.copy() for _ in range(3)]
    e = [np.zeros(n, dtype=np.int64) for _ in range(3)]
    b = [np.full(n, np.inf) if k % 2 == 0 else np.full(n, -np.inf) for k in range(6)]
    status = np.zeros(n, dtype=np.int32)
    done = np.full(n, steps, dtype=np.uint32)
    active = np.ones(n, dtype=bool)
    cx, cy, cz = c
    with np.errstate(all="ignore"):
        for t in range(steps):
            if not active.any():
                break
            x2, y2, z2 = x + x, y + y, z + z
            J = []
            for r in (cx, cy, cz):
                J.append((((r[1] + x2 * r[2]) + y * r[3]) + z * r[4],
                          ((x * r[3] + r[5]) + y2 * r[6]) + z * r[7],
                          ((x * r[4] + y * r[7]) + r[8]) + z2 * r[9]))
            v = [[(J[a][0] * q[k][0] + J[a][1] * q[k][1]) + J[a][2] * q[k][2] for a in range(3)] for k in range(3)]
            norms = []

            def normalise(w):
                nn = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
                r_ = 1.0 / nn
                return nn, [w[0] * r_, w[1] * r_, w[2] * r_]

            def reject(qq, w):
                d = (qq[0] * w[0] + qq[1] * w[1]) + qq[2] * w[2]
                return [w[0] - d * qq[0], w[1] - d * qq[1], w[2] - d * qq[2]]

            n1, v[0] = normalise(v[0])
            v[1] = reject(v[0], v[1])
            n2, v[1] = normalise(v[1])
            v[2] = reject(v[0], v[2])
            v[2] = reject(v[1], v[2])
            n3, v[2] = normalise(v[2])
            nx, ny, nz = next_point(c, x, y, z)
            st = _norm_status(n1)
            st = np.where(st == BOUNDED, _norm_status(n2), st)
            st = np.where(st == BOUNDED, _norm_status(n3), st)
            st = np.where((st == BOUNDED) & ~_within(nx, ny, nz, bound), DIVERGED, st)
            fail = active & (st != BOUNDED)
            status[fail] = st[fail]
            done[fail] = t + 1
            ok = active & (st == BOUNDED)
            active = ok
            for i, nn in enumerate((n1, n2, n3)):
                mm, ee = np.frexp(m[i] * nn)
                m[i] = np.where(ok, mm, m[i])
                e[i] = np.where(ok, e[i] + ee, e[i])
            x, y, z = (np.where(ok, a_, b_) for a_, b_ in ((nx, x), (ny, y), (nz, z)))
            for k, w in enumerate((x, y, z)):
                b[2 * k] = np.where(ok & (w < b[2 * k]), w, b[2 * k])
                b[2 * k + 1] = np.where(ok & (w > b[2 * k + 1]), w, b[2 * k + 1])
            q = [[np.where(ok, v[k][a], q[k][a]) for a in range(3)] for k in range(3)]
    return {"status": status, "steps_done": done, "log2_exp": np.stack(e, 1), "mant": np.stack(m, 1), "extent": np.stack(b, 1)}


def finish(status: int, steps_done: int, log2_exp, mant):
    """lambda (sorted descending) and the Kaplan-Yorke dimension, as the host finish does."""
    folded = steps_done if status == BOUNDED else steps_done - 1
    if not folded:
        return [math.nan] * 3, math.nan
    lam = sorted(((float(log2_exp[i]) * 0.6931471805599453 + math.log(float(mant[i]))) / folded for i in range(3)), reverse=True)
    s, j = 0.0, 0
    for i in range(3):
        if s + lam[i] < 0.0:
            break
        s = s + lam[i]
        j = i + 1
    ky = 3.0 if j == 3 else (0.0 if j == 0 else j + s / abs(lam[j]))
    return lam, ky


def search(seed: int, first: int, n: int, transient: int = 1000, steps: int = 20000, bound: float = 1e6, start=(0.05, 0.05, 0.05),
           lo: float = -1.2, hi: float = 1.2, coeffs=None, min_lyapunov: float = 0.005, min_ky_dim: float = 0.0,
           keep_rejected: bool = False):
    """The whole of sar_runtime_search on the host: (records as a list of dicts sorted by candidate, stats dict)."""
    cs = candidates(seed, first, n, lo, hi) if coeffs is None else 0.0 + 1.0 * np.asarray(coeffs, np.float64).reshape(n, 30)
    alive, x, y, z = screen(cs, start, transient, bound)
    idx = np.nonzero(alive)[0]
    raw = lyapunov(cs[idx], x[idx], y[idx], z[idx], steps, bound)
    stats = dict(tested=n, diverged_transient=int(n - idx.size), diverged_late=0, degenerate=0, below_lyapunov=0, below_dim=0,
                 accepted=0)
    records = []
    for k, i in enumerate(idx):
        r = {key: raw[key][k] for key in raw}
        r["candidate"] = first + int(i)
        r["lyapunov"], r["ky_dim"] = finish(int(r["status"]), int(r["steps_done"]), r["log2_exp"], r["mant"])
        acc = False
        if r["status"] == DIVERGED:
            stats["diverged_late"] += 1
        elif r["status"] == DEGENERATE:
            stats["degenerate"] += 1
        elif not r["lyapunov"][0] >= min_lyapunov:
            stats["below_lyapunov"] += 1
        elif not r["ky_dim"] >= min_ky_dim:
            stats["below_dim"] += 1
        else:
            acc = True
            stats["accepted"] += 1
        if acc or keep_rejected:
            records.append(r)
    return records, stats
