"""numpy restatement of the Lyapunov planes (include/sar.h: sar_plane_coeffs, sar_runtime_plane, sar_runtime_plane_colorize),
vectorised over the pixels: the same multiplies, adds, divides, square roots and frexp in the same order as the device, so that
the raw fields of the records (status, transient_done, steps_done, log2_exp, mant) are bit-identical; the spectrum mode is
search_restatement.lyapunov itself, and the finish is search_restatement.finish (math.log)."""
from __future__ import annotations

import math

import numpy as np

import search_restatement as R

BOUNDED, DIVERGED, DEGENERATE = R.BOUNDED, R.DIVERGED, R.DEGENERATE
LN2 = 0.6931471805599453


def sweep(lo: float, hi: float, n: int) -> np.ndarray:
    """The n values of one axis: lo + (hi - lo) * (i / (n - 1)), t = 0 when n == 1."""
    i = np.arange(n, dtype=np.float64)
    t = i / np.float64(n - 1) if n > 1 else np.zeros(n)
    return np.float64(lo) + np.float64(hi - lo) * t


def coeffs(base, axes, x_range, y_range, width: int, height: int) -> np.ndarray:
    """(height, width, 30): pixel (x, y) is base with axes[0] = sweep(x_range)[x] and axes[1] = sweep(y_range)[height-1-y]."""
    b = np.asarray(base, dtype=np.float64).reshape(30)
    out = np.broadcast_to(b, (height, width, 30)).copy()
    out[:, :, axes[0]] = sweep(*x_range, width)[None, :]
    out[:, :, axes[1]] = sweep(*y_range, height)[::-1][:, None]
    return 0.0 + 1.0 * out


def transient(cs: np.ndarray, start, steps: int, bound: float):
    """(alive, transient_done, x, y, z) after `steps` steps: transient_done is the first step outside the box (1-based)."""
    c = R._rows(cs)
    n = cs.shape[0]
    x, y, z = (np.full(n, float(v)) for v in start)
    alive = np.ones(n, dtype=bool)
    done = np.full(n, steps, dtype=np.uint32)
    with np.errstate(all="ignore"):
        for t in range(steps):
            x, y, z = R.next_point(c, x, y, z)
            out = alive & ~R._within(x, y, z, bound)
            done[out] = t + 1
            alive &= ~out
    return alive, done, x, y, z


def l1(cs: np.ndarray, x, y, z, steps: int, bound: float) -> dict:
    """The L1 recurrence: q1 = e1, per step v = J(p) q1, n1 = |v|, q1 = v / n1, M *= n1 folded by frexp; the status rules of
    the search on n1 alone, then the bound test."""
    c = R._rows(cs)
    n = cs.shape[0]
    x, y, z = (np.array(v, dtype=np.float64) for v in (x, y, z))
    q = [np.ones(n), np.zeros(n), np.zeros(n)]
    m = np.ones(n)
    e = np.zeros(n, dtype=np.int64)
    status = np.zeros(n, dtype=np.int32)
    done = np.full(n, steps, dtype=np.uint32)
    active = np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for t in range(steps):
            if not active.any():
                break
            x2, y2, z2 = x + x, y + y, z + z
            v = []
            for r in c:
                jx = ((r[1] + x2 * r[2]) + y * r[3]) + z * r[4]
                jy = ((x * r[3] + r[5]) + y2 * r[6]) + z * r[7]
                jz = ((x * r[4] + y * r[7]) + r[8]) + z2 * r[9]
                v.append((jx * q[0] + jy * q[1]) + jz * q[2])
            n1 = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
            rr = 1.0 / n1
            v = [v[0] * rr, v[1] * rr, v[2] * rr]
            nx, ny, nz = R.next_point(c, x, y, z)
            st = R._norm_status(n1)
            st = np.where((st == BOUNDED) & ~R._within(nx, ny, nz, bound), DIVERGED, st)
            fail = active & (st != BOUNDED)
            status[fail] = st[fail]
            done[fail] = t + 1
            ok = active & (st == BOUNDED)
            active = ok
            mm, ee = np.frexp(m * n1)
            m = np.where(ok, mm, m)
            e = np.where(ok, e + ee, e)
            x, y, z = (np.where(ok, a_, b_) for a_, b_ in ((nx, x), (ny, y), (nz, z)))
            q = [np.where(ok, v[k], q[k]) for k in range(3)]
    return {"status": status, "steps_done": done, "log2_exp": e, "mant": m}


def folded(status: int, steps_done: int) -> int:
    return steps_done if status == BOUNDED else max(steps_done - 1, 0)


def plane(base, axes, x_range, y_range, width: int, height: int, mode: str = "l1", start=(0.05, 0.05, 0.05),
          transient_steps: int = 1000, steps: int = 20000, bound: float = 1e6) -> dict:
    """The whole of sar_runtime_plane on the host: a dict of (height, width[, 3]) arrays named as the record's fields."""
    cs = coeffs(base, axes, x_range, y_range, width, height).reshape(-1, 30)
    n = cs.shape[0]
    alive, tdone, x, y, z = transient(cs, start, transient_steps, bound)
    idx = np.nonzero(alive)[0]
    out = {"status": np.full(n, DIVERGED, dtype=np.int32), "transient_done": tdone, "steps_done": np.zeros(n, dtype=np.uint32),
           "log2_exp": np.zeros((n, 3), dtype=np.int64), "mant": np.ones((n, 3)), "lyapunov": np.full((n, 3), np.nan),
           "ky_dim": np.full(n, np.nan)}
    if mode == "l1":
        raw = l1(cs[idx], x[idx], y[idx], z[idx], steps, bound)
        out["log2_exp"][idx, 0] = raw["log2_exp"]
        out["mant"][idx, 0] = raw["mant"]
    else:
        raw = R.lyapunov(cs[idx], x[idx], y[idx], z[idx], steps, bound)
        out["log2_exp"][idx] = raw["log2_exp"]
        out["mant"][idx] = raw["mant"]
    out["status"][idx] = raw["status"]
    out["steps_done"][idx] = raw["steps_done"]
    for i in idx:
        f = folded(int(out["status"][i]), int(out["steps_done"][i]))
        if mode == "l1":
            if f:
                out["lyapunov"][i, 0] = (float(out["log2_exp"][i, 0]) * LN2 + math.log(float(out["mant"][i, 0]))) / f
        else:
            lam, ky = R.finish(int(out["status"][i]), int(out["steps_done"][i]), out["log2_exp"][i], out["mant"][i])
            out["lyapunov"][i], out["ky_dim"][i] = lam, ky
    return {k: v.reshape((height, width) + v.shape[1:]) for k, v in out.items()}


def _as_u16(v: np.ndarray) -> np.ndarray:
    """Rust `as u16` of an f64: saturating, NaN -> 0."""
    v = np.where(np.isnan(v), 0.0, v)
    return np.clip(np.trunc(v), 0.0, 65535.0).astype(np.uint16)


def colorize(status, steps_done, lam1, palette_rgb, threshold: float = 0.0, chaos_scale: float = 0.25,
             order_scale: float = 1.0) -> np.ndarray:
    """(H, W, 4) RGBA16 of sar_runtime_plane_colorize from the records' status, steps_done and lambda_1 (the host finish's)."""
    pal = np.asarray(palette_rgb, dtype=np.float64)
    pal = np.concatenate([pal, pal[-1:]])          # Palette::new duplicates the last entry
    length = pal.shape[0] - 1
    h, w = status.shape
    out = np.zeros((h, w, 4), dtype=np.uint16)
    out[..., 3] = 65535
    out[status == DIVERGED, 3] = 0
    ok = (status == BOUNDED) & (steps_done != 0)
    hot = ok & (lam1 >= threshold)
    cold = ok & ~(lam1 >= threshold)
    with np.errstate(all="ignore"):
        v = (lam1 - threshold) / chaos_scale
        v = np.where(v < 0.0, 0.0, np.where(v >= 1.0, 0.999999, v))
        v = v * float(length)
        fl = np.floor(v)
        n = np.where(np.isnan(fl), 0, fl).astype(np.int64)
        n = np.clip(np.minimum(n, length - 1), 0, length - 1)
        t = v - fl
        t1 = 1.0 - t
        for ch in range(3):
            col = np.sqrt(pal[n + 1, ch] * t + pal[n, ch] * t1)
            out[..., ch] = np.where(hot, _as_u16(col * 65535.0), out[..., ch])
        f = 1.0 - (threshold - lam1) / order_scale
        g = 0.5 * np.where(f > 0.0, f, 0.0)
        grey = _as_u16(g * 65535.0)
    for ch in range(3):
        out[..., ch] = np.where(cold, grey, out[..., ch])
    return out
