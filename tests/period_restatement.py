"""numpy restatement of the period planes (include/sar.h: sar_period_coeffs, sar_runtime_period, sar_runtime_period_colorize),
vectorised over the pixels: the planes' coefficients and transient (plane_restatement), then the first return of the orbit to within
eps of the point after the transient, in the max norm — multiplies, adds, subtractions, absolute values and compares in the device's
order, so that every field of the records, `residual` included, is bit-identical; the colours have one division and three square
roots."""
from __future__ import annotations

import numpy as np

import plane_restatement as P
import search_restatement as R

BOUNDED, DIVERGED = R.BOUNDED, R.DIVERGED
START = (0.05, 0.05, 0.05)


def period_list(cs, start=START, transient: int = 2000, max_period: int = 256, eps: float = 1e-9, bound: float = 1e6) -> dict:
    """sar_runtime_period's list form on (n, 30) coefficient sets: a dict of (n,) arrays named as the record's fields."""
    cs = 0.0 + 1.0 * np.asarray(cs, dtype=np.float64).reshape(-1, 30)
    n = cs.shape[0]
    alive, tdone, x, y, z = P.transient(cs, start, transient, bound)
    c = R._rows(cs)
    rx, ry, rz = x.copy(), y.copy(), z.copy()
    status = np.where(alive, BOUNDED, DIVERGED).astype(np.int32)
    period = np.zeros(n, dtype=np.uint32)
    done = np.where(alive, max_period, 0).astype(np.uint32)
    residual = np.full(n, np.nan)
    live = alive.copy()
    with np.errstate(all="ignore"):
        for k in range(1, max_period + 1):
            if not live.any():
                break
            x, y, z = R.next_point(c, x, y, z)
            inside = R._within(x, y, z, bound)
            d = np.maximum(np.maximum(np.abs(x - rx), np.abs(y - ry)), np.abs(z - rz))
            out = live & ~inside
            hit = live & inside & (d <= eps)
            status[out] = DIVERGED
            done[out | hit] = k
            period[hit] = k
            residual[hit] = d[hit]
            live &= ~(out | hit)
    return {"status": status, "period": period, "transient_done": tdone.astype(np.uint32), "steps_done": done, "residual": residual}


def coeffs(base, axes, x_range, y_range, width: int, height: int) -> np.ndarray:
    """(height * width, 30): the plane's coefficient sets, row-major — what the list form takes."""
    return P.coeffs(base, axes, x_range, y_range, width, height).reshape(-1, 30)


def period_plane(base, axes, x_range, y_range, width: int, height: int, **params) -> dict:
    """The whole of sar_runtime_period on the host: (height, width) arrays named as the record's fields."""
    out = period_list(coeffs(base, axes, x_range, y_range, width, height), **params)
    return {k: v.reshape(height, width) for k, v in out.items()}


def stats(rec: dict) -> dict:
    div = rec["status"] == DIVERGED
    per = rec["period"][~div]
    return {"pixels": int(rec["status"].size), "diverged_transient": int(np.count_nonzero(div & (rec["steps_done"] == 0))),
            "diverged_late": int(np.count_nonzero(div & (rec["steps_done"] != 0))), "periodic": int(np.count_nonzero(per)),
            "aperiodic": int(np.count_nonzero(per == 0)), "max_period_found": int(rec["period"].max(initial=0))}


def colorize(status, period, palette_rgb, colours: int = 16) -> np.ndarray:
    """(H, W, 4) RGBA16 of sar_runtime_period_colorize."""
    pal = np.asarray(palette_rgb, dtype=np.float64)
    pal = np.concatenate([pal, pal[-1:]])          # Palette::new duplicates the last entry
    length = pal.shape[0] - 1
    h, w = status.shape
    out = np.zeros((h, w, 4), dtype=np.uint16)
    out[..., 3] = 65535
    out[status == DIVERGED, 3] = 0
    hot = (status == BOUNDED) & (period != 0)
    slot = (np.where(hot, period, 1).astype(np.int64) - 1) % int(colours)
    with np.errstate(all="ignore"):
        v = (slot.astype(np.float64) + 0.5) / np.float64(colours)
        v = np.where(v < 0.0, 0.0, np.where(v >= 1.0, 0.999999, v))
        v = v * float(length)
        fl = np.floor(v)
        n = np.clip(fl.astype(np.int64), 0, length - 1)
        t = v - fl
        t1 = 1.0 - t
        for ch in range(3):
            col = np.sqrt(pal[n + 1, ch] * t + pal[n, ch] * t1)
            out[..., ch] = np.where(hot, P._as_u16(col * 65535.0), out[..., ch])
    return out
