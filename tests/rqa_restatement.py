"""numpy restatement of the recurrence analysis (include/sar.h: sar_runtime_recurrence, sar_runtime_recurrence_plot, sar_runtime_rqa,
sar_rqa_measures), written from the contract alone: the boolean recurrence matrix of every trajectory, built whole (T up to about
1000), its maximal diagonal runs in the upper triangle and its maximal vertical runs in the full matrix, scanned one by one; a map's
points from corr_restatement's orbits and its threshold from their extent; the measures in the stated order. Every count is
bit-identical to the device's."""
from __future__ import annotations

import math

import numpy as np

import corr_restatement as CR

BOUNDED, DIVERGED = CR.BOUNDED, CR.DIVERGED
COUNTS = ("recurrences", "pairs", "diag_lines", "vert_lines", "diag_longest", "vert_longest")


def matrix(traj, eps2, theiler=0) -> np.ndarray:
    """R[i, j] = |i - j| > theiler and r2(i, j) < eps2 of one trajectory (T, 3), with r2 = (dx dx + dy dy) + dz dz, dx = x_j - x_i."""
    p = np.asarray(traj, dtype=np.float64).reshape(-1, 3)
    t = p.shape[0]
    with np.errstate(all="ignore"):
        d = p[None, :, :] - p[:, None, :]                       # d[i, j] = p_j - p_i
        r2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        near = r2 < eps2                                        # (False for NaN and +inf)
    i = np.arange(t)
    return near & (np.abs(i[:, None] - i[None, :]) > theiler)


def runs(seq) -> list:
    """The lengths of the maximal runs of ones of a boolean sequence, in order."""
    edges = np.diff(np.concatenate(([0], np.asarray(seq, dtype=np.int8), [0])))      # +1 where a run starts, -1 behind its end
    return (np.nonzero(edges == -1)[0] - np.nonzero(edges == 1)[0]).tolist()


def _count(hist, lengths, bins):
    for l in lengths:
        hist[min(l, bins)] += 1


def lines(points, eps2, samples=None, theiler=0, line_bins=256):
    """(diag uint64 (B + 1,), vert uint64 (B + 1,), counts dict) of one set (n, 3)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    t = n if not samples else samples
    assert t and n % t == 0
    diag, vert = np.zeros(line_bins + 1, dtype=np.uint64), np.zeros(line_bins + 1, dtype=np.uint64)
    c = dict.fromkeys(COUNTS, 0)
    for job in range(n // t):
        r = matrix(p[job * t:(job + 1) * t], eps2, theiler)
        c["recurrences"] += int(np.triu(r, 1).sum())
        c["pairs"] += (t - theiler - 1) * (t - theiler) // 2 if t > theiler + 1 else 0
        for k in range(theiler + 1, t):
            ls = runs(np.diagonal(r, k))                       # R(i, i + k), i = 0 .. T - k - 1
            _count(diag, ls, line_bins)
            c["diag_lines"] += len(ls)
            c["diag_longest"] = max([c["diag_longest"]] + ls)
        for j in range(t):
            ls = runs(r[:, j])
            _count(vert, ls, line_bins)
            c["vert_lines"] += len(ls)
            c["vert_longest"] = max([c["vert_longest"]] + ls)
    return diag, vert, c


def ends_at_the_end(points, eps2, samples=None, theiler=0) -> bool:
    """Whether a diagonal line of some trajectory ends with its diagonal (at the trajectory's last point)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    t = p.shape[0] if not samples else samples
    return any(bool(matrix(p[a:a + t], eps2, theiler)[:t - 1 - theiler, t - 1].any()) for a in range(0, p.shape[0], t))


def map_eps2(extent, eps2=0.0, eps_fraction=0.05) -> float:
    """The threshold of a BOUNDED map: eps2 > 0 as given, otherwise (f f) ((dx dx + dy dy) + dz dz) of the extent's spans; 0 where that
    is 0 or not finite."""
    if eps2 > 0.0:
        return eps2
    with np.errstate(all="ignore"):
        ext = np.asarray(extent, dtype=np.float64)
        dx, dy, dz = ext[1] - ext[0], ext[3] - ext[2], ext[5] - ext[4]
        e = float((np.float64(eps_fraction) * np.float64(eps_fraction)) * ((dx * dx + dy * dy) + dz * dz))
    return e if e > 0.0 and math.isfinite(e) else 0.0


def rqa(coeffs, starts, samples, stride=1, transient=1000, theiler=0, line_bins=256, bound=1e6, eps2=0.0, eps_fraction=0.05) -> dict:
    """sar_runtime_rqa for one map on the host."""
    status, job, step, pts = CR.record_points(coeffs, starts, samples, stride, transient, bound)
    zero = np.zeros(line_bins + 1, dtype=np.uint64)
    if status == DIVERGED:
        return dict(status=status, fail_job=job, fail_step=step, points=pts, extent=np.array([np.inf, -np.inf] * 3), eps2=0.0, diag=zero,
                    vert=zero.copy(), counts=dict.fromkeys(COUNTS, 0))
    ext = CR.extent(pts)
    e = map_eps2(ext, eps2, eps_fraction)
    if e == 0.0:
        diag, vert, c = zero, zero.copy(), dict.fromkeys(COUNTS, 0)
    else:
        diag, vert, c = lines(pts, e, samples, theiler, line_bins)
    return dict(status=status, fail_job=0, fail_step=0, points=pts, extent=ext, eps2=e, diag=diag, vert=vert, counts=c)


def _ratio(num: int, den: int) -> float:
    return float(np.float64(num) / np.float64(den)) if den else math.nan


def _line_measures(hist, l_min, total):
    hist = [int(v) for v in hist]
    below = sum(l * hist[l] for l in range(1, l_min))
    n_lines = sum(hist[l_min:])
    h = 0.0 if n_lines else math.nan
    for l in range(l_min, len(hist)):
        if hist[l] and n_lines:
            p = np.float64(hist[l]) / np.float64(n_lines)
            h = h - p * np.log(p)
    return _ratio(total - below, total), _ratio(total - below, n_lines), float(h)


def measures(diag, vert, counts, l_min=2, v_min=2) -> dict:
    """sar_rqa_measures in its stated order."""
    rec = int(counts["recurrences"])
    det, l_mean, entr = _line_measures(diag, l_min, rec)
    lam, tt, _ = _line_measures(vert, v_min, 2 * rec)
    return dict(rr=_ratio(rec, int(counts["pairs"])), det=det, l_mean=l_mean, div=_ratio(1, int(counts["diag_longest"])), entr=entr, lam=lam,
                tt=tt, l_max=int(counts["diag_longest"]), v_max=int(counts["vert_longest"]))
