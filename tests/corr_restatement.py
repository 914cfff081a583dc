"""numpy restatement of the correlation dimension (include/sar.h: sar_runtime_pairs, sar_runtime_corrdim, sar_corrdim_fit), written
from the contract alone: the bin of a pair from the bits of r^2, every pair i < j outside the Theiler window, the recorded points of a
map (search_restatement's map step), and the least-squares line. The histograms, counts, statuses and points are bit-identical to the
device's; the line agrees with the library's to the conditioning of the fit."""
from __future__ import annotations

import math

import numpy as np

import search_restatement as R

BOUNDED, DIVERGED = 0, 1
FIT_OK, NO_WINDOW = 0, 1


def n_bins(sub_bits=2, e_min=-64, e_max=8) -> int:
    return ((e_max - e_min) << sub_bits) + 2


def edges_r2(sub_bits=2, e_min=-64, e_max=8) -> np.ndarray:
    """r2_b for b < bins - 1: (1 + m / 2^s) 2^(e_min + e), (e, m) = divmod(b, 2^s) — exact."""
    b = np.arange(n_bins(sub_bits, e_min, e_max) - 1)
    e, m = b >> sub_bits, b & ((1 << sub_bits) - 1)
    return np.ldexp(1.0 + m / float(1 << sub_bits), e_min + e)


def bin_of(r2, sub_bits=2, e_min=-64, e_max=8) -> np.ndarray:
    bits = np.ascontiguousarray(r2, dtype=np.float64).view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)
    key = (bits >> np.uint64(52 - sub_bits)).astype(np.int64) - ((1023 + e_min) << sub_bits)
    top = (e_max - e_min) << sub_bits
    return np.where(key < 0, 0, np.where(key < top, key + 1, top + 1))


def pair_hist(points, samples=None, theiler=0, sub_bits=2, e_min=-64, e_max=8):
    """(hist uint64 (bins,), counted, skipped) of one set (n, 3), pair by pair."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    samples = n if samples is None else samples
    assert samples and n % samples == 0
    bins = n_bins(sub_bits, e_min, e_max)
    hist = np.zeros(bins, dtype=np.int64)
    skipped = 0
    traj = np.arange(n) // samples
    with np.errstate(all="ignore"):
        for i in range(n - 1):
            j = np.arange(i + 1, n)
            skip = (traj[j] == traj[i]) & (j - i <= theiler)
            skipped += int(skip.sum())
            d = p[i + 1:] - p[i]
            r2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
            hist += np.bincount(bin_of(r2, sub_bits, e_min, e_max)[~skip], minlength=bins)
    return hist.astype(np.uint64), int(hist.sum()), skipped


def record_points(coeffs, starts, samples, stride, transient, bound=1e6):
    """One map's run: (status, fail_job, fail_step, points (jobs * samples, 3)). Steps are numbered from 1, the transient included; a
    DIVERGED map names its lowest failing job and that job's step, and its points are all zero."""
    c = R._rows((0.0 + 1.0 * np.asarray(coeffs, dtype=np.float64).reshape(1, 30)).repeat(len(starts), axis=0))
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, 3)
    jobs = starts.shape[0]
    x, y, z = starts[:, 0].copy(), starts[:, 1].copy(), starts[:, 2].copy()
    fail = np.zeros(jobs, dtype=np.int64)
    pts = np.zeros((jobs, samples, 3))
    with np.errstate(all="ignore"):
        for t in range(1, transient + stride * samples + 1):
            x, y, z = R.next_point(c, x, y, z)
            out = ~R._within(x, y, z, bound)
            fail = np.where((fail == 0) & out, t, fail)
            if t > transient and (t - transient) % stride == 0:
                pts[:, (t - transient) // stride - 1] = np.stack([x, y, z], axis=1)
    if fail.any():
        job = int(np.nonzero(fail)[0][0])
        return DIVERGED, job, int(fail[job]), np.zeros((jobs * samples, 3))
    return BOUNDED, 0, 0, pts.reshape(jobs * samples, 3)


def extent(points) -> np.ndarray:
    p = np.asarray(points).reshape(-1, 3)
    return np.array([p[:, 0].min(), p[:, 0].max(), p[:, 1].min(), p[:, 1].max(), p[:, 2].min(), p[:, 2].max()])


def fit(hist, c_lo=100.0, r_hi=math.inf, sub_bits=2, e_min=-64, e_max=8) -> dict:
    """The line of ln C_b on 0.5 ln r2_b over the bins 1 .. bins - 2 with C_b >= c_lo and sqrt(r2_b) <= r_hi, in bin order."""
    hist = [int(v) for v in hist]
    r2 = edges_r2(sub_bits, e_min, e_max)
    c, xs, ys, used = hist[0], [], [], []
    for b in range(1, len(hist) - 1):
        c += hist[b]
        if c >= c_lo and math.sqrt(r2[b]) <= r_hi:
            xs.append(0.5 * math.log(r2[b]))
            ys.append(math.log(c))
            used.append(b)
    nan = math.nan
    if len(xs) < 3:
        return dict(slope=nan, intercept=nan, rms=nan, first_bin=0, last_bin=0, used=0, status=NO_WINDOW)
    k = len(xs)
    mx, my = sum(xs) / k, sum(ys) / k
    sxx = sum((x - mx) * (x - mx) for x in xs)
    sxy = sum((x - mx) * (y - my) for x, y in zip(xs, ys))
    slope = sxy / sxx
    icpt = my - slope * mx
    rms = math.sqrt(sum((y - (icpt + slope * x)) ** 2 for x, y in zip(xs, ys)) / k)
    return dict(slope=slope, intercept=icpt, rms=rms, first_bin=used[0], last_bin=used[-1], used=k, status=FIT_OK)


def corrdim(coeffs, starts, samples, stride, transient, theiler=0, bound=1e6, c_lo=100.0, r_hi_fraction=2.0 ** -4, sub_bits=2, e_min=-64,
            e_max=8) -> dict:
    """sar_runtime_corrdim for one map on the host."""
    status, job, step, pts = record_points(coeffs, starts, samples, stride, transient, bound)
    bins = n_bins(sub_bits, e_min, e_max)
    if status == DIVERGED:
        return dict(status=status, fail_job=job, fail_step=step, hist=np.zeros(bins, dtype=np.uint64), counted=0, skipped=0, points=pts,
                    extent=np.array([np.inf, -np.inf] * 3), r_hi=math.nan, line=fit(np.zeros(bins, dtype=np.uint64)))
    hist, counted, skipped = pair_hist(pts, samples, theiler, sub_bits, e_min, e_max)
    ext = extent(pts)
    dx, dy, dz = ext[1] - ext[0], ext[3] - ext[2], ext[5] - ext[4]
    r_hi = r_hi_fraction * math.sqrt((dx * dx + dy * dy) + dz * dz)
    return dict(status=status, fail_job=0, fail_step=0, hist=hist, counted=counted, skipped=skipped, points=pts, extent=ext, r_hi=r_hi,
                line=fit(hist, c_lo, r_hi, sub_bits, e_min, e_max))
