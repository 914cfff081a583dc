"""numpy restatement of the power spectra (include/sar.h: sar_runtime_spectra, sar_runtime_spectrum), written from the contract alone
and vectorised over whatever axes lead the last one (jobs, maps): the plotted value, the segments, the pairwise sums, the taper, the
plain radix-2 decimation-in-time transform stage by stage, the periodogram and the left folds over segments and jobs — the same
multiplies, adds and subtractions in the same order, so that every output double is bit-identical to the device's. The tables are
built here, element by element, with math.cos and math.sin; the maps step through search_restatement.next_point
(corr_restatement.record_points)."""
from __future__ import annotations

import math

import numpy as np

import corr_restatement as CR

BOUNDED, DIVERGED = CR.BOUNDED, CR.DIVERGED
RECT, HANN = 0, 1


def twiddles(n: int) -> np.ndarray:
    """(n / 2, 2): tw[k] = (cos(2.0 * pi * k / n), -sin(the same))."""
    return np.array([[math.cos(2.0 * math.pi * float(k) / float(n)), -math.sin(2.0 * math.pi * float(k) / float(n))] for k in range(n // 2)])


def window(kind: int, n: int) -> np.ndarray:
    if kind == RECT:
        return np.ones(n)
    assert kind == HANN
    return np.array([0.5 - 0.5 * math.cos(2.0 * math.pi * float(t) / float(n)) for t in range(n)])


def tree(a: np.ndarray) -> np.ndarray:
    """a <- a[0::2] + a[1::2] along the last axis until one value is left."""
    while a.shape[-1] > 1:
        a = a[..., 0::2] + a[..., 1::2]
    return a[..., 0]


def bit_reversal(n: int) -> np.ndarray:
    bits = n.bit_length() - 1
    return np.array([int(format(i, f"0{bits}b")[::-1], 2) for i in range(n)])


def transform(a: np.ndarray, tw: np.ndarray):
    """(re, im) of the transform of (a, 0) along the last axis: every butterfly of every stage, none skipped."""
    n = a.shape[-1]
    lead = a.shape[:-1]
    re, im = a[..., bit_reversal(n)].copy(), np.zeros(a.shape)
    length = 2
    while length <= n:
        half = length // 2
        w = tw[np.arange(half) * (n // length)]
        wr, wi = w[:, 0], w[:, 1]
        re, im = re.reshape(*lead, n // length, length), im.reshape(*lead, n // length, length)
        ur, ui, br, bi = re[..., :half], im[..., :half], re[..., half:], im[..., half:]
        tr = wr * br - wi * bi
        ti = wr * bi + wi * br
        re = np.concatenate([ur + tr, ur - tr], axis=-1).reshape(*lead, n)
        im = np.concatenate([ui + ti, ui - ti], axis=-1).reshape(*lead, n)
        length *= 2
    return re, im


def n_segments(samples: int, n: int, hop: int) -> int:
    return (samples - n) // hop + 1


def job_sums(v: np.ndarray, n: int, hop: int, kind: int):
    """(P_j (..., n / 2 + 1), E_j (...)) of trajectories v (..., samples): the left folds over the segments from +0.0."""
    tw, w, inv_n = twiddles(n), window(kind, n), 1.0 / float(n)
    power, energy = np.zeros(v.shape[:-1] + (n // 2 + 1,)), np.zeros(v.shape[:-1])
    with np.errstate(all="ignore"):
        for s in range(n_segments(v.shape[-1], n, hop)):
            seg = v[..., s * hop:s * hop + n]
            m = tree(seg) * inv_n
            a = (seg - m[..., None]) * w
            energy = energy + tree(a * a)
            re, im = transform(a, tw)
            power = power + (re[..., :n // 2 + 1] * re[..., :n // 2 + 1] + im[..., :n // 2 + 1] * im[..., :n // 2 + 1])
    return power, energy


def fold_jobs(power_j: np.ndarray, energy_j: np.ndarray):
    """The left folds over the jobs (axis -2 of the power, -1 of the energy) from +0.0, in job order."""
    power, energy = np.zeros(power_j.shape[:-2] + power_j.shape[-1:]), np.zeros(energy_j.shape[:-1])
    with np.errstate(all="ignore"):
        for j in range(power_j.shape[-2]):
            power = power + power_j[..., j, :]
            energy = energy + energy_j[..., j]
    return power, energy


def series(points, proj=(1.0, 0.0, 0.0)) -> np.ndarray:
    p = np.asarray(points, dtype=np.float64)
    p0, p1, p2 = (np.float64(c) for c in proj)
    with np.errstate(all="ignore"):
        return (p0 * p[..., 0] + p1 * p[..., 1]) + p2 * p[..., 2]


def spectra(points, n=1024, hop=None, kind=HANN, samples=None, proj=(1.0, 0.0, 0.0)):
    """sar_runtime_spectra on the host: points (..., n_points, 3) -> (power (..., n / 2 + 1), energy (...), jobs, segments)."""
    p = np.asarray(points, dtype=np.float64)
    n_points = p.shape[-2]
    hop = n // 2 if hop is None else hop
    samples = n_points if samples is None else samples
    assert samples >= n and n_points % samples == 0
    v = series(p, proj).reshape(p.shape[:-2] + (n_points // samples, samples))
    power, energy = fold_jobs(*job_sums(v, n, hop, kind))
    return power, energy, n_points // samples, n_segments(samples, n, hop)


def spectrum(coeffs, starts, segments=15, n=1024, hop=512, kind=HANN, stride=1, transient=1000, bound=1e6, proj=(1.0, 0.0, 0.0)) -> dict:
    """sar_runtime_spectrum for one map on the host."""
    samples = (segments - 1) * hop + n
    status, job, step, pts = CR.record_points(coeffs, starts, samples, stride, transient, bound)
    if status == DIVERGED:
        return dict(status=status, fail_job=job, fail_step=step, power=np.zeros(n // 2 + 1), energy=0.0, segments=0, points=pts,
                    extent=np.array([np.inf, -np.inf] * 3))
    power, energy, _, segs = spectra(pts, n, hop, kind, samples, proj)
    return dict(status=status, fail_job=0, fail_step=0, power=power, energy=float(energy), segments=segs, points=pts, extent=CR.extent(pts))


def flatness(power) -> float:
    p = np.asarray(power)[1:]
    if not np.all(p > 0.0):
        return 0.0
    return float(np.exp(np.mean(np.log(p))) / np.mean(p))
