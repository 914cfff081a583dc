"""What the power-spectrum tests share (tests/test_spectrum_host.py, tests/test_gpu_spectrum.py): the maps, in the search's row order,
the planted series at N = 8, random sets, and every parameter set the calls must refuse, with a piece of the message they leave."""
import math

import numpy as np

from corr_cases import henon
from orbit_cases import logistic

ROTATION_BIN = 37     # of 256


def logistic_map(r):
    """x' = r x - r x^2."""
    return logistic(r, r)[0]


def rotation(k=ROTATION_BIN, n=256):
    """The rotation of the (x, y) plane by 2 pi k / n per step (z' = 0): a line at bin k of an n-point spectrum."""
    c = np.zeros((3, 10))
    a = 2.0 * math.pi * k / n
    c[0, 1], c[0, 5] = math.cos(a), -math.sin(a)
    c[1, 1], c[1, 5] = math.sin(a), math.cos(a)
    return c.reshape(30)


def six_maps():
    """Henon, the logistic map at r = 3.2 (period 2), 3.5 (period 4) and 3.9 (chaos), the rotation, and the logistic map at r = 4.5,
    which leaves the bound box."""
    return np.stack([henon(), logistic_map(3.2), logistic_map(3.5), logistic_map(3.9), rotation(), logistic_map(4.5)])


def unit_starts(jobs, seed=5):
    """Start points with x and z in [0.1, 0.9] and y in [0, 0.1]: on the logistic map's interval, off the rotation's centre, inside
    Henon's basin."""
    return np.array([0.1, 0.0, 0.1]) + np.array([0.8, 0.1, 0.8]) * np.random.default_rng(seed).random((jobs, 3))


def random_sets(n_points, n_sets=3, seed=23):
    """Random points whose magnitudes spread over 20 binades."""
    rng = np.random.default_rng(seed + n_points)
    return rng.standard_normal((n_sets, n_points, 3)) * np.exp2(rng.integers(-18, 3, size=(n_sets, n_points, 1)).astype(np.float64))


def planted_series():
    """name -> (series, parameters of power_spectra) at N = 8."""
    sub = np.array([5e-324, -5e-324, 1e-310, -0.0, 0.0, -1e-310, 2.5e-308, -0.0, 5e-324, 0.0, -0.0, 1e-320])
    big = np.array([1e200, -1e200, 3e199, 0.0, -2e200, 1e200, 5e199, -1e199])
    huge = np.array([1.7e308, 1.7e308, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    return {
        "constant": (np.full(20, 0.375), dict(n=8, hop=4, window="hann")),
        "alternating": (np.array([1.0, -1.0] * 6), dict(n=8, hop=4, window="rect")),
        "subnormals": (sub, dict(n=8, hop=2, window="hann")),
        "minus zero": (np.full(8, -0.0), dict(n=8, hop=8, window="rect")),
        "1e200": (big, dict(n=8, hop=8, window="rect")),
        "1.7e308": (huge, dict(n=8, hop=8, window="rect")),
    }


# sar_spectra_segments / sar_runtime_spectra: changes to (n=8, hop=4, window=hann, samples=0, chunk=0, proj=(1, 0, 0); n_points=16)
SPECTRA_REFUSED = [
    (dict(n=0), "power of two"), (dict(n=4), "power of two"), (dict(n=12), "power of two"), (dict(n=8192), "power of two"),
    (dict(hop=0), "hop must be"), (dict(hop=9), "hop must be"),
    (dict(window=2), "window"),
    (dict(proj=(1.0, math.nan, 0.0)), "proj"), (dict(proj=(math.inf, 0.0, 0.0)), "proj"),
    (dict(chunk=2 ** 30 + 1), "chunk"),
    (dict(n_points=0), "points"), (dict(n_points=2 ** 20 + 1), "points"),
    (dict(samples=5), "samples must divide"), (dict(samples=32), "samples must divide"),
    (dict(samples=4), "at least n"), (dict(n_points=4), "at least n"),
]

# sar_runtime_spectrum: changes to (jobs=2, segments=3, n=8, hop=4, stride=1, transient=10, bound=1e6)
SPECTRUM_REFUSED = [
    (dict(jobs=0), "jobs must be"), (dict(jobs=2 ** 16 + 1, segments=1), "jobs must be"),
    (dict(segments=0), "segments"),
    (dict(n=24), "power of two"), (dict(n=2), "power of two"), (dict(n=8192, hop=8), "power of two"),
    (dict(hop=0), "hop must be"), (dict(hop=9), "hop must be"),
    (dict(window=7), "window"),
    (dict(stride=0), "at least 1"),
    (dict(jobs=2 ** 16, segments=1, n=32, hop=16), "2^20 points"), (dict(segments=2 ** 32 - 1, n=4096, hop=4096), "2^20 points"),
    (dict(transient=2 ** 31 + 1), "at most 2^31"), (dict(jobs=1, segments=256, n=4096, hop=4096, stride=2 ** 11 + 1), "at most 2^31"),
    (dict(bound=0.0), "bound"), (dict(bound=math.inf), "bound"), (dict(bound=math.nan), "bound"),
    (dict(proj=(0.0, 0.0, math.nan)), "proj"), (dict(proj=(-math.inf, 0.0, 0.0)), "proj"),
    (dict(chunk=2 ** 30 + 1), "chunk"),
]
