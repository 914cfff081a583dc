"""What the correlation-dimension tests share (tests/test_corr_host.py, tests/test_gpu_corr.py): the lattices with their closed-form
counts, the Henon map, the point sets with planted edge cases, and every parameter set the calls must refuse, with a piece of the
message they leave."""
import math

import numpy as np


def line_lattice(n=300):
    """x_i = i 2^-10, y = z = 0: every r^2 = (d 2^-10)^2 is exact."""
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n) * 2.0 ** -10
    return p


def line_cumulative(n, D):
    """pairs of the line lattice at distance <= D 2^-10"""
    D = min(D, n - 1)
    return sum(n - d for d in range(1, D + 1))


def plane_lattice(m=16):
    i, j = np.meshgrid(np.arange(m), np.arange(m), indexing="ij")
    p = np.zeros((m * m, 3))
    p[:, 0], p[:, 1] = i.ravel() * 2.0 ** -6, j.ravel() * 2.0 ** -6
    return p


def plane_cumulative(m, q):
    """unordered pairs of the m x m lattice whose squared index distance a^2 + b^2 is < q (integer arithmetic only)"""
    total = 0
    for a in range(-(m - 1), m):
        for b in range(-(m - 1), m):
            if (a, b) != (0, 0) and a * a + b * b < q:
                total += (m - abs(a)) * (m - abs(b))
    return total // 2


def henon():
    """x' = 1 - 1.4 x^2 + y, y' = 0.3 x, z' = 0.5 z in the search's row order."""
    c = np.zeros((3, 10))
    c[0, 0], c[0, 2], c[0, 5] = 1.0, -1.4, 1.0
    c[1, 1] = 0.3
    c[2, 8] = 0.5
    return c.reshape(30)


def planted_sets(n, n_sets=3, seed=11):
    """Random points scaled over 20 binades with, where n allows, duplicates (r^2 = 0), a pair at r^2 = inf (finite coordinates whose
    difference squares past the largest double) and a pair a subnormal distance apart."""
    rng = np.random.default_rng(seed + n)
    p = rng.standard_normal((n_sets, n, 3)) * np.exp2(rng.integers(-18, 3, size=(n_sets, n, 1)).astype(np.float64))
    if n >= 2:
        p[0, n - 1] = p[0, 0]                                  # a duplicate across the whole set
    if n >= 6:
        p[1, 1], p[1, n - 2] = (1e200, 0.0, 0.0), (-1e200, 0.0, 0.0)     # r^2 = inf
        p[2, 2], p[2, 3] = (0.5, 0.25, 0.125), (0.5 + 2.0 ** -53, 0.25, 0.125)   # r^2 = 2^-106, below 2^e_min
        p[2, 4], p[2, 5] = (0.0, 0.0, 1e-170), (0.0, 0.0, 0.0)                 # r^2 = 1e-340, a subnormal
        p[1, 3] = p[1, 4]                                      # neighbours: inside a Theiler window
    return p


PAIRS_REFUSED = [
    (dict(n=0), "points"), (dict(n=2 ** 20 + 1), "points"),
    (dict(n=10, samples=3), "samples must divide"), (dict(n=10, samples=20), "samples must divide"),
    (dict(sub_bits=5), "sub_bits"), (dict(e_min=3, e_max=3), "exponents"), (dict(e_min=4, e_max=3), "exponents"),
    (dict(e_min=-1023), "exponents"), (dict(e_max=1024), "exponents"),
    (dict(sub_bits=4, e_min=-64, e_max=0), "bins"), (dict(sub_bits=0, e_min=-1022, e_max=1), "bins"),
]

CORRDIM_REFUSED = [
    (dict(jobs=0), "jobs must be"), (dict(jobs=2 ** 16 + 1, samples=1), "jobs must be"),
    (dict(samples=0), "at least 1"), (dict(stride=0), "at least 1"),
    (dict(jobs=2 ** 16, samples=17), "2^20 points"), (dict(jobs=1025, samples=1024), "2^20 points"),
    (dict(transient=2 ** 31 + 1), "at most 2^31"), (dict(jobs=1, samples=2 ** 20, stride=2 ** 11 + 1), "at most 2^31"),
    (dict(bound=0.0), "bound"), (dict(bound=math.inf), "bound"), (dict(bound=math.nan), "bound"),
    (dict(c_lo=0.5), "c_lo"), (dict(c_lo=math.nan), "c_lo"), (dict(r_hi_fraction=0.0), "r_hi_fraction"), (dict(r_hi_fraction=math.nan), "r_hi_fraction"),
    (dict(sub_bits=5), "sub_bits"), (dict(e_min=8, e_max=8), "exponents"), (dict(sub_bits=4, e_min=-64, e_max=0), "bins"),
]
