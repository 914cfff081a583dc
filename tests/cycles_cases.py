"""The maps and the cases of the cycles tests (tests/test_cycles_host.py, tests/test_gpu_cycles.py): small maps whose cycles are known,
written into the 30 coefficients (rows x, y, z over 1, x, x^2, xy, xz, y, y^2, yz, z, z^2), and the table of calls the GPU test holds
against the restatement field by field."""
import numpy as np

import cycles_restatement as R
import search_restatement as S


def _map(**entries) -> np.ndarray:
    """30 coefficients, zero but for entries like x1=..., y5=..., z8=... (row letter, term index)."""
    c = np.zeros(30)
    for name, v in entries.items():
        c["xyz".index(name[0]) * 10 + int(name[1:])] = v
    return c


def henon(a=1.4, b=0.3):
    """x' = 1 - a x^2 + b y, y' = x, z' = 0"""
    return _map(x0=1.0, x2=-a, x5=b, y1=1.0)


def logistic(r):
    """x' = r x - r x^2 in the x row, the other rows zero: the Jacobian is singular everywhere, M - I is not"""
    return _map(x1=r, x2=-r)


IDENTITY = _map(x1=1.0, y5=1.0, z8=1.0)
NO_ROOT = _map(x0=1.0, x1=1.0, x2=1.0)        # x' = x^2 + x + 1: x' - x = x^2 + 1 has no real root
DOUBLE_ROOT = _map(x1=1.0, x2=1.0)            # x' = x + x^2: the double root 0
AFFINE = _map(x0=1.0, x1=0.5, y0=-1.0, y5=0.25, z0=0.5, z8=-0.5)   # a contraction: Newton is exact in one step


def rotation(z_scale):
    """a quarter turn in (x, y): x' = -y, y' = x; z' = z_scale z"""
    return _map(x5=-1.0, y1=1.0, z8=z_scale)


HENON_MINUS_ZERO = np.where(henon() == 0.0, -0.0, henon())
SEARCH_MAPS = S.candidates(7, 100, 4)         # four maps of the search stream, as sar_search_candidate(7, 100 .. 103) gives them
LATTICE = R.starts()                          # the default 8^3 lattice over [-2, 2]^3
AXIS_STARTS = np.array([[0.0, 0.0, 0.5], [0.0, 0.0, -1.25], [0.5, 0.0, 0.0], [0.0, -0.75, 0.25], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
WILD_STARTS = np.array([[np.inf, 0.0, 0.0], [0.0, -np.inf, 0.0], [0.5, 0.5, np.inf], [-np.inf, np.inf, -np.inf], [2e6, 0.0, 0.0],
                        [0.0, -3e6, 1e7], [1e200, 1e200, 1e200], [0.6, 0.6, 0.0], [-1.1, -1.1, 0.0], [1e-300, -1e-300, 0.0]])

# the published numbers of cycles of the Henon map a = 1.4, b = 0.3 by minimal period, and what the 8^3 lattice gives at p = 1
HENON_CYCLES = {1: 2, 2: 1, 3: 0, 4: 1, 5: 0, 6: 2, 7: 4}
HENON_P1_COUNTS = dict(converged=448, escaped=64)

# name -> (coeffs, keyword arguments of the call: period, starts, grid, box, and the parameters). One call each.
CASES = {}
for _p in range(1, 8):
    CASES[f"henon_p{_p}"] = (henon(), dict(period=_p))
for _p in range(1, 5):
    CASES[f"logistic_3.9_p{_p}"] = (logistic(3.9), dict(period=_p))
CASES.update({
    "identity_cap16": (IDENTITY, dict(period=1, grid=4, cap=16)),
    "rotation_half_p1": (rotation(0.5), dict(period=1)),
    "rotation_half_p2": (rotation(0.5), dict(period=2)),
    "rotation_half_p4": (rotation(0.5), dict(period=4)),
    "rotation_p4": (rotation(1.0), dict(period=4, starts=np.concatenate([LATTICE[:58], AXIS_STARTS]))),
    "no_root": (NO_ROOT, dict(period=1)),
    "double_root": (DOUBLE_ROOT, dict(period=1)),
    "affine": (AFFINE, dict(period=1)),
    "affine_p3": (AFFINE, dict(period=3)),
    "search_p1": (SEARCH_MAPS, dict(period=1)),
    "search_p2": (SEARCH_MAPS, dict(period=2)),
    "search_p3": (SEARCH_MAPS, dict(period=3)),
    "minus_zero": (HENON_MINUS_ZERO, dict(period=2)),
    "wild_starts": (henon(), dict(period=1, starts=WILD_STARTS)),
    "wild_starts_p2_small_bound": (henon(), dict(period=2, starts=np.concatenate([WILD_STARTS, LATTICE[:20]]), bound=1.5)),
    "jobs_1": (henon(), dict(period=2, starts=LATTICE[219:220])),
    "jobs_63": (henon(), dict(period=2, starts=LATTICE[:63])),
    "jobs_64": (henon(), dict(period=2, starts=LATTICE[:64])),
    "jobs_65": (henon(), dict(period=2, starts=LATTICE[:65])),
    "jobs_4096": (henon(), dict(period=2, grid=16)),
    "max_newton_0": (henon(), dict(period=1, max_newton=0)),
    "max_newton_0_identity": (IDENTITY, dict(period=2, max_newton=0, grid=3)),
    "max_newton_1": (henon(), dict(period=1, max_newton=1)),
    "merge_0": (henon(), dict(period=4, merge=0.0)),
    "merge_wide": (henon(), dict(period=4, merge=10.0)),
    "cap_1": (henon(), dict(period=4, cap=1)),
    "box_grid": (henon(), dict(period=1, grid=5, box=((-1.5, -1.0, -0.5), (1.0, 1.5, 0.25)))),
    "tol_above_same": (henon(), dict(period=2, tol=1e-6, same=1e-12)),
    "several_maps": (np.stack([henon(), logistic(3.9), rotation(0.5), DOUBLE_ROOT, AFFINE, IDENTITY, henon(1.2, 0.3)]), dict(period=2)),
})


def reference(name):
    """The restatement of a case: (list of record dicts, (n_maps, cap) orbit slots)."""
    coeffs, kw = CASES[name]
    kw = dict(kw)
    box = kw.pop("box", None)
    if box is not None:
        kw.update(box_lo=box[0], box_hi=box[1])
    return R.cycles(coeffs, kw.pop("starts", None), **kw)
