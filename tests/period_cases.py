"""The fixtures the period tests share (tests/test_period_host.py, tests/test_gpu_period.py): map families with periods known
independently of the code — the logistic family's bifurcation points 3, 1 + sqrt 6, 3.544... and its period-3 window above
1 + sqrt 8, Hénon's cascade at b = 0.3, linear maps that are exact cycles —, and the planes whose pixel counts a prototype of the
definition gave. Coefficient order within a row: 1, x, x^2, xy, xz, y, y^2, yz, z, z^2."""
from __future__ import annotations

import numpy as np

BOUNDED, DIVERGED = 0, 1


def logistic(r: float) -> np.ndarray:
    """x' = r x - r x^2; y' = z' = 0."""
    c = np.zeros(30)
    c[1], c[2] = r, -r
    return c


def henon(a: float, b: float = 0.3) -> np.ndarray:
    """x' = 1 - a x^2 + y, y' = b x; z' = 0."""
    c = np.zeros(30)
    c[0], c[2], c[5], c[11] = 1.0, -a, 1.0, b
    return c


def linear(m) -> np.ndarray:
    """p' = M p for a 3 x 3 matrix M."""
    c = np.zeros(30)
    for row in range(3):
        for col, k in enumerate((1, 5, 8)):
            c[10 * row + k] = m[row][col]
    return c


# (r, status, period): DIVERGED entries leave the box in the transient
LOGISTIC = [(0.5, BOUNDED, 1), (1.5, BOUNDED, 1), (2.9, BOUNDED, 1), (3.2, BOUNDED, 2), (3.5, BOUNDED, 4), (3.55, BOUNDED, 8),
            (3.566, BOUNDED, 16), (3.74, BOUNDED, 5), (3.83, BOUNDED, 3), (3.835, BOUNDED, 3), (3.9, BOUNDED, 0), (4.0, BOUNDED, 0),
            (4.2, DIVERGED, 0)]
LOGISTIC_PARAMS = dict(start=(0.3, 0.0, 0.0), transient=1000, max_period=256, eps=1e-9)
LOGISTIC_DIVERGED_AT = 9   # r = 4.2: transient_done

HENON = [(0.2, 1), (0.5, 2), (1.0, 4), (1.04, 8), (1.24, 7), (1.4, 0)]
HENON_PARAMS = dict(start=(0.05, 0.05, 0.05), transient=2000, max_period=256, eps=1e-9)

# (name, matrix, period)
CYCLES = [("identity", [[1, 0, 0], [0, 1, 0], [0, 0, 1]], 1),
          ("negate", [[-1, 0, 0], [0, -1, 0], [0, 0, -1]], 2),
          ("rotate", [[0, 1, 0], [0, 0, 1], [1, 0, 0]], 3),                 # (x, y, z) -> (y, z, x)
          ("quarter_turn", [[0, -1, 0], [1, 0, 0], [0, 0, 1]], 4),          # (x, y, z) -> (-y, x, z)
          ("negated_rotate", [[0, -1, 0], [0, 0, -1], [-1, 0, 0]], 6)]      # (x, y, z) -> (-y, -z, -x)
CYCLE_PARAMS = dict(start=(0.1, 0.2, 0.3), transient=7, max_period=256, eps=0.0)   # (0.05^3 would make the 3-cycle a fixed point)

# the Hénon plane: a along the columns (coefficient 2 = -a), b along the rows (coefficient 11)
HENON_PLANE = dict(base=henon(0.0, 0.0), axes=(2, 11), x_range=(-1.45, 0.0), y_range=(0.0, 0.4))
# (width, height, parameters, diverged, bounded with period 0, {period: pixels}, distinct non-zero periods or None)
HENON_PLANES = [
    (48, 40, dict(transient=1000, max_period=128, eps=1e-9), 43, 370, {1: 632, 2: 666, 4: 143, 8: 29}, 17),
    (37, 21, dict(transient=300, max_period=64, eps=1e-9), 21, 204, {1: 235, 2: 252, 4: 50, 8: 8}, None),
]

# the orbit-diagram line of the logistic family
LOGISTIC_LINE = dict(r_range=(2.8, 3.56), width=64, start=(0.3, 0.0, 0.0), max_zero_columns=6)
