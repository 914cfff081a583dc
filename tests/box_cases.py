"""What the box-counting tests share (tests/test_box_host.py, tests/test_gpu_box.py): the cubes, the point sets with planted edge
cases, the lattices with their closed-form rows, and every parameter set the calls must refuse, with a piece of the message they
leave."""
import math

import numpy as np

# (origin, size): the first scales by a power of two (a point on origin + size has u = 2^L exactly), the second does not (the
# multiply rounds)
CUBE_EXACT = ((-0.5, 0.125, -1.0), 2.0)
CUBE_ROUNDED = ((-0.75, -0.3, 0.2), 1.5)


def planted_sets(n, cube=CUBE_EXACT, seed=23):
    """(3, n, 3). Set 0: random points over 20 binades around the cube's centre, inside and outside it, with — where n allows —
    duplicates, a point exactly on origin + size (the clamp), one just below the origin, infinite coordinates of both signs and a
    -0.0. Set 1: all points equal (wave combining; sum_sq = n^2). Set 2: alternates between two points."""
    origin, size = np.asarray(cube[0]), cube[1]
    rng = np.random.default_rng(seed + n)
    p = np.zeros((3, n, 3))
    p[0] = origin + 0.5 * size + size * rng.standard_normal((n, 3)) * np.exp2(rng.integers(-18, 3, size=(n, 1)).astype(np.float64))
    if n >= 2:
        p[0, n - 1] = p[0, 0]                                  # a duplicate across the whole set
    if n >= 63:
        p[0, 1] = origin + size                                # on the far corner: the last cell on every axis
        p[0, 2] = np.nextafter(origin, -np.inf)                # just below the origin: cell 0
        p[0, 3] = (math.inf, -math.inf, origin[2] + 0.25 * size)
        p[0, 4] = (-math.inf, origin[1] + 0.5 * size, math.inf)
        p[0, 5] = (-0.0, 0.0, -0.0)
        p[0, 6] = p[0, 7] = p[0, 40]                           # a triple inside one wave
        p[0, n - 2] = p[0, 5]                                  # -0.0 and +0.0 share a cell
        p[0, n - 2, 0] = 0.0
    p[1] = origin + size * np.array([0.3, 0.6, 0.9])
    p[2, 0::2] = origin + size * np.array([0.1, 0.2, 0.7])
    p[2, 1::2] = origin + size * np.array([0.8, 0.2, 0.7000001])
    return p


def cube_lattice():
    """The 8 x 8 x 8 lattice (i, j, k) / 8 in the unit cube: 512 points, one per cell at level 3."""
    i, j, k = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    return np.stack([i.ravel(), j.ravel(), k.ravel()], axis=1) / 8.0


def cube_lattice_row(l):
    """(cells, singles, sum_sq, n_log_n) of the lattice at level l, in integers."""
    if l <= 3:
        per = 512 // 8 ** l
        return 8 ** l, (8 ** l if per == 1 else 0), 8 ** l * per * per, 512 * (9 - 3 * l) << 32
    return 512, 512, 512, 0


def line_lattice(n=300):
    """x_i = i 2^-10, y = z = 0."""
    p = np.zeros((n, 3))
    p[:, 0] = np.arange(n) * 2.0 ** -10
    return p


def distinct_cells(n, seed=5):
    """n points in n distinct cells of the unit cube at level 16 (cell centres)."""
    rng = np.random.default_rng(seed)
    c = np.unique(rng.integers(0, 1 << 16, size=(2 * n, 3)), axis=0)
    assert len(c) >= n
    return (rng.permutation(c)[:n] + 0.5) / 65536.0


def uniform_rows(L=16, n=2 ** 20):
    """The synthetic rows of n points spread evenly over a lattice filling the cube: 8^l cells of n / 8^l points while that is a
    whole number — every slope is exactly 3."""
    rows = []
    for l in range(L + 1):
        cells = 8 ** l
        if n % cells:
            break
        per = n // cells
        rows.append((cells, cells if per == 1 else 0, cells * per * per, n * (per.bit_length() - 1) << 32))
    return rows


BOXES_REFUSED = [
    (dict(n=0), "points"), (dict(n=2 ** 20 + 1), "points"),
    (dict(levels=0), "levels"), (dict(levels=17), "levels"),
    (dict(size=0.0), "size"), (dict(size=-1.0), "size"), (dict(size=math.inf), "size"), (dict(size=math.nan), "size"),
    (dict(size=5e-324), "scale"), (dict(origin=(0.0, math.nan, 0.0)), "origin"), (dict(origin=(math.inf, 0.0, 0.0)), "origin"),
]

BOXDIM_REFUSED = [
    (dict(jobs=0), "jobs must be"), (dict(jobs=2 ** 16 + 1, samples=1), "jobs must be"),
    (dict(samples=0), "at least 1"), (dict(stride=0), "at least 1"),
    (dict(jobs=2 ** 16, samples=17), "2^20 points"), (dict(jobs=1025, samples=1024), "2^20 points"),
    (dict(transient=2 ** 31 + 1), "at most 2^31"), (dict(jobs=1, samples=2 ** 20, stride=2 ** 11 + 1), "at most 2^31"),
    (dict(bound=0.0), "bound"), (dict(bound=math.inf), "bound"), (dict(bound=math.nan), "bound"),
    (dict(levels=0), "levels"), (dict(levels=17), "levels"),
    (dict(min_occupancy=0.0), "min_occupancy"), (dict(min_occupancy=-1.0), "min_occupancy"), (dict(min_occupancy=math.nan), "min_occupancy"),
]
