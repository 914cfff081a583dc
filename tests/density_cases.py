"""The frames density estimation is tested on (tests/test_density_host.py, tests/test_gpu_density.py), each named for what it
catches, and their references: tests/density_restatement.py applied once and twice, computed once per case and shared.

Sizes: 1 x 1 (smaller than any halo), 5 x 3, 31 x 33 and 67 x 45 (no multiple of a tile), 96 x 80 (several tiles both ways, whatever
the tile option). S: the smallest, a small odd one, the default and the largest. A pattern that does not fit a size is not made."""
import functools
from collections import namedtuple

import numpy as np

import density_restatement as D

SIZES = ((1, 1), (5, 3), (31, 33), (67, 45), (96, 80))      # (width, height)
SAMPLES = (2, 5, 64, 256)
SEAMS = (15, 16, 31, 32, 63, 64)                            # both sides of the seams of 16-, 32- and 64-pixel tiles

Case = namedtuple("Case", "name width height S count steps zbuf max")
Reference = namedtuple("Reference", "count steps max stats count2 steps2 max2 stats2")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _seed(name, w, h, S):
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), w, h, S])


def _lone(w, h, x, y):
    c = np.zeros((h, w), dtype=np.uint32)
    c[y, x] = 1
    return c


def _patterns(w, h, S, rng):
    """name -> (count, steps or None, max or None); steps None: random hues under the covered pixels, max None: the true maximum."""
    out = {}
    out["lone_centre"] = (_lone(w, h, w // 2, h // 2), None, None)
    for name, x, y in (("top_left", 0, 0), ("top_right", w - 1, 0), ("bottom_left", 0, h - 1), ("bottom_right", w - 1, h - 1)):
        out[f"lone_corner_{name}"] = (_lone(w, h, x, y), None, None)
    out["lone_edge_top"] = (_lone(w, h, w // 2, 0), None, None)
    out["lone_edge_left"] = (_lone(w, h, 0, h // 2), None, None)
    for s in SEAMS:
        if s < w:
            out[f"lone_seam_x{s}"] = (_lone(w, h, s, h // 2), None, None)
        if s < h:
            out[f"lone_seam_y{s}"] = (_lone(w, h, w // 2, s), None, None)
    yy, xx = np.mgrid[0:h, 0:w]
    out["checkerboard_ones"] = (((xx + yy) & 1).astype(np.uint32), None, None)
    sparse = rng.integers(0, 2 * S + 1, size=(h, w)).astype(np.uint32) * (rng.random((h, w)) < 0.30)
    out["sparse_random"] = (sparse.astype(np.uint32), None, None)
    ident = rng.integers(S, 4 * S + 1000, size=(h, w)).astype(np.uint32) * (rng.random((h, w)) < 0.5)
    out["identity_all_bright"] = (ident.astype(np.uint32), None, None)
    out["empty"] = (np.zeros((h, w), dtype=np.uint32), None, None)
    if w >= 3:
        borders = np.zeros((h, w), dtype=np.uint32)
        borders[h // 2, w // 2 - 1:w // 2 + 2] = (S - 1, S, S + 1)
        out["class_borders"] = (borders, None, None)
    sat = np.ones((h, w), dtype=np.uint32)
    sat[h // 2, w // 2] = 0xFFFFFFFF
    out["saturating_pixel_in_ones"] = (sat, None, None)
    # hues that are not finite next to finite ones (den > 0), alone (den == 0), and -0.0
    cnt = rng.integers(1, 2 * S, size=(h, w)).astype(np.uint32) * (rng.random((h, w)) < 0.6)
    st = rng.random((h, w))
    odd = rng.integers(0, 8, size=(h, w))
    st[odd == 0] = np.nan
    st[odd == 1] = np.inf
    st[odd == 2] = -np.inf
    st[odd == 3] = -0.0
    out["steps_not_finite_mixed"] = (cnt.astype(np.uint32), st, None)
    for tag, v in (("nan", np.nan), ("neg_zero", -0.0), ("inf", np.inf)):
        out[f"steps_lone_{tag}"] = (_lone(w, h, w // 2, h // 2), np.full((h, w), v), None)
    allnan = np.where(cnt != 0, np.nan, 0.25)
    out["steps_all_nan"] = (cnt.astype(np.uint32), allnan, None)
    out["loaded_max_too_small"] = (sparse.astype(np.uint32) + (sparse != 0) * np.uint32(3), None, 1)
    return out


@functools.lru_cache(maxsize=None)
def _cases():
    cases = {}
    for (w, h) in SIZES:
        for S in SAMPLES:
            for name, (count, steps, mx) in _patterns(w, h, S, _seed("patterns", w, h, S)).items():
                rng = _seed(name, w, h, S)
                count = np.ascontiguousarray(count, dtype=np.uint32)
                if steps is None:
                    steps = np.where(count != 0, rng.random((h, w)), 0.0)
                zbuf = np.where(count != 0, rng.random((h, w)) * 2.0 - 0.5, -1.0).astype(np.float32)
                full = f"{name}-{w}x{h}-S{S}"
                cases[full] = Case(full, w, h, S, count, np.ascontiguousarray(steps, dtype=np.float64), zbuf,
                                   int(count.max()) if mx is None else mx)
    return cases


NAMES = tuple(_cases())


def case(name) -> Case:
    return _cases()[name]


@functools.lru_cache(maxsize=None)
def reference(name) -> Reference:
    """The restatement applied once and twice to the case; computed once, shared, read-only."""
    k = case(name)
    c1, s1, m1, st1 = D.filter(k.count, k.steps, k.S)
    c2, s2, m2, st2 = D.filter(c1, s1, k.S)
    for a in (c1, s1, c2, s2):
        a.setflags(write=False)
    return Reference(c1, s1, m1, st1, c2, s2, m2, st2)


def select(*fragments):
    """Case names that contain every fragment."""
    return tuple(n for n in NAMES if all(f in n for f in fragments))
