"""The loaded states shaded rendering is tested on (tests/test_shade_host.py, tests/test_gpu_shade.py), each named for what it
catches, and their references: tests/shade_restatement.py applied once per case, shared and read-only.

Sizes: 1 x 1 (smaller than any halo), 5 x 3, 33 x 17 (one pixel past both seams of the 32 x 16 tile), 70 x 40 and 96 x 80 (several
tiles both ways). R: none, the smallest, a middle one and the largest, each with the smoothing on and off. A pattern that does not fit
a size is not made. The depths of most patterns differ by a few pixels of height (a few / k), so that smooth_range and ao_range both
decide something."""
import functools
from collections import namedtuple

import numpy as np

import shade_restatement as S

SIZES = ((1, 1), (5, 3), (33, 17), (70, 40), (96, 80))      # (width, height)
COMBOS = tuple((R, sm) for R in (0, 1, 3, 8) for sm in (0, 1))
SCALE = 1.7                                                 # solar-sail's
PALETTE = ((0.9, 0.1, 0.05), (0.2, 0.8, 0.3), (0.05, 0.2, 0.95), (1.0, 1.0, 0.6))

Case = namedtuple("Case", "name width height count steps zbuf max cfg params window")
Reference = namedtuple("Reference", "rgba stats")


def _seed(name, w, h):
    return np.random.default_rng([sum(ord(ch) * (i + 1) for i, ch in enumerate(name)), w, h])


def _field(w, h, rng, k, cover=0.7, spread=6.0):
    """Random depths within `spread` pixels of height of each other under `cover` of the pixels, -1 elsewhere."""
    z = (0.5 + rng.random((h, w)) * spread / k).astype(np.float32)
    on = rng.random((h, w)) < cover
    return np.where(on, z, np.float32(-1.0)).astype(np.float32), on


def _lone(w, h, x, y):
    z = np.full((h, w), -1.0, dtype=np.float32)
    z[y, x] = 0.25
    return z


def _patterns(w, h):
    """name -> dict(zbuf, and optionally count, steps, scale, transparent, params, window)."""
    k = w * SCALE
    out = {}
    rng = _seed("patterns", w, h)
    yy, xx = np.mgrid[0:h, 0:w]
    flat = np.full((h, w), 0.5, dtype=np.float32)

    out["empty"] = dict(zbuf=np.full((h, w), -1.0, dtype=np.float32))
    for name, x, y in (("corner_tl", 0, 0), ("corner_tr", w - 1, 0), ("corner_bl", 0, h - 1), ("corner_br", w - 1, h - 1),
                       ("edge_top", w // 2, 0), ("edge_bottom", w // 2, h - 1), ("edge_left", 0, h // 2), ("edge_right", w - 1, h // 2)):
        out[f"lone_{name}"] = dict(zbuf=_lone(w, h, x, y))
    for s in (31, 32, 63, 64):
        if s < w:
            out[f"lone_seam_x{s}"] = dict(zbuf=_lone(w, h, s, h // 2))
    for s in (15, 16, 31, 32, 63, 64):
        if s < h:
            out[f"lone_seam_y{s}"] = dict(zbuf=_lone(w, h, w // 2, s))
    # z = a x + b y + c, dyadic: every depth, difference and 3 x 3 mean is exact
    out["plane_dyadic"] = dict(zbuf=(xx * 2.0 ** -7 - yy * 2.0 ** -8 + 0.25).astype(np.float32), scale=64.0 / w)
    step = np.where(xx < w // 2, xx * 2.0 ** -7 + 0.25, xx * 2.0 ** -7 + 8.25 - yy * 2.0 ** -6).astype(np.float32)
    out["two_planes_far_apart"] = dict(zbuf=step, scale=64.0 / w)
    if w >= 3 and h >= 3:
        pit, peak = flat.copy(), flat.copy()
        pit[h // 2, w // 2] -= np.float32(3.0 / k)
        peak[h // 2, w // 2] += np.float32(3.0 / k)
        out["pit_in_flat"] = dict(zbuf=pit)
        out["peak_in_flat"] = dict(zbuf=peak)
    out["flat"] = dict(zbuf=flat)
    z, _ = _field(w, h, rng, k, cover=1.0)
    out["checkerboard"] = dict(zbuf=np.where((xx + yy) & 1, z, np.float32(-1.0)).astype(np.float32))
    out["random"] = dict(zbuf=_field(w, h, rng, k)[0])
    out["random_dense_rough"] = dict(zbuf=_field(w, h, rng, k, cover=0.97, spread=40.0)[0])
    out["random_wide"] = dict(zbuf=np.where(rng.random((h, w)) < 0.8, rng.random((h, w)) * 2.0 - 0.5, -1.0).astype(np.float32))
    # depths that are not numbers, or odd ones, beside real ones
    z, _ = _field(w, h, rng, k, cover=0.9)
    odd = rng.integers(0, 12, size=(h, w))
    for tag, v in ((0, np.inf), (1, -np.inf), (2, np.nan), (3, -0.0), (4, 1e-42), (5, -1.0)):
        z[odd == tag] = np.float32(v)
    out["depths_not_numbers"] = dict(zbuf=z)
    near0 = np.where(odd < 6, np.float32(-0.0), np.float32(2e-42))
    out["depths_zero_and_subnormal"] = dict(zbuf=near0.astype(np.float32), scale=1e6 / w)
    z, _ = _field(w, h, rng, k, cover=1.0)
    out["count_zero_under_depth"] = dict(zbuf=z, count=(rng.random((h, w)) < 0.6).astype(np.uint32) * 7)
    out["min_count_both_sides"] = dict(zbuf=z, count=rng.integers(0, 7, size=(h, w)).astype(np.uint32), params=dict(min_count=3))
    out["min_count_zero"] = dict(zbuf=z, count=(rng.random((h, w)) < 0.5).astype(np.uint32), params=dict(min_count=0))
    st = rng.random((h, w)) * 1.5 - 0.25                      # below 0, inside, at and above 1
    kind = rng.integers(0, 10, size=(h, w))
    for tag, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, 1.0), (4, -0.0), (5, 0.999999)):
        st[kind == tag] = v
    out["steps_not_in_range"] = dict(zbuf=z, steps=st)
    for name, win in (("window_not_applied", dict(lo=0.2, hi=0.7, pos_lo=0.1, pos_hi=0.9, applied=0)),
                      ("window_applied", dict(lo=0.2, hi=0.7, pos_lo=0.1, pos_hi=0.9, applied=1)),
                      ("window_reversed", dict(lo=0.2, hi=0.7, pos_lo=1.0, pos_hi=0.0, applied=1)),
                      ("window_flat_position", dict(lo=-0.5, hi=0.25, pos_lo=0.5, pos_hi=0.5, applied=1))):
        out[name] = dict(zbuf=z, steps=st, window=win)
    z, _ = _field(w, h, rng, k)
    out["transparent_on_coloured_ground"] = dict(zbuf=z, transparent=1, params=dict(background=(1000, 20000, 65535)))
    out["opaque_on_coloured_ground"] = dict(zbuf=z, transparent=0, params=dict(background=(1000, 20000, 65535)))
    for name, light in (("light_grazing", (1.0, 0.0, 2.0 ** -20)), ("light_ahead", (0.0, 0.0, 1.0)), ("light_behind", (0.3, -0.2, -0.5)),
                        ("light_straight_behind", (0.0, 0.0, -1.0)), ("light_tiny", (0.0, 1e-200, 0.0))):
        out[name] = dict(zbuf=z, params=dict(light=light))
    out["light_ahead_on_flat"] = dict(zbuf=flat, params=dict(light=(0.0, 0.0, 1.0)))
    out["shininess_0"] = dict(zbuf=z, params=dict(shininess_log2=0, specular=0.6))
    out["shininess_10"] = dict(zbuf=z, params=dict(shininess_log2=10, specular=0.6))
    out["ao_range_0"] = dict(zbuf=z, params=dict(ao_range=0.0))
    out["ao_strong"] = dict(zbuf=z, params=dict(ao_strength=40.0, ao_range=3.0, smooth_range=0.0))
    out["weights_zero"] = dict(zbuf=z, params=dict(ambient=0.0, diffuse=0.0, specular=0.0))
    out["k_about_1e6"] = dict(zbuf=_field(w, h, rng, 1e6)[0], scale=1e6 / w)
    out["k_about_1e-3"] = dict(zbuf=np.where(rng.random((h, w)) < 0.8, rng.random((h, w)) * 4000.0, -1.0).astype(np.float32), scale=1e-3 / w)
    return out


# which (R, smooth) a pattern runs with at a size: the random field takes all eight everywhere, every other pattern the largest radius
# with smoothing and one more that rotates with its position in the list
def _combos(name, i):
    if name == "random":
        return COMBOS
    return ((8, 1), COMBOS[i % 7])


@functools.lru_cache(maxsize=None)
def _cases():
    cases = {}
    for (w, h) in SIZES:
        for i, (name, d) in enumerate(_patterns(w, h).items()):
            rng = _seed(name, w, h)
            zbuf = np.ascontiguousarray(d["zbuf"], dtype=np.float32)
            count = d.get("count")
            if count is None:
                count = np.where(zbuf != np.float32(-1.0), rng.integers(1, 50, size=(h, w)), 0)
            count = np.ascontiguousarray(count, dtype=np.uint32)
            steps = d.get("steps")
            if steps is None:
                steps = rng.random((h, w))
            steps = np.ascontiguousarray(steps, dtype=np.float64)
            cfg = dict(width=w, height=h, scale=float(d.get("scale", SCALE)), transparent=int(d.get("transparent", i & 1)),
                       palette_rgb=PALETTE)
            for R, sm in _combos(name, i):
                params = dict(d.get("params", {}), ao_radius=R, smooth=sm)
                full = f"{name}-{w}x{h}-R{R}-s{sm}"
                cases[full] = Case(full, w, h, count, steps, zbuf, int(count.max()), cfg, params, d.get("window"))
    return cases


NAMES = tuple(_cases())


def case(name) -> Case:
    return _cases()[name]


def shade(k: Case, count=None, steps=None, zbuf=None, detail=False):
    """The restatement on a case (or on other buffers under the case's config and parameters)."""
    return S.shade(k.count if count is None else count, k.steps if steps is None else steps, k.zbuf if zbuf is None else zbuf,
                   k.cfg["width"], k.cfg["scale"], PALETTE, k.cfg["transparent"], S.params(**k.params), k.window, detail=detail)


@functools.lru_cache(maxsize=None)
def reference(name) -> Reference:
    """The restatement applied to the case; computed once, shared, read-only."""
    rgba, stats = shade(case(name))
    rgba.setflags(write=False)
    return Reference(rgba, stats)


def select(*fragments):
    """Case names that contain every fragment."""
    return tuple(n for n in NAMES if all(f in n for f in fragments))
