"""Volumes no run of jobs reaches in a test's time, for the three kernels that READ a volume and for add = 1 — the cases of
tests/test_volume_edge_cases_host.py and tests/test_gpu_volume_edges.py. On the device they go in through the hooks build's
sar_runtime_debug_volume_load (include/sar_test_hooks.h); here they are arrays, and what is expected of them is
tests/volume_restatement.py's march and section, computed once per (case, march, transparent) and left unchanged.

A case is a volume from a seeded numpy.random.default_rng, the marches it is marched under — (label, palette, parameters), each
with transparent 0 and 1 — and the windows it is sectioned over. `check_condition` asserts, on the restatement alone, that a case still
reaches what it is for. The palettes are this module's own rows (a Config takes them as palette_rgb), so nothing here needs a library.

    deep_half      1024 slabs of ones under half_count 1: T runs down to 2^-1024, a subnormal; k_volume_march's slab-colour loop takes
                   four trips and fills every row of its LDS table
    sparse_1024    1024 slabs, 2 % of the voxels non-empty with counts over all of u32, on one workgroup (65 x 3) and on four with a
                   ragged last one (300 x 3, `sparse_1024_wide`); a window that starts beyond slab 255 and stops some rays
    d257           257 slabs: one slab beyond a trip of 256
    alpha_one      half_count so small that a voxel's opacity rounds to exactly 1: T = 0, every later slab weighs 0
    alpha_nil      half_count so large that T stays exactly 1: covered pixels whose transparent image is (0, 0, 0, 0)
    stop_first     t_min just below 1: every ray stops at its first non-empty slab
    max_counts     voxels of 2^32 - 1 and 2^31; the default half count comes from vmax = 2^32 - 1; the section wraps
    wrap_to_zero   two slabs of 2^31: a section whose count is 0 although nearest is a slab
    empty          no hit at all
    positions      pos_lo / pos_hi that put slabs below 0, at 1 and above 1, that coincide, and that run backwards
    palettes       palettes of 1 and of SAR_PALETTE_MAX entries
    one_pixel      a 1 x 1 image 1024 slabs deep
    big_reduce     1 092 608 voxels, more than one trip of k_volume_reduce's 2048 x 256 lanes: the largest count in the very last
                   voxel, the second largest in the first voxel of the second trip"""
from __future__ import annotations

import sys

import numpy as np

import volume_restatement as R

SMALL, WIDE, ONE, REDUCE = (65, 3), (300, 3), (1, 1), (97, 11)     # (width, height)
Z_RANGE = (-1.0, 1.0)
PALETTE_MAX = 15                                                   # SAR_PALETTE_MAX
U32 = 1 << 32
_prng = np.random.default_rng(2810)
PALETTES = {"five": _prng.random((5, 3)).tolist(), "one": _prng.random((1, 3)).tolist(), "max": _prng.random((PALETTE_MAX, 3)).tolist()}
BACKGROUND = (65535, 1000, 30000)
COLOURED = dict(half_count=3.0, pos_lo=0.9, pos_hi=0.15, background=BACKGROUND)    # volume_cases.MARCHES["coloured"]
NAMES = ("deep_half", "sparse_1024", "sparse_1024_wide", "d257", "alpha_one", "alpha_nil", "stop_first", "max_counts", "wrap_to_zero", "empty",
         "positions", "palettes", "one_pixel", "big_reduce")
MAX_COLUMN = (1, 7)                                                # max_counts: the pixel (j, i) whose voxels hold 2^31
BIG_SECOND = 2048 * 256                                            # big_reduce: the first voxel of the reduction's second trip


def _sparse(rng, shape, share, low, high) -> np.ndarray:
    """`share` of the voxels non-empty, their counts uniform in [low, high)."""
    on = rng.random(shape) < share
    return np.where(on, rng.integers(low, high, size=shape, dtype=np.uint64), 0).astype(np.uint32)


def _alternate(size) -> np.ndarray:
    """8 slabs, the odd ones (7, the nearest, among them) hold 1 everywhere."""
    vol = np.zeros((8, size[1], size[0]), dtype=np.uint32)
    vol[1::2] = 1
    return vol


def _d257() -> np.ndarray:
    return _sparse(np.random.default_rng(2813), (257, SMALL[1], SMALL[0]), 0.05, 1, 50)


def _build(name):
    """(vol, [(label, palette, parameters)], [(k0, k1)])"""
    whole = [(0, None)]
    if name == "deep_half":
        return np.ones((1024, SMALL[1], SMALL[0]), dtype=np.uint32), [("half1", "five", dict(half_count=1.0))], whole
    if name in ("sparse_1024", "sparse_1024_wide"):
        size = WIDE if name.endswith("_wide") else SMALL
        vol = _sparse(np.random.default_rng(2811 if size is SMALL else 2812), (1024, size[1], size[0]), 0.02, 1, U32)
        marches = [("default", "five", dict()), ("window", "five", dict(k0=300, k1=900, half_count=3e9, t_min=0.25))]
        return vol, marches, whole + [(0, 1), (1023, 1024), (256, 257), (300, 900)]
    if name == "d257":
        return _d257(), [("coloured", "five", dict(COLOURED)), ("default", "five", dict())], whole + [(256, 257), (0, 256), (255, 257)]
    if name == "alpha_one":
        return _alternate(SMALL), [("denormal", "five", dict(half_count=5e-324)), ("tiny", "five", dict(half_count=1e-17))], whole
    if name == "alpha_nil":
        return _alternate(SMALL), [("huge", "five", dict(half_count=1e300, background=BACKGROUND)),
                                   ("large", "five", dict(half_count=1e17, background=BACKGROUND))], whole
    if name == "stop_first":
        return _alternate(SMALL), [("first", "five", dict(half_count=1.0, t_min=float(np.nextafter(1.0, 0.0))))], whole
    if name == "max_counts":
        vol = np.full((8, SMALL[1], SMALL[0]), U32 - 1, dtype=np.uint32)
        vol[:, MAX_COLUMN[0], MAX_COLUMN[1]] = 1 << 31
        vol[3] = 0
        return vol, [("default", "five", dict())], whole + [(0, 3), (4, 8)]
    if name == "wrap_to_zero":
        vol = _sparse(np.random.default_rng(2814), (4, SMALL[1], SMALL[0]), 0.7, 1, 50)
        vol[:, :, ::2] = 0
        vol[0, :, ::2] = vol[2, :, ::2] = 1 << 31                   # the even columns: half the pixels (and one more)
        return vol, [("default", "five", dict())], whole + [(0, 2), (0, 3), (2, 4)]
    if name == "empty":
        return np.zeros((8, SMALL[1], SMALL[0]), dtype=np.uint32), [("background", "five", dict(background=BACKGROUND))], whole
    if name == "positions":
        return _d257(), [("outside", "five", dict(pos_lo=-0.5, pos_hi=1.5)), ("equal", "five", dict(pos_lo=0.3, pos_hi=0.3)),
                         ("backwards", "five", dict(pos_lo=1.0, pos_hi=0.0)), ("at_one", "five", dict(pos_lo=1.0, pos_hi=1.0))], []
    if name == "palettes":
        return _d257(), [("one", "one", dict()), ("one_coloured", "one", dict(COLOURED)), ("max", "max", dict()),
                         ("max_coloured", "max", dict(COLOURED))], []
    if name == "one_pixel":
        vol = _sparse(np.random.default_rng(2815), (1024, 1, 1), 0.3, 1, U32)
        return vol, [("default", "five", dict()), ("window", "five", dict(k0=700, k1=1024))], whole + [(700, 1024), (0, 1)]
    if name == "big_reduce":
        vol = _sparse(np.random.default_rng(2816), (1024, REDUCE[1], REDUCE[0]), 0.01, 1, 1 << 31)
        vol.reshape(-1)[BIG_SECOND] = U32 - 2
        vol.reshape(-1)[-1] = U32 - 1
        return vol, [], []
    raise KeyError(name)


def stats_of(vol) -> dict:
    """sar_volume_stats of a loaded volume: the visits are the voxels' sum, no depth is known."""
    total = int(vol.sum(dtype=np.uint64))
    return dict(visits=total, stored=total, below=0, above=0, nan=0, nonempty=int(np.count_nonzero(vol)), vmax=int(vol.max(initial=0)),
                z_min=float("inf"), z_max=float("-inf"))


class Case:
    def __init__(self, name):
        self.name = name
        self.vol, self.marches, self.windows = _build(name)
        self.vol.setflags(write=False)
        self.slabs, self.height, self.width = self.vol.shape
        self.stats = stats_of(self.vol)
        self._marched, self._sections = {}, {}

    def params(self, label) -> tuple:
        """(palette's name, parameters) of the march `label`."""
        return next((pal, dict(p)) for l, pal, p in self.marches if l == label)

    def config(self, sar, label=None, transparent=1):
        """The library's Config of this size with the march's palette."""
        pal = self.params(label)[0] if label is not None else "five"
        return sar.Config.solar_sail(width=self.width, height=self.height, transparent=transparent, palette_rgb=PALETTES[pal])

    def march(self, label, transparent, reverse=False, vol=None):
        """The restatement's (image, statistics); of this case's own volume computed once."""
        pal, p = self.params(label)
        if vol is not None or reverse:
            v = self.vol if vol is None else vol
            return R.march(v, int(v.max(initial=0)), PALETTES[pal], transparent, reverse=reverse, **p)
        key = (label, transparent)
        if key not in self._marched:
            img, st = R.march(self.vol, self.stats["vmax"], PALETTES[pal], transparent, **p)
            img.setflags(write=False)
            self._marched[key] = (img, st)
        return self._marched[key]

    def section(self, k0=0, k1=None):
        if (k0, k1) not in self._sections:
            self._sections[(k0, k1)] = R.section(self.vol, k0, k1)
        return self._sections[(k0, k1)]


_CASES = {}


def case(name) -> Case:
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def positions(k: Case, label) -> np.ndarray:
    """The slabs' palette positions v_k under the march `label`, one fp64 operation at a time as include/sar.h gives them."""
    p = {**R.MARCH_DEFAULTS, **k.params(label)[1]}
    F = np.float64
    return F(p["pos_lo"]) + ((np.arange(k.slabs, dtype=F) + F(0.5)) / F(k.slabs)) * (F(p["pos_hi"]) - F(p["pos_lo"]))


def _differs(a, b) -> np.ndarray:
    return (a != b).any(axis=-1)


def check_condition(name) -> dict:
    """Asserts that the restatement's result of the case still reaches what the case is for; returns the figures."""
    k = case(name)
    npix = k.width * k.height
    f = dict(k.stats, npix=npix)
    what = f"{name}: {f}"
    assert k.vol.dtype == np.uint32 and k.slabs * npix <= 1 << 30
    if name == "deep_half":
        assert k.slabs == 1024 and (k.width, k.height) == SMALL, what
        T = 1.0
        for _ in range(1024):
            T = T * (1.0 - 1.0 / (1.0 + 1.0))
        assert 0.0 < T < sys.float_info.min and T == 2.0 ** -1024, T         # subnormal, not zero
        for transparent in (0, 1):
            img, st = k.march("half1", transparent)
            assert st == dict(slabs_seen=195 * 1024, covered=195, stopped=0), (what, st)
            assert _differs(img, k.march("half1", transparent, reverse=True)[0]).all(), what
    elif name in ("sparse_1024", "sparse_1024_wide"):
        assert k.slabs == 1024 and (k.width, k.height) == (WIDE if name.endswith("_wide") else SMALL), what
        assert int(k.vol.max()) >= 1 << 31 and k.vol[300:900].any() and k.vol[1023].any() and k.vol[0].any() and k.vol[256].any(), what
        for transparent in (0, 1):
            img, st = k.march("default", transparent)
            assert len(np.unique(img.reshape(-1, 4), axis=0)) >= 100, what
            assert _differs(img, k.march("default", transparent, reverse=True)[0]).all(), what
            stopped = k.march("window", transparent)[1]["stopped"]
            f[f"stopped_{transparent}"] = stopped
            assert 0 < stopped < npix, (what, stopped)
    elif name in ("d257", "positions", "palettes"):
        assert k.slabs == 257 and k.vol[256].any() and k.vol[0].any() and int(k.vol.max()) < 50, what
        if name == "positions":
            v = positions(k, "outside")
            assert (v < 0.0).any() and (v > 1.0).any() and ((v > 0.0) & (v < 1.0)).any(), what
            assert (positions(k, "at_one") == 1.0).all() and (positions(k, "equal") == 0.3).all(), what
            back = positions(k, "backwards")
            assert (np.diff(back) < 0.0).all() and (back > 0.0).all() and (back < 1.0).all(), what
        if name == "palettes":
            assert len(PALETTES["one"]) == 1 and len(PALETTES["max"]) == PALETTE_MAX, what
    elif name in ("alpha_one", "alpha_nil", "stop_first"):
        assert k.slabs == 8 and not k.vol[0::2].any() and (k.vol[1::2] == 1).all(), what
        if name == "alpha_one":
            nearest, second = np.zeros_like(k.vol), np.zeros_like(k.vol)
            nearest[7], second[5] = 1, 1
            for label in ("denormal", "tiny"):
                half = k.params(label)[1]["half_count"]
                assert 1.0 / (1.0 + half) == 1.0, what                       # alpha is exactly 1
                for transparent in (0, 1):
                    img, st = k.march(label, transparent)
                    assert st == dict(slabs_seen=4 * npix, covered=npix, stopped=0), (what, st)
                    assert np.array_equal(img, k.march(label, transparent, vol=nearest)[0]), what
                    assert _differs(img, k.march(label, transparent, vol=second)[0]).all(), what
        elif name == "alpha_nil":
            for label in ("huge", "large"):
                half = k.params(label)[1]["half_count"]
                assert 1.0 - 1.0 / (1.0 + half) == 1.0 and 1.0 / (1.0 + half) > 0.0, what     # T stays exactly 1, the weight is not 0
                img, st = k.march(label, 1)
                assert st == dict(slabs_seen=4 * npix, covered=npix, stopped=0) and not img.any(), (what, st)
                img, st = k.march(label, 0)
                assert st["covered"] == npix and (img == (*BACKGROUND, 65535)).all(), what
        else:
            for transparent in (0, 1):
                assert k.march("first", transparent)[1] == dict(slabs_seen=npix, covered=npix, stopped=npix), what
    elif name == "max_counts":
        assert k.stats["vmax"] == U32 - 1 and not k.vol[3].any(), what
        count, nearest = k.section()
        column = np.zeros((k.height, k.width), dtype=bool)
        column[MAX_COLUMN] = True
        assert (count[~column] == (7 * (U32 - 1)) % U32).all() and count[MAX_COLUMN] == (7 << 31) % U32 == 1 << 31, what
        assert (nearest == 7).all(), what
    elif name == "wrap_to_zero":
        for window in ((0, None), (0, 3)):
            count, nearest = k.section(*window)
            assert (count[:, ::2] == 0).all() and (nearest[:, ::2] == 2).all(), what
        count, nearest = k.section(0, 2)
        assert (count[:, ::2] == 1 << 31).all() and (nearest[:, ::2] == 0).all(), what
        assert np.count_nonzero(k.section()[0][:, 1::2]) >= 50, what          # the other pixels are ordinary ones
    elif name == "empty":
        assert k.stats["nonempty"] == k.stats["vmax"] == 0, what
        img, st = k.march("background", 0)
        assert st == dict(slabs_seen=0, covered=0, stopped=0) and (img == (*BACKGROUND, 65535)).all(), what
        img, st = k.march("background", 1)
        assert st["covered"] == 0 and not img.any(), what
        count, nearest = k.section()
        assert not count.any() and (nearest == -1).all(), what
    elif name == "one_pixel":
        assert k.vol.shape == (1024, 1, 1) and k.vol[700:].any() and k.vol[:700].any(), what
    elif name == "big_reduce":
        flat = k.vol.reshape(-1)
        assert flat.size == 1092608 > 2048 * 256 and flat[-1] == k.stats["vmax"] == U32 - 1 and flat[BIG_SECOND] == U32 - 2, what
        assert int(np.delete(flat, [BIG_SECOND, flat.size - 1]).max()) < 1 << 31, what
        assert np.count_nonzero(flat[:BIG_SECOND]) >= 1000 and np.count_nonzero(flat[BIG_SECOND:]) >= 1000, what
    return f
