"""The cases of the volume tests (tests/test_volume_host.py, tests/test_gpu_volume.py) and the restatement's result for each, computed
once and left unchanged.

The presets are oracle_lib's, the start points oracle_lib.start_points(0, 0, jobs). A case with a LEARNED range takes it as
volume(z_range=None) does: from the depths of a one-slab run of the same jobs. `check_condition` asserts, on the restatement alone,
that a case still reaches what it was built for; the figures measured when the cases were made stand next to them."""
from __future__ import annotations

import numpy as np

import depth_cases
import oracle_lib
import volume_restatement as R

SEED = 0
DEPTH_SIZE = (96, 64)
DEPTH_RANGES = {"wide": (8, -8.0, 8.0), "tiny": (7, -1e-23, 1e-23)}
DEPTH_NAMES = ("alt_inf", "overflow_mid", "shrink_alt", "const_pos", "falling_sentinel")
HOT_C, HOT_JOBS, HOT_ITERS = 0.125, 4096, 64     # x' = 0.5 x + 0.125 on every axis: the fixed point 0.25, reached exactly

# name -> preset, (width, height), jobs, iterations, slabs; the range is learned
LEARNED = {
    "ps_small": ("poisson_saturne", (64, 48), 64, 256, 8),    # 8 slabs used, 406 pixels with >= 2 non-empty slabs, vmax 111
    "ss_small": ("solar_sail", (64, 48), 64, 256, 8),         # nan 4864, 324 such pixels
    "odd_ps": ("poisson_saturne", (33, 17), 64, 128, 5),      # a row that is no multiple of anything; all 5 slabs used
    "odd_ss": ("solar_sail", (33, 17), 64, 128, 5),
    "wide_ps": ("poisson_saturne", (200, 3), 64, 256, 33),    # a row of three waves and a tail, D no power of two; >= 28 slabs used
    "wide_ss": ("solar_sail", (200, 3), 64, 256, 33),
    "one_slab": ("poisson_saturne", (64, 48), 64, 256, 1),
    "one_pixel": ("solar_sail", (1, 1), 64, 256, 8),
}
MARCHED = ("ps_small", "ss_small", "odd_ps", "odd_ss", "wide_ps", "wide_ss")
NAMES = tuple(LEARNED) + ("clipped", "hot") + tuple(f"{c}_{r}" for c in DEPTH_NAMES for r in DEPTH_RANGES)

# the march parameter sets, by name; "window" is cut to the case's D
MARCHES = {
    "default": dict(),
    "stopping": dict(half_count=1.0, t_min=1.0 / 16.0),
    "window": dict(k0=2, k1=-1),
    "coloured": dict(half_count=3.0, pos_lo=0.9, pos_hi=0.15, background=(65535, 1000, 30000)),
}


class Case:
    def __init__(self, name):
        self.name = name
        if name in LEARNED or name == "clipped":
            preset, size, self.jobs, self.iterations, self.slabs = LEARNED["ps_small" if name == "clipped" else name]
            self.oracle_config = getattr(oracle_lib, preset)()
            self.starts = oracle_lib.start_points(SEED, 0, self.jobs)
            self.z_range = None
        elif name == "hot":
            size, self.jobs, self.iterations, self.slabs = (16, 16), HOT_JOBS, HOT_ITERS, 8
            c = oracle_lib.solar_sail()
            for k in range(10):
                c.coeff_x[k] = c.coeff_y[k] = c.coeff_z[k] = (HOT_C, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)[k]
            c.coeff_x[1], c.coeff_y[5], c.coeff_z[8] = 0.5, 0.5, 0.5
            c.center_camera[0] = c.center_camera[1] = c.center_camera[2] = 0.0
            c.rotation_axis[0], c.rotation_axis[1], c.rotation_axis[2] = 0.0, 0.0, 1.0
            c.rotation_angle, c.scale = 0.0, 1.0
            self.oracle_config = c
            self.starts = oracle_lib.start_points(SEED, 0, self.jobs)
            self.z_range = (-1.0, 1.0)
        else:
            case, rng = name.rsplit("_", 1)
            size, self.jobs, self.iterations = DEPTH_SIZE, depth_cases.JOBS, depth_cases.CASES[case]["n"]
            self.slabs, *z = DEPTH_RANGES[rng]
            self.oracle_config = depth_cases.config(oracle_lib, case, size)
            self.starts = depth_cases.starts(case)
            self.z_range = tuple(z)
        self.width, self.height = size
        self.oracle_config.width, self.oracle_config.height = size
        self.oracle_config.iterations, self.oracle_config.jobs_total = self.jobs * self.iterations, self.jobs
        self.view = R.view_of(self.oracle_config)
        self.palette = R.palette_of(self.oracle_config)
        if self.z_range is None:
            _, probe = R.volume(self.view, self.starts, self.iterations, 1, -1.0, 1.0)
            self.probe = probe
            lo, hi = R.learned_range(probe["z_min"], probe["z_max"])
            if name == "clipped":   # the middle half of the learned range
                lo, hi = lo + (hi - lo) / 4.0, hi - (hi - lo) / 4.0
            self.z_range = (lo, hi)
        self.vol, self.stats = R.volume(self.view, self.starts, self.iterations, self.slabs, *self.z_range)
        self.vol.setflags(write=False)

    def config(self, sar, **kw):
        """The case as the library's Config."""
        c = self.oracle_config
        f = dict(center_camera=tuple(c.center_camera),
                 rotation_axis=tuple(c.rotation_axis), rotation_angle=c.rotation_angle, scale=c.scale, angle=c.angle,
                 color_transform=c.color_transform, ct_offset=c.ct_offset, ct_factor=c.ct_factor, width=self.width, height=self.height,
                 iterations=self.jobs * self.iterations, jobs_total=self.jobs, transparent=1)
        f.update(kw)
        return sar.Config.from_coefficients([list(c.coeff_x), list(c.coeff_y), list(c.coeff_z)]).replace(**f)

    def march_params(self, which) -> dict:
        p = dict(MARCHES[which])
        if p.get("k1") == -1:
            p["k1"] = self.slabs - 1
        return p

    def march(self, which, transparent, reverse=False):
        return R.march(self.vol, self.stats["vmax"], self.palette, transparent, reverse=reverse, **self.march_params(which))


_CASES = {}


def case(name) -> Case:
    if name not in _CASES:
        _CASES[name] = Case(name)
    return _CASES[name]


def slabs_used(k: Case) -> int:
    return int(np.count_nonzero(k.vol.reshape(k.slabs, -1).any(axis=1)))


def multi_slab_pixels(k: Case) -> int:
    return int(np.count_nonzero((k.vol != 0).sum(axis=0) >= 2))


def check_condition(name) -> dict:
    """Asserts that the restatement's result of the case still reaches what the case is for; returns the figures."""
    k = case(name)
    s = k.stats
    f = dict(s, slabs_used=slabs_used(k), multi=multi_slab_pixels(k))
    what = f"{name}: {f}"
    if name in ("ps_small", "ss_small"):
        assert f["slabs_used"] == 8 and f["multi"] >= 100, what
        for transparent in (0, 1):
            assert k.march("stopping", transparent)[1]["stopped"] > 0, what
            # the direction of the march matters: the opposite order gives another image
            assert np.count_nonzero((k.march("default", transparent)[0] != k.march("default", transparent, reverse=True)[0]).any(axis=-1)) >= 100, what
    elif name.startswith("odd_"):
        assert f["slabs_used"] == 5, what
    elif name.startswith("wide_"):
        assert f["slabs_used"] >= 28, what
    elif name == "clipped":
        assert s["below"] > 0 and s["above"] > 0 and s["stored"] > 0, what
    elif name == "hot":
        n = HOT_JOBS * HOT_ITERS
        assert s["stored"] == s["vmax"] == n == 262144 and s["nonempty"] == 1 and int(k.vol.max()) == n, what
    elif name == "alt_inf_wide":
        assert s["below"] == s["above"] == 240000, what
    elif name.startswith("overflow_mid_"):
        assert s["nan"] == 75025, what
    elif name == "shrink_alt_tiny":
        assert f["slabs_used"] == 5, what
    elif name.startswith("const_pos_"):
        assert f["slabs_used"] == (1 if name.endswith("_wide") else 0) and s["z_min"] == s["z_max"] == 0.25, what
    if name == "ss_small":
        assert s["nan"] > 0, what
    return f
