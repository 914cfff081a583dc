"""The cases of the section tests (tests/test_gpu_section.py) and the restatement's result for each, computed once and left unchanged.

A case is a field in a view, a surface, a set of start points and a call's parameters. The views are framed with the library's own
host arithmetic (frame_view_box) on boxes written here, so no case needs a device to be stated. The start points are the library's
stream spread over the attractor's neighbourhood (starts_of) unless a case brings its own: from the stream's own small cube around the
origin every job of Lorenz leaves along the same branch of the origin's unstable manifold, and a section of them is a handful of pixels."""
from __future__ import annotations

import numpy as np

import flow_cases as FK
import flow_restatement as R
import section_restatement as P

SEED = 0
BOX = {"lorenz": [-20.0, 20.0, -27.0, 27.0, 0.0, 50.0], "rossler": [-12.0, 13.0, -12.0, 9.0, 0.0, 25.0]}
DT = {"lorenz": 0.01, "rossler": 0.05}
Z27 = P.plane((0.0, 0.0, 1.0), 27.0)
QUADRIC = np.array([-40.0, 0.7, 0.11, -0.09, 0.05, -0.6, 0.13, 0.07, 1.3, -0.021])     # all ten coefficients non-zero


SPREAD = {"lorenz": ((100.0, 100.0, 100.0), (0.0, 0.0, 25.0)), "rossler": ((50.0, 50.0, 1.0), (0.0, 0.0, 0.0))}


def starts_of(sar, system, jobs):
    """start_points(SEED, 0, jobs), the cube of half-width 0.1, scaled and shifted: Lorenz |x|, |y| <= 10, 15 <= z <= 35."""
    scale, shift = SPREAD[system]
    return sar.start_points(SEED, 0, jobs) * np.array(scale) + np.array(shift)


def surface(sar, system, kind):
    if kind == "z27":
        return Z27
    if kind == "y0":
        return P.plane((0.0, 1.0, 0.0))
    if kind == "zmax":
        return sar.section_extremum(sar.flow_coefficients(system), 2)
    assert kind == "quadric"
    return QUADRIC


# name -> system, surface, (width, height), jobs, samples, max_steps, transient, direction, the two launch shapes (chunk_jobs, chunk_steps)
PARITY = {
    "lorenz-z27-64x48-j257-s3-up-t1000": ("lorenz", "z27", (64, 48), 257, 3, 600, 1000, 1, ((64, 5), (100, 64))),
    "lorenz-z27-7x5-j64-s40-down-t0": ("lorenz", "z27", (7, 5), 64, 40, 3000, 0, -1, ((64, 64), (100, 4096))),
    "lorenz-z27-1x1-j1-s1-both-t0": ("lorenz", "z27", (1, 1), 1, 1, 400, 0, 0, ((64, 5), (100, 64))),
    "lorenz-z27-64x48-j63-s3-both-t1000": ("lorenz", "z27", (64, 48), 63, 3, 600, 1000, 0, ((64, 4096), (100, 5))),
    "lorenz-z27-7x5-j65-s1-up-t0": ("lorenz", "z27", (7, 5), 65, 1, 400, 0, 1, ((64, 64), (100, 5))),
    "lorenz-z27-64x48-j65-s40-down-t1000-short": ("lorenz", "z27", (64, 48), 65, 40, 1500, 1000, -1, ((64, 5), (100, 2000))),
    "rossler-y0-64x48-j65-s3-up-t200": ("rossler", "y0", (64, 48), 65, 3, 800, 200, 1, ((64, 5), (100, 64))),
    "lorenz-zmax-64x48-j64-s3-down-t1000": ("lorenz", "zmax", (64, 48), 64, 3, 600, 1000, -1, ((64, 64), (100, 5))),
    "lorenz-quadric-7x5-j65-s40-both-t0": ("lorenz", "quadric", (7, 5), 65, 40, 1500, 0, 0, ((64, 5), (100, 1500))),
}

_RESULTS = {}


def framed(sar, system, size, shrink=1.0, **kw):
    """(config, view) of a named system framed on its box — with shrink < 1 on that share of it around its middle."""
    e = np.array(BOX[system]).reshape(3, 2)
    mid, half = e.mean(axis=1), (e[:, 1] - e[:, 0]) * (0.5 * shrink)
    cfg = sar.frame_view_box(FK.rows_config(sar, sar.flow_coefficients(system), size, **kw), np.stack([mid - half, mid + half], axis=1).reshape(6))
    return cfg, R.view_of(cfg.c)


def restated(key, view, surface_, starts, frame=None, **params):
    """P.section, remembered under `key` (hashable: the case and what varies)."""
    if key not in _RESULTS:
        out = P.section(view, surface_, starts, frame=frame, **params)
        for a in (out[0], out[1], out[2], out[4]["count"], out[4]["zbuf"], out[4]["steps"]):
            a.setflags(write=False)
        _RESULTS[key] = out
    return _RESULTS[key]


class Parity:
    def __init__(self, sar, name):
        self.name = name
        self.system, kind, self.size, self.jobs, samples, max_steps, transient, direction, self.shapes = PARITY[name]
        self.cfg, self.view = framed(sar, self.system, self.size)
        self.surface = surface(sar, self.system, kind)
        self.starts = starts_of(sar, self.system, self.jobs)
        self.params = dict(dt=DT[self.system], samples=samples, max_steps=max_steps, transient=transient, direction=direction)

    def want(self, plot=1):
        return restated((self.name, plot), self.view, self.surface, self.starts, plot=plot, **self.params)


def same_outputs(got, want) -> list:
    """The names of what differs between a FlowSection and the restatement's (points, ret, records, stats, frame): the points, the
    return times and the records bit for bit, the counters, and the statistics' doubles by value (of -0.0 and +0.0 a minimum may
    report either)."""
    points, ret, records, stats = want[:4]
    bad = [n for n, a, b in (("points", got.points, points), ("ret", got.ret, ret)) if not np.array_equal(FK.bits(a), FK.bits(b))]
    bad += ["records." + f for f in P.RECORD_DTYPE.names if not np.array_equal(got.records[f], records[f])]
    bad += ["stats." + f for f in P.COUNTERS if int(got.stats[f]) != int(stats[f])]
    bad += ["stats." + f for f in ("extent", "ret_min", "ret_max", "residual_max") if not np.array_equal(np.asarray(got.stats[f]), np.asarray(stats[f]))]
    return bad
