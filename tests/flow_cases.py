"""The cases of the flow tests (tests/test_gpu_flow.py) and the restatement's result for each, computed once and left unchanged.

A case is a named field in a view, a set of start points and a call's parameters. The views of Lorenz and Roessler are framed with
the library's own host arithmetic (frame_view_box) on the extent the RESTATEMENT finds, so no case needs a device to be stated. The
start points are the library's stream (start_points(0, 0, jobs)) unless a case brings its own."""
from __future__ import annotations

import numpy as np

import flow_restatement as R

SEED = 0
TRANSIENT = 200                    # enough to reach both attractors' neighbourhood from the start cube; keeps the restatement quick
DT = {"lorenz": 0.01, "rossler": 0.05}

# name -> system, (width, height), jobs, steps_per_job, stride, the two launch shapes (chunk_jobs, chunk_steps), base preset
PARITY = {
    "lorenz-64x48-j257-s300": ("lorenz", (64, 48), 257, 300, 1, ((64, 64), (100, 5)), "solar_sail"),
    "rossler-64x48-j65-s300-k3": ("rossler", (64, 48), 65, 300, 3, ((64, 5), (100, 64)), "solar_sail"),
    "lorenz-7x5-j64-s37-k7": ("lorenz", (7, 5), 64, 37, 7, ((64, 5), (100, 64)), "solar_sail"),
    "rossler-7x5-j63-s37-k3": ("rossler", (7, 5), 63, 37, 3, ((64, 64), (100, 5)), "solar_sail"),
    "lorenz-1x1-j1-s1": ("lorenz", (1, 1), 1, 1, 1, ((64, 64), (100, 5)), "solar_sail"),
    "rossler-1x1-j257-s300-k7": ("rossler", (1, 1), 257, 300, 7, ((64, 5), (100, 64)), "solar_sail"),
    "lorenz-64x48-j1-s300": ("lorenz", (64, 48), 1, 300, 1, ((64, 5), (100, 64)), "solar_sail"),
    "rossler-64x48-j65-s37-poisson": ("rossler", (64, 48), 65, 37, 1, ((64, 64), (100, 5)), "poisson_saturne"),
    "lorenz-7x5-j65-s1": ("lorenz", (7, 5), 65, 1, 1, ((64, 64), (100, 5)), "solar_sail"),
    "lorenz-64x48-j63-s300-k7-poisson": ("lorenz", (64, 48), 63, 300, 7, ((64, 5), (100, 64)), "poisson_saturne"),
}

_FRAMED, _EXTENTS, _RESULTS = {}, {}, {}


def rows_config(sar, rows, size, base="solar_sail", **kw):
    """The field `rows` (3, 10) in base's view and colours, at `size`."""
    cfg = sar.Config.from_coefficients(rows, base=getattr(sar.Config, base)())
    return cfg.replace(width=size[0], height=size[1], **kw)


def framed(sar, system, size, base="solar_sail", shrink=1.0, margin=0.05, dt=None, jobs=65, steps=300):
    """(config, view) of a named system framed on the extent the restatement finds for the run itself — start_points(SEED, 0, jobs),
    TRANSIENT uncounted and `steps` counted steps of dt (None: the system's own). With shrink < 1 the box is that share of the extent
    around its middle, so that the trajectory leaves the image and returns."""
    dt = DT[system] if dt is None else dt
    key = (system, size, base, shrink, margin, dt, jobs, steps)
    if key not in _FRAMED:
        cfg = rows_config(sar, sar.flow_coefficients(system), size, base)
        run = (system, dt, jobs, steps)
        if run not in _EXTENTS:
            _EXTENTS[run] = R.flow(R.view_of(cfg.c), sar.start_points(SEED, 0, jobs), steps, dt=dt, transient=TRANSIENT, plot=0)[1]["extent"]
        e = _EXTENTS[run].reshape(3, 2)
        mid, half = e.mean(axis=1), (e[:, 1] - e[:, 0]) * (0.5 * shrink)
        half = np.where(half > 0.0, half, 0.5)                              # (one counted point: a box around it)
        box = np.stack([mid - half, mid + half], axis=1).reshape(6)
        cfg = sar.frame_view_box(cfg, box, margin=margin)
        _FRAMED[key] = (cfg, R.view_of(cfg.c))
    return _FRAMED[key]


def restated(key, view, starts, steps, frame=None, **params):
    """R.flow, remembered under `key` (hashable: the case and what varies)."""
    if key not in _RESULTS:
        out, s = R.flow(view, starts, steps, frame=frame, **params)
        for a in (out["count"], out["zbuf"], out["steps"]):
            a.setflags(write=False)
        _RESULTS[key] = (out, s)
    return _RESULTS[key]


class Parity:
    def __init__(self, sar, name):
        self.name = name
        self.system, self.size, self.jobs, self.steps, self.stride, self.shapes, self.base = PARITY[name]
        self.cfg, self.view = framed(sar, self.system, self.size, self.base, jobs=self.jobs, steps=self.steps)
        self.starts = sar.start_points(SEED, 0, self.jobs)
        self.params = dict(dt=DT[self.system], transient=TRANSIENT, stride=self.stride)

    def want(self, chunk_steps):
        return restated((self.name, chunk_steps), self.view, self.starts, self.steps, chunk_steps=chunk_steps, **self.params)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def same_frame(got, want) -> list:
    """The names of the buffers of two frames that differ, bit for bit."""
    bad = [f for f in ("count", "zbuf", "steps") if not np.array_equal(bits(got[f]), bits(want[f]))]
    return bad + (["max"] if int(got["max"]) != int(want["max"]) else [])


def same_stats(got, want, atomics=True) -> list:
    skip = () if atomics else ("count_atomics", "key_atomics")
    bad = [f for f in R.COUNTERS if f not in skip and int(got[f]) != int(want[f])]
    # the extent by value: of -0.0 and +0.0 a minimum may report either
    return bad + (["extent"] if not np.array_equal(np.asarray(got["extent"]), np.asarray(want["extent"])) else [])
