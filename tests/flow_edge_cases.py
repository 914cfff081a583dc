"""What the flow edge tests share (tests/test_flow_edge_cases_host.py, tests/test_gpu_flow_edges.py): flows built so that a call
itself reaches the depths, hues, counts and launch shapes the named systems never show — depths of +-inf, at and below the -1
sentinel, f32 subnormals, -0.0 and NaN; hues that are -0.0, f32 subnormals and +-inf; counts that wrap u32 on a full frame; a frame
that already holds +-inf and NaN depths; an image larger than one trip of the resolve's launch with a second chunk of one job; the
phase carried over the default 4096-step launch boundary.

The carrier is x' = y, y' = -x, z' = a z + b under the identity view (rotation_angle 0 and angle 0: sin 0 is exactly 0), so the
pixel comes from (x, y) alone — circles — and the depth is exactly -(z + cy), cy = center_camera[1]. JOBS jobs start at (r, 0, z0),
r = linspace(0.05, 1.1, JOBS), and take STEPS steps of DT with no transient: every plotted point of the edge cases falls inside the
16 x 16 image. Colours are solar-sail's AdjustedVelocity unless a case replaces offset and factor.

`check_condition` asserts, on the RESTATEMENT's result only, that a case still reaches the state it was built for; the figures
measured when the cases were made are in the tables' comments, and each is asserted as a looser bound (about half)."""
from __future__ import annotations

import numpy as np

import flow_cases as K
import flow_restatement as R

SIZE, SCALE, JOBS, STEPS, DT = (16, 16), 0.4, 40, 200, 0.05
SHAPES = ((64, 64), (100, 5))                      # (chunk_jobs, chunk_steps): every edge case runs under both
AT_HALF = (0.0, -0.5, 0.0)                         # center_camera that puts z = 0 at the depth 0.5
POS_NAN, NEG_NAN = 0x7FC00000, 0xFFC00000
# the depths a loaded frame cycles through pixel by pixel, as f32 bit patterns: +inf, -inf, the sentinel, the flow's own depth, the
# f32 just below it, a positive and a negative NaN
HELD_BITS = (0x7F800000, 0xFF800000, 0xBF800000, 0x3F000000, 0x3EFFFFFF, POS_NAN, NEG_NAN)
FULL = 0xFFFFFFF0

# name -> a, z0, bound, center_camera, (ct_offset, ct_factor) or None, the frame the call accumulates onto (None: a reset runtime's).
# Covered pixels: 180 in every case but nan_depth.
EDGE = {
    # z = -1e30 * 1.284^t: the depth passes f32::MAX on the way. +inf on 179 of 180 covered pixels, one finite (2.94e38); the hue
    # (|d| + 0.8) * -0.2 leaves f32 a few steps later: steps = -inf on 155
    "grow_to_plus_inf": dict(a=5.0, z0=-1e30, bound=1e300),
    # the mirror image: every depth <= -1e30, a key offered by every run (key_atomics 1888) and the sentinel kept on all 180
    "grow_to_minus_inf": dict(a=5.0, z0=1e30, bound=1e300),
    # z = 1e-30 * 0.779^t: the depth rises to -0.0 through the f32 subnormals. 84 subnormal depths, 96 exactly +0.0 (from -0.0)
    "shrink_negative_depth": dict(a=-5.0, z0=1e-30),
    # the depth falls to +0.0 from above: the largest of a pixel wins. 70 subnormal depths, none 0
    "shrink_positive_depth": dict(a=-5.0, z0=-1e-30),
    # a NaN camera x: fi is NaN, passes the bounds test and lands in column 0 with a NaN depth. 8000 visits on 16 pixels, no key
    # offered, zbuf -1 and steps 0 everywhere, max 1502
    "nan_depth": dict(camera=(float("nan"), 0.0, 0.0)),
    # one depth (0.5) everywhere, so the hue alone picks each pixel's winner. -0.0 on all 180
    "hue_minus_zero": dict(camera=AT_HALF, ct=(0.0, -0.0)),
    # (|d| + 0.8) * 1e-42: f32 subnormals, 23 distinct values on 180 pixels
    "hue_subnormal": dict(camera=AT_HALF, ct=(0.8, 1e-42)),
    "hue_plus_inf": dict(camera=AT_HALF, ct=(0.8, 1e39)),
    "hue_minus_inf": dict(camera=AT_HALF, ct=(0.8, -1e39)),
    # every count 16 below 2^32: 157 pixels wrap; max ends at 0xFFFFFFFC, the largest final count, not at u32::MAX
    "wrapping_counts": dict(camera=AT_HALF, frame="full"),
    # a loaded max (7) below the frame's largest count: max rises to the largest final count, 0xFFFFFFFC
    "wrapping_counts_low_max": dict(camera=AT_HALF, frame="full_low_max"),
    # depth 0.5 onto held +inf, -inf, -1, 0.5, the f32 below 0.5, +NaN, -NaN: 24 to 28 visited pixels over each. IEEE zf > zbuf
    # replaces -inf, -1 and the f32 below; +inf, 0.5 itself and both NaNs stay
    "held_depths": dict(camera=AT_HALF, frame="held"),
}
# name -> size, jobs ("circles": the carrier's; an int: default_rng(1).uniform(-1, 1, (n, 3))), steps, stride; chunk_jobs = chunk_steps = 0
SHAPE = {
    # 533 027 pixels, both sides odd; two chunks, the second of one job. 247 926 visits on 188 428 pixels, 359 of those in the last row,
    # whose pixels (from index 532 480) lie beyond the first trip of the resolve's 2048 x 256 lanes
    "big_image": dict(size=(1031, 517), jobs=(1 << 17) + 1, steps=3, stride=1),
    # 4096 % 7 == 1: the second launch starts with a phase that is not 0. 585 plotted steps a job
    "default_chunk_steps": dict(size=SIZE, jobs="circles", steps=4097, stride=7),
}
NAMES, SHAPE_NAMES = tuple(EDGE), tuple(SHAPE)
REVERSIBLE = ("grow_to_plus_inf", "hue_subnormal")


def rows(a=0.0, b=0.0) -> np.ndarray:
    out = np.zeros((3, 10))
    out[0, 5], out[1, 1], out[2, 8], out[2, 0] = 1.0, -1.0, a, b
    return out


def circles(z0=0.0, jobs=JOBS) -> np.ndarray:
    return np.stack([np.linspace(0.05, 1.1, jobs), np.zeros(jobs), np.full(jobs, z0)], axis=1)


def loaded_frame(kind, size=SIZE) -> dict:
    """The frame a case accumulates onto: what Runtime.load is given."""
    f = R.empty_frame(*size)
    if kind == "full":
        f["count"][...], f["max"] = FULL, FULL
    elif kind == "full_low_max":
        f["count"][...], f["max"] = FULL, 7
    else:
        assert kind == "held", kind
        npix = size[0] * size[1]
        f["zbuf"] = np.array(HELD_BITS, dtype=np.uint32)[np.arange(npix) % len(HELD_BITS)].view(np.float32).reshape(size[1], size[0])
        f["steps"][...] = 0.25
        f["count"][...], f["max"] = 3, 3
    return f


class Case:
    """One case: its config, view, start points, the call's parameters, the frame it starts from and its launch shapes."""

    def __init__(self, sar, name):
        self.name = name
        d = EDGE[name] if name in EDGE else SHAPE[name]
        self.size, self.steps, self.stride = d.get("size", SIZE), d.get("steps", STEPS), d.get("stride", 1)
        kw = dict(rotation_axis=(0.0, 0.0, 1.0), rotation_angle=0.0, angle=0.0, scale=SCALE,
                  center_camera=d.get("camera", (0.0, 0.0, 0.0) if name in EDGE else AT_HALF))
        if d.get("ct") is not None:
            kw.update(ct_offset=d["ct"][0], ct_factor=d["ct"][1])
        self.cfg = K.rows_config(sar, rows(d.get("a", 0.0)), self.size, **kw)
        self.view = R.view_of(self.cfg.c)
        jobs = d.get("jobs", "circles")
        self.starts = circles(d.get("z0", 0.0)) if jobs == "circles" else np.random.default_rng(1).uniform(-1.0, 1.0, (jobs, 3))
        self.params = dict(dt=DT, transient=0, bound=d.get("bound", 1e6), stride=self.stride)
        self.before = loaded_frame(d["frame"], self.size) if d.get("frame") else None
        self.shapes = SHAPES if name in EDGE else ((0, 0),)

    def want(self, chunk_steps, reverse=False):
        """(frame, stats) of the restatement, once per launch shape and job order; read-only."""
        starts = self.starts[::-1].copy() if reverse else self.starts
        return K.restated(("edge", self.name, chunk_steps, reverse), self.view, starts, self.steps, frame=self.before, chunk_steps=chunk_steps,
                          **self.params)


def figures(case: Case) -> dict:
    """The numbers the conditions are about, from the restatement's result under the case's first launch shape."""
    frame, s = case.want(case.shapes[0][1])
    before = case.before if case.before is not None else R.empty_frame(*case.size)
    added = (frame["count"].astype(np.int64) - before["count"].astype(np.int64)) % (1 << 32)
    covered = added > 0
    z, hue = frame["zbuf"][covered], frame["steps"][covered]
    tiny = np.finfo(np.float32).tiny
    return dict(covered=int(covered.sum()), covered_rows=covered.sum(axis=1), covered_columns=np.flatnonzero(covered.any(axis=0)),
                visits=int(s["visits"]), outside=int(s["outside"]), key_atomics=int(s["key_atomics"]), max=int(s["max"]),
                z_pos_inf=int(np.isposinf(z).sum()), z_sentinel=int((z == np.float32(-1.0)).sum()),
                z_subnormal=int(((z != 0) & (np.abs(z) < tiny)).sum()), z_pos_zero=int((K.bits(z) == 0).sum()),
                z_neg_zero=int((K.bits(z) == 0x80000000).sum()),
                hue_neg_zero=int((K.bits(hue) == 1 << 63).sum()), hue_pos_inf=int(np.isposinf(hue).sum()), hue_neg_inf=int(np.isneginf(hue).sum()),
                hue_subnormal=int(((hue != 0) & (np.abs(hue) < tiny)).sum()), hue_distinct=len(np.unique(hue)),
                wrapped=int((frame["count"] < before["count"]).sum()), largest_count=int(frame["count"].max()),
                untouched=bool(np.array_equal(K.bits(frame["zbuf"]), K.bits(before["zbuf"]))
                               and np.array_equal(K.bits(frame["steps"]), K.bits(before["steps"]))),
                held={b: int((covered & (K.bits(before["zbuf"]) == b)).sum()) for b in HELD_BITS},
                replaced={b: int((covered & (K.bits(before["zbuf"]) == b) & (K.bits(frame["zbuf"]) != b)).sum()) for b in HELD_BITS})


_CHECKED = {}


def check_condition(case: Case) -> dict:
    """Asserts that the restatement's result of the case still reaches what the case is for; returns the figures."""
    name = case.name
    if name in _CHECKED:
        return _CHECKED[name]
    f = figures(case)
    what = f"{name}: {f}"
    if name == "big_image":
        assert len(case.starts) == R.DEFAULT_CHUNK_JOBS + 1 and case.size[0] * case.size[1] > 2048 * 256, what
        assert f["visits"] >= 120000 and f["covered"] >= 90000 and f["covered_rows"][-1] >= 100, what
        assert (case.size[1] - 1) * case.size[0] >= 2048 * 256, what           # the whole last row: the resolve's second trip
    elif name == "default_chunk_steps":
        assert R.DEFAULT_CHUNK_STEPS < case.steps and R.DEFAULT_CHUNK_STEPS % case.stride != 0, what
        assert f["visits"] == JOBS * (case.steps // case.stride) and f["outside"] == 0, what
    else:
        assert f["visits"] == JOBS * STEPS and f["outside"] == 0, what
        assert f["covered"] == 16 if name == "nan_depth" else f["covered"] >= 90, what
    if name == "grow_to_plus_inf":
        assert f["z_pos_inf"] >= 90 and f["hue_neg_inf"] >= 75, what
    elif name == "grow_to_minus_inf":
        assert f["z_sentinel"] == f["covered"] and f["key_atomics"] >= 900 and f["untouched"], what
    elif name == "shrink_negative_depth":
        assert f["z_subnormal"] >= 40 and f["z_pos_zero"] >= 45 and f["z_neg_zero"] == 0, what
    elif name == "shrink_positive_depth":
        assert f["z_subnormal"] >= 35 and f["z_pos_zero"] == 0, what
    elif name == "nan_depth":
        assert list(f["covered_columns"]) == [0] and f["key_atomics"] == 0 and f["untouched"] and f["max"] >= 750, what
    elif name == "hue_minus_zero":
        assert f["hue_neg_zero"] == f["covered"], what
    elif name == "hue_subnormal":
        assert f["hue_subnormal"] == f["covered"] and f["hue_distinct"] >= 14, what
    elif name == "hue_plus_inf":
        assert f["hue_pos_inf"] == f["covered"], what
    elif name == "hue_minus_inf":
        assert f["hue_neg_inf"] == f["covered"], what
    elif name in ("wrapping_counts", "wrapping_counts_low_max"):
        assert f["wrapped"] >= 78 and case.before["max"] < f["max"] == f["largest_count"] < 0xFFFFFFFF, what
        assert (name == "wrapping_counts") == (case.before["max"] == int(case.before["count"].max())), what
    elif name == "held_depths":
        assert min(f["held"].values()) >= 10, what
        # the header's IEEE zf > zbuf[pix] with zf = 0.5: -inf, the sentinel and the f32 below 0.5 give way; +inf, 0.5 and the NaNs stay
        for b in HELD_BITS:
            assert f["replaced"][b] == (f["held"][b] if b in (0xFF800000, 0xBF800000, 0x3EFFFFFF) else 0), what
    _CHECKED[name] = f
    return f
