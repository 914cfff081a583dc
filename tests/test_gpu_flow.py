"""GPU: flow rendering (sar_runtime_render_flow, include/sar.h) against the numpy restatement bit for bit — count, zbuf, steps, max,
every statistic and the Gas and Depth colorize bytes on the cases of tests/flow_cases.py (Lorenz and Roessler at 64 x 48, 7 x 5 and
1 x 1; 1, 63, 64, 65 and 257 jobs; 1, 37 and 300 steps; strides 1, 3 and 7), each under two launch shapes that must differ in the
two atomics counters only; run merging at its two extremes; a trajectory that leaves the image and returns; depth ties; escapes;
accumulation on top of a flow and of a map's render, and a map's render on top of a flow; plot = 0; flow_view; the downstream calls;
the runtime afterwards."""
import numpy as np
import pytest

import color_range_restatement as CR
import density_restatement as D
import flow_cases as K
import flow_restatement as R
import shade_restatement as S
from test_gpu_exposure import restate as restate_exposure

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rts(sar, gpu):
    """Two runtimes: the one the flows run on and the one restated states are loaded into."""
    cfg = sar.Config.solar_sail(width=64, height=48)
    pair = (sar.Runtime(cfg, device=0), sar.Runtime(cfg, device=0))
    yield pair
    for r in pair:
        r.close()


def _sized(rt, cfg):
    rt.set_width_height(cfg.c.width, cfg.c.height)
    rt.reset()
    return rt


def _frame(rt) -> dict:
    return dict(count=rt.count(), zbuf=rt.zbuf(), steps=rt.steps(), max=rt.max())


def _load(rt, frame):
    rt.load(np.ascontiguousarray(frame["count"]), np.ascontiguousarray(frame["steps"]), np.ascontiguousarray(frame["zbuf"]), int(frame["max"]))


def _flow(sar, cfg, rt, starts, steps, **params):
    return sar.render_flow(cfg, rt, jobs=len(starts), steps=steps, starts=starts, stats=True, **params)


def _assert_same(got_frame, got_stats, want_frame, want_stats, what, atomics=True):
    assert not K.same_frame(got_frame, want_frame), (what, K.same_frame(got_frame, want_frame))
    bad = K.same_stats(got_stats, want_stats, atomics)
    assert not bad, (what, bad, {f: (got_stats[f], want_stats[f]) for f in bad})


def _images(sar, cfg, rt):
    return [sar.colorize(cfg.replace(render_kind=kind), rt) for kind in (sar.SAR_RENDER_GAS, sar.SAR_RENDER_DEPTH)]


# ---- 1. parity, case by case, under two launch shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(K.PARITY))
def test_case_equals_the_restatement(sar, rts, name):
    rt, rt2 = rts
    k = K.Parity(sar, name)
    frames = []
    for chunk_jobs, chunk_steps in k.shapes:
        want_frame, want = k.want(chunk_steps)
        _sized(rt, k.cfg)
        got = _flow(sar, k.cfg, rt, k.starts, k.steps, chunk_jobs=chunk_jobs, chunk_steps=chunk_steps, **k.params)
        frames.append(_frame(rt))
        _assert_same(frames[-1], got, want_frame, want, (name, chunk_jobs, chunk_steps))
    assert not K.same_frame(frames[0], frames[1])                          # any two launch shapes: one frame
    _load(_sized(rt2, k.cfg), k.want(k.shapes[-1][1])[0])
    for mine, loaded in zip(_images(sar, k.cfg, rt), _images(sar, k.cfg, rt2)):
        assert np.array_equal(mine, loaded)


# ---- 2. run merging at its two extremes --------------------------------------------------------------------------------------------
def test_a_tiny_step_keeps_whole_launches_in_one_pixel(sar, rts):
    rt, _ = rts
    cfg = sar.frame_view_box(K.rows_config(sar, sar.flow_coefficients("lorenz"), (7, 5)), [-20.0, 20.0] * 3)   # the start cube: mid-image
    view = R.view_of(cfg.c)
    starts, steps, chunk_steps = sar.start_points(K.SEED, 0, 64), 300, 64
    launches = -(-steps // chunk_steps)
    p = dict(dt=1e-5, transient=0)
    want_frame, want = K.restated("tiny-step", view, starts, steps, chunk_steps=chunk_steps, **p)
    assert want["visits"] == 64 * steps and np.count_nonzero(want_frame["count"]) == 1      # every job sits in one pixel throughout,
    assert want["count_atomics"] == 64 * launches                                           # so every launch of a job saw a visit
    got = _flow(sar, cfg, _sized(rt, cfg), starts, steps, chunk_steps=chunk_steps, **p)
    _assert_same(_frame(rt), got, want_frame, want, "tiny step")
    assert got["count_atomics"] == 64 * launches and got["visits"] == 64 * steps


def test_a_large_step_changes_pixel_nearly_every_time(sar, rts):
    rt, _ = rts
    cfg, view = K.framed(sar, "lorenz", (64, 48), dt=0.05, jobs=64)
    starts, steps = sar.start_points(K.SEED, 0, 64), 300
    p = dict(dt=0.05, transient=K.TRANSIENT)
    want_frame, want = K.restated("large-step", view, starts, steps, chunk_steps=64, **p)
    assert want["visits"] > 64 * 200 and want["count_atomics"] >= 0.9 * want["visits"]
    got = _flow(sar, cfg, _sized(rt, cfg), starts, steps, chunk_steps=64, **p)
    _assert_same(_frame(rt), got, want_frame, want, "large step")


# ---- 3. out of the image and back --------------------------------------------------------------------------------------------------
def test_a_trajectory_that_leaves_the_image_and_returns(sar, rts):
    rt, _ = rts
    cfg, view = K.framed(sar, "lorenz", (64, 48), shrink=0.3)
    starts, steps = sar.start_points(K.SEED, 0, 65), 300
    p = dict(dt=0.01, transient=K.TRANSIENT)
    want_frame, want = K.restated("half-view", view, starts, steps, chunk_steps=64, **p)
    assert want["outside"] > 1000 and want["visits"] > 1000 and want["visits"] + want["outside"] == want["steps"] == 65 * steps
    got = _flow(sar, cfg, _sized(rt, cfg), starts, steps, chunk_steps=64, **p)
    _assert_same(_frame(rt), got, want_frame, want, "half view")


# ---- 4. depth ties -----------------------------------------------------------------------------------------------------------------
def test_depth_ties_go_to_the_largest_hue_in_any_order(sar, rts):
    """x' = y, y' = -x, z' = 0 under the identity rotation: circles in a plane of one depth, every job at its own speed."""
    rt, _ = rts
    rows = np.zeros((3, 10))
    rows[0, 5], rows[1, 1] = 1.0, -1.0
    cfg = K.rows_config(sar, rows, (16, 16), rotation_axis=(0.0, 0.0, 1.0), rotation_angle=0.0, center_camera=(0.0, -0.5, 0.0), scale=0.4, angle=0.0)
    view = R.view_of(cfg.c)
    radii = np.linspace(0.05, 1.1, 40)
    starts = np.stack([radii, np.zeros(40), np.zeros(40)], axis=1)
    p = dict(dt=0.05, transient=0)
    want_frame, want = K.restated("ties", view, starts, 200, chunk_steps=64, **p)
    seen = want_frame["count"] > 0
    assert (want_frame["zbuf"][seen] == np.float32(0.5)).all() and want["visits"] == 40 * 200 and (want_frame["count"] >= 50).sum() >= 10
    # the largest (float)c of a pixel's visits: (|d| + 0.8) * -0.2 falls with the speed, so the slowest visitor's hue
    assert len(np.unique(want_frame["steps"][seen])) >= 10
    back, _ = R.flow(view, starts[::-1], 200, chunk_steps=64, **p)
    assert not K.same_frame(back, want_frame)
    for order in (starts, starts[::-1].copy()):
        got = _flow(sar, cfg, _sized(rt, cfg), order, 200, chunk_steps=64, **p)
        _assert_same(_frame(rt), got, want_frame, want, "ties", atomics=order is starts)


# ---- 5. escapes --------------------------------------------------------------------------------------------------------------------
def _escape_field(sar):
    """x' = x^2 - 1, y' = -z, z' = y: a start with x > 1 blows up after ln((x + 1) / (x - 1)) / 2, one with x < 1 settles on x = -1."""
    rows = np.zeros((3, 10))
    rows[0, 0], rows[0, 2], rows[1, 8], rows[2, 5] = -1.0, 1.0, -1.0, 1.0
    cfg = K.rows_config(sar, rows, (64, 48), center_camera=(0.0, 0.0, 0.0), scale=0.2)
    x0 = np.array([-0.5, 0.0, 0.5, 0.9, 1.0001, 1.01, 1.02, 1.1, 1.3, 2.0, 5.0, 0.99, 1.003, 30.0])
    starts = np.stack([x0, np.linspace(0.1, 1.0, len(x0)), np.zeros(len(x0))], axis=1)
    return cfg, R.view_of(cfg.c), np.tile(starts, (5, 1))                 # 70 jobs: more than one wave


@pytest.mark.parametrize("transient", (0, 1000))
def test_escaped_jobs_are_counted_once_and_plot_nothing_more(sar, rts, transient):
    rt, _ = rts
    cfg, view, starts = _escape_field(sar)
    p = dict(dt=0.01, transient=transient)
    want_frame, want = K.restated(("escape", transient), view, starts, 300, chunk_steps=64, **p)
    if transient == 0:      # seven of the nine starts above 1 escape, spread over the launches; two outlive the call
        assert want["escaped"] == 5 * 7 and want["alive"] == 5 * 7 and want["escaped_transient"] == 0
    else:
        assert want["escaped_transient"] == 5 * 9 and want["escaped"] == 0 and want["alive"] == 5 * 5
    assert 0 < want["steps"] < len(starts) * 300 and want["visits"] > 0
    for chunk_jobs, chunk_steps in ((64, 64), (100, 64), (64, 5)):
        w_frame, w = K.restated(("escape", transient, chunk_steps), view, starts, 300, chunk_steps=chunk_steps, **p)
        got = _flow(sar, cfg, _sized(rt, cfg), starts, 300, chunk_jobs=chunk_jobs, chunk_steps=chunk_steps, **p)
        _assert_same(_frame(rt), got, w_frame, w, ("escape", transient, chunk_jobs, chunk_steps))
        assert not K.same_frame(w_frame, want_frame)


def test_all_jobs_escaping_in_the_transient_leave_the_frame_untouched(sar, rts):
    rt, _ = rts
    rows = np.zeros((3, 10))
    rows[0, 0], rows[0, 2] = 1.0, 1.0                                       # x' = 1 + x^2: tan t, gone at step 158
    cfg = K.rows_config(sar, rows, (64, 48))
    starts = np.zeros((65, 3))
    _sized(rt, cfg)
    before = _frame(rt)
    got = _flow(sar, cfg, rt, starts, 100, dt=0.01, transient=1000, chunk_steps=64)
    assert (got["escaped_transient"], got["escaped"], got["alive"], got["visits"], got["outside"], got["steps"]) == (65, 0, 0, 0, 0, 0)
    assert got["count_atomics"] == got["key_atomics"] == 0 and np.array_equal(got["extent"], [np.inf, -np.inf] * 3)
    assert not K.same_frame(_frame(rt), before)
    got = _flow(sar, cfg, rt, starts, 300, dt=0.01, transient=0, chunk_steps=64)      # and in the counted steps: 157 each, then gone
    assert (got["escaped_transient"], got["escaped"], got["alive"], got["steps"]) == (0, 65, 0, 65 * 157)


# ---- 6. accumulation ---------------------------------------------------------------------------------------------------------------
def test_two_calls_equal_one_call_of_all_the_jobs(sar, rts):
    rt, _ = rts
    k = K.Parity(sar, "rossler-64x48-j65-s300-k3")
    want_frame, want = k.want(64)
    _sized(rt, k.cfg)
    a = _flow(sar, k.cfg, rt, k.starts[:30], k.steps, chunk_steps=64, **k.params)
    b = _flow(sar, k.cfg, rt, k.starts[30:], k.steps, chunk_steps=64, **k.params)
    assert not K.same_frame(_frame(rt), want_frame)
    for f in ("steps", "visits", "outside", "escaped", "escaped_transient", "alive", "count_atomics"):
        assert a[f] + b[f] == want[f], f
    assert b["max"] == want["max"]


def _map_config(sar, size, jobs, iters):
    return sar.Config.poisson_saturne(width=size[0], height=size[1], iterations=jobs * iters, jobs_total=jobs, scale=1.0)


def test_a_flow_on_top_of_a_maps_frame(sar, rts):
    rt, _ = rts
    cfg, view = K.framed(sar, "lorenz", (64, 48))
    jobs, iters = 64, 100
    mcfg, mstarts = _map_config(sar, (64, 48), jobs, iters), sar.start_points(3, 0, jobs)
    _sized(rt, cfg)
    sar.render_jobs(mcfg, rt, mstarts)
    before = _frame(rt)
    starts = sar.start_points(K.SEED, 0, 65)
    p = dict(dt=0.01, transient=K.TRANSIENT)
    want_frame, want = R.flow(view, starts, 300, frame=before, chunk_steps=64, **p)
    visited = want_frame["count"] != before["count"]
    kept = visited & (want_frame["zbuf"] == before["zbuf"])
    assert (kept & (before["zbuf"] != np.float32(-1.0))).sum() >= 10          # the map's depth stays in front
    assert (kept & (before["zbuf"] == np.float32(-1.0))).sum() >= 1           # a flow depth at or below -1 leaves the sentinel
    assert (visited & (before["zbuf"] == np.float32(-1.0)) & (want_frame["zbuf"] != np.float32(-1.0))).sum() >= 10
    assert (visited & (before["zbuf"] != np.float32(-1.0)) & (want_frame["zbuf"] > before["zbuf"])).sum() >= 10
    got = _flow(sar, cfg, rt, starts, 300, chunk_steps=64, **p)
    _assert_same(_frame(rt), got, want_frame, want, "on a map")


def test_a_maps_render_on_top_of_a_flow(sar, oracle, rts):
    """The depth-hint hand-over: the render that follows must not trust hints from before the flow raised zbuf."""
    rt, _ = rts
    cfg, _ = K.framed(sar, "lorenz", (64, 48))
    jobs, iters = 2048, 200                                                  # enough jobs for the binned path and its hints
    mcfg, mstarts = _map_config(sar, (64, 48), jobs, iters), sar.start_points(3, 0, jobs)
    _sized(rt, cfg)
    sar.render_jobs(mcfg, rt, mstarts)                                       # hints learned ...
    _flow(sar, cfg, rt, sar.start_points(K.SEED, 0, 65), 300, dt=0.01, transient=K.TRANSIENT)
    state = _frame(rt)                                                       # ... zbuf raised by the flow ...
    sar.render_jobs(mcfg, rt, mstarts)                                       # ... and the map again
    ort = oracle.Runtime(64, 48)
    ort.count[...], ort.zbuf[...], ort.steps[...] = state["count"], state["zbuf"], state["steps"]
    ort.set_max(state["max"])
    oracle.render_jobs(mcfg.c, ort, mstarts, iters)
    assert not K.same_frame(_frame(rt), dict(count=ort.count, zbuf=ort.zbuf, steps=ort.steps, max=ort.max))


# ---- 7. plot = 0, flow_view --------------------------------------------------------------------------------------------------------
def test_measure_only_leaves_the_frame(sar, rts):
    rt, _ = rts
    k = K.Parity(sar, "lorenz-64x48-j257-s300")
    _, want = k.want(64)
    _sized(rt, k.cfg)
    sar.render_jobs(_map_config(sar, (64, 48), 64, 100), rt, sar.start_points(3, 0, 64))
    before = _frame(rt)
    got = _flow(sar, k.cfg, rt, k.starts, k.steps, plot=0, chunk_steps=64, **k.params)
    assert not K.same_frame(_frame(rt), before)
    assert not K.same_stats(dict(got, max=want["max"]), want, atomics=False) and got["count_atomics"] == got["key_atomics"] == 0
    assert got["max"] == before["max"]
    assert np.array_equal(sar.flow_extent(k.cfg, rt, jobs=k.jobs, steps=k.steps, starts=k.starts, **k.params), want["extent"])


def test_flow_view_frames_lorenz(sar, rts):
    rt, _ = rts
    base = K.rows_config(sar, sar.flow_coefficients("lorenz"), (64, 48))
    starts, steps = sar.start_points(K.SEED, 0, 65), 300
    p = dict(dt=0.01, transient=K.TRANSIENT)
    _, s = R.flow(R.view_of(base.c), starts, steps, plot=0, **p)
    want_cfg = sar.frame_view_box(base, s["extent"], margin=0.05)
    _, framed = K.restated("flow-view", R.view_of(want_cfg.c), starts, steps, **p)
    assert framed["outside"] == 0 and framed["visits"] == 65 * steps         # the restatement alone satisfies it
    _sized(rt, base)
    cfg = sar.flow_view(base, rt, jobs=65, steps=steps, starts=starts, margin=0.05, **p)
    assert bytes(cfg.c) == bytes(want_cfg.c)
    got = _flow(sar, cfg, rt, starts, steps, **p)
    assert got["outside"] == 0 and got["visits"] == 65 * steps


# ---- 8. what follows a flow --------------------------------------------------------------------------------------------------------
def test_downstream_calls_match_their_restatements_on_a_flows_frame(sar, rts):
    rt, rt2 = rts
    k = K.Parity(sar, "lorenz-7x5-j64-s37-k7")
    cfg = k.cfg.replace(transparent=0)
    _sized(rt, cfg)
    _flow(sar, cfg, rt, k.starts, k.steps, **k.params)
    f = _frame(rt)
    assert np.count_nonzero(f["count"]) >= 5
    # auto exposure
    e = sar.exposure(cfg, rt)
    want = restate_exposure(f["count"], f["max"], cfg_offset=cfg.c.brightness_offset, cfg_factor=cfg.c.brightness_factor)
    assert (e.black_count, e.white_count, e.covered, e.max, int(e.applied)) == tuple(want[2:])
    assert np.float64(e.offset).view(np.uint64) == np.float64(want[0]).view(np.uint64) and np.float64(e.factor).view(np.uint64) == np.float64(want[1]).view(np.uint64)
    assert sar.auto_exposure(cfg, rt).c.brightness_factor == e.factor
    # auto colour range: the record, and the mode's colorize against a frame loaded with the restated positions
    w = CR.window(f["count"], f["steps"])
    c = sar.color_range(cfg, rt)
    assert (c.lo, c.hi, c.pos_lo, c.pos_hi, c.covered, int(c.applied)) == (w.lo, w.hi, w.pos_lo, w.pos_hi, w.covered, w.applied)
    rt.set_color_range()
    try:
        windowed = sar.colorize(cfg, rt)
    finally:
        rt.set_color_range(None)
    _load(_sized(rt2, cfg), dict(f, steps=CR.positions(f["steps"], w)))
    assert np.array_equal(windowed, sar.colorize(cfg, rt2))
    # shade
    palette = [[cfg.c.palette_rgb[i][ch] for ch in range(3)] for i in range(cfg.c.palette_len)]
    want_img, want_stats = S.shade(f["count"], f["steps"], f["zbuf"], cfg.c.width, cfg.c.scale, palette, cfg.c.transparent, S.params())
    img, stats = sar.shade(cfg, rt, stats=True)
    assert stats == want_stats and np.array_equal(img, want_img)
    # density estimation (in place: last)
    count2, steps2, max2, dstats = D.filter(f["count"], f["steps"], 64)
    assert rt.density_filter(samples=64) == dstats
    after = _frame(rt)
    assert not K.same_frame(after, dict(count=count2, steps=steps2, zbuf=f["zbuf"], max=max2))


def test_the_runtime_is_otherwise_unchanged(sar, oracle, rts):
    rt, _ = rts
    cfg, _ = K.framed(sar, "rossler", (64, 48))
    _sized(rt, cfg)
    _flow(sar, cfg, rt, sar.start_points(K.SEED, 0, 65), 300, dt=0.05, transient=K.TRANSIENT)
    rt.reset()
    jobs, iters = 2048, 200
    mcfg, mstarts = _map_config(sar, (64, 48), jobs, iters), sar.start_points(3, 0, jobs)
    sar.render_jobs(mcfg, rt, mstarts)
    ort = oracle.Runtime(64, 48)
    oracle.render_jobs(mcfg.c, ort, mstarts, iters)
    assert not K.same_frame(_frame(rt), dict(count=ort.count, zbuf=ort.zbuf, steps=ort.steps, max=ort.max))
    assert np.array_equal(sar.colorize(mcfg, rt), oracle.colorize(mcfg.c, ort))


def test_timing_books_the_three_kernels(sar, rts):
    rt, _ = rts
    k = K.Parity(sar, "lorenz-7x5-j64-s37-k7")
    _sized(rt, k.cfg)
    rt.enable_timing(True)
    try:
        _flow(sar, k.cfg, rt, k.starts, k.steps, chunk_steps=5, **k.params)
        t = rt.last_timing()
        assert t.iterate_launches == -(-k.steps // 5) and t.iterate_ms > 0 and t.warmup_ms > 0 and t.colorize_ms > 0
    finally:
        rt.enable_timing(False)
