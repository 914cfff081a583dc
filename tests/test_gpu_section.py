"""GPU: Poincare sections of flows (sar_runtime_section, include/sar.h) against the numpy restatement bit for bit — the crossings,
the return times, the records, every statistic, the frame and the Gas and Depth colorize bytes on the cases of
tests/section_cases.py (64 x 48, 7 x 5 and 1 x 1; 1, 63, 64, 65 and 257 jobs; 1, 3 and 40 samples; up to 3000 steps; a plane, a
half-plane, an extremum surface and a quadric), each under two launch shapes that must agree in every output; the edges (one sample,
a crossing in step 0, a start on the surface, a surface never left, a grazing plane, max_steps running out, escapes); the picture on
a reset runtime, on a map's frame, on a flow's, partly outside the image, face-on, and with plot = 0; the hand-over to the pair
histogram and to frame_view_box; the timing and the runtime afterwards."""
import math

import numpy as np
import pytest

import corr_restatement as X
import flow_cases as FK
import flow_restatement as R
import manifold_restatement as M
import section_cases as K
import section_restatement as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rts(sar, gpu):
    """Two runtimes: the one the sections run on and the one restated frames are loaded into."""
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


def _section(sar, cfg, rt, surface, starts, **params):
    return sar.flow_section(cfg, rt, surface, jobs=len(starts), starts=starts, **params)


def _assert_same(got, rt, want, what):
    bad = K.same_outputs(got, want)
    assert not bad, (what, bad, {f[6:]: (got.stats[f[6:]], want[3][f[6:]]) for f in bad if f.startswith("stats.")})
    assert not FK.same_frame(_frame(rt), want[4]), (what, FK.same_frame(_frame(rt), want[4]))


def _images(sar, cfg, rt):
    return [sar.colorize(cfg.replace(render_kind=kind), rt) for kind in (sar.SAR_RENDER_GAS, sar.SAR_RENDER_DEPTH)]


# ---- 1. parity, case by case, under two launch shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(K.PARITY))
def test_case_equals_the_restatement(sar, rts, name):
    rt, rt2 = rts
    k = K.Parity(sar, name)
    want = k.want()
    assert want[3]["crossings"] >= 1 and want[3]["clocked"] >= 1
    for chunk_jobs, chunk_steps in k.shapes:
        _sized(rt, k.cfg)
        got = _section(sar, k.cfg, rt, k.surface, k.starts, plot=True, chunk_jobs=chunk_jobs, chunk_steps=chunk_steps, **k.params)
        _assert_same(got, rt, want, (name, chunk_jobs, chunk_steps))
        assert np.array_equal(got.full, want[2]["status"] == P.FULL)
    _load(_sized(rt2, k.cfg), want[4])
    for mine, loaded in zip(_images(sar, k.cfg, rt), _images(sar, k.cfg, rt2)):
        assert np.array_equal(mine, loaded)


def test_the_cases_cover_what_they_name(sar):
    """(The restatement alone.)"""
    w = K.Parity(sar, "lorenz-z27-7x5-j65-s1-up-t0").want()
    full = w[2]["status"] == P.FULL
    assert full.sum() >= 60 and (w[2]["found"][full] == 1).all() and (w[2]["steps"][full] < 400).all()     # one sample: the job stops there
    w = K.Parity(sar, "lorenz-z27-64x48-j65-s40-down-t1000-short").want()
    short = w[2]["status"] == P.SHORT
    assert short.sum() >= 60 and (w[2]["found"][short] > 0).all() and (w[2]["steps"][short] == 1500).all()  # max_steps ran out mid-way
    w = K.Parity(sar, "lorenz-z27-7x5-j64-s40-down-t0").want()
    assert (w[2]["status"] == P.FULL).sum() >= 32 and w[3]["rough"] == 0
    w = K.Parity(sar, "lorenz-quadric-7x5-j65-s40-both-t0").want()
    assert w[3]["crossings"] >= 200 and w[3]["residual_max"] > 0.0


# ---- 2. edges ----------------------------------------------------------------------------------------------------------------------
def test_a_crossing_in_step_0_and_starts_on_the_surface(sar, rts):
    rt, _ = rts
    cfg, view = K.framed(sar, "lorenz", (64, 48))
    # z' = x y - 8/3 z: +28 at (10, 10, .), -71 at (1, 1, .). Just below the plane and rising; exactly on it, rising and falling
    starts = np.array([[10.0, 10.0, 26.99], [10.0, 10.0, 27.0], [1.0, 1.0, 27.0], [1.0, 1.0, 27.01]])
    for direction, clocks in ((1, (0, None, None, None)), (-1, (None, None, 0, 0)), (0, (0, None, 0, 0))):
        p = dict(dt=0.01, transient=0, samples=3, max_steps=600, direction=direction)
        want = K.restated(("step0", direction), view, K.Z27, starts, plot=1, **p)
        for j, c in enumerate(clocks):
            assert (want[2]["clock_step"][j] == 0) == (c == 0), (direction, j, want[2]["clock_step"])
        got = _section(sar, cfg, _sized(rt, cfg), K.Z27, starts, plot=True, chunk_steps=5, **p)
        _assert_same(got, rt, want, ("step 0", direction))


def test_a_surface_never_left_finds_nothing(sar, rts):
    rt, _ = rts
    cfg, view = K.framed(sar, "lorenz", (64, 48))
    starts = np.zeros((65, 3))                                               # Lorenz's origin, on the plane z = 0: g is 0 throughout
    p = dict(dt=0.01, transient=10, samples=3, max_steps=200, direction=0)
    surface = P.plane((0.0, 0.0, 1.0))
    want = K.restated("origin", view, surface, starts, plot=1, **p)
    assert (want[2]["status"] == P.SHORT).all() and (want[2]["clock_step"] == P.NONE).all() and np.isnan(want[0]).all()
    _sized(rt, cfg)
    before = _frame(rt)
    got = _section(sar, cfg, rt, surface, starts, plot=True, chunk_steps=64, **p)
    _assert_same(got, rt, want, "origin")
    assert np.isnan(got.points).all() and np.isnan(got.ret).all() and not got.full.any() and got.stats["short_jobs"] == 65
    assert not FK.same_frame(_frame(rt), before) and got.trajectories().shape == (0, 3, 3)


def test_a_grazing_plane_gives_rough_crossings(sar, rts):
    rt, _ = rts
    rows = np.zeros((3, 10))
    rows[0, 5], rows[1, 1] = 1.0, -1.0                                       # x' = y, y' = -x
    cfg = sar.frame_view_box(FK.rows_config(sar, rows, (64, 48)), [-1.5, 1.5, -1.5, 1.5, -1.0, 1.0])
    view = R.view_of(cfg.c)
    radii = np.array([1.0, 1.0 + 1e-6, 1.0 - 5e-6, 1.00001, 2.0])            # the first is the host test's; the last cuts the plane squarely
    starts = np.stack([radii, np.zeros(5), np.zeros(5)], axis=1)
    surface = P.plane((0.0, 1.0, 0.0), math.cos(0.005))
    p = dict(dt=0.01, transient=0, samples=40, max_steps=3000, direction=0)
    want = K.restated("grazing", view, surface, starts, plot=1, **p)
    assert want[2]["rough"][0] >= 1 and want[2]["found"][0] - want[2]["rough"][0] >= 1 and want[2]["rough"][4] == 0 and want[2]["found"][4] >= 2
    for chunk_steps in (7, 4096):
        got = _section(sar, cfg, _sized(rt, cfg), surface, starts, plot=True, chunk_steps=chunk_steps, **p)
        _assert_same(got, rt, want, ("grazing", chunk_steps))


@pytest.mark.parametrize("transient", (0, 1000))
def test_escaped_jobs_keep_what_they_found(sar, rts, transient):
    """x' = x^2 - 1, y' = -z, z' = y (flows' escape field): y and z turn with period 2 pi whatever x does, so g = y is crossed until a
    job with x > 1 blows up."""
    rt, _ = rts
    rows = np.zeros((3, 10))
    rows[0, 0], rows[0, 2], rows[1, 8], rows[2, 5] = -1.0, 1.0, -1.0, 1.0
    cfg = FK.rows_config(sar, rows, (64, 48), center_camera=(0.0, 0.0, 0.0), scale=0.2)
    view = R.view_of(cfg.c)
    x0 = np.array([-0.5, 0.0, 0.5, 0.9, 1.0001, 1.01, 1.02, 1.1, 1.3, 2.0, 5.0, 0.99, 1.003, 1.0 + 1e-6])
    starts = np.tile(np.stack([x0, np.linspace(0.1, 1.0, len(x0)), np.zeros(len(x0))], axis=1), (5, 1))     # 70 jobs: more than one wave
    p = dict(dt=0.01, transient=transient, samples=40, max_steps=1500, direction=0)
    want = K.restated(("escape", transient), view, P.plane((0.0, 1.0, 0.0)), starts, plot=1, **p)
    rec, s = want[2], want[3]
    if transient == 0:
        esc = rec["status"] == P.ESCAPED
        assert esc.sum() >= 10 and (rec["found"][esc] > 0).sum() >= 5 and s["escaped_transient"] == 0 and s["short_jobs"] >= 10
        assert (rec["steps"][esc] < 1500).all()
    else:
        assert s["escaped_transient"] >= 10 and (rec["steps"][rec["status"] == P.ESCAPED_TRANSIENT] == 0).all()
    assert s["escaped"] + s["escaped_transient"] + s["short_jobs"] + s["full"] == 70
    for chunk_jobs, chunk_steps in ((64, 64), (100, 5)):
        got = _section(sar, cfg, _sized(rt, cfg), P.plane((0.0, 1.0, 0.0)), starts, plot=True, chunk_jobs=chunk_jobs, chunk_steps=chunk_steps, **p)
        _assert_same(got, rt, want, ("escape", transient, chunk_jobs, chunk_steps))


# ---- 3. the picture ----------------------------------------------------------------------------------------------------------------
def _map_config(sar, size, jobs, iters):
    return sar.Config.poisson_saturne(width=size[0], height=size[1], iterations=jobs * iters, jobs_total=jobs, scale=1.0)


def test_a_section_on_top_of_a_maps_frame_and_of_a_flow(sar, rts):
    rt, rt2 = rts
    k = K.Parity(sar, "lorenz-z27-64x48-j63-s3-both-t1000")
    mcfg, mstarts = _map_config(sar, (64, 48), 64, 100), sar.start_points(3, 0, 64)
    _sized(rt, k.cfg)
    sar.render_jobs(mcfg, rt, mstarts)
    before = _frame(rt)
    want = P.section(k.view, k.surface, k.starts, frame=before, plot=1, **k.params)
    assert (want[4]["count"] != before["count"]).sum() >= 10 and want[4]["max"] >= before["max"]
    got = _section(sar, k.cfg, rt, k.surface, k.starts, plot=True, chunk_steps=64, **k.params)
    _assert_same(got, rt, want, "on a map")
    _sized(rt, k.cfg)
    sar.render_flow(k.cfg, rt, jobs=65, steps=300, starts=sar.start_points(K.SEED, 0, 65), dt=0.01, transient=200)
    before = _frame(rt)
    want = P.section(k.view, k.surface, k.starts, frame=before, plot=1, **k.params)
    kept = (want[4]["count"] != before["count"]) & (want[4]["zbuf"] == before["zbuf"])
    assert kept.sum() >= 1 and (want[4]["zbuf"] != before["zbuf"]).sum() >= 1                   # some crossings behind the flow, some in front
    got = _section(sar, k.cfg, rt, k.surface, k.starts, plot=True, chunk_steps=64, **k.params)
    _assert_same(got, rt, want, "on a flow")
    _load(_sized(rt2, k.cfg), want[4])
    for mine, loaded in zip(_images(sar, k.cfg, rt), _images(sar, k.cfg, rt2)):
        assert np.array_equal(mine, loaded)


def test_crossings_outside_the_image(sar, rts):
    rt, _ = rts
    k = K.Parity(sar, "lorenz-z27-64x48-j257-s3-up-t1000")
    cfg, view = K.framed(sar, "lorenz", (64, 48), shrink=0.3)
    want = K.restated("outside", view, k.surface, k.starts, plot=1, **k.params)
    assert want[3]["outside"] >= 50 and want[3]["visits"] >= 50 and want[3]["visits"] + want[3]["outside"] == want[3]["crossings"]
    got = _section(sar, cfg, _sized(rt, cfg), k.surface, k.starts, plot=True, chunk_steps=64, **k.params)
    _assert_same(got, rt, want, "outside")


def test_face_on_every_depth_ties_and_the_largest_return_time_wins(sar, rts):
    """The plane z = 27 under the identity rotation and angle 0: one depth for every crossing."""
    rt, _ = rts
    cfg = FK.rows_config(sar, sar.flow_coefficients("lorenz"), (16, 12), rotation_axis=(0.0, 0.0, 1.0), rotation_angle=0.0,
                         center_camera=(0.0, -30.0, 0.0), scale=1.0 / 80.0, angle=0.0)    # depth 30 - z = 3: in front of the sentinel
    view = R.view_of(cfg.c)
    starts = K.starts_of(sar, "lorenz", 64)
    p = dict(dt=0.01, transient=200, samples=40, max_steps=3000, direction=0)
    want = K.restated("face-on", view, K.Z27, starts, plot=1, **p)
    seen = want[4]["count"] > 0
    assert len(np.unique(want[4]["zbuf"][seen])) == 1 and (want[4]["count"] >= 5).sum() >= 10 and len(np.unique(want[4]["steps"][seen])) >= 10
    # the hue of a pixel is the largest (float)r of its crossings
    have = ~np.isnan(want[1])
    inb, idx, _, _ = R.project(view, M.constants(view), *(want[0][have][:, a] for a in range(3)))
    top = np.zeros(16 * 12, dtype=np.float32)
    np.maximum.at(top, idx[inb], want[1][have][inb].astype(np.float32))
    assert np.array_equal(want[4]["steps"].reshape(-1)[seen.reshape(-1)], top[seen.reshape(-1)].astype(np.float64))
    for order in (np.arange(64), np.arange(64)[::-1]):
        got = _section(sar, cfg, _sized(rt, cfg), K.Z27, starts[order], plot=True, chunk_jobs=64 if order[0] == 0 else 24, **p)
        assert not FK.same_frame(_frame(rt), want[4]), order[0]
        assert np.array_equal(FK.bits(got.points[np.argsort(order)]), FK.bits(want[0]))


def test_plot_0_leaves_the_frame(sar, rts):
    rt, _ = rts
    k = K.Parity(sar, "lorenz-z27-64x48-j63-s3-both-t1000")
    _sized(rt, k.cfg)
    sar.render_jobs(_map_config(sar, (64, 48), 64, 100), rt, sar.start_points(3, 0, 64))
    before = _frame(rt)
    got = _section(sar, k.cfg, rt, k.surface, k.starts, chunk_steps=64, **k.params)
    assert not FK.same_frame(_frame(rt), before) and got.stats["max"] == before["max"]
    assert got.stats["visits"] == got.stats["outside"] == 0
    assert [b for b in K.same_outputs(got, k.want(plot=0)) if b != "stats.max"] == []     # (the restated run starts from a reset frame)


def test_a_maps_render_after_a_section_is_the_oracles(sar, oracle, rts):
    """The depth-hint hand-over: the render that follows must not trust hints from before the section raised zbuf."""
    rt, _ = rts
    k = K.Parity(sar, "lorenz-z27-64x48-j257-s3-up-t1000")
    jobs, iters = 2048, 200                                                  # enough jobs for the binned path and its hints
    mcfg, mstarts = _map_config(sar, (64, 48), jobs, iters), sar.start_points(3, 0, jobs)
    _sized(rt, k.cfg)
    sar.render_jobs(mcfg, rt, mstarts)                                       # hints learned ...
    _section(sar, k.cfg, rt, k.surface, k.starts, plot=True, **k.params)
    state = _frame(rt)                                                       # ... zbuf raised by the section ...
    sar.render_jobs(mcfg, rt, mstarts)                                       # ... and the map again
    ort = oracle.Runtime(64, 48)
    ort.count[...], ort.zbuf[...], ort.steps[...] = state["count"], state["zbuf"], state["steps"]
    ort.set_max(state["max"])
    oracle.render_jobs(mcfg.c, ort, mstarts, iters)
    assert not FK.same_frame(_frame(rt), dict(count=ort.count, zbuf=ort.zbuf, steps=ort.steps, max=ort.max))


# ---- 4. the hand-over --------------------------------------------------------------------------------------------------------------
def test_the_crossings_go_to_the_pair_histogram_and_frame_their_own_view(sar, rts):
    rt, _ = rts
    k = K.Parity(sar, "lorenz-z27-7x5-j64-s40-down-t0")
    want = k.want()
    _sized(rt, k.cfg)
    fs = _section(sar, k.cfg, rt, k.surface, k.starts, **k.params)
    full = want[2]["status"] == P.FULL
    traj = fs.trajectories()
    assert traj.shape == (int(full.sum()), 40, 3) and np.array_equal(FK.bits(traj), FK.bits(want[0][full]))
    hist = sar.pair_histogram(rt, traj.reshape(-1, 3), samples=40)
    assert np.array_equal(hist, X.pair_hist(want[0][full].reshape(-1, 3), 40)[0])
    rm = fs.return_map()
    assert rm.shape == (int(full.sum()) * 39, 2) and np.array_equal(rm[:39, 0], traj[0, :-1, 2]) and np.array_equal(rm[:39, 1], traj[0, 1:, 2])
    rm2 = fs.return_map(proj=(1.0, 0.0, 0.0), lag=2)
    assert rm2.shape == (int(full.sum()) * 38, 2) and np.array_equal(rm2[:38, 1], traj[0, 2:, 0])
    big = FK.rows_config(sar, sar.flow_coefficients("lorenz"), (64, 48))
    cfg = fs.view(big)
    assert bytes(cfg.c) == bytes(sar.frame_view_box(big, want[3]["extent"], margin=0.05).c)
    got = _section(sar, cfg, _sized(rt, cfg), k.surface, k.starts, plot=True, **k.params)
    assert got.stats["outside"] == 0 and got.stats["visits"] == got.stats["crossings"] == want[3]["crossings"]


# ---- 5. timing, and the runtime afterwards -----------------------------------------------------------------------------------------
def test_timing_books_the_kernels(sar, rts):
    rt, _ = rts
    k = K.Parity(sar, "lorenz-z27-7x5-j65-s1-up-t0")
    _sized(rt, k.cfg)
    rt.enable_timing(True)
    try:
        _section(sar, k.cfg, rt, k.surface, k.starts, plot=True, chunk_steps=64, **dict(k.params, transient=100))
        t = rt.last_timing()
        assert t.iterate_launches == -(-k.params["max_steps"] // 64) and t.iterate_ms > 0 and t.warmup_ms > 0 and t.colorize_ms > 0
    finally:
        rt.enable_timing(False)


def test_the_runtime_is_otherwise_unchanged(sar, oracle, rts):
    rt, _ = rts
    k = K.Parity(sar, "rossler-y0-64x48-j65-s3-up-t200")
    _sized(rt, k.cfg)
    _section(sar, k.cfg, rt, k.surface, k.starts, plot=True, **k.params)
    rt.reset()
    jobs, iters = 2048, 200
    mcfg, mstarts = _map_config(sar, (64, 48), jobs, iters), sar.start_points(3, 0, jobs)
    sar.render_jobs(mcfg, rt, mstarts)
    ort = oracle.Runtime(64, 48)
    oracle.render_jobs(mcfg.c, ort, mstarts, iters)
    assert not FK.same_frame(_frame(rt), dict(count=ort.count, zbuf=ort.zbuf, steps=ort.steps, max=ort.max))
    assert np.array_equal(sar.colorize(mcfg, rt), oracle.colorize(mcfg.c, ort))
