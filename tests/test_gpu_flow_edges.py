"""GPU: flow rendering on the cases of tests/flow_edge_cases.py against the numpy restatement bit for bit — depths of +-inf, below
the sentinel, subnormal, -0.0 and NaN; hues of -0.0, subnormal and +-inf; counts wrapping u32 on a full frame; a loaded frame that
holds +-inf and NaN depths; each under two launch shapes that must give one frame and exact atomics counters, with the Gas and Depth
colorize of the result. Then the shapes: an image beyond one trip of the resolve's launch with the default chunk of jobs crossed by
one job, the phase carried over the default 4096-step launch, the runtime shrunk again afterwards; the jobs in reverse order; and a
map's render with 16-bit tiled depth hints before and after a flow."""
import numpy as np
import pytest

import flow_cases as K
import flow_edge_cases as E
import flow_restatement as R
from test_gpu_flow import _assert_same, _flow, _frame, _images, _load, _map_config, _sized

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rts(sar, gpu):
    """Two runtimes: the one the flows run on and the one restated states are loaded into."""
    cfg = sar.Config.solar_sail(width=E.SIZE[0], height=E.SIZE[1])
    pair = (sar.Runtime(cfg, device=0), sar.Runtime(cfg, device=0))
    yield pair
    for r in pair:
        r.close()


def _run(sar, rt, case, chunk_jobs, chunk_steps, reverse=False):
    """The case's call on rt, sized and reset (or loaded with the case's frame) first: (frame, stats)."""
    _sized(rt, case.cfg)
    if case.before is not None:
        _load(rt, case.before)
    starts = case.starts[::-1].copy() if reverse else case.starts
    stats = _flow(sar, case.cfg, rt, starts, case.steps, chunk_jobs=chunk_jobs, chunk_steps=chunk_steps, **case.params)
    return _frame(rt), stats


def _assert_case(sar, rt, case, chunk_jobs, chunk_steps, reverse=False):
    want_frame, want = case.want(chunk_steps, reverse)
    frame, got = _run(sar, rt, case, chunk_jobs, chunk_steps, reverse)
    _assert_same(frame, got, want_frame, want, (case.name, chunk_jobs, chunk_steps, reverse))     # the two atomics counters included
    return frame


# ---- 1. parity and images, case by case, under two launch shapes -------------------------------------------------------------------
@pytest.mark.parametrize("name", E.NAMES)
def test_edge_case_equals_the_restatement(sar, rts, name):
    rt, rt2 = rts
    case = E.Case(sar, name)
    E.check_condition(case)
    frames = [_assert_case(sar, rt, case, *shape) for shape in case.shapes]
    assert not K.same_frame(frames[0], frames[1])                          # any two launch shapes: one frame
    _load(_sized(rt2, case.cfg), case.want(case.shapes[-1][1])[0])
    for mine, loaded in zip(_images(sar, case.cfg, rt), _images(sar, case.cfg, rt2)):
        assert np.array_equal(mine, loaded)


# ---- 2. the default launch shape across its boundaries, the resolve's second trip, the runtime afterwards ---------------------------
def test_default_chunk_steps_carry_the_phase(sar, rts):
    case = E.Case(sar, "default_chunk_steps")
    E.check_condition(case)
    _assert_case(sar, rts[0], case, 0, 0)


def test_a_big_image_and_a_second_chunk_of_one_job_then_a_small_case(sar, rts):
    rt, _ = rts
    big = E.Case(sar, "big_image")
    E.check_condition(big)
    frame = _assert_case(sar, rt, big, 0, 0)
    last = frame["count"][-1]
    assert np.array_equal(last, big.want(0)[0]["count"][-1]) and np.count_nonzero(last) >= 100      # beyond the resolve's first trip
    small = E.Case(sar, "hue_subnormal")                                    # the key buffer shrunk in use, zeroed per call
    _assert_case(sar, rt, small, *small.shapes[0])


# ---- 3. the jobs in reverse order --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.REVERSIBLE)
def test_reversed_jobs_give_the_same_frame(sar, rts, name):
    case = E.Case(sar, name)
    forward, _ = case.want(64)
    assert not K.same_frame(case.want(64, reverse=True)[0], forward)        # the restatement's maximum commutes, infinities included
    frame = _assert_case(sar, rts[0], case, 64, 64, reverse=True)
    assert not K.same_frame(frame, forward)


# ---- 4. the depth-hint hand-over with 16-bit tiled hints ---------------------------------------------------------------------------
def test_a_maps_render_with_narrow_hints_on_top_of_a_flow(sar, oracle, gpu):
    """test_a_maps_render_on_top_of_a_flow's sequence at 256 x 64 (a power-of-two width: 16-bit hints in 8 x 8 tiles)."""
    size = (256, 64)
    cfg, view = K.framed(sar, "lorenz", size)
    jobs, iters = 2048, 200
    mcfg, mstarts = _map_config(sar, size, jobs, iters), sar.start_points(3, 0, jobs)
    # what the hints are learned from, and what the flow then does to it, from the two references alone: the flow's depth replaces
    # the map's on 211 pixels, so hints that outlived the flow would pass visits the raised zbuf refuses
    ort = oracle.Runtime(*size)
    oracle.render_jobs(mcfg.c, ort, mstarts, iters)
    before = dict(count=ort.count.copy(), zbuf=ort.zbuf.copy(), steps=ort.steps.copy(), max=ort.max)
    fstarts, p = sar.start_points(K.SEED, 0, 65), dict(dt=0.01, transient=K.TRANSIENT)
    want_frame, want = R.flow(view, fstarts, 300, frame=before, **p)
    assert np.count_nonzero((before["zbuf"] != np.float32(-1.0)) & (want_frame["zbuf"] > before["zbuf"])) >= 100
    rt = sar.Runtime(cfg, device=0)
    try:
        rt.set_option("hint_bits", 16)
        sar.render_jobs(mcfg, rt, mstarts)                                   # hints learned ...
        assert "hints=q16" in rt.describe_last_launch(), rt.describe_last_launch()
        got = _flow(sar, cfg, rt, fstarts, 300, **p)
        state = _frame(rt)                                                   # ... zbuf raised by the flow ...
        _assert_same(state, got, want_frame, want, "a flow on a map's frame at 256 x 64")
        sar.render_jobs(mcfg, rt, mstarts)                                   # ... and the map again
        assert "hints=q16" in rt.describe_last_launch(), rt.describe_last_launch()
        ort.count[...], ort.zbuf[...], ort.steps[...] = state["count"], state["zbuf"], state["steps"]
        ort.set_max(state["max"])
        oracle.render_jobs(mcfg.c, ort, mstarts, iters)
        assert not K.same_frame(_frame(rt), dict(count=ort.count, zbuf=ort.zbuf, steps=ort.steps, max=ort.max))
    finally:
        rt.close()
