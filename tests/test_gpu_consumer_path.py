"""GPU: the consumer wave's per-visit path in k_iterate_split (PoolStager::step with a FlaggedVisit). A lane without a visit arrives
as the hand-over word 0x80000000: its mask is one compare of that word, its depth-hint load reads element 0 because `idx << 2` drops
the flag, the record placement works on lane masks, the swap of a full buffer re-points the bin through the control word's kept LDS
address, and a trip of the consumer's loop is two barrier phases. None of it may show: every case is held to the CPU oracle bit for
bit on count, max, zbuf and steps (zbuf after `+ 0.0f` on both sides where a case reaches -0.0: DESIGN.md section 4). The wave-pair
kernel is forced (`set_tuning(variant=3, split_waves=2)`) and the launch description is asserted on.

The oracle's state of a case is computed once and shared by the tests that need it."""
import math

import numpy as np
import pytest

import depth_cases as DC
from strange_attractor_renderer_amd.sequence import frame_seed

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _oracle_state(oracle, cfg, starts, n):
    ort = oracle.Runtime(cfg.c.width, cfg.c.height)
    oracle.render_jobs(cfg.c, ort, starts, n)
    return ort.count.copy(), ort.max, ort.zbuf.copy(), ort.steps.copy()


def _state(rt):
    return rt.count(), rt.max(), rt.zbuf(), rt.steps()


def _assert_same(got, want, what, fold_neg_zero=False):
    assert np.array_equal(got[0], want[0]), f"{what}: count differs on {int((got[0] != want[0]).sum())} pixels"
    assert got[1] == want[1], f"{what}: max {got[1]} vs {want[1]}"
    z_got, z_want = (got[2] + np.float32(0.0), want[2] + np.float32(0.0)) if fold_neg_zero else (got[2], want[2])
    assert np.array_equal(DC.bits(z_got), DC.bits(z_want)), f"{what}: zbuf differs on {int((DC.bits(z_got) != DC.bits(z_want)).sum())} pixels"
    assert np.array_equal(DC.bits(got[3]), DC.bits(want[3])), f"{what}: steps differs on {int((DC.bits(got[3]) != DC.bits(want[3])).sum())} pixels"


def _render(sar, cfg, starts, park=None, **options):
    """One render call on a fresh runtime through the wave-pair kernel (park window `park`, None = the library's own choice); the
    runtime and what it launched."""
    rt = sar.Runtime(cfg)
    rt.set_tuning(variant=3, split_waves=2)
    if park is not None:
        rt.set_option("depth_park", park)
    for k, v in options.items():
        rt.set_option(k, v)
    sar.render_jobs(cfg, rt, starts)
    d = rt.describe_last_launch()
    assert "k_iterate_split" in d, d
    if park is not None:
        assert f" park={park} " in d, d
    return rt, d


JOBS, N, SEED = 2048, 200, 7


def _saturne(sar, size=256, n=N, **kw):
    return sar.Config.poisson_saturne(iterations=JOBS * n, width=size, height=size, jobs_total=JOBS, seed=SEED, **kw)


@pytest.mark.parametrize("park", [0, 8])
def test_plain_frame(sar, oracle, gpu, park):
    """poisson-saturne 256 x 256, 2 048 jobs x 200 iterations, with and without a park window."""
    cfg = _saturne(sar)
    st = sar.start_points(SEED, 0, JOBS)
    want = _ref("plain", lambda: _oracle_state(oracle, cfg, st, N))
    rt, d = _render(sar, cfg, st, park)
    assert "hints=f32" in d, d
    _assert_same(_state(rt), want, f"plain, window {park} ({d})")
    rt.close()


# what the oracle counts inside the image of the 409 600 iterations at these scales (78 % and 29 %): the rest are lanes without a visit
INSIDE = {2.0: 320_645, 3.0: 119_411}


@pytest.mark.parametrize("park", [0, 8])
@pytest.mark.parametrize("scale", sorted(INSIDE))
def test_lanes_without_a_visit(sar, oracle, gpu, scale, park):
    """The same frame zoomed in: a fifth and two thirds of the iterations leave the image. Nobody visits pixel (0, 0), whose depth
    hint every lane without a visit loads: a visit filed for such a lane would show there."""
    cfg = _saturne(sar, scale=scale)
    st = sar.start_points(SEED, 0, JOBS)
    want = _ref(("scale", scale), lambda: _oracle_state(oracle, cfg, st, N))
    inside = int(want[0].sum(dtype=np.uint64))
    assert abs(inside - INSIDE[scale]) <= INSIDE[scale] // 100, f"scale {scale}: the oracle counts {inside} iterations inside, expected about {INSIDE[scale]}"
    assert want[0][0, 0] == 0, "pixel (0, 0) was meant to stay empty"
    rt, d = _render(sar, cfg, st, park)
    assert "hints=f32" in d, d
    _assert_same(_state(rt), want, f"scale {scale}, window {park} ({d})")
    rt.close()


@pytest.mark.parametrize("n", [200, 37, 5])
def test_one_control_word_for_everybody(sar, oracle, gpu, n):
    """64 x 64 is the smallest image the planner gives the wave-pair kernel, and it is ONE bin: all 64 lanes of a wave ask the same
    control word for a slot, so more than R = 60 lanes cross a buffer boundary in one request (place_overflow). n = 200 is whole
    trips of the consumer's two-phase loop, 37 = 4 * 9 + 1 leaves half a pass, 5 = 4 + 1 one trip and half a pass (and 37 and 5
    end inside a park window)."""
    cfg = _saturne(sar, size=64, n=n)
    st = sar.start_points(SEED, 0, JOBS)
    want = _ref(("one bin", n), lambda: _oracle_state(oracle, cfg, st, n))
    assert int(want[0].sum(dtype=np.uint64)) > JOBS * n // 2, "most iterations were meant to land inside"
    rt, d = _render(sar, cfg, st)
    assert " bins=1x" in d and " R=60 " in d, d
    _assert_same(_state(rt), want, f"64 x 64, n = {n} ({d})")
    rt.close()


def test_shorter_than_a_trip(sar, oracle, gpu):
    """n = 3: no whole trip of the two-phase loop, only the left-over pass of the depth pipeline and half a pass."""
    cfg = _saturne(sar, size=64, n=3)
    st = sar.start_points(SEED, 0, JOBS)
    rt, d = _render(sar, cfg, st)
    _assert_same(_state(rt), _oracle_state(oracle, cfg, st, 3), f"64 x 64, n = 3 ({d})")
    rt.close()


def test_solar_sail_with_nan_jobs(sar, oracle, gpu):
    """~38 % of solar-sail's start points end in NaN during the warm-up: waves whose last lanes never have a visit, and every dead
    job's iterations on pixel (0, 0) — the pixel whose hint the lanes without a visit load."""
    jobs, n, w, h = 2048, 300, 200, 180
    cfg = sar.Config.solar_sail(iterations=jobs * n, width=w, height=h, jobs_total=jobs, render_kind=sar.SAR_RENDER_DEPTH, scale=1.0)
    st = sar.start_points(5, 0, jobs)
    want = _oracle_state(oracle, cfg, st, n)
    assert want[0][0, 0] > 100 * n, "expected many divergent jobs in this sample"
    rt, d = _render(sar, cfg, st)
    _assert_same(_state(rt), want, f"solar-sail ({d})")
    rt.close()


def test_narrow_hints_forced_on_the_plain_frame(sar, oracle, gpu):
    """The 16-bit hints keep the select in front of their load (the tile permutation would carry the flag bit into the index)."""
    cfg = _saturne(sar)
    st = sar.start_points(SEED, 0, JOBS)
    want = _ref("plain", lambda: _oracle_state(oracle, cfg, st, N))
    rt, d = _render(sar, cfg, st, 4, hint_bits=16)
    assert "hints=q16" in d, d
    _assert_same(_state(rt), want, f"hint_bits 16, window 4 ({d})")
    rt.close()


@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", ["rising", "rising_tied", "overflow_mid"])
def test_narrow_hints_forced_on_depth_cases(sar, oracle, gpu, case, size):
    """Every visit a winner, every visit a tie, and trajectories that diverge after the warm-up, through the 16-bit hints."""
    DC.check_condition(oracle, case, size)
    ref = DC.reference(oracle, case, size)
    rt, d = _render(sar, DC.config(sar, case, size), DC.starts(case), 4, hint_bits=16)
    assert "hints=q16" in d, d
    _assert_same(_state(rt), (ref.count, ref.max, ref.zbuf, ref.steps), f"{case} {size} hint_bits 16 ({d})", fold_neg_zero=True)
    rt.close()


def test_a_batch(sar, oracle, gpu):
    """sar_render_jobs_batch, three solar-sail frames of 128 x 128: k_iterate_split_batch shares the consumer's code. Its frames equal
    per-frame renders and the oracle."""
    F, w, h, jobs, n = 3, 128, 128, 1024, 300
    cfgs, starts = [], []
    for k in range(F):
        cfgs.append(sar.Config.solar_sail(iterations=jobs * n, width=w, height=h, jobs_total=jobs, render_kind=sar.SAR_RENDER_DEPTH, scale=1.0,
                                          angle=k * math.pi / 180.0 * 7.0, seed=11))
        starts.append(sar.start_points(frame_seed(11, k), 0, jobs))
    rts = sar.Runtime.group(cfgs[0], F)
    sar.render_jobs_batch(cfgs, rts, starts)
    d = rts[0].describe_last_launch()
    assert "k_iterate_split" in d and f"batch of {F} frames" in d, d
    for i, (cfg, rt, st) in enumerate(zip(cfgs, rts, starts)):
        got = _state(rt)
        one, d1 = _render(sar, cfg, st)
        assert "batch" not in d1, d1
        _assert_same(got, _state(one), f"frame {i} of the batch vs its own render call")
        _assert_same(got, _oracle_state(oracle, cfg, st, n), f"frame {i} of the batch vs the oracle")
        one.close()
    for rt in reversed(rts):
        rt.close()
