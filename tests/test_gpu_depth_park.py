"""GPU: the park window of k_iterate_split's consumer wave (test option "depth_park": 0, 2, 4, 8). A visit that passes its depth hint
waits in its lane's registers and the wave runs stage 2 of the depth test — key load, compare, atomic max, hint store — once per
window for all parked lanes; a lane that passes again while it holds a parked visit flushes the wave first, and the end of a job
flushes what is parked before it settles the pipeline. Nothing of that may show: every case is held to the CPU oracle bit for bit
on count, max, zbuf and steps (zbuf after `+ 0.0f` on both sides where a case reaches -0.0: DESIGN.md section 4), and the parked
forms to the unparked one byte for byte.

The oracle's state of a case is computed once and shared by the tests that need it."""
import math

import numpy as np
import pytest

import depth_cases as DC
from strange_attractor_renderer_amd.sequence import frame_seed

pytestmark = pytest.mark.gpu

WINDOWS = (0, 2, 4, 8)
_REF = {}


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _oracle_state(oracle, cfg, starts, n):
    w, h = cfg.c.width, cfg.c.height
    ort = oracle.Runtime(w, h)
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


def _render(sar, cfg, starts, park, **options):
    """One render call on a fresh runtime through the wave-pair kernel with park window `park`; the runtime and what it launched."""
    rt = sar.Runtime(cfg)
    rt.set_tuning(variant=3, split_waves=2)
    rt.set_option("depth_park", park)
    for k, v in options.items():
        rt.set_option(k, v)
    sar.render_jobs(cfg, rt, starts)
    d = rt.describe_last_launch()
    assert "k_iterate_split" in d and f" park={park} " in d, d
    return rt, d


def test_every_window_equals_the_oracle_and_the_unparked_kernel(sar, oracle, gpu):
    """256 x 256, 2 048 jobs x 200 iterations of poisson-saturne: windows 0 / 2 / 4 / 8 all equal the oracle, and the three parked
    forms are byte-identical to window 0."""
    jobs, n = 2048, 200
    cfg = sar.Config.poisson_saturne(iterations=jobs * n, width=256, height=256, jobs_total=jobs, seed=7)
    st = sar.start_points(7, 0, jobs)
    want = _ref("plain", lambda: _oracle_state(oracle, cfg, st, n))
    got = {}
    for park in WINDOWS:
        rt, d = _render(sar, cfg, st, park)
        got[park] = _state(rt)
        _assert_same(got[park], want, f"window {park} vs the oracle ({d})")
        rt.close()
    for park in WINDOWS[1:]:
        _assert_same(got[park], got[0], f"window {park} vs window 0")


# One pixel wins again and again: every visit of `rising` beats all earlier ones of its job, `rising_tied` and `const_pos` tie on every
# pixel — a lane passes stage 1 while it still holds a parked visit, and the wave flushes early. n = 37 is no multiple of the window
# (and odd: the job ends on half a pass of the pipeline), n = 5 ends inside the first window: the drain finds parked visits and an
# unfinished window.
@pytest.mark.parametrize("n", [None, 37, 5], ids=["n-own", "n-37", "n-5"])
@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("case", ["rising", "rising_tied", "const_pos"])
def test_repeated_winners_flush_early(sar, oracle, gpu, case, size, n):
    if n is None:
        DC.check_condition(oracle, case, size)
    cfg = DC.config(sar, case, size, n=n)
    ref = DC.reference(oracle, case, size, n=n)
    rt, d = _render(sar, cfg, DC.starts(case), 8)
    _assert_same(_state(rt), (ref.count, ref.max, ref.zbuf, ref.steps), f"{case} {size} n={n} window 8 ({d})", fold_neg_zero=True)
    rt.close()


@pytest.mark.parametrize("park", [4, 8])
def test_solar_sail_with_nan_jobs(sar, oracle, gpu, park):
    """~38 % of solar-sail's start points end in NaN during the warm-up: waves with idle lanes, lanes that never park."""
    jobs, n, w, h = 2048, 300, 200, 180
    cfg = sar.Config.solar_sail(iterations=jobs * n, width=w, height=h, jobs_total=jobs, render_kind=sar.SAR_RENDER_DEPTH, scale=1.0)
    st = sar.start_points(5, 0, jobs)
    want = _ref("solar-sail", lambda: _oracle_state(oracle, cfg, st, n))
    assert want[0][0, 0] > 100 * n, "expected many divergent jobs in this sample"
    rt, d = _render(sar, cfg, st, park)
    _assert_same(_state(rt), want, f"solar-sail window {park} ({d})")
    rt.close()


@pytest.mark.parametrize("park", [4, 8])
@pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_trajectories_that_diverge_after_the_warm_up(sar, oracle, gpu, size, park):
    """overflow_mid: ~365 counted iterations at +-inf depth, then x is NaN and the rest land on pixel (0, 0) through the ordinary
    record path — while visits are parked."""
    case = "overflow_mid"
    DC.check_condition(oracle, case, size)
    ref = DC.reference(oracle, case, size)
    rt, d = _render(sar, DC.config(sar, case, size), DC.starts(case), park)
    _assert_same(_state(rt), (ref.count, ref.max, ref.zbuf, ref.steps), f"{case} {size} window {park} ({d})", fold_neg_zero=True)
    rt.close()


@pytest.mark.parametrize("hint_bits", [32, 16])
def test_both_hint_types(sar, oracle, gpu, hint_bits):
    """The f32 hints and — forced at 256 x 256 — the 16-bit ones (8 x 8 tiles: the width is a power of two), window 4 each; then the
    depth cases whose depths leave the 16-bit quantiser's range or are all ties."""
    jobs, n = 2048, 200
    cfg = sar.Config.poisson_saturne(iterations=jobs * n, width=256, height=256, jobs_total=jobs, seed=7)
    st = sar.start_points(7, 0, jobs)
    want = _ref("plain", lambda: _oracle_state(oracle, cfg, st, n))
    rt, d = _render(sar, cfg, st, 4, hint_bits=hint_bits)
    assert ("q16" if hint_bits == 16 else "f32") in d, d
    _assert_same(_state(rt), want, f"hint_bits {hint_bits} window 4 ({d})")
    rt.close()
    size = DC.SIZES[1]
    for case in ("rising_far", "alt_inf", "shrink_alt", "const_neg"):
        ref = DC.reference(oracle, case, size)
        rt, d = _render(sar, DC.config(sar, case, size), DC.starts(case), 4, hint_bits=hint_bits)
        assert ("q16" if hint_bits == 16 else "f32") in d, d
        _assert_same(_state(rt), (ref.count, ref.max, ref.zbuf, ref.steps), f"{case} hint_bits {hint_bits} window 4 ({d})", fold_neg_zero=True)
        rt.close()


@pytest.mark.parametrize("overlap", [0, 1])
def test_depth_resolve_beside_and_behind_the_accumulate(sar, oracle, gpu, overlap):
    """The depth resolve reads the keys the parked stage 2 wrote: on the launch stream and on the side stream, window 4, two calls
    into one runtime (the second finds the first call's keys and hints)."""
    jobs, n, w, h = 2048, 200, 256, 256
    cfg = sar.Config.poisson_saturne(iterations=jobs * n, width=w, height=h, jobs_total=jobs, seed=7)
    st = sar.start_points(7, 0, 2 * jobs)

    def make():
        ort = oracle.Runtime(w, h)
        oracle.render_jobs(cfg.c, ort, st[:jobs], n)
        oracle.render_jobs(cfg.c, ort, st[jobs:], n)
        return ort.count.copy(), ort.max, ort.zbuf.copy(), ort.steps.copy()
    want = _ref("two calls", make)
    rt, d = _render(sar, cfg, st[:jobs], 4, tail_overlap=overlap)
    sar.render_jobs(cfg, rt, st[jobs:])
    _assert_same(_state(rt), want, f"tail_overlap {overlap} window 4 ({d})")
    rt.close()


def test_a_batched_launch_is_unaffected(sar, oracle, gpu):
    """sar_render_jobs_batch, three frames of 128 x 128: the batched kernel has no park window whatever the option says, and its
    frames equal per-frame renders (which park) and the oracle."""
    F, w, h, jobs, n = 3, 128, 128, 1024, 300
    cfgs, starts = [], []
    for k in range(F):
        cfgs.append(sar.Config.solar_sail(iterations=jobs * n, width=w, height=h, jobs_total=jobs, render_kind=sar.SAR_RENDER_DEPTH, scale=1.0,
                                          angle=k * math.pi / 180.0 * 7.0, seed=11))
        starts.append(sar.start_points(frame_seed(11, k), 0, jobs))
    rts = sar.Runtime.group(cfgs[0], F)
    for rt in rts:
        rt.set_option("depth_park", 8)
    sar.render_jobs_batch(cfgs, rts, starts)
    d = rts[0].describe_last_launch()
    assert f"batch of {F} frames" in d and " park=0 " in d, d
    for i, (cfg, rt, st) in enumerate(zip(cfgs, rts, starts)):
        got = _state(rt)
        one, d1 = _render(sar, cfg, st, 4)
        assert "batch" not in d1, d1
        _assert_same(got, _state(one), f"frame {i} of the batch vs its own render call")
        _assert_same(got, _oracle_state(oracle, cfg, st, n), f"frame {i} of the batch vs the oracle")
        one.close()
    for rt in reversed(rts):
        rt.close()


def test_the_option_refuses_other_windows(sar, gpu):
    cfg = sar.Config.poisson_saturne(iterations=64 * 8, width=64, height=64, jobs_total=64)
    rt = sar.Runtime(cfg)
    for bad in (1, 3, 6, 16):
        with pytest.raises(Exception):
            rt.set_option("depth_park", bad)
    rt.close()
