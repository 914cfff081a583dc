"""GPU: the tail of a launch chunk of the binned path — k_bin_accumulate adds its histograms straight into count (one atomic per
live counter, the running max and the wrap flag from what the adds return) while k_depth_resolve settles key / steps beside it on
the side stream ("tail_overlap" 1) or behind it on the launch stream ("tail_overlap" 0, the default: the faster order).

Every case is held to the CPU oracle bit for bit (count, max, zbuf, steps, RGBA16) under both orders. The oracle's state of a
case is computed once and shared by both."""
import math

import numpy as np
import pytest

from strange_attractor_renderer_amd.sequence import frame_seed

pytestmark = pytest.mark.gpu

OVERLAP = pytest.mark.parametrize("overlap", [1, 0])
_REF = {}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _cfg(sar, preset, **kw):
    return getattr(sar.Config, preset)(**kw)


def _freeze(oracle, cfg, ort):
    return ort.count.copy(), ort.max, ort.zbuf.copy(), ort.steps.copy(), oracle.colorize(cfg.c, ort)


def _ref(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _state(sar, cfg, rt):
    return rt.count(), rt.max(), rt.zbuf(), rt.steps(), sar.colorize(cfg, rt)


def _assert_same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: count differs"
    assert got[1] == want[1], f"{what}: max differs ({got[1]} vs {want[1]})"
    assert np.array_equal(_bits(got[2]), _bits(want[2])), f"{what}: zbuf differs"
    assert np.array_equal(_bits(got[3]), _bits(want[3])), f"{what}: steps differs"
    assert np.array_equal(got[4], want[4]), f"{what}: RGBA16 differs"


def _runtime(sar, cfg, overlap, **tuning):
    rt = sar.Runtime(cfg)
    rt.set_option("tail_overlap", overlap)
    if tuning:
        rt.set_tuning(**tuning)
    return rt


def _binned(rt):
    assert "k_bin_accumulate" in rt.describe_last_launch(), rt.describe_last_launch()


@OVERLAP
def test_plain_frame(sar, oracle, gpu, overlap):
    jobs, n, w, h = 2048, 512, 256, 256
    cfg = _cfg(sar, "poisson_saturne", iterations=jobs * n, width=w, height=h, jobs_total=jobs, seed=7)
    st = sar.start_points(7, 0, jobs)

    def make():
        ort = oracle.Runtime(w, h)
        oracle.render_jobs(cfg.c, ort, st, n)
        return _freeze(oracle, cfg, ort)
    rt = _runtime(sar, cfg, overlap)
    sar.render_jobs(cfg, rt, st)
    _binned(rt)
    _assert_same(_state(sar, cfg, rt), _ref("plain", make), f"256x256 tail_overlap={overlap}")
    rt.close()


@OVERLAP
@pytest.mark.parametrize("size", [(61, 47), (2049, 3)])
def test_odd_shapes(sar, oracle, gpu, size, overlap):
    """61 x 47: the pixel count is no multiple of four (the scalar loads of the depth resolve) and below one 2048-pixel block;
    2049 x 3: the last block ends one pixel into a 2048-pixel segment."""
    w, h = size
    jobs, n = 700, 400
    cfg = _cfg(sar, "solar_sail", iterations=jobs * n, width=w, height=h, jobs_total=jobs, scale=0.9)
    st = sar.start_points(29, 0, jobs)

    def make():
        ort = oracle.Runtime(w, h)
        oracle.render_jobs(cfg.c, ort, st, n)
        return _freeze(oracle, cfg, ort)
    rt = _runtime(sar, cfg, overlap)
    sar.render_jobs(cfg, rt, st)
    _binned(rt)
    _assert_same(_state(sar, cfg, rt), _ref(("odd", size), make), f"{w}x{h} tail_overlap={overlap}")
    rt.close()


@OVERLAP
def test_two_calls_without_a_reset_ties_go_to_the_first_counts_add(sar, oracle, gpu, overlap):
    """The second call visits exactly what the first visited: every depth it offers ties with what the runtime holds (strict `>`,
    :821 — the first call keeps every pixel), and every count doubles."""
    jobs, n, w, h = 1024, 500, 192, 160
    cfg = _cfg(sar, "poisson_saturne", iterations=jobs * n, width=w, height=h, jobs_total=jobs)
    st = sar.start_points(3, 0, jobs)

    def make():
        ort = oracle.Runtime(w, h)
        oracle.render_jobs(cfg.c, ort, st, n)
        once = _freeze(oracle, cfg, ort)
        oracle.render_jobs(cfg.c, ort, st, n)
        return once, _freeze(oracle, cfg, ort)
    once, twice = _ref("two calls", make)
    assert np.array_equal(twice[0], 2 * once[0]) and np.array_equal(_bits(twice[3]), _bits(once[3]))   # (what the case is about)
    rt = _runtime(sar, cfg, overlap)
    sar.render_jobs(cfg, rt, st)
    sar.render_jobs(cfg, rt, st)
    _binned(rt)
    _assert_same(_state(sar, cfg, rt), twice, f"two calls tail_overlap={overlap}")
    rt.close()


@OVERLAP
def test_launch_chunks(sar, oracle, gpu, overlap):
    """A render call cut into four launch chunks (iterate, then accumulate beside depth resolve, then the join — per chunk): a later
    chunk's iterate kernel and its depth test find the earlier chunks' keys final."""
    jobs, n, w, h = 1000, 600, 128, 128
    cfg = _cfg(sar, "poisson_saturne", iterations=jobs * n, width=w, height=h, jobs_total=jobs)
    st = sar.start_points(9, 0, jobs)

    def make():
        ort = oracle.Runtime(w, h)
        oracle.render_jobs(cfg.c, ort, st, n)
        return _freeze(oracle, cfg, ort)
    want = _ref("chunks", make)
    one = _runtime(sar, cfg, overlap, block_threads=64, variant=3)
    sar.render_jobs(cfg, one, st)
    assert "chunks=1 " in one.describe_last_launch()
    cut = _runtime(sar, cfg, overlap, block_threads=64, variant=3 | (333 << 8))
    sar.render_jobs(cfg, cut, st)
    assert "chunks=4 " in cut.describe_last_launch(), cut.describe_last_launch()
    got = _state(sar, cfg, cut)
    _assert_same(got, _state(sar, cfg, one), f"four chunks vs one, tail_overlap={overlap}")
    _assert_same(got, want, f"four chunks vs the oracle, tail_overlap={overlap}")
    one.close()
    cut.close()


def _fixed_point_config(sar, **kw):
    """Every coordinate's polynomial is a constant: every visit of every job lands on ONE pixel (a point of the poisson-saturne
    attractor, so the preset's view shows it)."""
    pt = (float.fromhex("0x1.d37397ce5279dp-3"), float.fromhex("0x1.494519191dfdbp-3"), float.fromhex("-0x1.ff8befd61a1b4p-3"))
    coef = lambda c: [c] + [0.0] * 9
    return _cfg(sar, "poisson_saturne", coeff_x=coef(pt[0]), coeff_y=coef(pt[1]), coeff_z=coef(pt[2]), **kw)


def _hot_pixel(sar, oracle, cfg, w, h, total):
    """What `total` visits of the one pixel leave: depth and payload of the FIRST visit, count = total mod 2^32 (:811), max =
    u32::MAX once the count has wrapped (:813-815)."""
    small = cfg.replace(iterations=64 * 8, jobs_total=64)
    ort = oracle.Runtime(w, h)
    oracle.render_jobs(small.c, ort, sar.start_points(5, 0, 64), 8)
    (ys, xs) = np.nonzero(ort.count)
    assert len(ys) == 1 and ort.count[ys[0], xs[0]] == 64 * 8
    ort.count[ys[0], xs[0]] = total & 0xFFFFFFFF
    ort.set_max(0xFFFFFFFF if total >> 32 else total)
    return _freeze(oracle, cfg, ort)


@OVERLAP
def test_one_pixel_past_u32(sar, oracle, gpu, overlap):
    """2^32 + 131072 visits of one pixel through the default path: the add that carries the pixel past 2^32 - 1 raises the wrap
    flag — `max` reads u32::MAX — and the count is the total mod 2^32."""
    w = h = 2048
    jobs, n = 131072, 32769
    cfg = _fixed_point_config(sar, iterations=jobs * n, width=w, height=h, jobs_total=jobs, transparent=1)
    want = _ref("wrap", lambda: _hot_pixel(sar, oracle, cfg, w, h, jobs * n))
    assert want[1] == 0xFFFFFFFF and want[0].max() == 131072
    rt = _runtime(sar, cfg, overlap)
    sar.render_jobs(cfg, rt, sar.start_points(5, 0, jobs))
    _binned(rt)
    _assert_same(_state(sar, cfg, rt), want, f"one pixel past 2^32, tail_overlap={overlap}")
    assert rt.max() == 0xFFFFFFFF
    rt.close()


@OVERLAP
def test_one_pixel_through_the_packed_counters_guard_events(sar, oracle, gpu, overlap):
    """1.6e7 visits of one pixel through ONE workgroup's packed 16-bit counters: some 500 guard events — each worth 32768 hits
    added to count when the histogram goes out — and the adds that find the guard bit set, which count their hit in memory."""
    w = h = 512
    jobs, n = 8192, 2001
    cfg = _fixed_point_config(sar, iterations=jobs * n, width=w, height=h, jobs_total=jobs)
    want = _ref("guard", lambda: _hot_pixel(sar, oracle, cfg, w, h, jobs * n))
    assert want[1] == jobs * n > 500 * 32768
    rt = _runtime(sar, cfg, overlap, variant=3, bin_shift=16, splits=1)
    sar.render_jobs(cfg, rt, sar.start_points(5, 0, jobs))
    assert "counters=u16-packed" in rt.describe_last_launch(), rt.describe_last_launch()
    _assert_same(_state(sar, cfg, rt), want, f"guard events, tail_overlap={overlap}")
    rt.close()


@OVERLAP
def test_solar_sail_nan_iterations_land_on_pixel_zero_once(sar, oracle, gpu, overlap):
    """~38 % of solar-sail's start points end in NaN: their iterations are counted on the side and reach count[0] through ONE
    workgroup of the accumulate kernel, whatever bin 0 holds. Twice into one runtime: the side counter was cleared in between."""
    jobs, n, w, h = 2048, 600, 200, 180
    cfg = _cfg(sar, "solar_sail", iterations=jobs * n, width=w, height=h, jobs_total=jobs, render_kind=sar.SAR_RENDER_DEPTH, scale=1.0)
    st = sar.start_points(5, 0, 2 * jobs)

    def make():
        ort = oracle.Runtime(w, h)
        oracle.render_jobs(cfg.c, ort, st[:jobs], n)
        once = _freeze(oracle, cfg, ort)
        oracle.render_jobs(cfg.c, ort, st[jobs:], n)
        return once, _freeze(oracle, cfg, ort)
    once, twice = _ref("nan", make)
    assert once[0][0, 0] > 100 * n and twice[0][0, 0] > once[0][0, 0] + 100 * n, "expected many divergent jobs in this sample"
    rt = _runtime(sar, cfg, overlap)
    sar.render_jobs(cfg, rt, st[:jobs])
    _binned(rt)
    _assert_same(_state(sar, cfg, rt), once, f"solar-sail tail_overlap={overlap}")
    sar.render_jobs(cfg, rt, st[jobs:])
    _assert_same(_state(sar, cfg, rt), twice, f"solar-sail, second call, tail_overlap={overlap}")
    rt.close()


@OVERLAP
def test_two_frame_batch_equals_per_frame_renders(sar, oracle, gpu, overlap):
    """sar_render_jobs_batch shares the bodies but keeps the partial-image form of the tail (the accumulate workgroups store, the
    fold sums, clears and resolves over the flagged segments): its frames must equal the direct adds of per-frame renders."""
    F, w, h, jobs, n = 2, 600, 500, 4096, 300
    cfgs, starts = [], []
    for k in range(F):
        cfgs.append(_cfg(sar, "solar_sail", iterations=jobs * n, width=w, height=h, jobs_total=jobs, render_kind=0, scale=1.0,
                         transparent=0, angle=k * math.pi / 180.0 * 7.0, seed=11))
        starts.append(sar.start_points(frame_seed(11, k), 0, jobs))

    def make():
        out = []
        for cfg, st in zip(cfgs, starts):
            ort = oracle.Runtime(w, h)
            oracle.render_jobs(cfg.c, ort, st, n)
            out.append(_freeze(oracle, cfg, ort))
        return out
    want = _ref("batch", make)
    rts = [_runtime(sar, c, overlap) for c in cfgs]
    sar.render_jobs_batch(cfgs, rts, starts)
    assert "batch of 2 frames" in rts[0].describe_last_launch(), rts[0].describe_last_launch()
    for i, (cfg, rt, st) in enumerate(zip(cfgs, rts, starts)):
        got = _state(sar, cfg, rt)
        one = _runtime(sar, cfg, overlap)
        sar.render_jobs(cfg, one, st)
        assert "batch" not in one.describe_last_launch()
        _assert_same(got, _state(sar, cfg, one), f"frame {i} vs its own render call, tail_overlap={overlap}")
        _assert_same(got, want[i], f"frame {i} vs the oracle, tail_overlap={overlap}")
        one.close()
    for rt in reversed(rts):
        rt.close()


@OVERLAP
def test_three_renders_give_identical_bytes(sar, gpu, overlap):
    """The order in which the accumulate workgroups' adds land on a pixel differs from run to run; what they leave must not."""
    jobs, n = 8192, 500
    cfg = _cfg(sar, "poisson_saturne", iterations=jobs * n, width=512, height=512, jobs_total=jobs)
    st = sar.start_points(1, 0, jobs)
    outs = []
    for _ in range(3):
        rt = _runtime(sar, cfg, overlap)
        sar.render_jobs(cfg, rt, st)
        outs.append(_state(sar, cfg, rt))
        rt.close()
    for k in (1, 2):
        _assert_same(outs[k], outs[0], f"render {k} vs render 0, tail_overlap={overlap}")
