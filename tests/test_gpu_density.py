"""GPU: density estimation (sar_runtime_density, k_density) against the numpy restatement (tests/density_restatement.py), bit for
bit: count, steps (as u64 bit patterns), max and every statistic, on the frames of tests/density_cases.py loaded into a runtime — one
call, two calls, every tile option, with and without the statistics' wait — on a rendered frame and its colorize, with auto exposure
and auto colour range measuring the filtered buffers, through render_sequence in its single-frame and batched paths, on a runtime of a
frame group, and beside a runtime that never filters."""
import math

import numpy as np
import pytest

import density_cases as K
import density_restatement as D

pytestmark = pytest.mark.gpu

ALL_CASES = pytest.mark.parametrize("name", K.NAMES)
TILES = (8, 16, 32)


def _diff(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return f"{len(bad)} differ, first at {bad[:4].tolist()}: got {[got[tuple(i)].tolist() for i in bad[:4]]}, " \
           f"want {[want[tuple(i)].tolist() for i in bad[:4]]}"


@pytest.fixture(scope="module")
def runtimes(sar, gpu):
    """One runtime per frame size, shared by the loaded-state tests (each test loads what it needs)."""
    made = {}

    def get(w, h):
        if (w, h) not in made:
            made[(w, h)] = sar.Runtime(sar.Config.solar_sail(width=w, height=h))
        rt = made[(w, h)]
        rt.set_option("density_tile", 0)
        return rt

    yield get
    for rt in made.values():
        rt.close()


def _load(rt, k):
    rt.load(k.count, k.steps, k.zbuf, k.max)


def _assert_state(rt, count, steps, mx, what):
    got_c, got_s = rt.count(), rt.steps()
    assert np.array_equal(got_c, count), f"{what}: count: {_diff(got_c, count)}"
    assert np.array_equal(K.bits(got_s), K.bits(steps)), f"{what}: steps: {_diff(K.bits(got_s), K.bits(steps))}"
    assert rt.max() == mx, f"{what}: max {rt.max()} vs {mx}"


@ALL_CASES
def test_one_and_two_calls_match_the_restatement(sar, runtimes, name):
    k, ref = K.case(name), K.reference(name)
    rt = runtimes(k.width, k.height)
    _load(rt, k)
    zbuf = rt.zbuf()
    stats = rt.density_filter(samples=k.S)
    assert stats == ref.stats, f"{name}: stats {stats} vs {ref.stats}"
    _assert_state(rt, ref.count, ref.steps, ref.max, name)
    assert np.array_equal(rt.zbuf().view(np.uint32), zbuf.view(np.uint32)), f"{name}: zbuf changed"
    stats2 = sar.density_filter(rt, samples=k.S)                  # not idempotent: the second call filters the filtered frame
    assert stats2 == ref.stats2, f"{name}: second call: stats {stats2} vs {ref.stats2}"
    _assert_state(rt, ref.count2, ref.steps2, ref.max2, f"{name}: second call")
    assert np.array_equal(rt.zbuf().view(np.uint32), zbuf.view(np.uint32)), f"{name}: zbuf changed by the second call"


@ALL_CASES
def test_every_tile_option_gives_the_same_bits(sar, runtimes, name):
    k, ref = K.case(name), K.reference(name)
    rt = runtimes(k.width, k.height)
    for tile in TILES:
        rt.set_option("density_tile", tile)
        _load(rt, k)
        stats = rt.density_filter(samples=k.S)
        assert stats == ref.stats, f"{name} tile {tile}: stats {stats} vs {ref.stats}"
        _assert_state(rt, ref.count, ref.steps, ref.max, f"{name} tile {tile}")
        tiles, copied = rt.density_tiles()
        assert tiles == -(-k.width // 32) * -(-k.height // tile) and 0 <= copied <= tiles
        if ref.stats["spread"] == 0:
            assert copied == tiles, f"{name} tile {tile}: a frame nothing spreads in is copied through whole"


def test_bad_tile_option_is_refused(sar, runtimes):
    rt = runtimes(5, 3)
    with pytest.raises(sar.SarError):
        rt.set_option("density_tile", 12)


@pytest.mark.parametrize("name", K.select("96x80"))
def test_without_statistics_the_buffers_are_the_same(sar, runtimes, name):
    k, ref = K.case(name), K.reference(name)
    rt = runtimes(k.width, k.height)
    _load(rt, k)
    assert rt.density_filter(stats=False, samples=k.S) is None
    _assert_state(rt, ref.count, ref.steps, ref.max, name)


def test_defaults_and_null_params(sar, runtimes):
    k = K.case("sparse_random-67x45-S64")
    rt = runtimes(k.width, k.height)
    _load(rt, k)
    assert sar.load_library().sar_runtime_density(rt.handle, None, None) == 0      # NULL parameters: the defaults, samples 64
    _assert_state(rt, *K.reference(k.name)[:3], "NULL parameters")
    with pytest.raises(sar.SarError):
        rt.density_filter(samples=1)
    with pytest.raises(sar.SarError):
        rt.density_filter(samples=257)
    _assert_state(rt, *K.reference(k.name)[:3], "after the refusals")


def test_timing_books_the_kernel_as_iterate(sar, runtimes):
    k = K.case("sparse_random-96x80-S64")
    rt = runtimes(k.width, k.height)
    _load(rt, k)
    rt.enable_timing(True)
    try:
        rt.density_filter(samples=k.S)
        t = rt.last_timing()
        assert t.iterate_launches == 1
    finally:
        rt.enable_timing(False)


# ---- a rendered frame ----------------------------------------------------------------------------------------------------------
def _rendered(sar, **more):
    jobs = 512
    cfg = sar.Config.solar_sail(width=256, height=256, iterations=jobs * 600, jobs_total=jobs, scale=1.0, transparent=0, **more)
    rt = sar.Runtime(cfg)
    sar.render_jobs(cfg, rt, sar.start_points(11, 0, jobs))
    return cfg, rt


@pytest.mark.parametrize("modes", [False, True], ids=["plain", "exposure+color_range"])
def test_rendered_frame_and_its_colorize(sar, gpu, modes):
    cfg, rt = _rendered(sar)
    count, steps, zbuf = rt.count(), rt.steps(), rt.zbuf()
    want_c, want_s, want_m, want_stats = D.filter(count, steps, 64)
    assert 0 < want_stats["spread"] < want_stats["covered_in"]                                  # a veil and a bright part
    stats = rt.density_filter()
    assert stats == want_stats
    _assert_state(rt, want_c, want_s, want_m, "rendered frame")
    other = sar.Runtime(cfg)
    other.load(want_c, want_s, zbuf, want_m)
    if modes:
        for r in (rt, other):
            r.set_exposure()
            r.set_color_range()
    img, want = sar.colorize(cfg, rt), sar.colorize(cfg, other)
    assert np.array_equal(img, want), _diff(img, want)
    depth = cfg.replace(render_kind=sar.SAR_RENDER_DEPTH)
    assert np.array_equal(sar.colorize(depth, rt), sar.colorize(depth, other))
    plain = sar.Runtime(cfg)
    plain.load(count, steps, zbuf, int(count.max()))
    assert not np.array_equal(img, sar.colorize(cfg, plain)), "the filter changed nothing a picture shows"
    assert np.array_equal(sar.colorize(depth, rt), sar.colorize(depth, plain)), "a Depth colorize must not change"
    for r in (rt, other, plain):
        r.close()


def test_group_runtime_gives_the_same_bits(sar, gpu):
    k = K.case("sparse_random-96x80-S64")
    ref = K.reference(k.name)
    cfg = sar.Config.solar_sail(width=k.width, height=k.height)
    grp = sar.Runtime.group(cfg, 3)
    try:
        for rt in grp:                                              # one stream: enqueued back to back, read afterwards
            _load(rt, k)
        for rt in grp:
            rt.density_filter(stats=False, samples=k.S)
        for i, rt in enumerate(grp):
            _assert_state(rt, ref.count, ref.steps, ref.max, f"group runtime {i}")
        assert grp[1].density_filter(samples=k.S) == ref.stats2
    finally:
        for rt in reversed(grp):
            rt.close()


def test_a_runtime_that_never_filters_is_untouched(sar, gpu):
    """The same small frame rendered and colorized before and after another runtime of the device has filtered: the same checksum."""
    import ctypes as C

    def frame():
        cfg, rt = _rendered(sar)
        img = np.ascontiguousarray(sar.colorize(cfg, rt))
        state = (rt.count(), rt.steps(), rt.zbuf(), rt.max())
        rt.close()
        h = C.c_uint64()
        assert sar.load_library().sar_checksum_fnv1a64(img.ctypes.data_as(C.c_void_p), img.nbytes, C.byref(h)) == 0
        return int(h.value), state

    before, state0 = frame()
    cfg, other = _rendered(sar)
    other.density_filter()
    other.close()
    after, state1 = frame()
    assert before == after
    assert np.array_equal(state0[0], state1[0]) and np.array_equal(K.bits(state0[1]), K.bits(state1[1])) and state0[3] == state1[3]


# ---- the sequence driver -------------------------------------------------------------------------------------------------------
def _sequence_reference(sar, cfg, k, units, jpt, seed, density, modes):
    from strange_attractor_renderer_amd.sequence import frame_seed
    jobs = units * jpt
    c = cfg.replace(angle=k * math.pi / 180.0, jobs_total=jobs, iterations=(cfg.c.iterations // units // jpt) * jobs, seed=seed)
    rt = sar.Runtime(c)
    if modes:
        rt.set_exposure()
        rt.set_color_range()
    sar.render_jobs(c, rt, sar.start_points(frame_seed(seed, k), 0, jobs))
    rt.density_filter(**density)
    img = sar.colorize(c, rt)
    rt.close()
    return img


@pytest.mark.parametrize("modes", [False, True], ids=["plain", "exposure+color_range"])
def test_sequence_filters_every_frame_in_both_paths(sar, gpu, modes):
    from strange_attractor_renderer_amd.sequence import render_sequence
    cfg = sar.Config.solar_sail(iterations=300_000, width=128, height=128, scale=1.0, transparent=0)
    units, jpt, seed = 128, 2, 4
    kw = dict(units=units, jobs_per_thread=jpt, seed=seed, density={})
    if modes:
        kw.update(exposure={}, color_range={})
    single = render_sequence(cfg, 0.0, 3.0, 1.0, batch=1, **kw)
    batched = render_sequence(cfg, 0.0, 3.0, 1.0, batch=3, **kw)
    unfiltered = render_sequence(cfg, 0.0, 3.0, 1.0, batch=3, **{**kw, "density": None})
    assert [k for k, _, _ in single] == [k for k, _, _ in batched] == [0, 1, 2]
    for (k, _, a), (_, _, b), (_, _, u) in zip(single, batched, unfiltered):
        want = _sequence_reference(sar, cfg, k, units, jpt, seed, {}, modes)
        assert np.array_equal(np.asarray(a).reshape(-1), want.reshape(-1)), f"frame {k}, a frame per launch"
        assert np.array_equal(np.asarray(b).reshape(-1), want.reshape(-1)), f"frame {k}, one batch"
        assert not np.array_equal(np.asarray(u).reshape(-1), want.reshape(-1)), f"frame {k}: density=None must not filter"


@pytest.mark.parametrize("delivery", ["frame", "batch"])
def test_sequence_filters_for_both_deliveries(sar, gpu, delivery):
    from strange_attractor_renderer_amd.sequence import SequenceRenderer, frames
    cfg = sar.Config.solar_sail(iterations=300_000, width=128, height=128, scale=1.0, transparent=0)
    units, jpt, seed = 128, 2, 4
    with SequenceRenderer(cfg, units=units, jobs_per_thread=jpt, seed=seed, batch=3, delivery=delivery, density={"samples": 16}) as seq:
        got = seq.run(frames(0.0, 3.0, 1.0))
    for k, _, a in got:
        want = _sequence_reference(sar, cfg, k, units, jpt, seed, {"samples": 16}, False)
        assert np.array_equal(np.asarray(a).reshape(-1), want.reshape(-1)), f"frame {k}, delivery {delivery}"


def test_sequence_refuses_an_unknown_density_field(sar, gpu):
    from strange_attractor_renderer_amd.sequence import render_sequence
    cfg = sar.Config.solar_sail(iterations=300_000, width=128, height=128, scale=1.0, transparent=0)
    with pytest.raises(AttributeError):
        render_sequence(cfg, 0.0, 3.0, 1.0, units=128, jobs_per_thread=2, density={"radius": 3})
