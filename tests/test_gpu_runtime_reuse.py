"""GPU: ONE long-lived runtime, frame group or renderer taken through several image sizes (sar_runtime_set_width_height) and used on
every path after each — the journeys of tests/reuse_cases.py: size orders that shrink, grow, shrink to 1 x 1 and back, return to
their first size and change shape at equal pixel count (so that identically sized arrays are addressed in another hint layout), and
pairs of sizes for the journeys of three runtimes, a frame group and the multi-device renderer.

References (computed once in reuse_cases.py): the CPU oracle on the same start points, bit for bit (count, max, zbuf, steps, images,
merge; oracle_lib.convert for the image formats), density_restatement.filter and shade_restatement.shade. The exposure, colour-range
and held-window modes are compared with a FRESH runtime of the new size given the same mode and the oracle's state —
tests/test_gpu_exposure.py and tests/test_gpu_color_range.py already hold a fresh runtime to the oracle with restated constants.

Every step asserts through describe_last_launch() that it took the form it is here to test (the hint type, the whole or the
wave-pair iterate kernel, one atomic per visit, a batch of N frames): a plan that falls back fails the test."""
import re

import numpy as np
import pytest

import oracle_lib as O
import reuse_cases as K

pytestmark = pytest.mark.gpu

ORDER_NAMES = list(K.ORDERS)
PAIR_NAMES = list(K.PAIRS)
FILTER_ORDER = K.FILTER_ORDER
ORDERS = pytest.mark.parametrize("order", ORDER_NAMES)
PAIRS = pytest.mark.parametrize("pair", PAIR_NAMES)
ATOMICS = "one global atomic per visit"


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _cfg(sar, f):
    """The device's config of a frame (or of an oracle config): a copy of the struct the oracle renders with."""
    return sar.Config(O.copy_config(K.config(f) if isinstance(f, K.Frame) else f))


def assert_state(rt, st, what):
    np.testing.assert_array_equal(rt.count(), st.count, err_msg=f"count: {what}")
    assert rt.max() == st.max, f"max: {what}"
    np.testing.assert_array_equal(_bits(rt.zbuf()), _bits(st.zbuf), err_msg=f"zbuf: {what}")
    np.testing.assert_array_equal(_bits(rt.steps()), _bits(st.steps), err_msg=f"steps: {what}")


def assert_reset(rt, size, what):
    """The read-backs have the new shape and hold what Runtime::reset leaves."""
    w, h = size
    count, steps, zbuf = rt.count(), rt.steps(), rt.zbuf()
    assert rt.dims() == size and count.shape == steps.shape == zbuf.shape == (h, w), what
    assert not count.any() and rt.max() == 0, f"count / max: {what}"
    assert not _bits(steps).any(), f"steps: {what}"
    assert np.array_equal(_bits(zbuf), np.full((h, w), _bits(np.float32(-1.0))[()])), f"zbuf: {what}"


def _render(sar, rt, f):
    sar.render_jobs(_cfg(sar, f), rt, K.starts(f))
    return rt.describe_last_launch()


def _warmups_found(rt):
    return int(re.search(r"warmup_ahead=(\d+)", rt.describe_last_launch()).group(1))


# ---- 1. render after every kind of resize ------------------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("hint_bits", [16, 32])
@pytest.mark.parametrize("split_waves", [1, 2])
def test_render_after_every_kind_of_resize(sar, gpu, order, hint_bits, split_waves):
    """The binned path with both hint types and both iterate kernels: at every size a frame, a second one on the un-reset runtime
    (the first one's hints filter it), a reset() and a third — each the oracle's state."""
    steps = K.render_steps(K.ORDERS[order])
    rt = sar.Runtime(_cfg(sar, steps[0][1][0][0]))
    rt.set_tuning(variant=3, hint_bits=hint_bits, split_waves=split_waves)
    kernel, hints = ("k_iterate_lean", "k_iterate_split")[split_waves - 1], "hints=q16" if hint_bits == 16 else "hints=f32"
    for i, (size, groups) in enumerate(steps):
        if i:
            rt.set_width_height(*size)
            assert_reset(rt, size, f"{order} step {i}: after the resize to {size}")
        for j, g in enumerate(groups):
            if j == 2:
                rt.reset()
            d = _render(sar, rt, g[-1])
            assert kernel in d and hints in d and "batch" not in d, d
            assert_state(rt, K.rendered(*g), f"{order} step {i} {size} hint_bits={hint_bits} split_waves={split_waves}: frames {[f.seed for f in g]}")
    rt.close()


@ORDERS
def test_one_atomic_per_visit_and_binned_launches_take_turns_across_resizes(sar, gpu, order):
    """path 1 then 3 on the same runtime: the binned path's scratch image is freed by every resize, made by the first binned launch
    and not needed by the launches with one atomic per visit around it (the default hints and kernel choice)."""
    steps = K.render_steps(K.ORDERS[order])
    rt = sar.Runtime(_cfg(sar, steps[0][1][0][0]))
    for i, (size, groups) in enumerate(steps):
        if i:
            rt.set_width_height(*size)
        for j, g in enumerate(groups):
            if j == 2:
                rt.reset()
            path = (1, 3, 1 if i % 2 else 3)[j]
            rt.set_option("path", path)
            d = _render(sar, rt, g[-1])
            assert (ATOMICS in d) == (path == 1) and ("k_bin_accumulate" in d) == (path == 3), d
            assert_state(rt, K.rendered(*g), f"{order} step {i} {size} path {path}: frames {[f.seed for f in g]}")
    rt.close()


# ---- 2. batches across a resize ----------------------------------------------------------------------------------------------------
def _batch(sar, rts, groups):
    frames = [g[-1] for g in groups]
    sar.render_jobs_batch([_cfg(sar, f) for f in frames], rts, [K.starts(f) for f in frames])


@PAIRS
def test_batches_of_three_runtimes_across_a_resize_and_their_tails(sar, gpu, pair):
    """Three runtimes batched at size A (partial histograms per split, segment flags), all resized to B and batched again, then a
    single-frame tail on each un-reset runtime (its own number of histogram copies on the buffers the batch left)."""
    a, b = K.PAIRS[pair]
    fr = K.batch_frames(pair)
    rts = [sar.Runtime(_cfg(sar, g[0])) for g in fr["first"]]
    for what, size in (("first", a), ("second", b)):
        for rt in rts:
            rt.set_width_height(*size)
        _batch(sar, rts, fr[what])
        for m, rt in enumerate(rts):
            assert "batch of 3 frames" in rt.describe_last_launch() and "k_iterate_split" in rt.describe_last_launch(), rt.describe_last_launch()
            assert_state(rt, K.rendered(*fr[what][m]), f"{pair}: {what} batch at {size}, member {m}")
    for m, rt in enumerate(rts):
        d = _render(sar, rt, fr["tails"][m][-1])
        assert "batch" not in d and "k_bin_accumulate" in d, d
        assert_state(rt, K.rendered(*fr["tails"][m]), f"{pair}: tail of member {m} on its un-reset runtime")
        view = fr["tails"][m][-1]
        np.testing.assert_array_equal(sar.colorize(_cfg(sar, view), rt), K.image(fr["tails"][m], view))
    for rt in reversed(rts):
        rt.close()


@PAIRS
def test_a_frame_group_whose_member_is_resized_and_comes_back(sar, gpu, pair):
    """Runtime.group: batched at size A; member 1 alone at size B — the frames can no longer share a launch and run one after the
    other; member 1 back at A — one launch again. Every frame the oracle's."""
    a, b = K.PAIRS[pair]
    fr = K.group_frames(pair)
    rts = sar.Runtime.group(_cfg(sar, fr["group together"][0][0]), 3)
    for what, size_of_1, batched in (("group together", a, True), ("group apart", b, False), ("group again", a, True)):
        rts[1].set_width_height(*size_of_1)
        sar.reset_batch(rts)
        _batch(sar, rts, fr[what])
        for m, rt in enumerate(rts):
            d = rt.describe_last_launch()
            assert ("batch of 3 frames" in d) == batched and ("batch" in d) == batched, d
            assert_state(rt, K.rendered(*fr[what][m]), f"{pair}: {what}, member {m}")
    for rt in reversed(rts):
        rt.close()


# ---- 3. an announcement that outlives its size ---------------------------------------------------------------------------------
@ORDERS
@pytest.mark.parametrize("hint_bits", [16, 32])
def test_announcements_before_and_after_a_resize(sar, gpu, order, hint_bits):
    """sar_runtime_prefetch_device, then the resize, then the announced jobs at the new size: the oracle's state whether or not the
    warm-up that ran ahead is used (it is the map alone). Then the other way round — resize, announce, render: found done."""
    import torch
    sizes = K.ORDERS[order]
    rt = sar.Runtime(_cfg(sar, K.frame(sizes[0], 0)))
    rt.set_option("hint_bits", hint_bits)
    keep = []
    for size, announced, after, then in K.announcement_steps(sizes):
        dev = torch.from_numpy(np.array(K.starts(announced))).cuda()
        dev2 = torch.from_numpy(np.array(K.starts(then))).cuda()
        torch.cuda.synchronize()
        keep += [dev, dev2]
        sar.prefetch_device(_cfg(sar, announced), rt, announced.jobs, announced.n, dev.data_ptr())
        rt.set_width_height(*size)
        sar.render_job_range_device(_cfg(sar, after), rt, after.jobs, after.n, dev.data_ptr())
        assert_state(rt, K.rendered(after), f"{order} {size}: announced before the resize")
        found = _warmups_found(rt)
        rt.reset()
        sar.prefetch_device(_cfg(sar, then), rt, then.jobs, then.n, dev2.data_ptr())
        sar.render_job_range_device(_cfg(sar, then), rt, then.jobs, then.n, dev2.data_ptr())
        assert_state(rt, K.rendered(then), f"{order} {size}: announced after the resize")
        d = rt.describe_last_launch()
        assert _warmups_found(rt) == found + 1 and ("hints=q16" if hint_bits == 16 else "hints=f32") in d, d
    rt.close()


# ---- 4. colorize and the read-back ring --------------------------------------------------------------------------------------------
@ORDERS
def test_colorize_every_format_and_the_read_back_ring_after_a_resize(sar, gpu, order):
    """Gas and Depth colorize, the four converted formats, the conversion left in device memory and fetched into a page-locked image
    of the new size; straight after a resize there is no image to fetch (as on a fresh runtime), and an image of the old size is
    refused before and after the new size's conversion."""
    steps = K.render_steps(K.ORDERS[order])
    formats = (sar.SAR_FMT_RGBA16, sar.SAR_FMT_RGB16, sar.SAR_FMT_RGBA8, sar.SAR_FMT_RGB8)
    rt = sar.Runtime(_cfg(sar, steps[0][1][0][0]))
    old = None
    for i, (size, groups) in enumerate(steps):
        g = groups[0]
        f = g[0]._replace(transparent=i % 2)
        cfg = _cfg(sar, f)
        host = sar.HostImage(size[0], size[1], formats[i % 4])
        if i:
            rt.set_width_height(*size)
            with pytest.raises(sar.SarError):
                sar.read_image_async(rt, host)                         # nothing colorized since the resize
            with pytest.raises(ValueError):
                sar.read_image_async(rt, old)
        _render(sar, rt, g[0])
        gas = K.image(g, f)
        np.testing.assert_array_equal(sar.colorize(cfg, rt), gas, err_msg=f"{order} {size}: Gas")
        depth = f._replace(kind=1)
        np.testing.assert_array_equal(sar.colorize(_cfg(sar, depth), rt), K.image(g, depth), err_msg=f"{order} {size}: Depth")
        for fmt in formats:
            np.testing.assert_array_equal(sar.colorize_format(cfg, rt, fmt), O.convert(fmt, gas), err_msg=f"{order} {size}: format {fmt}")
        sar.colorize_format_device(cfg, rt, host.fmt)
        if old is not None:
            with pytest.raises(ValueError):
                sar.read_image_async(rt, old)                          # the old size's image, with the new size's conversion waiting
            with pytest.raises(ValueError):
                sar.colorize_format_async(cfg, rt, old)
            old.close()
        ticket = sar.read_image_async(rt, host)
        sar.wait_image(rt, ticket)
        assert sar.image_done(rt, ticket)
        np.testing.assert_array_equal(host.array, O.convert(host.fmt, gas), err_msg=f"{order} {size}: read-back of format {host.fmt}")
        old = host
    old.close()
    rt.close()


# ---- 5. modes that stay on -----------------------------------------------------------------------------------------------------------
def _set_mode(sar, rt, mode):
    if mode == "exposure":
        rt.set_exposure()
    elif mode == "color_range":
        rt.set_color_range()
    elif mode == "exposure+color_range":
        rt.set_exposure(q_white=0.9)
        rt.set_color_range(q_lo=0.1)
    else:   # a window that spans both presets' steps (solar-sail's lie below 0 at this scale, poisson-saturne's in [0, 1))
        rt.hold_color_range(sar.ColorRange(-0.5, 1.0, 0.1, 0.9))


@ORDERS
@pytest.mark.parametrize("mode", ["exposure", "color_range", "exposure+color_range", "held_window"])
def test_modes_set_before_a_resize_measure_the_new_frame(sar, gpu, order, mode):
    """set_exposure / set_color_range / hold_color_range stay on across set_width_height; their histogram scratch and records are the
    previous size's. The image after a resize equals that of a fresh runtime of the new size with the same mode and the oracle's state,
    and the records count the NEW frame's covered pixels."""
    import color_range_restatement as R
    steps = K.render_steps(K.ORDERS[order])
    rt = sar.Runtime(_cfg(sar, steps[0][1][0][0]))
    _set_mode(sar, rt, mode)
    for i, (size, groups) in enumerate(steps):
        f = groups[0][0]
        cfg, st = _cfg(sar, f), K.rendered(f)
        if i:
            rt.set_width_height(*size)
        _render(sar, rt, f)
        assert_state(rt, st, f"{order} {size} {mode}")
        img = sar.colorize(cfg, rt)
        fresh = sar.Runtime(cfg)
        _set_mode(sar, fresh, mode)
        fresh.load(st.count, st.steps, st.zbuf, st.max)
        np.testing.assert_array_equal(img, sar.colorize(cfg, fresh), err_msg=f"{order} {size}: image with {mode} on")
        plain = K.image(groups[0], f)
        if K.npix(size) > 1:
            assert not np.array_equal(img, plain), f"{order} {size}: {mode} changed nothing a picture shows"
        e, w = sar.exposure(cfg, rt), sar.color_range(cfg, rt)
        assert e.covered == int((st.count != 0).sum()) and e.max == st.max, f"{order} {size}: exposure record {e}"
        assert w.covered == R.window(st.count, st.steps).covered, f"{order} {size}: colour range record {w}"
        assert e == sar.exposure(cfg, fresh) and w == sar.color_range(cfg, fresh), f"{order} {size}: records {e} {w}"
        np.testing.assert_array_equal(sar.colorize(cfg, rt), img, err_msg=f"{order} {size}: a second colorize")
        fresh.close()
    rt.close()


# ---- 6. density and shade --------------------------------------------------------------------------------------------------------
def test_density_filter_at_every_size_of_a_shrink_then_grow_order(sar, gpu):
    """The density snapshot only ever grows: after a shrink it is the larger frame's. Samples 2 / 64 / 256 under every tile option at
    every size, against density_restatement."""
    rt = sar.Runtime(sar.Config.solar_sail(width=FILTER_ORDER[0][0], height=FILTER_ORDER[0][1]))
    for i, size in enumerate(FILTER_ORDER):
        if i:
            rt.set_width_height(*size)
        for S in K.DENSITY_SAMPLES:
            k = K.density_state(size, S)
            want_c, want_s, want_m, want_stats = K.density_reference(size, S)
            for tile in K.DENSITY_TILES:
                what = f"{size} samples {S} tile {tile}"
                rt.set_option("density_tile", tile)
                rt.load(k.count, k.steps, k.zbuf, k.max)
                stats = rt.density_filter(samples=S)
                assert stats == want_stats, f"{what}: stats {stats} vs {want_stats}"
                np.testing.assert_array_equal(rt.count(), want_c, err_msg=what)
                np.testing.assert_array_equal(_bits(rt.steps()), _bits(want_s), err_msg=what)
                assert rt.max() == want_m, what
                np.testing.assert_array_equal(_bits(rt.zbuf()), _bits(k.zbuf), err_msg=f"{what}: zbuf changed")
                tiles, copied = rt.density_tiles()
                assert tiles == -(-size[0] // 32) * -(-size[1] // tile) and 0 <= copied <= tiles, what
    rt.close()


def test_shade_at_every_size_of_a_shrink_then_grow_order(sar, gpu):
    """sar_shade with and without the smoothing, ao_radius 0 and 6, at every size, against shade_restatement; the buffers are only read."""
    rt = sar.Runtime(sar.Config.solar_sail(width=FILTER_ORDER[0][0], height=FILTER_ORDER[0][1]))
    for i, size in enumerate(FILTER_ORDER):
        if i:
            rt.set_width_height(*size)
        k, cfg = K.shade_state(size), sar.Config.solar_sail(**K.shade_config(size))
        rt.load(k.count, k.steps, k.zbuf, k.max)
        before = (rt.count(), _bits(rt.steps()), _bits(rt.zbuf()), rt.max())
        for combo in K.SHADE_COMBOS:
            want, want_stats = K.shade_reference(size, combo["ao_radius"], combo["smooth"])
            img, stats = rt.shade(cfg, stats=True, **combo)
            assert stats == want_stats, f"{size} {combo}: stats {stats} vs {want_stats}"
            np.testing.assert_array_equal(img, want, err_msg=f"{size} {combo}")
            np.testing.assert_array_equal(sar.shade(cfg, rt, **combo), want, err_msg=f"{size} {combo}: without statistics")
        after = (rt.count(), _bits(rt.steps()), _bits(rt.zbuf()), rt.max())
        assert all(np.array_equal(x, y) for x, y in zip(before, after)), f"{size}: shade changed the buffers"
    rt.close()


# ---- 7. load, read-backs, merge ----------------------------------------------------------------------------------------------------
@ORDERS
def test_load_read_backs_and_merge_after_a_resize(sar, gpu, order):
    steps = K.render_steps(K.ORDERS[order])
    rt = sar.Runtime(_cfg(sar, steps[0][1][0][0]))
    previous = None
    for i, (size, groups) in enumerate(steps):
        a, c = groups[0], groups[2]
        if i:
            rt.set_width_height(*size)
            assert_reset(rt, size, f"{order}: after the resize to {size}")
        st = K.rendered(*c)
        rt.load(st.count, st.steps, st.zbuf, st.max)                      # sar_runtime_load, then the read-backs: a round trip
        assert_state(rt, st, f"{order} {size}: load round trip")
        rt.reset()
        assert_reset(rt, size, f"{order} {size}: reset after a load")
        _render(sar, rt, a[0])
        other = sar.Runtime(_cfg(sar, c[0]))
        _render(sar, other, c[0])
        rt.merge(other)
        assert_state(rt, K.merged(a, c), f"{order} {size}: merge with a fresh runtime")
        other.merge(rt)                                                   # and the resized runtime as the source
        assert_state(other, K.merge_states(K.rendered(*c), K.merged(a, c)), f"{order} {size}: merged into a fresh runtime")
        if previous is not None:
            with pytest.raises(sar.SarError) as e:
                rt.merge(previous)
            assert e.value.status == 2                                    # SAR_ERR_DIM_MISMATCH
            with pytest.raises(sar.SarError) as e:
                previous.merge(rt)
            assert e.value.status == 2
            assert_state(rt, K.merged(a, c), f"{order} {size}: after the refused merges")
            previous.close()
        previous = other
    previous.close()
    rt.close()


# ---- 8. timing across a resize -----------------------------------------------------------------------------------------------------
@ORDERS
def test_timing_after_a_resize_reports_that_call_only(sar, gpu, order):
    steps = K.render_steps(K.ORDERS[order])
    rt = sar.Runtime(_cfg(sar, steps[0][1][0][0]))
    rt.enable_timing(True)
    for i, (size, groups) in enumerate(steps):
        a, b = groups[1]
        if i:
            rt.set_width_height(*size)
        _render(sar, rt, a)
        _render(sar, rt, b)
        t = rt.last_timing()
        assert t.iterate_launches == 1 and t.iterations_counted == b.jobs * b.n, f"{order} {size}: {t}"
        assert len(rt.debug_spans(0)) == 1 and t.iterate_ms >= 0.0
        assert_state(rt, K.rendered(a, b), f"{order} {size}: with timing on")
    rt.close()


# ---- 9. the multi-device renderer at changing sizes -----------------------------------------------------------------------------
@PAIRS
@pytest.mark.parametrize("devices,exchange", [(None, 0), ([0, 0, 0], 0), ([0, 0, 0], 1), ([0, 0, 0], 2)])
def test_parallel_renderer_at_sizes_a_b_a(sar, gpu, pair, devices, exchange):
    """sar_render_parallel resizes every shard in every call (ensure_shard): three calls at sizes A, B, A on one renderer — one device,
    and one device listed as three shards under each exchange mode. Image and gathered runtime() state after every call against the
    oracle: start points continue across the calls, jobs sharded like the devices, folded in rank order."""
    r = K.RENDERER
    a, b = K.PAIRS[pair]
    if devices is None:
        pr = sar.ParallelRenderer(device=0, units=r["units"], seed=r["seed"])
    else:
        pr = sar.ParallelRenderer(devices=devices, units=r["units"], seed=r["seed"])
        pr.set_exchange(exchange)
    ndev = 1 if devices is None else len(devices)
    assert pr.num_devices() == ndev and pr.num_threads() == r["units"]
    refs = K.renderer_references(pair, ndev)
    for call, size in enumerate((a, b, a)):
        oc = K.renderer_config(size)
        img = sar.render_parallel(pr, _cfg(sar, oc), r["jobs_per_unit"])
        what = f"{pair} x{ndev} exchange {exchange}: call {call} at {size}"
        np.testing.assert_array_equal(img, O.colorize(oc, K.oracle_runtime(refs[call])), err_msg=what)
        rm = pr.runtime()
        assert rm.dims() == size, what
        assert_state(rm, refs[call], what)
    pr.shutdown()
