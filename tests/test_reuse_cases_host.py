"""The conditions the journeys of tests/reuse_cases.py rely on, held with the oracle and the host entry points only: a journey that
renders nothing, sizes that are not what their names say, or a list the device module walks only in part would let
tests/test_gpu_runtime_reuse.py pass without testing what it is for."""
import numpy as np
import pytest

import reuse_cases as K


def test_every_render_reference_counts_visits_and_holds_depths():
    n = 0
    for what, st in K.all_render_references():
        assert int(st.count.sum(dtype=np.uint64)) > 0, f"{what}: nothing counted"
        assert (st.zbuf != np.float32(-1.0)).any(), f"{what}: no depth"
        n += 1
    assert n > 100


def test_frames_stay_within_the_limits_and_alternate_the_presets():
    seen = set()
    for order in K.ORDERS.values():
        for _, groups in K.render_steps(order):
            for g in groups:
                for f in g:
                    assert 1 <= f.jobs <= K.MAX_JOBS and 1 <= f.n <= K.MAX_ITERS and f.preset in ("solar_sail", "poisson_saturne")
                    seen.add(f.preset)
            assert {f.preset for g in groups for f in g} == {"solar_sail", "poisson_saturne"}   # the survivor share moves at every size
    for name in K.PAIRS:
        for groups in list(K.batch_frames(name).values()) + list(K.group_frames(name).values()):
            frames = [g[-1] for g in groups]
            assert len({(f.preset, f.jobs, f.n) for f in frames}) == 1, "the frames of a batch share preset and job shape"
            assert len({f.seed for f in frames}) == 3 and len({f.angle for f in frames}) == 3
            assert all(f.jobs <= K.MAX_JOBS and f.n <= K.MAX_ITERS for f in frames)
    assert seen == {"solar_sail", "poisson_saturne"}
    r = K.RENDERER
    assert r["units"] * r["jobs_per_unit"] <= K.MAX_JOBS and r["iterations"] // r["units"] // r["jobs_per_unit"] <= K.MAX_ITERS


def test_solar_sail_loses_jobs_in_the_warm_up_and_poisson_saturne_none():
    """Dead jobs only feed count[0, 0]: the share of jobs lost is what moves the survivor share between the steps."""
    size = (320, 200)
    sail, saturne = K.frame(size, 0), K.frame(size, 1)
    assert (sail.preset, saturne.preset) == ("solar_sail", "poisson_saturne")
    lost = int(K.rendered(sail).count[0, 0]) / sail.n
    assert 0.3 * sail.jobs < lost < 0.5 * sail.jobs
    assert int(K.rendered(saturne).count[0, 0]) < saturne.n


def test_equal_npix_sizes_have_equal_npix_and_other_shapes():
    assert len({K.npix(s) for s in K.EQUAL_NPIX}) == 1 and len(set(K.EQUAL_NPIX)) == 3
    assert all(s in K.SIZES for s in K.EQUAL_NPIX)
    assert K.npix((97, 53)) % 4 == 1
    assert max(K.SIZES, key=K.npix) == (320, 200) and min(K.SIZES, key=K.npix) == (1, 1)
    assert K.npix((320, 200)) // 2048 >= 2 * K.GEOMETRY[(320, 200)][0]           # more than one 2048-pixel segment per bin


@pytest.mark.parametrize("size", list(K.SIZES))
def test_bin_geometry_is_what_the_docstring_claims(sar, size):
    g = sar.bin_geometry(*size)
    assert g["ok"] == 1
    assert (g["bins"], g["bin_shift"], g["interleaved"]) == K.GEOMETRY[size]
    assert g["seg_shift"] == 11                                                   # segments of 2048 pixels


def test_sizes_named_tiled_satisfy_the_rule_and_the_others_do_not():
    for size, tiled in K.SIZES.items():
        w, h = size
        rule = w >= 8 and (w & (w - 1)) == 0 and h % 8 == 0                       # a power-of-two width, a height in blocks of eight rows
        assert rule == tiled == K.is_tiled(size), size
    assert K.SIZES[(256, 64)] and K.SIZES[(128, 48)] and not K.SIZES[(96, 64)]
    # the equal-npix sizes hold both layouts: identically sized hint arrays under another addressing
    assert {K.SIZES[s] for s in K.EQUAL_NPIX} == {True, False}


@pytest.mark.parametrize("name", list(K.ORDERS))
def test_every_order_shrinks_grows_and_changes_shape_at_equal_npix(name):
    order = K.ORDERS[name]
    assert all(s in K.SIZES for s in order)
    assert K.transitions(order) >= {"shrink", "grow", "equal_npix", "to_1x1", "from_1x1", "back_to_first", "other_hint_layout"}
    assert all(a != b for a, b in zip(order, order[1:])), "a resize to the same size returns early"


def test_orders_begin_in_both_hint_layouts_and_visit_every_size():
    assert {K.is_tiled(o[0]) for o in K.ORDERS.values()} == {True, False}
    assert {s for o in K.ORDERS.values() for s in o} == set(K.SIZES)


def test_pair_journeys_are_what_their_names_say():
    a, b = K.PAIRS["smaller"]
    assert K.npix(b) < K.npix(a)
    a, b = K.PAIRS["larger"]
    assert K.npix(b) > K.npix(a)
    a, b = K.PAIRS["same_npix"]
    assert K.npix(b) == K.npix(a) and a != b and K.is_tiled(a) != K.is_tiled(b)
    assert all(s in K.SIZES for p in K.PAIRS.values() for s in p)


def test_filter_order_shrinks_grows_and_uses_the_shared_cases():
    import density_cases as DK
    import shade_cases as SK
    assert K.transitions(K.FILTER_ORDER) >= {"shrink", "grow", "equal_npix", "to_1x1", "from_1x1"}
    for size in ((96, 80), (1, 1)):
        assert size in K.FILTER_ORDER and size in DK.SIZES and size in SK.SIZES
        for S in K.DENSITY_SAMPLES:
            assert K.density_state(size, S).count is DK.case(f"sparse_random-{size[0]}x{size[1]}-S{S}").count
        assert K.shade_state(size).zbuf is SK.case(f"random-{size[0]}x{size[1]}-R8-s1").zbuf
    for size in K.FILTER_ORDER:
        if K.npix(size) > 1:
            assert K.density_reference(size, 64)[3]["spread"] > 0, f"{size}: the density filter has nothing to spread"
            assert K.shade_reference(size, 6, 1)[1]["surface"] > 0, f"{size}: nothing to shade"


def test_renderer_references_differ_from_call_to_call():
    """The start points continue across the calls: the third call, at the first call's size, is another frame."""
    for name in K.PAIRS:
        for ndev in (1, 3):
            first, second, third = K.renderer_references(name, ndev)
            assert first.count.shape == third.count.shape == K.PAIRS[name][0][::-1] and second.count.shape == K.PAIRS[name][1][::-1]
            assert not np.array_equal(first.count, third.count)
    jobs = K.RENDERER["units"] * K.RENDERER["jobs_per_unit"]
    from strange_attractor_renderer_amd.distributed import shard_jobs
    for world in (1, 3):
        assert [K.shard_jobs(jobs, world, r) for r in range(world)] == [tuple(shard_jobs(jobs, world, r)) for r in range(world)]


def test_the_device_module_walks_the_whole_list():
    """No journey is skipped or filtered out: what tests/test_gpu_runtime_reuse.py parametrises over is the list itself."""
    import test_gpu_runtime_reuse as G
    assert G.ORDER_NAMES == list(K.ORDERS) and G.PAIR_NAMES == list(K.PAIRS)
    assert G.FILTER_ORDER is K.FILTER_ORDER
    marks = {}
    for name in dir(G):
        fn = getattr(G, name)
        if name.startswith("test_") and callable(fn):
            for m in getattr(fn, "pytestmark", []):
                assert m.name not in ("skip", "skipif", "xfail"), f"{name} is marked {m.name}"
                if m.name == "parametrize":
                    marks.setdefault(name, []).append(m.args)
    by_order = [n for n, ms in marks.items() if any(a[0] == "order" and list(a[1]) == G.ORDER_NAMES for a in ms)]
    by_pair = [n for n, ms in marks.items() if any(a[0] == "pair" and list(a[1]) == G.PAIR_NAMES for a in ms)]
    assert len(by_order) >= 6 and len(by_pair) >= 3, (by_order, by_pair)
    for n, ms in marks.items():
        for a in ms:
            if a[0] == "order":
                assert list(a[1]) == G.ORDER_NAMES, f"{n} walks only {a[1]}"
            if a[0] == "pair":
                assert list(a[1]) == G.PAIR_NAMES, f"{n} walks only {a[1]}"
