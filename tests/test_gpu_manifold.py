"""GPU: the unstable-manifold family (sar_runtime_manifold, include/sar.h) — `count`, `first` and every field of the records against the
numpy restatement bit for bit on the cases of tests/manifold_cases.py (2 / 63 / 64 / 65 / 127 / 4096 samples, where a wave's seam
sits; 0 / 1 / 32 steps; 1 and 3 branches with two equal ones; period 1 and 2; max_span 1 and 4096; 1 x 1, 64 x 48, 67 x 45 and
128 x 96 images; a rotated view; -0.0 coefficients; a DOMAIN_ESCAPED branch among good ones; points that die midway; endpoints that
are far); what is known of those cases; a second call at another size; no side effect on the runtime's image buffers; the timing
fields; and manifold_branches -> manifolds -> overlay on a rendered Henon frame."""
import numpy as np
import pytest

import manifold_cases as K
import manifold_restatement as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=64, height=64), device=0)
    yield r
    r.close()


def _run(sar, rt, name):
    case = K.CASES[name]
    return sar.manifolds(rt, K.config_of(sar, case["view"]), R.branches_array(case["branches"]), **K.parameters(case))


def _same(got, want):
    count, first, records = want
    assert got.count.dtype == np.uint32 and got.first.dtype == np.uint32 and got.count.shape == count.shape == got.first.shape
    assert len(got.records) == len(records)
    for f in R.RECORD_DTYPE.names:
        if f in ("a", "b"):
            assert np.array_equal(got.records[f].view(np.uint64), records[f].view(np.uint64)), f
        else:
            assert got.records[f].tolist() == records[f].tolist(), f
    assert got.records.tobytes() == records.tobytes()
    assert np.array_equal(got.count, count), (int((got.count != count).sum()), np.argwhere(got.count != count)[:4].tolist())
    assert np.array_equal(got.first, first), (int((got.first != first).sum()), np.argwhere(got.first != first)[:4].tolist())


# ---- 1. parity, case by case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_case_equals_the_restatement(sar, rt, name):
    _same(_run(sar, rt, name), K.reference(name))


# ---- 2. what is known of the cases, on the device's own results ------------------------------------------------------------------
def test_known_cases(sar, rt):
    for s in (2, 63, 64, 65, 127):       # every segment is classified once per step, the seam's two included
        r = _run(sar, rt, f"samples_{s}").records[0]
        assert int(r["n_drawn"]) + int(r["n_long"]) + int(r["n_dead"]) + int(r["n_far"]) == (s - 1) * 33 and int(r["alive_end"]) == s
    m = _run(sar, rt, "steps_0")         # delta 1e-6: the whole domain sits in one pixel, every segment plots it once
    assert int(m.count.max()) == 126 == int(m.count.sum()) and int(m.records["length_px"][0]) == 0
    assert int(_run(sar, rt, "image_1x1").count[0, 0]) == int(K.reference("image_1x1")[2]["pixels"][0])
    m = _run(sar, rt, "branches_3_two_equal")
    assert m.records[0:1].tobytes() == m.records[1:2].tobytes() and not (m.branch == 1).any() and (m.branch == 0).any() and (m.branch == 2).any()
    assert np.array_equal(m.count > 0, ~m.age.mask) and int(m.age.max()) <= 32 and m.branch.max() <= 2
    m = _run(sar, rt, "domain_escaped_among_good")
    r = m.records[1]
    assert r["status"] == sar.SAR_MANIFOLD_DOMAIN_ESCAPED and not (m.branch == 1).any() and r["first_long_step"] == sar.MANIFOLD_NONE
    assert [int(r[f]) for f in ("n_drawn", "n_dead", "n_far", "n_long", "pixels", "length_px", "alive_end")] == [0] * 7
    assert tuple(r["a"]) == (50.0 + 1e-3 * 1.0, 0.0, 0.0) and abs(r["b"][0]) > 1e6
    m = _run(sar, rt, "dies_midway")
    assert int(m.records["n_dead"][0]) > 0 and int(m.records["alive_end"][0]) == 0 and int(m.records["n_dead"][1]) == 0
    m = _run(sar, rt, "far_endpoints")
    assert int(m.records["n_far"].min()) > 0 and int(m.count.sum()) == 0 and int(m.records["length_px"][0]) > 4096
    assert int(_run(sar, rt, "max_span_1").records["length_px"][0]) <= int(_run(sar, rt, "max_span_1").records["n_drawn"][0])


def test_henon_attractor_lies_inside_the_manifold(sar, rt):
    m = _run(sar, rt, "image_128x96")
    visited = K.attractor_pixels(K.HENON["view"])
    assert visited.size > 700 and int((m.count.reshape(-1)[visited] == 0).sum()) == 0


# ---- 3. a second call, the runtime's own state, the timing ----------------------------------------------------------------------
def test_second_call_at_another_size_on_the_same_runtime(sar, rt):
    for name in ("image_128x96", "image_1x1", "image_67x45", "samples_65", "image_128x96"):   # larger, smaller, larger again
        _same(_run(sar, rt, name), K.reference(name))


def test_render_and_colorize_are_the_same_before_and_after(sar, gpu):
    cfg = sar.Config.poisson_saturne(iterations=1024 * 200, width=64, height=64, jobs_total=1024, seed=5)
    r = sar.Runtime(cfg, device=0)
    try:
        sar.render_jobs(cfg, r)
        before = (r.count().tobytes(), r.steps().tobytes(), r.zbuf().tobytes(), r.max(), sar.colorize(cfg, r).tobytes())
        _same(_run(sar, r, "image_67x45"), K.reference("image_67x45"))     # not the runtime's size
        _same(_run(sar, r, "samples_64"), K.reference("samples_64"))
        after = (r.count().tobytes(), r.steps().tobytes(), r.zbuf().tobytes(), r.max(), sar.colorize(cfg, r).tobytes())
        assert before == after
    finally:
        r.close()


def test_timing_fields(sar, rt):
    rt.enable_timing(True)
    try:
        _run(sar, rt, "samples_4096")
        t = rt.last_timing()
        assert t.iterate_launches == 1 and t.iterate_ms > 0
    finally:
        rt.enable_timing(False)


def test_refusals_leave_the_runtime_usable(sar, rt):
    case = K.CASES["samples_65"]
    with pytest.raises(sar.SarError, match="samples must be 2 to 2\\^20"):
        sar.manifolds(rt, K.config_of(sar, case["view"]), R.branches_array(case["branches"]), samples=1)
    empty = sar.manifolds(rt, K.config_of(sar, case["view"]), np.zeros(0, dtype=sar.MANIFOLD_BRANCH_DTYPE))
    assert len(empty.records) == 0 and int(empty.count.sum()) == 0 and (empty.first == sar.MANIFOLD_NONE).all()
    _same(_run(sar, rt, "samples_65"), K.reference("samples_65"))
    rows = sar.manifolds(rt, K.config_of(sar, case["view"]), case["branches"], samples=65)      # rows instead of the array
    _same(rows, K.reference("samples_65"))


# ---- 4. cycles -> branches -> manifolds -> overlay ----------------------------------------------------------------------------------
def test_from_cycles_to_an_overlay_on_a_rendered_frame(sar, gpu):
    view = K.henon_view(128, 96)
    cfg = K.config_of(sar, view).replace(iterations=256 * 400, jobs_total=256, seed=3)
    r = sar.Runtime(cfg, device=0)
    try:
        sar.render_jobs(cfg, r)
        image = sar.colorize(cfg, r)
        kept = image.copy()
        cyc = sar.cycles(r, cfg, period=1)
        branches, index = sar.manifold_branches(cyc, delta=1e-6)
        # the two saddles: the left one's two sides with one step per return, the right one's single branch with two
        assert sorted(branches["period"].tolist()) == [1, 1, 2] and len(set(index.tolist())) == 2
        right = branches[branches["period"] == 2][0]
        assert np.allclose(right["base"], K.BASE_R, atol=1e-9) and np.allclose(right["dir"], K.DIR_R, atol=1e-6)
        m = sar.manifolds(r, cfg, branches)
        want = R.manifold(view, branches, **R.DEFAULTS)
        _same(m, want)
        colours = ((1, 2, 3, 65535), (65535, 4, 5, 6))
        out = m.overlay(image, colours=colours)
        assert np.array_equal(image, kept) and out is not image and out.shape == image.shape and out.dtype == np.uint16
        hit = m.count > 0
        assert hit.sum() > 500 and np.array_equal(out[~hit], image[~hit])
        assert all(tuple(out[y, x]) == colours[int(m.first[y, x] % 4096) % 2] for y, x in np.argwhere(hit))
        black = m.colorize(colours)
        assert np.array_equal(black[hit], out[hit]) and (black[~hit] == (0, 0, 0, 65535)).all()
        # the frame's own pixels lie on the manifold of the saddle inside the attractor
        visited = r.count() > 0
        assert visited.sum() > 300 and not (visited & ~hit).any()
        with pytest.raises(ValueError):
            m.overlay(image[:-1])
    finally:
        r.close()
