"""GPU: box counting (sar_runtime_boxes, sar_runtime_boxdim, include/sar.h) — all four sums of every level against the numpy
restatement bit for bit at every wave and workgroup boundary with planted edge cases, lattices against their closed forms, nearly
full hash tables, independence of the launch, maps against the restatement (rows, records, cubes, points), no side effect on the
runtime, the Henon map's D0, D1 and D2 against the published values, and the way up from search records."""
import math

import numpy as np
import pytest

import box_cases as K
import box_restatement as B
from corr_cases import henon
from orbit_cases import logistic

pytestmark = pytest.mark.gpu

MAPS_SHAPE = dict(jobs=70, samples=8, stride=3, transient=200)     # 70 jobs: a partial second wave (the corr tests' shape)
HENON_SHAPE = dict(jobs=64, samples=1024, stride=1)                 # 65 536 points


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=48, height=40), device=0)
    yield r
    r.close()


def _coeffs(cfg):
    return np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])


@pytest.fixture(scope="module")
def four_maps(sar):
    """The two presets (solar-sail loses some of these start points to infinity: DIVERGED, with a failing job that is not the first),
    Henon, and the logistic map at r = 4.4, which leaves for infinity from every start point."""
    return np.stack([_coeffs(sar.Config.poisson_saturne()), _coeffs(sar.Config.solar_sail()), henon(), logistic(4.4, 4.4)[0]])


@pytest.fixture(scope="module")
def maps_reference(sar, four_maps):
    """The restatement of the four maps at MAPS_SHAPE, computed once and left unchanged."""
    starts = sar.start_points(0, 0, MAPS_SHAPE["jobs"])
    return [B.boxdim(c, starts, MAPS_SHAPE["samples"], MAPS_SHAPE["stride"], MAPS_SHAPE["transient"], l_min=1, min_occupancy=2.0)
            for c in four_maps]


@pytest.fixture(scope="module")
def maps_result(sar, rt, four_maps):
    return sar.box_dimension(rt, four_maps, points=True, l_min=1, min_occupancy=2.0, **MAPS_SHAPE)


def _same_rows(got, want, what):
    assert got.dtype == B.LEVEL_DTYPE and got.shape == want.shape, what
    for f in B.LEVEL_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (what, f, got[f], want[f])


# 1 and 2: a lone point, a pair; 63 / 64 / 65: the wave; 255 / 256 / 257: the workgroup; 700: three workgroups, the last one partial
@pytest.mark.parametrize("levels", [1, 5, 16])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 700])
def test_sets_equal_the_restatement(sar, rt, n, levels):
    for cube in ((K.CUBE_EXACT, K.CUBE_ROUNDED) if levels == 16 else (K.CUBE_ROUNDED,) if levels == 5 else (K.CUBE_EXACT,)):
        pts = K.planted_sets(n, cube)
        rows = sar.box_counts(rt, pts, origin=cube[0], size=cube[1], levels=levels)
        assert rows.shape == (3, levels + 1)
        for s in range(3):
            _same_rows(rows[s], B.level_rows(pts[s], cube[0], cube[1], levels), (n, levels, s))
            assert np.all(rows[s]["cells"] <= n) and np.all(np.diff(rows[s]["cells"].astype(np.int64)) >= 0)
        assert np.all(rows[1]["cells"] == 1) and np.all(rows[1]["sum_sq"] == n * n) and np.all(rows[1]["n_log_n"] == n * B.lg32(n))
        if n >= 2:
            assert rows[2]["cells"][levels] == 2 and rows[2]["sum_sq"][levels] == (n // 2) ** 2 + (n - n // 2) ** 2
        one = sar.box_counts(rt, pts[0], origin=cube[0], size=cube[1], levels=levels)     # (n, 3): one set
        assert one.shape == (levels + 1,) and one.tobytes() == rows[0].tobytes()


def test_lattices_against_their_closed_forms(sar, rt):
    rows = sar.box_counts(rt, K.cube_lattice(), levels=6)
    for l in range(7):
        assert tuple(int(v) for v in rows[l]) == K.cube_lattice_row(l), l
    n = 300
    rows = sar.box_counts(rt, K.line_lattice(n))
    for l in range(11):
        assert int(rows[l]["cells"]) == -(-n // 2 ** (10 - l)), l
    assert np.all(rows["cells"][10:] == n) and np.all(rows["singles"][10:] == n) and np.all(rows["n_log_n"][10:] == 0)


def test_nearly_full_tables(sar, rt):
    full, most = K.distinct_cells(1023), K.planted_sets(700)[0]
    want_full, want_most = B.level_rows(full), B.level_rows(most, *K.CUBE_EXACT)
    assert want_full["cells"][16] == 1023 and want_full["singles"][16] == 1023
    base_full = sar.box_counts(rt, full)
    base_most = sar.box_counts(rt, most, origin=K.CUBE_EXACT[0], size=K.CUBE_EXACT[1])
    try:
        rt.set_option("box_slots", 1024)                       # one free slot in 1024: probe sequences as long as they get
        _same_rows(sar.box_counts(rt, full), want_full, "1023 of 1024")
        _same_rows(sar.box_counts(rt, most, origin=K.CUBE_EXACT[0], size=K.CUBE_EXACT[1]), want_most, "700 of 1024")
        with pytest.raises(sar.SarError):                      # 1024 points need more than 1024 slots
            sar.box_counts(rt, np.concatenate([full, full[:1]]))
        rt.set_option("box_slots", 512)
        with pytest.raises(sar.SarError):
            sar.box_counts(rt, most)
        assert "box_slots" in sar.load_library().sar_last_error().decode()
        for bad in (1000, 1, 3, 2 ** 25):
            with pytest.raises(sar.SarError):
                rt.set_option("box_slots", bad)
        rt.set_option("box_slots", 2 ** 14)                    # a sparse table
        _same_rows(sar.box_counts(rt, full), want_full, "1023 of 16384")
    finally:
        rt.set_option("box_slots", 0)
    _same_rows(base_full, want_full, "default")
    _same_rows(base_most, want_most, "default")


def test_results_do_not_depend_on_the_launch(sar, rt, four_maps, maps_result):
    pts = np.concatenate([K.planted_sets(700), K.planted_sets(700, seed=77)[:2]])     # five sets
    base = sar.box_counts(rt, pts, origin=K.CUBE_EXACT[0], size=K.CUBE_EXACT[1])
    try:
        for chunk, groups5, groups4 in ((1, 5, 4), (2, 3, 2), (0, 1, 1)):
            rt.set_option("box_chunk", chunk)
            rt.enable_timing(True)
            rows = sar.box_counts(rt, pts, origin=K.CUBE_EXACT[0], size=K.CUBE_EXACT[1])
            t = rt.last_timing()
            assert t.iterate_launches == 17 * groups5 and t.iterate_ms > 0, chunk     # k_box_insert and 16 k_box_level per launch group
            assert rows.tobytes() == base.tobytes(), chunk
            res = sar.box_dimension(rt, four_maps, points=True, l_min=1, min_occupancy=2.0, **MAPS_SHAPE)
            t = rt.last_timing()
            rt.enable_timing(False)
            assert t.warmup_ms > 0 and t.iterate_ms > 0 and t.iterate_launches == 17 * groups4, chunk
            assert res.levels.tobytes() == maps_result.levels.tobytes() and res.records.tobytes() == maps_result.records.tobytes(), chunk
            assert np.array_equal(res.points.view(np.uint64), maps_result.points.view(np.uint64)), chunk
    finally:
        rt.set_option("box_chunk", 0)
        rt.enable_timing(False)
    for k in range(4):                                         # one map per call
        one = sar.box_dimension(rt, four_maps[k], points=True, l_min=1, min_occupancy=2.0, **MAPS_SHAPE)
        assert one.levels[0].tobytes() == maps_result.levels[k].tobytes() and one.records[0].tobytes() == maps_result.records[k].tobytes(), k
        assert np.array_equal(one.points[0].view(np.uint64), maps_result.points[k].view(np.uint64))
    given = sar.box_dimension(rt, four_maps, starts=sar.start_points(0, 0, 70), l_min=1, min_occupancy=2.0, **MAPS_SHAPE)
    assert given.levels.tobytes() == maps_result.levels.tobytes() and given.points is None     # the caller's start points are the seed's
    with pytest.raises(sar.SarError):
        rt.set_option("box_chunk", 65536)


def _same_lines(got, want):
    assert (int(got["status"]), int(got["first_level"]), int(got["last_level"]), int(got["used"])) == \
        (want["status"], want["first_level"], want["last_level"], want["used"])
    for d in ("d0", "d1", "d2"):
        for f in ("slope", "intercept", "rms"):
            if math.isnan(want[d][f]):
                assert math.isnan(got[d][f]), (d, f)
            else:
                assert abs(got[d][f] - want[d][f]) <= 1e-9 * max(abs(want[d][f]), 1.0), (d, f)     # (tests/test_box_host.py)


def _same_record(rec, want):
    assert int(rec["status"]) == want["status"]
    assert (int(rec["fail_job"]), int(rec["fail_step"])) == (want["fail_job"], want["fail_step"])
    assert np.array_equal(rec["extent"], want["extent"])       # by value: -0.0 == 0.0
    if want["status"] == B.DIVERGED:
        assert np.all(np.isnan(rec["origin"])) and math.isnan(rec["size"])
    else:
        assert np.array_equal(rec["origin"], want["origin"]) and rec["size"] == want["size"]
    _same_lines(rec["lines"], want["lines"])


def test_maps_equal_the_restatement(sar, rt, maps_result, maps_reference):
    res = maps_result
    assert res.levels.shape == (4, 17) and res.points.shape == (4, 560, 3) and res.n == 560
    assert [w["status"] for w in maps_reference] == [B.BOUNDED, B.DIVERGED, B.BOUNDED, B.DIVERGED]
    assert maps_reference[1]["fail_job"] > 0 and maps_reference[3]["fail_job"] == 0
    for k, want in enumerate(maps_reference):
        _same_rows(res.levels[k], want["levels"], k)
        _same_record(res.records[k], want)
        assert np.array_equal(res.points[k].view(np.uint64), want["points"].view(np.uint64)), k
    for k in (1, 3):                                           # DIVERGED: all zero, no window
        assert not res.levels[k].view(np.uint64).any() and not res.points[k].any() and res.records["fail_step"][k] > 0
        assert res.records["lines"]["status"][k] == sar.SAR_BOXDIM_NO_WINDOW and math.isnan(res.d0[k]) and math.isnan(res.d1[k]) and math.isnan(res.d2[k])
        assert np.all(np.isnan(res.epsilon(k)))
    assert np.array_equal(res.status, [0, sar.SAR_SEARCH_DIVERGED, 0, sar.SAR_SEARCH_DIVERGED])
    assert maps_reference[0]["lines"]["status"] == B.FIT_OK and np.isfinite(res.d0[0]) and np.isfinite(res.d1[0]) and np.isfinite(res.d2[0])
    # the returned points through sar_runtime_boxes with the record's cube: the same rows
    for k in (0, 2):
        again = sar.box_counts(rt, res.points[k], origin=res.records["origin"][k], size=res.records["size"][k])
        assert again.tobytes() == res.levels[k].tobytes(), k
        assert res.epsilon(k)[0] == res.records["size"][k] and res.epsilon(k)[16] == res.records["size"][k] * 2.0 ** -16
    # .fit refits on the host: the call's own window gives the record's lines, another window other lines
    for k in range(4):
        assert res.fit(k).tobytes() == res.records["lines"][k].tobytes(), k
    assert res.fit(0, l_min=0, min_occupancy=1.0)["used"] > res.records["lines"]["used"][0]
    assert res.fit(3, l_min=0, min_occupancy=1.0)["status"] == sar.SAR_BOXDIM_NO_WINDOW


def test_a_fixed_point_has_a_unit_cube(sar, rt):
    c = np.zeros(30)
    c[0], c[10], c[20] = 0.25, -0.5, 0.125                     # x' = 0.25, y' = -0.5, z' = 0.125 from everywhere
    res = sar.box_dimension(rt, c, jobs=70, samples=8, stride=1, transient=2)
    rec = res.records[0]
    assert rec["status"] == sar.SAR_SEARCH_BOUNDED and rec["size"] == 1.0 and rec["origin"].tolist() == [0.25, -0.5, 0.125]
    assert np.all(res.levels[0]["cells"] == 1) and np.all(res.levels[0]["sum_sq"] == 560 * 560) and np.all(res.levels[0]["singles"] == 0)
    assert np.all(res.levels[0]["n_log_n"] == 560 * B.lg32(560))
    assert rec["lines"]["status"] == sar.SAR_BOXDIM_FIT_OK and (rec["lines"]["first_level"], rec["lines"]["last_level"]) == (3, 16)
    assert abs(res.d0[0]) <= 1e-12 and abs(res.d1[0]) <= 1e-12 and abs(res.d2[0]) <= 1e-12     # constant rows: no slope
    _same_record(rec, B.boxdim(c, sar.start_points(0, 0, 70), 8, 1, 2))


def test_the_runtime_is_only_lent(sar, rt, four_maps):
    cfg = sar.Config.solar_sail(width=48, height=40, iterations=64 * 500, jobs_total=64, seed=3)
    rt.reset()
    rt.seed(9)
    sar.render_jobs(cfg, rt, sar.start_points(3, 0, 64))
    before = (rt.count().copy(), rt.steps().copy(), rt.zbuf().copy(), rt.max())
    assert before[0].any()
    sar.box_dimension(rt, four_maps, **MAPS_SHAPE)
    sar.box_counts(rt, K.planted_sets(65))
    assert np.array_equal(rt.count(), before[0]) and rt.max() == before[3]
    assert np.array_equal(rt.steps().view(np.uint64), before[1].view(np.uint64))
    assert np.array_equal(rt.zbuf().view(np.uint32), before[2].view(np.uint32))
    # the start-point stream: the next render draws what a runtime seeded alike and left alone draws
    other = sar.Runtime(cfg, device=0)
    other.seed(9)
    sar.render_jobs(cfg, other, sar.start_points(3, 0, 64))
    other.reset()
    rt.reset()
    sar.render_jobs(cfg, rt)
    sar.render_jobs(cfg, other)
    assert np.array_equal(rt.count(), other.count()) and rt.max() == other.max()
    other.close()
    rt.reset()


def test_henon_dimensions_lie_in_the_published_intervals(sar, rt):
    """x' = 1 - 1.4 x^2 + y, y' = 0.3 x (z' = 0.5 z): published D0 ~ 1.26, D1 ~ 1.26, D2 ~ 1.21-1.22 (Grassberger & Procaccia 1983;
    Russell, Hanson & Ott 1980; Sprott's tables). The restatement gives D0 1.2650, D1 1.2505, D2 1.2158 over levels 3..9 at this
    shape with the suite's start points (sar_start_points(0, 0, 64))."""
    res = sar.box_dimension(rt, henon(), **HENON_SHAPE)
    rec, rows, n = res.records[0], res.levels[0], 65536
    lines = rec["lines"]
    print("henon d0", res.d0[0], "d1", res.d1[0], "d2", res.d2[0], "window", lines["first_level"], lines["last_level"],
          "rms", lines["d0"]["rms"], lines["d1"]["rms"], lines["d2"]["rms"])
    want = B.boxdim(henon(), sar.start_points(0, 0, 64), 1024, 1, 1000)
    _same_rows(rows, want["levels"], "henon")
    _same_record(rec, want)
    assert rec["status"] == sar.SAR_SEARCH_BOUNDED and lines["status"] == sar.SAR_BOXDIM_FIT_OK and lines["used"] >= 5
    assert 1.20 <= res.d0[0] <= 1.32 and 1.20 <= res.d1[0] <= 1.32 and 1.15 <= res.d2[0] <= 1.28
    for l in range(17):                                        # the Renyi entropies are ordered; the slack is lg32's truncation
        y0, y1, y2 = B.entropies(rows, n, l)
        assert y0 >= y1 - 1e-8 >= y2 - 2e-8, l
    assert np.all(rows["cells"] <= n) and rows["cells"][0] == 1 and rows["sum_sq"][0] == n * n


def test_search_records_go_in_as_they_are(sar, rt):
    recs, _ = sar.search_attractors(rt, 4096, seed=1, transient=1000, steps=4000, keep_rejected=1)
    found = recs[recs["status"] == sar.SAR_SEARCH_BOUNDED][:8]
    assert found.size == 8
    shape = dict(jobs=4, samples=256, stride=1, transient=1000)
    starts = np.full((4, 3), 0.05) + np.arange(4)[:, None] * 1e-3
    res = sar.box_dimension(rt, found, search_seed=1, starts=starts, l_min=2, min_occupancy=4.0, **shape)
    assert np.array_equal(res.coeffs[0], sar.search_candidate(1, int(found["candidate"][0])).reshape(30))
    assert res.levels.shape == (8, 17)
    for k in range(8):
        want = B.boxdim(res.coeffs[k], starts, 256, 1, 1000, l_min=2, min_occupancy=4.0)
        _same_rows(res.levels[k], want["levels"], k)
        _same_record(res.records[k], want)
