"""GPU: the cycles family (sar_runtime_cycles, include/sar.h) — every field of the records and of all `cap` orbit slots against the
numpy restatement bit for bit on the cases of tests/cycles_cases.py (the Henon map at p = 1 .. 7, the logistic map, the identity, the
quarter turns, a map without a root, the double root, a contraction, maps of the search stream, -0.0 coefficients, infinite and far
starts, 1 / 63 / 64 / 65 / 4096 starts, max_newton 0 and 1, merge 0 and wide, cap 1); what is known of those cases; several maps in one
call against one at a time; independence of "cycles_chunk"; a second call; no side effect on the image buffers; the Python
conveniences; and the cycles of an orbit diagram's columns with their overlay."""
import numpy as np
import pytest

import cycles_cases as K
import cycles_restatement as R
from orbit_cases import logistic as logistic_line
from search_restatement import next_point

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=64, height=64), device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def references():
    """The restatement of every case, computed on first use and left unchanged."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = K.reference(name)
        return cache[name]
    return get


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _run(sar, rt, name):
    coeffs, kw = K.CASES[name]
    return sar.cycles(rt, coeffs, **kw)


def _same(got, want):
    recs, slots = want
    assert len(got.records) == len(recs) and got._slots.shape == slots.shape
    for m, r in enumerate(recs):
        assert {f: int(got.records[f][m]) for f in R.RECORD_FIELDS} == r, m
    for f in ("period", "head", "hits", "newton"):
        assert np.array_equal(got._slots[f], slots[f]), f
    for f in ("rep", "residual", "M"):
        assert np.array_equal(_bits(got._slots[f]), _bits(slots[f])), f
    assert got._slots.tobytes() == slots.tobytes()


# ---- 1. parity, case by case -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.CASES))
def test_case_equals_the_restatement(sar, rt, references, name):
    _same(_run(sar, rt, name), references(name))


# ---- 2. what is known of the cases, on the device's own results ------------------------------------------------------------------
def test_henon_cycle_counts(sar, rt):
    for p, want in K.HENON_CYCLES.items():
        c = _run(sar, rt, f"henon_p{p}")
        assert int((c.orbits(0)["period"] == p).sum()) == want, p
    r = _run(sar, rt, "henon_p1").records[0]
    assert (int(r["converged"]), int(r["escaped"])) == (K.HENON_P1_COUNTS["converged"], K.HENON_P1_COUNTS["escaped"])


def test_known_cases(sar, rt):
    r = _run(sar, rt, "identity_cap16").records[0]
    assert [int(r[f]) for f in ("converged", "n_orbits", "orbits_lost", "hits_lost", "newton_iterations")] == [64, 16, 48, 48, 0]
    for name in ("rotation_half_p1", "rotation_half_p2"):
        c = _run(sar, rt, name)
        assert len(c.orbits(0)) == 1 and c.orbits(0)["hits"][0] == 512 and np.all(np.abs(c.orbits(0)["rep"]) <= 1e-12)
    assert int(_run(sar, rt, "rotation_half_p4").records["singular"][0]) == 512
    o = _run(sar, rt, "rotation_p4").orbits(0)
    on_axis = (o["rep"][:, 0] == 0) & (o["rep"][:, 1] == 0)
    assert np.all(o["newton"] == 0) and on_axis.sum() == 3 and np.all(o["period"][on_axis] == 1) and np.all(o["period"][~on_axis] == 4)
    r = _run(sar, rt, "no_root").records[0]
    assert int(r["converged"]) == int(r["singular"]) == 0 and int(r["escaped"]) + int(r["not_converged"]) == 512
    o = _run(sar, rt, "double_root").orbits(0)
    assert len(o) == 2 and o["rep"][0, 0] < 0 < o["rep"][1, 0]          # the documented limit: one double root, two heads
    c = _run(sar, rt, "affine")
    assert len(c.orbits(0)) == 1 and int(c.records["newton_iterations"][0]) == 512 and c.orbits(0)["newton"][0] == 1
    assert len(_run(sar, rt, "merge_wide").orbits(0)) == 3 and len(_run(sar, rt, "merge_0").orbits(0)) > 4
    c = _run(sar, rt, "cap_1")
    assert c._slots.shape == (1, 1) and int(c.records["orbits_lost"][0]) == 3
    r = _run(sar, rt, "max_newton_0").records[0]
    assert int(r["not_converged"]) == 512 and int(r["newton_iterations"]) == 0


def test_unused_slots_are_zero_and_starts_are_reported(sar, rt):
    c = _run(sar, rt, "henon_p2")
    n = int(c.records["n_orbits"][0])
    assert c._slots.shape == (1, 64) and c._slots[0, n:].tobytes() == bytes(120 * (64 - n))
    assert np.array_equal(_bits(c.starts), _bits(K.LATTICE)) and c.params.period == 2
    w = _run(sar, rt, "wild_starts")
    assert np.array_equal(_bits(w.starts), _bits(K.WILD_STARTS)) and w.params.jobs == len(K.WILD_STARTS)


# ---- 3. several maps, the launch shape, a second call -------------------------------------------------------------------------------
def test_several_maps_equal_the_maps_one_at_a_time(sar, rt):
    coeffs, kw = K.CASES["several_maps"]
    together = sar.cycles(rt, coeffs, **kw)
    for m, c30 in enumerate(coeffs):
        alone = sar.cycles(rt, c30, **kw)
        assert alone.records.tobytes() == together.records[m:m + 1].tobytes(), m
        assert alone._slots.tobytes() == together._slots[m:m + 1].tobytes(), m


def test_result_does_not_depend_on_the_chunk(sar, rt, references):
    base = _run(sar, rt, "several_maps")
    _same(base, references("several_maps"))
    try:
        for chunk, launches in ((512, 7), (1536, 3), (1, 7), (1 << 30, 1)):
            rt.set_option("cycles_chunk", chunk)
            rt.enable_timing(True)
            got = _run(sar, rt, "several_maps")
            t = rt.last_timing()
            assert got.records.tobytes() == base.records.tobytes() and got._slots.tobytes() == base._slots.tobytes(), chunk
            assert t.iterate_launches == launches and t.iterate_ms > 0 and t.resolve_ms > 0
        with pytest.raises(sar.SarError):
            rt.set_option("cycles_chunk", (1 << 30) + 1)
    finally:
        rt.set_option("cycles_chunk", 0)
        rt.enable_timing(False)
    again = _run(sar, rt, "several_maps")                    # a second call on the same runtime, after other shapes
    assert again.records.tobytes() == base.records.tobytes() and again._slots.tobytes() == base._slots.tobytes()
    _same(_run(sar, rt, "jobs_65"), references("jobs_65"))   # and a smaller one on buffers grown for a larger


def test_search_records_are_taken_as_maps(sar, rt, references):
    recs = np.zeros(4, dtype=sar.SEARCH_RECORD_DTYPE)
    recs["candidate"] = np.arange(100, 104)
    _same(sar.cycles(rt, recs, period=2, search_seed=7), references("search_p2"))


# ---- 4. no side effects ---------------------------------------------------------------------------------------------------------------
def test_render_and_colorize_are_the_same_before_and_after(sar, gpu):
    cfg = sar.Config.poisson_saturne(iterations=1024 * 200, width=64, height=64, jobs_total=1024, seed=5)
    r = sar.Runtime(cfg, device=0)
    try:
        sar.render_jobs(cfg, r)
        before = (r.count().tobytes(), r.steps().tobytes(), r.zbuf().tobytes(), r.max(), sar.colorize(cfg, r).tobytes())
        c = sar.cycles(r, cfg, period=2)
        after = (r.count().tobytes(), r.steps().tobytes(), r.zbuf().tobytes(), r.max(), sar.colorize(cfg, r).tobytes())
        assert before == after and int(c.records["converged"][0]) > 0
    finally:
        r.close()


# ---- 5. the Python conveniences ---------------------------------------------------------------------------------------------------------
def test_points_multipliers_and_kinds(sar, rt):
    c = _run(sar, rt, "henon_p2")
    o = c.orbits(0)
    assert [int(q) for q in o["period"]] == [1, 2, 1]
    pts = c.points(0, 1)
    assert pts.shape == (2, 3) and np.array_equal(_bits(pts[0]), _bits(o["rep"][1]))
    step = np.array([float(v) for v in next_point(R._rows(K.henon()), *pts[0])])
    assert np.array_equal(_bits(pts[1]), _bits(step)) and np.all(pts[0, :2] != pts[1, :2])
    lam = c.multipliers(0)
    assert lam.shape == (3, 3) and np.all(np.abs(lam[:, 0]) >= np.abs(lam[:, 1])) and np.all(np.abs(lam[:, 2]) <= 1e-12)
    for k in range(3):     # the multipliers are the roots of the characteristic polynomial of M
        tr, minors, det = sar.cycle_charpoly(o["M"][k])
        for z in lam[k]:
            assert abs(((z - tr) * z + minors) * z - det) <= 1e-9 * max(1.0, abs(z)) ** 3
    assert c.unstable_dim(0).tolist() == [1, 1, 1]           # at a = 1.4 both fixed points and the 2-cycle are saddles
    kinds = c.kind(0)
    assert [k[0] for k in kinds] == ["saddle-1"] * 3 and sorted(k[1] for k in kinds) == [False, True, True]
    sink = sar.cycles(rt, K.AFFINE)
    assert sink.kind(0) == [("sink", False)] and sink.unstable_dim(0).tolist() == [0]
    source = sar.cycles(rt, K._map(x1=2.0, y5=-3.0, z8=1.5))
    assert source.kind(0) == [("source", True)]


# ---- 6. the orbit diagram's columns --------------------------------------------------------------------------------------------------------
LINE = dict(r_range=(2.5, 3.4), width=16, doubling=3.0)
# 64 starts along x: past the doubling the unstable branch keeps only a sliver of the plain Newton iteration's basin at p = 2, and the
# 8 distinct x of the default lattice miss it between r = 3.04 and 3.22
LINE_STARTS = np.stack([-0.5 + 2.0 * (np.arange(64) + 0.5) / 64, np.full(64, 0.1), np.full(64, -0.1)], axis=1)


@pytest.fixture(scope="module")
def diagram(sar, rt):
    return sar.orbit_diagram(rt, *logistic_line(*LINE["r_range"]), width=LINE["width"], height=64, jobs=64, transient=500, steps=256,
                             v_range=(0.0, 1.0))


def test_orbit_diagram_cycles_along_the_logistic_line(sar, rt, diagram):
    w = LINE["width"]
    cs = np.stack([diagram.coeffs(c).reshape(30) for c in range(w)])
    for p in (1, 2):
        got = diagram.cycles(rt, period=p, starts=LINE_STARTS)
        assert len(got.records) == w
        _same(got, R.cycles(cs, LINE_STARTS, period=p))
    r = cs[:, 1]
    for c in range(w):
        o, unstable = got.orbits(c), got.unstable_dim(c)
        fixed = [k for k in range(len(o)) if o["period"][k] == 1 and abs(o["rep"][k, 0]) > 1e-6]
        assert len(fixed) == 1 and abs(o["rep"][fixed[0], 0] - (1.0 - 1.0 / r[c])) <= 1e-9     # the branch x* = 1 - 1/r besides 0
        zero = [k for k in range(len(o)) if o["period"][k] == 1 and abs(o["rep"][k, 0]) <= 1e-6]
        assert len(zero) == 1 and unstable[zero[0]] == 1
        two = [k for k in range(len(o)) if o["period"][k] == 2]
        if r[c] < LINE["doubling"]:
            assert unstable[fixed[0]] == 0 and two == []          # before the doubling: stable, and no 2-cycle
        else:
            assert unstable[fixed[0]] == 1 and got.kind(c)[fixed[0]] == ("saddle-1", True)   # past it: the same branch, unstable
            assert len(two) == 1 and unstable[two[0]] == 0        # plus a stable 2-cycle
            lo, hi = sorted(got.points(c, two[0])[:, 0])
            assert lo < 1.0 - 1.0 / r[c] < hi
    assert (r < LINE["doubling"]).sum() >= 4 and (r > LINE["doubling"]).sum() >= 4


def test_overlay_touches_only_the_pixels_the_host_arithmetic_names(sar, rt, diagram):
    cfg = sar.Config.poisson_saturne()
    image = diagram.colorize(cfg)
    kept = image.copy()
    got = diagram.cycles(rt, period=2, starts=LINE_STARTS)
    stable, unstable = (1, 2, 3, 65535), (65535, 4, 5, 6)
    out = diagram.overlay(image, got, stable=stable, unstable=unstable)
    assert np.array_equal(image, kept) and out is not image and out.shape == image.shape and out.dtype == np.uint16
    h, w = diagram.count.shape
    scale = np.float64(h) / (np.float64(1.0) - np.float64(0.0))
    want = {}
    for c in range(w):
        rows = R._rows(diagram.coeffs(c).reshape(30))
        dims = got.unstable_dim(c)
        for k, o in enumerate(got.orbits(c)):
            p = [np.float64(v) for v in o["rep"]]
            for _ in range(int(o["period"])):
                u = ((np.float64(1.0) * p[0] + np.float64(0.0) * p[1]) + np.float64(0.0) * p[2] - np.float64(0.0)) * scale
                if 0.0 <= u < h:
                    want[(h - 1 - int(u), c)] = stable if dims[k] == 0 else unstable
                p = next_point(rows, *p)
    # 1 - 1/r in every column at least (the root 0 comes back as -1e-15 or so in most: below the window, not drawn)
    assert len(want) >= w and {c for _, c in want} == set(range(w)) and set(want.values()) == {stable, unstable}
    changed = {(int(y), int(x)) for y, x in zip(*np.nonzero((out != image).any(axis=2)))}
    assert changed <= set(want) and all(tuple(out[y, x]) == v for (y, x), v in want.items())
    assert changed == {k for k in want if tuple(image[k]) != want[k]}
    with pytest.raises(ValueError):
        diagram.overlay(image[:-1], got)
