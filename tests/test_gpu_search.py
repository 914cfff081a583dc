"""GPU: the chaotic-map search (sar_runtime_search, include/sar.h) — the records against the numpy restatement bit for bit
(several seeds, boxes, start points, bounds and transients, the acceptance thresholds, candidate indices past 30 * index = 2^32
and near 2^40, chunk boundaries, supplied against generated coefficients), analytic maps, non-normal affine maps and the sum
rule against the exact references of tests/lyapunov_reference.py, the presets cross-checked against sar_runtime_extent,
determinism across runs, splits and chunks, and the path from a found candidate to a framed render."""
import ctypes as C
import math

import numpy as np
import pytest

import lyapunov_reference as L
import search_restatement as R

pytestmark = pytest.mark.gpu

NOLIMIT = dict(min_lyapunov=-math.inf, min_ky_dim=-math.inf, keep_rejected=1)


@pytest.fixture(scope="module")
def rt(sar, gpu):
    r = sar.Runtime(sar.Config.solar_sail(width=64, height=64), device=0)
    yield r
    r.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_parity_with_the_restatement(sar, rt):
    n, transient, steps = 4096, 1000, 4000
    recs, stats = sar.search_attractors(rt, n, first=0, seed=1, transient=transient, steps=steps, **NOLIMIT)
    want, wstats = R.search(1, 0, n, transient=transient, steps=steps, min_lyapunov=-math.inf, min_ky_dim=-math.inf,
                            keep_rejected=True)
    assert list(recs["candidate"]) == [r["candidate"] for r in want]
    assert len(want) > 20
    assert np.array_equal(recs["status"], [r["status"] for r in want])
    assert np.array_equal(recs["steps_done"], [r["steps_done"] for r in want])
    assert np.array_equal(recs["log2_exp"], np.array([r["log2_exp"] for r in want]))
    assert np.array_equal(_bits(recs["mant"]), _bits(np.array([r["mant"] for r in want])))
    assert np.array_equal(_bits(recs["extent"]), _bits(np.array([r["extent"] for r in want])))
    lam = np.array([r["lyapunov"] for r in want])
    both_nan = np.isnan(recs["lyapunov"]) & np.isnan(lam)          # records without a folded step
    assert np.all(both_nan | (np.abs(recs["lyapunov"] - lam) <= 1e-15))
    assert np.allclose(recs["ky_dim"], [r["ky_dim"] for r in want], rtol=0, atol=1e-12, equal_nan=True)
    assert {k: stats[k] for k in wstats} == wstats and stats["records"] == len(want)


def _given(rows):
    c = np.zeros((len(rows), 3, 10))
    for i, (x, y, z) in enumerate(rows):
        c[i, 0], c[i, 1], c[i, 2] = x, y, z
    return c.reshape(len(rows), 30)


def _diag(a, b, c):
    x, y, z = np.zeros(10), np.zeros(10), np.zeros(10)
    x[1], y[5], z[8] = a, b, c
    return x, y, z


def test_analytic_maps(sar, rt):
    diags = [(0.5, -0.25, 0.9), (-0.7, 0.3, 0.1), (0.99, 0.98, -0.97)]
    zero = (np.zeros(10),) * 3
    coeffs = _given([_diag(*d) for d in diags] + [zero])
    recs, stats = sar.search_attractors(rt, len(coeffs), first=100, coeffs=coeffs, transient=1000, steps=5000, **NOLIMIT)
    assert list(recs["candidate"]) == [100, 101, 102, 103]
    for r, d in zip(recs[:3], diags):
        assert r["status"] == sar.SAR_SEARCH_BOUNDED and r["steps_done"] == 5000
        want = sorted((math.log(abs(v)) for v in d), reverse=True)
        assert np.max(np.abs(r["lyapunov"] - want)) < 1e-12, (r["lyapunov"], want)
    assert recs[3]["status"] == sar.SAR_SEARCH_DEGENERATE and recs[3]["steps_done"] == 1
    assert np.all(np.isnan(recs[3]["lyapunov"])) and np.isnan(recs[3]["ky_dim"])   # no folded step: no exponents, no dimension
    assert stats["degenerate"] == 1 and stats["accepted"] == 3
    # steps = 0: BOUNDED without a folded step -> NaN, never accepted
    recs, stats = sar.search_attractors(rt, 1, coeffs=coeffs[:1], transient=10, steps=0, **NOLIMIT)
    assert recs[0]["status"] == sar.SAR_SEARCH_BOUNDED and recs[0]["steps_done"] == 0 and np.isnan(recs[0]["ky_dim"])
    assert stats["below_lyapunov"] == 1 and stats["accepted"] == 0

    # x' = 2x + 1, y' = 0.5 y, z' = 0.5 z leaves the bound box at the step a plain loop predicts
    x, y, z = np.zeros(10), np.zeros(10), np.zeros(10)
    x[0], x[1], y[5], z[8] = 1.0, 2.0, 0.5, 0.5
    start, bound = (0.05, 0.05, 0.05), 1e6
    px, t = start[0], 0
    while abs(px) <= bound:
        px, t = 2.0 * px + 1.0, t + 1
    grow = _given([(x, y, z)])
    recs, stats = sar.search_attractors(rt, 1, coeffs=grow, transient=0, steps=1000, start=start, bound=bound, **NOLIMIT)
    assert len(recs) == 1 and recs[0]["status"] == sar.SAR_SEARCH_DIVERGED and recs[0]["steps_done"] == t
    assert stats["diverged_late"] == 1 and stats["diverged_transient"] == 0
    recs, stats = sar.search_attractors(rt, 1, coeffs=grow, transient=1000, steps=1000, start=start, bound=bound, **NOLIMIT)
    assert len(recs) == 0 and stats["diverged_transient"] == 1 and stats["tested"] == 1
    # the same map with zero y / z rows is DEGENERATE at its first step instead
    recs, _ = sar.search_attractors(rt, 1, coeffs=_given([(x, np.zeros(10), np.zeros(10))]), transient=0, steps=1000, **NOLIMIT)
    assert recs[0]["status"] == sar.SAR_SEARCH_DEGENERATE and recs[0]["steps_done"] == 1


@pytest.mark.parametrize("preset", ["poisson_saturne", "solar_sail"])
def test_presets_are_chaotic_and_their_extent_is_k_extents(sar, rt, preset):
    cfg = getattr(sar.Config, preset)()
    coeffs = np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])[None, :]
    start, steps = (0.05, 0.05, 0.05), 20000
    alive, *_ = R.screen(0.0 + 1.0 * coeffs, start, 1000 + steps, 1e6)
    assert alive[0], "the restatement says this start point leaves the preset's basin"
    recs, stats = sar.search_attractors(rt, 1, coeffs=coeffs, start=start, transient=1000, steps=steps, keep_rejected=1)
    assert stats["accepted"] == 1
    r = recs[0]
    assert r["status"] == sar.SAR_SEARCH_BOUNDED and r["lyapunov"][0] > 0.005
    ext = sar.attractor_extent(cfg, rt, 1, steps, starts=np.array([start]))
    assert np.array_equal(_bits(r["extent"]), _bits(ext[6:12]))


def test_determinism_across_runs_splits_chunks_and_cap(sar, rt):
    kw = dict(seed=5, transient=1000, steps=2000, **NOLIMIT)
    rt.set_option("search_chunk", 40000)       # chunk boundaries at 40000 and 80000 fall inside every range below
    try:
        a, sa = sar.search_attractors(rt, 100003, first=0, **kw)
        b, sb = sar.search_attractors(rt, 100003, first=0, **kw)
        p1, s1 = sar.search_attractors(rt, 50000, first=0, **kw)
        p2, s2 = sar.search_attractors(rt, 50003, first=50000, **kw)
        cap = 17
        c, sc = sar.search_attractors(rt, 100003, first=0, cap=cap, **kw)
    finally:
        rt.set_option("search_chunk", 0)
    assert len(a) > 1000 and sa["tested"] == 100003
    assert a.tobytes() == b.tobytes() and sa == sb
    assert a.tobytes() == np.concatenate([p1, p2]).tobytes()
    assert all(sa[k] == s1[k] + s2[k] for k in sa)
    assert np.all(np.diff(a["candidate"].astype(np.int64)) > 0)
    assert c.tobytes() == a[:cap].tobytes() and sc["records"] == len(a)
    d, _ = sar.search_attractors(rt, 100003, first=0, **kw)   # the default chunk: the same records
    assert d.tobytes() == a.tobytes()


def test_out_of_range_chunk_and_steps_are_refused(sar, rt):
    """search_chunk above 2^30 would wrap the kernels' 32-bit slot arithmetic; steps above 2^31 their step counters."""
    for bad in (2**30 + 1, 2**31, 2**32 + 5):
        with pytest.raises(sar.SarError):
            rt.set_option("search_chunk", bad)
    rt.set_option("search_chunk", 2**30)
    rt.set_option("search_chunk", 0)
    lib = sar.load_library()
    p = sar.search_params(seed=1)
    p.steps = 2**32 - 1
    n_out = C.c_uint32()
    assert lib.sar_runtime_search(rt.handle, C.byref(p), 0, 64, None, None, 0, C.byref(n_out), None) == sar._abi.SAR_ERR_INVALID
    recs, stats = sar.search_attractors(rt, 64, seed=1, steps=100)   # the runtime is fine afterwards
    assert stats["tested"] == 64


END_TO_END_SEED = 1   # the restatement finds 427 accepted candidates among its first 2^18 (min_lyapunov 0.01, min_ky_dim 1.2)


def test_found_attractor_renders_in_frame(sar, rt):
    recs, stats = sar.search_attractors(rt, 1 << 18, seed=END_TO_END_SEED, min_lyapunov=0.01, min_ky_dim=1.2)
    assert stats["accepted"] == len(recs) > 0
    assert np.all(recs["status"] == sar.SAR_SEARCH_BOUNDED) and np.all(recs["lyapunov"][:, 0] >= 0.01)
    assert np.all(recs["ky_dim"] >= 1.2)
    top = recs[np.argmax(recs["ky_dim"])]
    base = sar.Config.from_coefficients(sar.search_candidate(END_TO_END_SEED, int(top["candidate"])))
    w = h = 256
    jobs = 4096
    cfg = base.replace(width=w, height=h, iterations=10_000_000, jobs_total=jobs, seed=11)
    cfg = sar.frame_view(cfg, rt, 1024, 2000, margin=0.05)
    img_rt = sar.Runtime(cfg, device=0)
    try:
        img_rt.enable_timing(True)
        sar.render_jobs(cfg, img_rt)
        counted = img_rt.last_timing().iterations_counted
        count = img_rt.count()
    finally:
        img_rt.close()
    assert counted == (10_000_000 // jobs) * jobs
    inside = int(count.sum(dtype=np.uint64))
    assert inside >= 0.99 * counted, (inside, counted)
    assert np.count_nonzero(count) >= 0.005 * w * h


# ---- against the exact references (tests/lyapunov_reference.py) ---------------------------------------------------------
# Tolerance 1e-12 absolute on each exponent, on the Kaplan-Yorke dimension and on the sum of the exponents: the records are
# bit-identical to the restatement, which tests/test_lyapunov_reference.py holds to these references within 3e-13 (the
# conjugated Jordan block), 4e-15 (the other affine maps) and 4e-16 (the sum rule).
REF_TOL = 1e-12


def _check_affine(sar, rt, names, steps, transient=200, start=(0.05, 0.05, 0.05)):
    coeffs = np.array([L.affine_coeffs(*L.AFFINE_MAPS[k]) for k in names])
    recs, _ = sar.search_attractors(rt, len(names), coeffs=coeffs, transient=transient, steps=steps, bound=L.AFFINE_BOUND,
                                    start=start, **NOLIMIT)
    assert len(recs) == len(names)
    out = []
    for r, name, c in zip(recs, names, coeffs):
        alive, status, done, _ = L.orbit_fate(list(c), start, transient, steps, L.AFFINE_BOUND)
        assert alive and (int(r["status"]), int(r["steps_done"])) == (status, done), (name, r["status"], r["steps_done"])
        folded = done if status == L.BOUNDED else done - 1
        lam, ky = L.affine_spectrum(L.AFFINE_MAPS[name][0], folded)
        assert np.max(np.abs(r["lyapunov"] - lam)) <= REF_TOL, (name, r["lyapunov"], lam)
        assert abs(r["ky_dim"] - ky) <= REF_TOL, (name, r["ky_dim"], ky)
        out.append((status, done))
    return out


def test_non_normal_affine_maps_meet_the_decimal_reference(sar, rt):
    """x' = S B S^-1 x + b: a complex pair with an expanding direction, a Jordan block, real eigenvalues 0.8 / -0.6 / 0.05 and
    a nearly singular map (smallest singular value 5e-9) — the frame Q turns, Gram-Schmidt removes something every step."""
    names = sorted(L.AFFINE_MAPS)
    assert _check_affine(sar, rt, names, 1000) == [(L.BOUNDED, 1000)] * len(names)
    sv = np.linalg.svd(np.array(L.AFFINE_MAPS["nearly_singular"][0]), compute_uv=False)
    assert 1e-9 < sv[-1] < 1e-7


def test_an_expanding_map_leaves_the_box_at_the_predicted_step(sar, rt):
    (status, done), = _check_affine(sar, rt, ["complex_pair_expanding"], 1500)
    assert status == L.DIVERGED and 1000 < done < 1500        # the exponents are compared at folded = steps_done - 1


@pytest.mark.parametrize("seed,params", [
    (1, dict()),
    (3, dict(lo=-1.0, hi=1.1, start=(0.1, -0.05, 0.02), bound=1e4, transient=500)),
])
def test_found_maps_meet_the_sum_rule(sar, rt, seed, params):
    """Sum over i of lambda_i * folded == sum over the folded steps of log|det J(p_t)|, with det J exact: Gram-Schmidt does
    not enter it, so a wrong norm, rejection or Jacobian entry anywhere in the search shows."""
    steps = 3000
    recs, stats = sar.search_attractors(rt, 8192, seed=seed, steps=steps, **params)
    assert stats["accepted"] >= 3, stats
    lo, hi = params.get("lo", -1.2), params.get("hi", 1.2)
    start, transient, bound = params.get("start", (0.05, 0.05, 0.05)), params.get("transient", 1000), params.get("bound", 1e6)
    for r in recs[:5]:
        c = list(R.candidates(seed, int(r["candidate"]), 1, lo, hi)[0])
        alive, status, done, p0 = L.orbit_fate(c, start, transient, steps, bound)
        assert alive and (int(r["status"]), int(r["steps_done"])) == (status, done) == (L.BOUNDED, steps)
        want = L.log_det_sum(c, p0, steps) / steps
        assert abs(math.fsum(r["lyapunov"]) - want) <= REF_TOL, (int(r["candidate"]), math.fsum(r["lyapunov"]), want)


# ---- wider parity with the restatement -------------------------------------------------------------------------------
def _assert_parity(recs, stats, want, wstats):
    assert list(recs["candidate"]) == [r["candidate"] for r in want]
    assert np.array_equal(recs["status"], [r["status"] for r in want])
    assert np.array_equal(recs["steps_done"], [r["steps_done"] for r in want])
    if len(want):
        assert np.array_equal(recs["log2_exp"], np.array([r["log2_exp"] for r in want]))
        assert np.array_equal(_bits(recs["mant"]), _bits(np.array([r["mant"] for r in want])))
        assert np.array_equal(_bits(recs["extent"]), _bits(np.array([r["extent"] for r in want])))
        lam = np.array([r["lyapunov"] for r in want])
        both_nan = np.isnan(recs["lyapunov"]) & np.isnan(lam)
        assert np.all(both_nan | (np.abs(recs["lyapunov"] - lam) <= 1e-15))
        assert np.allclose(recs["ky_dim"], [r["ky_dim"] for r in want], rtol=0, atol=1e-12, equal_nan=True)
    assert {k: stats[k] for k in wstats} == wstats and stats["records"] == len(want)


CROSS_2_32 = 143_165_576        # 30 * index crosses 2^32 between this candidate and the next


THRESHOLDS = dict(min_lyapunov=0.01, min_ky_dim=1.8)   # seed 1's first 8192 candidates fall on both sides of each


@pytest.mark.parametrize("seed,first,n,params,chunk", [
    (7, 0, 2048, dict(), 0),
    (3, 5000, 2048, dict(lo=-1.0, hi=1.1, start=(0.1, -0.05, 0.02), bound=1e4, transient=500), 0),
    (1, 0, 8192, dict(THRESHOLDS, keep_rejected=0), 0),
    (1, 0, 8192, dict(THRESHOLDS, keep_rejected=1), 0),
    (11, CROSS_2_32 - 1000, 2048, dict(), 0),
    (11, 2**40 - 1024, 2048, dict(), 0),
    (11, CROSS_2_32 - 1000, 2500, dict(min_lyapunov=0.01, min_ky_dim=1.1), 700),   # chunk boundaries inside the range
])
def test_wider_parity_with_the_restatement(sar, rt, seed, first, n, params, chunk):
    steps = 3000
    p = dict(dict(min_lyapunov=-math.inf, min_ky_dim=-math.inf, keep_rejected=1), **params)
    if chunk:
        rt.set_option("search_chunk", chunk)
    try:
        recs, stats = sar.search_attractors(rt, n, first=first, seed=seed, steps=steps, **p)
    finally:
        rt.set_option("search_chunk", 0)
    want, wstats = R.search(seed, first, n, steps=steps, **dict(p, keep_rejected=bool(p["keep_rejected"])))
    _assert_parity(recs, stats, want, wstats)
    if params.get("min_ky_dim") == THRESHOLDS["min_ky_dim"]:    # the thresholds reject for both reasons
        assert wstats["below_lyapunov"] > 0 and wstats["below_dim"] > 0 and wstats["accepted"] > 0, wstats
        assert len(want) == (wstats["accepted"] if not params["keep_rejected"] else n - wstats["diverged_transient"])


def test_supplied_coefficients_give_the_generated_records(sar, rt):
    seed, first, n = 5, CROSS_2_32 - 300, 1024
    kw = dict(transient=1000, steps=2000, **NOLIMIT)
    gen, sg = sar.search_attractors(rt, n, first=first, seed=seed, **kw)
    sup, ss = sar.search_attractors(rt, n, first=first, coeffs=R.candidates(seed, first, n), seed=999, **kw)
    assert len(gen) > 10 and gen.tobytes() == sup.tobytes() and sg == ss
    # -0.0 through the supplied path: c0 is canonicalised (0. + 1. * c0), so y' = c0 + y c5 (+ zero terms) from y = +0 with
    # c5 < 0 stays +0.0 — the record, its extent included, is the one of c0 = +0.0
    x, y, z = np.zeros(10), np.full(10, -0.0), np.zeros(10)
    x[0], x[1], y[5], z[8] = 0.1, 0.5, -0.5, 0.5
    plus = y.copy()
    plus[plus == 0] = 0.0
    rows = [(x, y, z), (x, plus, z)]
    start = (0.05, 0.0, 0.05)
    recs, _ = sar.search_attractors(rt, 2, coeffs=_given(rows), transient=10, steps=100, start=start, **NOLIMIT)
    assert recs[0].tobytes()[8:] == recs[1].tobytes()[8:]          # (all but the candidate index)
    assert recs[0]["status"] == sar.SAR_SEARCH_BOUNDED
    assert _bits(recs[0]["extent"][2:4]).tolist() == [0, 0]       # ymin, ymax: +0.0, not -0.0
    want, _ = R.search(0, 0, 2, transient=10, steps=100, start=start, coeffs=_given(rows), min_lyapunov=-math.inf,
                       min_ky_dim=-math.inf, keep_rejected=True)
    assert np.array_equal(_bits(recs["extent"]), _bits(np.array([r["extent"] for r in want])))
