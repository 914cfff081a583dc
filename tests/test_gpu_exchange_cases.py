"""GPU: the exchange context (sar_exchange_*) — dense slices, sparse records behind the device-planned slot tables, and the rooted
form — on the states of tests/exchange_cases.py, where the ORDER of the fold shows: the depth cases cut over two and three ranks
(every pixel a tie, +-inf, visited pixels at the -1 sentinel, frames whose depths are all negative or all equal), a rank that rendered
nothing in every position, ranks that touch different granules (every presence pattern of three ranks, five ranks of which two own no
slice), and one pixel whose counts pass 2^32 inside the fold. All ranks live in this process on one GPU; tests/exchange_cases.py does
the collectives by hand (tests/test_exchange_cases_host.py proves that driver on a numpy stand-in and pins the states' conditions).

The reference is oracle.merge folded in rank order over the same partial states. The bar: count, max and steps bit for bit, zbuf bit
for bit after `+ 0.0f` with no -0.0 returned; for the sliced forms the Depth and Gas images put together from colorize_range_device of
every owner's slice, bit for bit (Gas within 1 LSB where ln leaves the host-libm table: a count + 1 or max + 1 above 2^20, DESIGN.md
section 3.4). The rooted form's max is what DESIGN.md section 7 states: max(rank 0's max, the final sums) — the fold's, unless a count wraps
inside a fold of three or more ranks; the rows `peak_at_1` and `rank0_absent` are such folds and hold it to the stated value.

One test cuts test_one_pixel_past_u32's work over three shards of the multi-device renderer: the pixel passes 2^32 only in the sum
over the shards, and max is the fold's largest intermediate sum, not u32::MAX."""
import time

import numpy as np
import pytest

import depth_cases as DC
import exchange_cases as XC

pytestmark = pytest.mark.gpu

DEPTH, GAS = DC.oracle_lib.SAR_RENDER_DEPTH, DC.oracle_lib.SAR_RENDER_GAS
ALL_SIZES = pytest.mark.parametrize("size", DC.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
TABLE = 1 << 20      # colorize's ln table: bit-exact up to here


def _ranks(sar, oracle, spec, plant=None):
    """Every rank's runtime holding its partial state — rendered by render_job_range, a fresh runtime where the rank renders nothing,
    then (plant) one pixel's count and max replaced through Runtime.load on top of what the render left — and its exchange context."""
    cfg, st, n = DC.config(sar, spec.case, spec.size), DC.starts(spec.case), XC.iterations(spec)
    planted = XC.planted(oracle, spec, plant)
    rts = []
    for r, (lo, hi) in enumerate(spec.parts):
        rt = sar.Runtime(cfg)
        if hi > lo:
            sar.render_job_range(cfg, rt, n, st[lo:hi])
        if plant is not None:
            assert np.array_equal(rt.count(), XC.partial(oracle, spec, r).count)      # (the site was chosen on the oracle's counts)
            rt.load(planted[r][0], rt.steps(), rt.zbuf(), planted[r][1])
        rts.append(rt)
    return cfg, rts, [sar.Exchange(rt, len(rts), r) for r, rt in enumerate(rts)]


def _kinds(cfg):
    return (("Depth", cfg.replace(render_kind=DEPTH), DEPTH, 1), ("Gas opaque", cfg.replace(render_kind=GAS, transparent=0), GAS, 0),
            ("Gas transparent", cfg.replace(render_kind=GAS, transparent=1), GAS, 1))


def _exchange(sar, oracle, spec, form, plant=None, images=True, dense_above=2.0):
    """One exchange of `form` over fresh ranks, held to the fold: the frame, max, and (sliced forms) the images. Returns the result."""
    ref = XC.fold(oracle, spec, plant)
    cfg, rts, exs = _ranks(sar, oracle, spec, plant)
    what = f"{spec.case} {spec.size[0]}x{spec.size[1]} {spec.parts} {plant or ''} {form}"
    kinds = _kinds(cfg) if images and form != "rooted" else ()
    res = XC.run(XC.DeviceMemory(sar), exs, form, dense_above=dense_above, colorize=[k[1] for k in kinds], dims=spec.size)
    for rt in rts:
        rt.close()
    XC.assert_frame(res, ref, what)
    stated = XC.rooted_max(oracle, spec, plant)
    print(f"{what}: max {[hex(m) for m in res.maxes]}, the fold's {hex(ref.max)}, max(rank 0's max, final sums) {hex(stated)}")
    if form == "rooted":
        XC.assert_max(res, stated, what)
        if plant is None or XC.ROWS[plant.row].rooted_exact:
            assert stated == ref.max, what
    else:
        XC.assert_max(res, ref.max, what)
    exact = max(int(ref.count.max()), ref.max) < TABLE
    for img, (name, _, kind, transparent) in zip(res.images, kinds):
        want = ref.image(kind, transparent)
        if kind == DEPTH or exact:
            assert np.array_equal(img, want), f"{what}: {name} image: {XC.diff(img, want)}"
        else:
            worst = int(np.abs(img.astype(np.int32) - want.astype(np.int32)).max())
            assert worst <= 1, f"{what}: {name} image: off by {worst}"
    return res


# ---- the depth cases cut over the ranks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", XC.FORMS)
@pytest.mark.parametrize("cuts", XC.CUTS)
@ALL_SIZES
@pytest.mark.parametrize("case", DC.NAMES)
def test_cuts(sar, oracle, gpu, case, size, cuts, form):
    """Every case over thirds and halves of its jobs: rising_tied (the earlier rank must win every pixel), falling_sentinel (records
    with counts and no depth), all-negative depths (the range's 0.0 seed), one depth everywhere (0 / 0), an infinite span."""
    spec = XC.cuts_spec(case, size, XC.CUTS[cuts])
    res = _exchange(sar, oracle, spec, form)
    whole = DC.reference(oracle, case, size)     # contiguous slices folded in order are the sequential render
    assert np.array_equal(res.count, whole.count.ravel()) and np.array_equal(DC.bits(res.steps), DC.bits(whole.steps.ravel()))


# ---- absent ranks ---------------------------------------------------------------------------------------------------------------------
STATES = [(f"empty-{w}", lambda c, s, w=w: XC.empty_spec(c, s, w)) for w in XC.EMPTY] + \
         [(f"scatter{g}", lambda c, s, g=g: XC.scatter_spec(c, s, g)) for g in (3, 5)]


@pytest.mark.parametrize("state", STATES, ids=[s[0] for s in STATES])
@ALL_SIZES
@pytest.mark.parametrize("case", XC.EDGE_CASES)
def test_empty_and_scattered_ranks(sar, oracle, gpu, case, size, state):
    """A rank that rendered nothing, first, in the middle and last; three and five ranks that touch different granules (the `at < 0`
    paths of the sparse fold: rank 0 absent, a middle rank absent, one sender alone, nobody). sparse == dense == rooted == the fold; the
    flags are the oracle's, the split sizes the flags' own counts, and pack goes sparse exactly while the touched share allows it."""
    spec = state[1](case, size)
    world, nseg = len(spec.parts), -(-size[0] * size[1] // XC.SEG)
    res = {form: _exchange(sar, oracle, spec, form) for form in XC.FORMS}
    for form in ("sparse", "rooted"):
        assert np.array_equal(res[form].count, res["dense"].count) and np.array_equal(DC.bits(res[form].steps), DC.bits(res["dense"].steps))
        assert np.array_equal(DC.bits(res[form].zbuf), DC.bits(res["dense"].zbuf))
    assert res["sparse"].sparse and not res["dense"].sparse
    want = np.stack([XC.touched(XC.partial(oracle, spec, r)) for r in range(world)])
    assert np.array_equal(res["sparse"].flags != 0, want), XC.diff(res["sparse"].flags != 0, want)
    slice_pixels = sar.exchange_slice_pixels(size[0] * size[1], world)
    XC.assert_plan(res["sparse"], slice_pixels, f"{case} {state[0]}")
    assert all(sb == [slice_pixels * 16] * world for sb in res["dense"].send_bytes)
    k = int(want.sum())
    for dense_above, sparse in ((0.5, k <= 0.5 * world * nseg), ((k + 0.5) / (world * nseg), True), ((k - 0.5) / (world * nseg), False)):
        r = _exchange(sar, oracle, spec, "sparse", images=False, dense_above=dense_above)
        assert r.sparse == sparse, (dense_above, k, world * nseg)


# ---- sums that pass 2^32 inside the fold ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("site", XC.SITES)
@ALL_SIZES
@pytest.mark.parametrize("row", list(XC.ROWS))
def test_wrapped_rows(sar, oracle, gpu, row, size, site):
    """One pixel's counts per rank, planted on a rendered scatter state: the running max sees every intermediate sum, rank 0's own max
    is kept (and only rank 0's), an absent rank's sum is the sum before it. Dense and sparse equal the fold at two, three and four
    ranks; the rooted form equals it at two ranks and wherever max(rank 0's max, the final sums) is the fold's, and states that value
    where an unordered SUM cannot know the prefix sums."""
    spec, plant = XC.scatter_spec("rising", size, len(XC.ROWS[row].counts)), XC.Plant(row, site)
    assert XC.fold(oracle, spec, plant).max == XC.ROWS[row].fold_max
    for form in XC.FORMS:
        _exchange(sar, oracle, spec, form, plant)


@pytest.mark.parametrize("site", XC.SITES)
@ALL_SIZES
def test_a_later_ranks_max_has_no_effect(sar, oracle, gpu, size, site):
    """Rank 1 is loaded with max = u32::MAX and no such count: Runtime::merge never looks at other.max (:716-724)."""
    spec, plant = XC.scatter_spec("rising", size, 3), XC.Plant("peak_at_1", site, True)
    assert XC.fold(oracle, spec, plant).max == 0xFFFFFFF5
    for form in XC.FORMS:
        _exchange(sar, oracle, spec, form, plant)


# ---- the multi-device renderer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2], ids=["dense", "sparse"])
def test_one_pixel_past_u32_over_three_shards(sar, oracle, gpu, mode):
    """The work of tests/test_gpu_tail.py::test_one_pixel_past_u32 — 2^32 + 131072 visits of one pixel — cut over three shards of one
    device: no shard's count wraps, the sum over the shards does. count is the total mod 2^32; max is the fold's running maximum
    max(s0, s0 + s1) over the shards' shares (the renderer cuts the jobs like distributed.shard_jobs), not the u32::MAX a single
    device reports for the same frame: the exchange has no wrap flag of its own, and neither has the reference's render_parallel
    (src/lib.rs:1068-1076)."""
    from strange_attractor_renderer_amd.distributed import shard_jobs
    from test_gpu_tail import _fixed_point_config, _hot_pixel
    w = h = 2048
    units, jpu, n = 4096, 32, 32769
    jobs = units * jpu
    cfg = _fixed_point_config(sar, iterations=jobs * n, width=w, height=h, jobs_total=jobs, transparent=1)
    count, _, zbuf, steps, _ = _hot_pixel(sar, oracle, cfg, w, h, jobs * n)
    shares = [shard_jobs(jobs, 3, r)[1] * n for r in range(3)]
    sums = XC.prefix_sums(shares)
    assert sum(shares) == (1 << 32) + 131072 and max(shares) < 1 << 32 and sums == [shares[0], shares[0] + shares[1], 131072]
    r = sar.ParallelRenderer(devices=[0, 0, 0], units=units, seed=5)
    r.set_exchange(mode)
    t0 = time.perf_counter()
    sar.render_parallel(r, cfg, jpu)
    print(f"three shards, exchange mode {mode}: render_parallel took {time.perf_counter() - t0:.2f} s")
    rm = r.runtime()
    got = rm.count(), rm.max(), rm.zbuf(), rm.steps()
    r.shutdown()
    assert np.array_equal(got[0], count) and got[0].max() == 131072, XC.diff(got[0], count)
    assert got[1] == sums[1] != 0xFFFFFFFF, f"max {hex(got[1])}, the fold's {hex(sums[1])}"
    assert np.array_equal(DC.bits(got[2]), DC.bits(zbuf)) and np.array_equal(DC.bits(got[3]), DC.bits(steps))
