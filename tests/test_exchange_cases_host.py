"""The reference side of the exchange cases (tests/exchange_cases.py), without a GPU: conditions on the oracle's partial states alone —
the states still hold what they were built for: every presence pattern of a granule over the ranks, exact depth ties between ranks with
different `steps`, visited pixels at the -1 sentinel, the intermediate sums of the wrapped rows — and the driver itself on the numpy
stand-in of tests/exchange_numpy.py: for every state and form the frame it puts together is the oracle's fold in rank order, bit for
bit. tests/test_gpu_exchange_cases.py runs the same driver on api.Exchange."""
import numpy as np
import pytest

import depth_cases as DC
import exchange_cases as XC
from exchange_numpy import NumpyApi, NumpyExchange, NumpyRuntime

SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")
ALL_SIZES = pytest.mark.parametrize("size", DC.SIZES, **SIZE_IDS)
DEPTH, GAS = DC.oracle_lib.SAR_RENDER_DEPTH, DC.oracle_lib.SAR_RENDER_GAS


# ---- conditions on the oracle's states --------------------------------------------------------------------------------------------------
@ALL_SIZES
@pytest.mark.parametrize("case", XC.EDGE_CASES)
def test_scatter_reaches_every_presence_pattern_of_three_ranks(oracle, case, size):
    """All eight patterns of who touches a granule occur: nobody, rank 0 absent, a middle rank absent, one sender alone."""
    seen = np.bincount(XC.presence(oracle, XC.scatter_spec(case, size, 3)), minlength=8)
    print(f"{case} {size[0]}x{size[1]}, 3 ranks: granules by presence pattern {seen.tolist()}")
    assert (seen > 0).all(), seen


@pytest.mark.parametrize("case", XC.EDGE_CASES)
def test_scatter_of_five_ranks(oracle, sar, case):
    """Ten jobs of 12 iterations over five ranks. At 256 x 64 at least twenty of the thirty-two presence patterns occur. 96 x 64 has
    96 granules, 67 of them untouched, and reaches 18 (as measured when the cases were made; pinned, like the twenty): there ranks 3
    and 4 own no slice, and what the sparse fold needs is named — granules only a slice-less rank touches, granules every rank touches,
    rank 0 absent, rank 0 alone, a rank absent between two senders."""
    seen = {size: np.bincount(XC.presence(oracle, XC.scatter_spec(case, size, 5)), minlength=32) for size in DC.SIZES}
    for size, s in seen.items():
        print(f"{case} {size[0]}x{size[1]}, 5 ranks: {np.count_nonzero(s)} patterns, granules by presence pattern {s.tolist()}")
    small, large = (seen[size] for size in DC.SIZES)
    assert np.count_nonzero(large) >= 20, large
    assert np.count_nonzero(small) >= 18, small
    npix = DC.SIZES[0][0] * DC.SIZES[0][1]
    assert 3 * sar.exchange_slice_pixels(npix, 5) >= npix                                # ranks 0..2 own the whole image
    pats = np.nonzero(small)[0]
    assert small[8] + small[16] + small[24] > 0 and small[31] > 0 and small[1] > 0, small   # only ranks 3 / 4; everybody; rank 0 alone
    assert any(p and not p & 1 for p in pats), small                                      # rank 0 absent
    assert any(p & (p >> 2) & ~(p >> 1) & 7 for p in pats), small                          # ranks r and r + 2 send, r + 1 does not


@pytest.mark.parametrize("cuts", XC.CUTS)
@ALL_SIZES
@pytest.mark.parametrize("case", ["rising_tied", "const_pos", "const_neg"])
def test_cuts_leave_ties_between_ranks(oracle, case, size, cuts):
    """Two ranks hold the same depth on a pixel with different `steps`: only the order of the fold says whose `steps` stay."""
    spec = XC.cuts_spec(case, size, XC.CUTS[cuts])
    parts = [XC.partial(oracle, spec, r) for r in range(len(spec.parts))]
    ties = 0
    for a in range(len(parts)):
        for b in range(a + 1, len(parts)):
            pa, pb = parts[a], parts[b]
            both = (pa.zbuf != np.float32(-1.0)) & (pb.zbuf != np.float32(-1.0))
            ties += int(np.count_nonzero(both & (pa.zbuf == pb.zbuf) & (DC.bits(pa.steps) != DC.bits(pb.steps))))
    print(f"{case} {size[0]}x{size[1]} {cuts}: {ties} tied pixels with different steps")
    assert ties > 0


@ALL_SIZES
def test_falling_sentinel_sends_visited_pixels_without_a_depth(oracle, size):
    """Visited pixels whose depth is still the -1 sentinel, in a rank's partial state (so its record travels with them) and in the fold."""
    for spec in [XC.cuts_spec("falling_sentinel", size, c) for c in XC.CUTS.values()] + [XC.scatter_spec("falling_sentinel", size, 3)]:
        per_rank = [int(np.count_nonzero((p.count > 0) & (p.zbuf == np.float32(-1.0)))) for p in (XC.partial(oracle, spec, r) for r in range(len(spec.parts)))]
        ref = XC.fold(oracle, spec)
        merged = int(np.count_nonzero((ref.count > 0) & (ref.zbuf == np.float32(-1.0))))
        print(f"{spec.parts}: visited and unset per rank {per_rank}, in the fold {merged}")
        assert max(per_rank) > 0 and merged > 0, (spec, per_rank, merged)


@pytest.mark.parametrize("site", XC.SITES)
@ALL_SIZES
@pytest.mark.parametrize("row", list(XC.ROWS))
def test_wrapped_rows_produce_their_intermediate_sums(oracle, row, size, site):
    """The table of tests/exchange_cases.py against the oracle's fold: the running max, the final count, whether the rooted form's
    stated max differs, and — on the untouched site — who sends a record."""
    r = XC.ROWS[row]
    sums = XC.prefix_sums(r.counts)
    assert max([r.counts[0]] + sums[1:]) == r.fold_max, (row, [hex(s) for s in sums])
    spec, plant = XC.scatter_spec("rising", size, len(r.counts)), XC.Plant(row, site)
    px = XC.site_pixel(oracle, spec, site)
    ref = XC.fold(oracle, spec, plant)
    assert ref.max == r.fold_max and ref.count.flat[px] == sums[-1], (hex(ref.max), hex(int(ref.count.flat[px])))
    assert (XC.rooted_max(oracle, spec, plant) == ref.max) == r.rooted_exact
    plain = XC.fold(oracle, spec)
    assert plain.max < 1 << 20 and np.array_equal(DC.bits(plain.steps), DC.bits(ref.steps)) and np.array_equal(DC.bits(plain.zbuf), DC.bits(ref.zbuf))
    senders = [bool(XC.touched(XC.Partial(c, XC.partial(oracle, spec, k).zbuf, None, mx))[px // XC.SEG]) for k, (c, mx) in enumerate(XC.planted(oracle, spec, plant))]
    assert senders == ([True] * len(r.counts) if site == "common" else [c != 0 for c in r.counts]), senders
    assert XC.fold(oracle, spec, XC.Plant(row, site, liar=True)).max == ref.max          # a later rank's max has no effect


# ---- the driver on the numpy stand-in ------------------------------------------------------------------------------------------------------
def _states():
    out = []
    for size in DC.SIZES:
        for case in DC.NAMES:
            for name, cuts in XC.CUTS.items():
                out.append((f"{case}-{name}", XC.cuts_spec(case, size, cuts), None))
        for case in XC.EDGE_CASES:
            for where in XC.EMPTY:
                out.append((f"{case}-empty-{where}", XC.empty_spec(case, size, where), None))
            for world in (3, 5):
                out.append((f"{case}-scatter{world}", XC.scatter_spec(case, size, world), None))
        for row, r in XC.ROWS.items():
            for site in XC.SITES:
                out.append((f"{row}-{site}", XC.scatter_spec("rising", size, len(r.counts)), XC.Plant(row, site)))
        out.append(("peak_at_1-common-liar", XC.scatter_spec("rising", size, 3), XC.Plant("peak_at_1", "common", True)))
    return [pytest.param(spec, plant, id=f"{spec.size[0]}x{spec.size[1]}-{name}") for name, spec, plant in out]


def _stand_in(oracle, sar, spec, plant):
    world = len(spec.parts)
    exs = [NumpyExchange(NumpyRuntime(ort, sar.exchange_slice_pixels), world, r) for r, ort in enumerate(XC.oracle_parts(oracle, spec, plant))]
    return XC.HostMemory(NumpyApi(oracle, sar)), exs


def _configs(oracle, spec):
    out = []
    for kind, transparent in ((DEPTH, 1), (GAS, 0), (GAS, 1)):
        c = oracle.copy_config(DC.config(oracle, spec.case, spec.size))
        c.render_kind, c.transparent = kind, transparent
        out.append((c, kind, transparent))
    return out


@pytest.mark.parametrize("form", XC.FORMS)
@pytest.mark.parametrize("spec,plant", _states())
def test_driver_reproduces_the_fold_on_the_stand_in(oracle, sar, spec, plant, form):
    ref = XC.fold(oracle, spec, plant)
    mem, exs = _stand_in(oracle, sar, spec, plant)
    what = f"{spec.case} {spec.size} {spec.parts} {plant} {form}"
    if form == "rooted":
        res = XC.run(mem, exs, form)
        XC.assert_frame(res, ref, what)
        # the stand-in restates k_exch_import: max(rank 0's max, the final sums) — the fold's unless a count wraps inside a fold of
        # three or more ranks
        XC.assert_max(res, XC.rooted_max(oracle, spec, plant), what)
        if plant is None or XC.ROWS[plant.row].rooted_exact:
            XC.assert_max(res, ref.max, what)
        return
    cfgs = _configs(oracle, spec)
    res = XC.run(mem, exs, form, colorize=[c for c, _, _ in cfgs], dims=spec.size)
    XC.assert_frame(res, ref, what)
    XC.assert_max(res, ref.max, what)
    assert res.sparse == (form == "sparse")
    if form == "sparse":
        want = np.stack([XC.touched(XC.Partial(c, XC.partial(oracle, spec, r).zbuf, None, mx)) for r, (c, mx) in enumerate(XC.planted(oracle, spec, plant))])
        assert np.array_equal(res.flags != 0, want), what
        XC.assert_plan(res, exs[0].slice_pixels, what)
    for img, (_, kind, transparent) in zip(res.images, cfgs):
        assert np.array_equal(img, ref.image(kind, transparent)), f"{what}: image kind {kind} transparent {transparent}: {XC.diff(img, ref.image(kind, transparent))}"


@pytest.mark.parametrize("spec", [XC.scatter_spec("alt_inf", DC.SIZES[1], 3), XC.empty_spec("rising", DC.SIZES[0], "middle")],
                         ids=["scatter", "empty"])
def test_driver_follows_the_touched_share_on_the_stand_in(oracle, sar, spec):
    """pack goes the sparse way while the touched share (over all ranks) is at most dense_above: on either side of the share itself."""
    world, nseg = len(spec.parts), -(-spec.size[0] * spec.size[1] // XC.SEG)
    k = sum(int(XC.touched(XC.partial(oracle, spec, r)).sum()) for r in range(world))
    ref = XC.fold(oracle, spec)
    for dense_above, sparse in ((0.5, k <= 0.5 * world * nseg), ((k + 0.5) / (world * nseg), True), ((k - 0.5) / (world * nseg), False)):
        mem, exs = _stand_in(oracle, sar, spec, None)
        res = XC.run(mem, exs, "sparse", dense_above=dense_above)
        assert res.sparse == sparse, (dense_above, k, world * nseg)
        XC.assert_frame(res, ref, f"dense_above {dense_above}")
        XC.assert_max(res, ref.max, f"dense_above {dense_above}")
