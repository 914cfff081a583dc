"""The conditions the journeys of tests/family_journeys.py rely on, held with the restatements alone: a journey that never hands a
buffer from one family to another, never shrinks after growing, repeats an answer a stale buffer would also give, or plots only where
the smaller image before it plotted, would let tests/test_gpu_family_journeys.py pass without testing what it is for."""
import numpy as np
import pytest

import family_journeys as J
import flow_cases as FK
import section_cases as SK
import volume_cases as VK
import volume_edge_cases as VE

HAND_OVER = {"grow", "shrink", "hand_over"}
POINT_JOURNEYS = [("J1", o) for o in J.J1] + [("J2", o) for o in J.J2]


def _steps(journey, order):
    return getattr(J, journey)[order]


def _frame(want) -> dict:
    return {f[6:]: v for f, v in want.items() if f.startswith("frame.")}


def _staged(st):
    """What the step leaves in d_points: the staged sets, or the map forms' recorded points."""
    return J.staged(st) if st.family in J.SET_FORMS else J.reference(st)["points"].reshape(-1)


# ---- the hand-over of each sharing group ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("journey,order", POINT_JOURNEYS)
def test_point_journeys_grow_shrink_and_hand_d_points_over(journey, order):
    steps = _steps(journey, order)
    kinds = J.transitions([J.footprint(st) for st in steps], [st.family for st in steps])
    assert kinds["d_points"] >= HAND_OVER, kinds
    if journey == "J2":
        assert kinds["d_state"] >= HAND_OVER, kinds
        forms = [st.family for st in steps]
        assert set(forms) == set(J.MAP_FORMS) | {"pairs", "boxes"} and all(forms.count(f) == 2 for f in J.MAP_FORMS)
        assert {J.arg(st, "maps") for st in steps if st.family in J.MAP_FORMS} == {1, 4, 6}
        # a set form stands between map forms: it stages over the orbits, and the next map form records over its points
        at = [i for i, f in enumerate(forms) if f in J.SET_FORMS]
        assert len(at) == 2 and all(0 < i < len(forms) - 1 and forms[i - 1] in J.MAP_FORMS and forms[i + 1] in J.MAP_FORMS for i in at)
    else:
        assert [st.family for st in J.J1_STEPS] == ["pairs", "plot", "boxes", "spectra", "lines", "pairs", "boxes", "spectra", "lines"]


def test_the_orders_are_each_others_reverse():
    assert J.J1["reversed"] == J.J1["forward"][::-1] and J.J2["shrink_then_grow"] == J.J2["grow_then_shrink"][::-1]
    sizes = [J.footprint(st)["d_points"] for st in J.J2["grow_then_shrink"]]
    assert sizes.index(max(sizes)) < sizes.index(min(sizes[3:]), 3), sizes     # grows to its largest, then shrinks


def test_flow_journeys_grow_shrink_and_hand_their_scratch_over():
    for steps in (J.J3_STEPS, J.J3_HEAD):
        kinds = J.transitions(*J.j3_footprints(steps))
        assert kinds["flow_scratch"] >= HAND_OVER, kinds
        assert kinds["d_keys"] >= ({"grow", "hand_over"} if steps is J.J3_HEAD else HAND_OVER), kinds
    fams = [st.family for st in J.J3_STEPS]
    # the first plotting call at the new, larger size is a section; the measuring calls follow it on the plotted frame
    first_plot_at = {}
    size = None
    for st in J.J3_STEPS:
        if st.family == "size":
            size = (J.arg(st, "width"), J.arg(st, "height"))
        elif st.family in ("flow", "section") and J.arg(st, "plot"):
            first_plot_at.setdefault(size, st.family)
    assert first_plot_at == {(7, 5): "flow", (64, 48): "section", (1, 1): "flow"}
    assert [J.arg(st, "plot") for st in J.J3_STEPS if st.family in ("flow", "section")] == [1, 1, 0, 0, 1, 1]
    # the volume: held, added to, dropped by a resize, refused, loaded smaller by another entry, read, written back, rendered on
    assert fams[fams.index("volume"):] == ["volume", "add", "size", "refuse", "size", "load_volume", "march", "load_section", "render"]
    made, loaded = VK.case(J.J3_VOLUME), VE.case(J.J3_LOADED)
    assert made.vol.size > loaded.vol.size and (made.width, made.height) == (96, 64) and (loaded.width, loaded.height) == VE.SMALL
    assert fams[-1] == "render" and J.J3_RENDER["jobs"] == 2048 and J.J3_RENDER["iters"] == 200     # enough jobs for the binned path's hints


def test_held_pictures_and_the_moded_frame_change_hands_as_far_as_their_journeys_go():
    """J4 and J5 by name, from their step lists. The held pictures are per family: each is written by its own call and read by its
    colorize (the basin's by the probes too) — a hand-over —, plane and basin shrink with their second picture, none grows. The frame
    under the modes keeps its size: every writer takes it over from another family."""
    kinds = J.transitions(*J.j4_footprints(J.J4_STEPS))
    assert kinds == {"held_plane": {"shrink", "hand_over"}, "held_period": {"hand_over"}, "held_basin": {"shrink", "hand_over"},
                     "held_ftle": {"hand_over"}}, kinds
    fams = [(st.family, J.arg(st, "of")) for st in J.J4_STEPS]
    four = [("colorize", f) for f in J.J4_ORDER]
    assert fams[:8] == [(k, f) for f in J.J4_ORDER for k in ("picture", "colorize")] and fams[8:12] == four[::-1]     # at once, then reversed
    assert fams[12:] == [("fates", None), ("picture", "plane"), ("colorize", "plane"), ("pairs", None), ("fates", None), ("picture", "basin"),
                         ("colorize", "basin"), ("fates", None), ("size", None), ("size", None)] + four + [("fates", None)]
    held = J.j4_held(J.J4_STEPS)
    assert held[12] == dict.fromkeys(J.J4_ORDER, False) and held[-1] == dict(plane=True, period=False, basin=True, ftle=False)
    sizes = [(J.arg(st, "width"), J.arg(st, "height")) for st in J.J4_STEPS if st.family == "size"]
    assert sizes == [(1, 1), J.J4_SIZE]
    kinds = J.transitions(*J.j5_footprints(J.J5_STEPS))
    assert kinds == {"frame": {"hand_over"}} and J.j5_footprints(J.J5_STEPS)[1] == ["flow", "section", "density", "load_section"]


def test_every_size_and_count_stays_within_the_limits():
    for steps in list(J.J1.values()) + list(J.J2.values()):
        for st in steps:
            if st.family in J.SET_FORMS:
                assert J.arg(st, "t") * J.arg(st, "jobs") <= 2048 or st.family == "lines" and J.arg(st, "t") <= 2048
            else:
                assert J.arg(st, "maps") <= 6 and J.arg(st, "jobs") <= 257 and J.arg(st, "jobs") * J.samples_of(st) <= 2048
    for st in J.J3_STEPS + J.J5_STEPS:
        if st.family == "size":
            assert J.arg(st, "width") <= 96 and J.arg(st, "height") <= 80
        if st.family == "flow" and J.arg(st, "case"):
            assert FK.PARITY[J.arg(st, "case")][2] <= 257 and FK.PARITY[J.arg(st, "case")][3] <= 3000
        if st.family == "section" and J.arg(st, "case"):
            assert SK.PARITY[J.arg(st, "case")][3] <= 257 and SK.PARITY[J.arg(st, "case")][5] <= 3000


# ---- no stale answers ------------------------------------------------------------------------------------------------------------
def _differ(a: dict, b: dict, names=None) -> bool:
    names = [n for n in a if n in b] if names is None else names
    return any(np.asarray(a[n]).shape != np.asarray(b[n]).shape or not np.array_equal(a[n], b[n], equal_nan=np.asarray(a[n]).dtype.kind == "f")
               for n in names)


@pytest.mark.parametrize("journey,order", POINT_JOURNEYS)
def test_successive_answers_of_one_family_differ(journey, order):
    last = {}
    for st in _steps(journey, order):
        want = J.reference(st)
        assert all(np.asarray(v).size for v in want.values()), st
        if st.family in last:
            main = {"pairs": ["hist"], "boxes": ["cells", "sum_sq"], "spectra": ["power"], "lines": ["diag", "vert"], "corrdim": ["hist", "points"],
                    "boxdim": ["cells", "points"], "spectrum": ["power", "points"], "rqa": ["diag", "points"]}[st.family]
            for n in main:                              # each alone: no part of the last answer would pass for this one
                a, b = np.asarray(last[st.family][n]), np.asarray(want[n])
                m = min(a.shape[0], b.shape[0])
                assert a.shape[1:] != b.shape[1:] or not np.array_equal(a[:m], b[:m]), (st, n)
        last[st.family] = want
    if journey == "J1":
        assert J.reference(J.J1_STEPS[1])["plot"].any() and not J.reference(J.J1_STEPS[1])["plot"].all()


def test_the_map_lists_hold_a_map_that_diverges_and_one_that_loses_a_later_job():
    import corr_restatement as X
    for st in J.J2_STEPS:
        if st.family not in J.MAP_FORMS:
            continue
        want = J.reference(st)
        gone = want["status"] == X.DIVERGED
        if J.arg(st, "maps") == 1:
            assert not gone.any() and want["points"].any(), st     # the single map is bounded: its points are read back
            continue
        assert (gone & (want["fail_job"] == 0)).any(), (st, "no map leaves from the first job")
        assert (gone & (want["fail_job"] > 0)).any(), (st, "no map loses a job that is not the first")
        assert (~gone).sum() >= 2 and not want["points"][gone].any() and all(want["points"][k].any() for k in np.nonzero(~gone)[0])


# ---- J1 and J2: smaller after larger ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("journey,order", POINT_JOURNEYS)
def test_a_smaller_sets_points_differ_from_the_head_of_what_a_larger_call_left(journey, order):
    steps = _steps(journey, order)
    checked = 0
    for j, st in enumerate(steps):
        mine = _staged(st)
        for earlier in steps[:j]:
            theirs = _staged(earlier)
            if theirs.size > mine.size:
                same = mine == theirs[:mine.size]
                assert np.count_nonzero(~same) >= mine.size // 4, (earlier, st, int(np.count_nonzero(~same)), mine.size)
                checked += 1
    assert checked >= 8
    # and the tail the smaller call leaves untouched is not all zero: reading past one's own points would show
    largest = max(steps, key=lambda s: _staged(s).size)
    assert np.count_nonzero(_staged(largest)) >= _staged(largest).size // 2


# ---- J3: plotted keys before and after the resize -------------------------------------------------------------------------------------
def test_the_section_after_the_resize_plots_beyond_and_inside_the_small_images_keys(sar):
    walked = J.walk(sar, "across_sizes", J.J3_STEPS)
    small, large = _frame(walked[1]), _frame(walked[3])
    assert J.J3_STEPS[1].family == "flow" and J.J3_STEPS[3].family == "section" and small["count"].shape == (5, 7)
    assert large["count"].shape == (48, 64)
    before, after = J.keys_of(small), J.keys_of(large)
    npix = before.size
    assert npix == 35 and np.count_nonzero(before) >= 8
    beyond = np.nonzero(after[npix:])[0]
    assert beyond.size >= 16, "no key beyond the 35 pixels d_keys had before the resize"
    inside = np.nonzero(after[:npix] != before)[0]
    assert inside.size >= 8 and np.count_nonzero(after[:npix]) >= 1, "the first 35 keys equal the small image's: a stale d_keys would pass"
    # a key left from the small image would win where the section plots nothing: every one of them lies in front of the sentinel
    stale_only = (before != 0) & (after[:npix] == 0)
    assert stale_only.sum() >= 4


def test_the_flow_journeys_frames_move_with_every_writer_and_stay_under_the_measuring_calls(sar):
    walked = J.walk(sar, "across_sizes", J.J3_STEPS)
    for i, (st, want) in enumerate(zip(J.J3_STEPS, walked)):
        f = _frame(want)
        if st.family == "size":
            assert not f["count"].any() and f["max"] == 0 and (f["zbuf"] == np.float32(-1.0)).all()
            continue
        prev = _frame(walked[i - 1])
        writes = st.family in ("load_section", "render") or st.family in ("flow", "section") and J.arg(st, "plot")
        assert _differ(prev, f, ["count"]) == bool(writes), (i, st)
        if st.family in ("flow", "section"):
            assert want["stats.steps"] > 0 and np.isfinite(want["extent"]).all(), (i, st)
    by_family = {}
    for st, want in zip(J.J3_STEPS, walked):
        if st.family in ("flow", "section"):
            if st.family in by_family:
                assert _differ(by_family[st.family], want, ["extent", "stats.steps"]), st
            by_family[st.family] = want
    sec = walked[3]
    assert sec["stats.crossings"] >= 500 and sec["stats.visits"] >= 100 and sec["stats.outside"] >= 100
    vol, added = walked[10], walked[11]
    assert 0 < vol["stats.stored"] < added["stats.stored"] and _differ(vol, added, ["slabs"])
    loaded = _frame(walked[17])
    assert ((loaded["count"] == 0) & (loaded["zbuf"] != np.float32(-1.0))).sum() >= 90      # depths where nothing is counted: what hints must not outlive
    assert _differ(loaded, _frame(walked[18]), ["zbuf"]) and _frame(walked[18])["max"] > loaded["max"]


# ---- J4: the probes reach the held picture -----------------------------------------------------------------------------------------
def test_the_probes_hit_two_labels_and_an_escape_and_the_pictures_have_something_to_show(sar):
    import fate_restatement as T
    f = J.probe_reference()
    bounded = f["status"] == T.BOUNDED
    assert len(f["status"]) == 65 and len(np.unique(f["label"][bounded])) >= 2 and (~bounded).sum() >= 1
    assert (np.bincount(f["label"][bounded]) >= 10).sum() >= 2 and not (f["label"][bounded] == T.NONE).any()
    cfg = sar.Config.poisson_saturne()
    palette = cfg.palette_rgb[:cfg.palette_len]
    shapes = {"plane": (21, 37), "period": (16, 16), "basin": (17, 33), "ftle": (24, 24)}
    for family in J.J4_ORDER:
        want = J.picture_reference(family)
        assert want["status"].shape == shapes[family] and len(np.unique(want["status"])) >= 2, family     # both fates in every picture
        # every family's restatement has a colorize; the pixels it states bit for bit are there and show more than one colour, so
        # an image made from another family's records or buffer would not pass for this one
        img, exact = J.picture_image(family, palette)
        assert img.shape == shapes[family] + (4,) and img.dtype == np.uint16 and exact.shape == shapes[family], family
        assert exact.sum() >= 20 and len(np.unique(img[exact].reshape(-1, 4), axis=0)) >= 2, family
        assert len(np.unique(img.reshape(-1, 4), axis=0)) >= 8, family
        assert exact.all() == (family in ("period", "basin")), family
    plane, ftle = J.picture_reference("plane"), J.picture_reference("ftle")
    import ftle_restatement as L
    import plane_restatement as N
    assert {N.DIVERGED, N.DEGENERATE} <= set(np.unique(plane["status"]))           # transparent, and opaque black
    assert (ftle["status"] == L.DIVERGED).any() and ((ftle["flags"] & L.EDGE) != 0).any() and np.isfinite(ftle["ftle"]).any()
    # the second plane is smaller than the first and is another picture
    small, big = J.picture_reference("plane", True), J.picture_reference("plane")
    assert small["status"].size < big["status"].size and len(np.unique(small["status"])) >= 2
    assert len({shapes[f][0] * shapes[f][1] for f in J.J4_ORDER}) == 4
    # the second basin picture has another grid, so another label table, and the probes answer otherwise on it: the first picture's
    # table left on the device would show
    g = J.probe_reference(True)
    gb = g["status"] == T.BOUNDED
    assert J.J4_BASIN_SMALL["grid"] != J.J4_BASIN["grid"] and len(np.unique(g["label"][gb])) >= 2 and (~gb).sum() >= 1
    assert np.array_equal(f["status"], g["status"]) and (f["label"][bounded] != g["label"][bounded]).sum() >= 20     # the labels swap


# ---- J5 and J6 ---------------------------------------------------------------------------------------------------------------------
def test_every_writer_under_the_modes_changes_counts_and_hues(sar):
    walked = J.walk_modes(sar)
    assert [st.family for st in J.J5_STEPS] == ["size", "flow", "section", "density", "load_volume", "load_section"]
    for i, st in enumerate(J.J5_STEPS):
        prev, f = _frame(walked[i - 1]) if i else None, _frame(walked[i])
        if st.family in ("flow", "section", "density", "load_section"):
            assert _differ(prev, f, ["count"]) and _differ(prev, f, ["steps"]), st     # exposure measures counts, the colour range steps
            assert np.count_nonzero(f["count"]) >= 5 and len(np.unique(f["steps"][f["count"] > 0])) >= 3, st
        elif st.family == "load_volume":
            assert not _differ(prev, f), st
    assert J.J5_SIZE == (VK.case(J.J5_VOLUME).width, VK.case(J.J5_VOLUME).height) == FK.PARITY[J.J5_FLOW][1] == SK.PARITY[J.J5_SECTION][2]


def test_the_group_members_journey_and_its_neighbours_frames():
    assert J.J6_STEPS == J.J1_STEPS[:4] + J.J3_STEPS[:6]
    assert [st.family for st in J.J3_HEAD] == ["size", "flow", "size", "section", "flow", "section"]
    steps = J.J1_STEPS[:4]
    assert J.transitions([J.footprint(st) for st in steps], [st.family for st in steps])["d_points"] >= HAND_OVER
    for member in (0, 2):
        one, two = J.neighbour_frame(member, 1), J.neighbour_frame(member, 2)
        assert one["count"].any() and _differ(one, two, ["count"]) and two["max"] >= one["max"]
    assert _differ(J.neighbour_frame(0, 1), J.neighbour_frame(2, 1), ["count"])


# ---- the device module walks the whole lists ---------------------------------------------------------------------------------------
def test_the_device_module_walks_every_journey_and_order():
    import test_gpu_family_journeys as G
    marks = {}
    for name in dir(G):
        fn = getattr(G, name)
        if name.startswith("test_") and callable(fn):
            for m in getattr(fn, "pytestmark", []):
                assert m.name not in ("skip", "skipif", "xfail"), f"{name} is marked {m.name}"
                if m.name == "parametrize":
                    marks[name] = list(m.args[1])
    assert marks["test_j1_point_sets_through_d_points"] == list(J.J1) == ["forward", "reversed"]
    assert marks["test_j2_map_forms_through_the_orbit_buffers"] == list(J.J2) == ["grow_then_shrink", "shrink_then_grow"]
    assert marks["test_j3_flows_sections_and_the_volume_across_sizes"] == list(J.J3)
    assert marks["test_j4_held_pictures_keep_their_records_images_and_probes"] == list(J.J4)
    assert marks["test_j5_frame_writers_under_exposure_and_colour_range"] == list(J.J5)
    assert G.pytestmark.name == "gpu"


# ---- the comparison itself ---------------------------------------------------------------------------------------------------------
def test_differences_sees_bits_dtypes_signs_names_and_axes():
    want = dict(a=np.array([[1.0, -0.0, np.nan]]), n=np.array([1, 2], dtype=np.int64), extent=np.array([0.0, 1.0]))
    same = dict(a=np.array([1.0, -0.0, np.nan]), n=np.array([1, 2], dtype=np.uint32), extent=np.array([-0.0, 1.0]))
    assert J.differences(same, want) == []                                  # the sets' axis, integer widths, the extent by value
    for name, value, word in (("a", np.array([[1.0, 0.0, np.nan]]), "first at [0, 1]"),                       # +0.0 for -0.0
                              ("a", np.array([[1.0, -0.0, np.nan]], dtype=np.float32), "dtype float32"),
                              ("a", np.array([[[1.0, -0.0, np.nan]]]), "shape"), ("a", np.array([[1.0], [-0.0], [np.nan]]), "shape"),
                              ("n", np.array([1, -2], dtype=np.int32), "first at [1]"), ("n", np.array([1.0, 2.0]), "dtype float64"),
                              ("extent", np.array([0.0, np.nextafter(1.0, 2.0)]), "first at [1]")):
        bad = J.differences(dict(same, **{name: value}), want)
        assert len(bad) == 1 and bad[0].startswith(name + ":") and word in bad[0], (name, bad)
    assert J.differences(dict(n=np.array([-1], dtype=np.int32)), dict(n=np.array([-1], dtype=np.int64))) == []
    assert J.differences(dict(n=np.array([-1], dtype=np.int32)), dict(n=np.array([2 ** 64 - 1], dtype=np.uint64))) != []
    assert J.differences(dict(same, more=np.zeros(1)), want) == ["more: not in the reference"]
    assert J.differences({k: v for k, v in same.items() if k != "n"}, want) == ["n: missing"]
    img = np.full((2, 2, 4), 100, dtype=np.uint16)
    off = img.copy()
    off[0, 0, 1], off[1, 1, 2] = 101, 102
    exact = np.array([[True, False], [False, False]])
    assert J.image_differences(img, img, exact) == [] and len(J.image_differences(off, img, exact)) == 2
    assert J.image_differences(off, img, ~exact)[0].startswith("image on the exact pixels") and len(J.image_differences(off, img, ~exact)) == 1
