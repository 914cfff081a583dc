"""GPU: one runtime walked through the families that share its device scratch (tests/family_journeys.py): point sets and the map
forms through d_points, d_state, d_coeffs and d_starts in growing and shrinking orders; flows, sections and the volume across five
sizes with a map's render on the loaded section; the held pictures of plane, period, basin and FTLE with the basin probes, across a
resize; the frame writers under auto exposure and auto colour range; a member of a frame
group between its neighbours' renders, two of its steps timed; and the timing spans after other families' calls. Every answer and
every frame equals its restatement bit for bit — the plane and FTLE images on the pixels include/sar.h states exactly, within one unit
on the others —; a failure names the journey, the step, the family and the first element that differs."""
import numpy as np
import pytest

import family_journeys as J
import flow_cases as FK
import rqa_cases as QK
import rqa_restatement as Q
import section_cases as SK
import volume_cases as VK
import volume_edge_cases as VE
import volume_restatement as V

pytestmark = pytest.mark.gpu

SIZE = (48, 40)                                    # of the runtimes the point sets and the map forms are lent


def _runtime(sar, size=SIZE):
    return sar.Runtime(sar.Config.solar_sail(width=size[0], height=size[1]), device=0)


def _frame(rt) -> dict:
    return {"frame." + f: v for f, v in J.frame_dict(dict(count=rt.count(), zbuf=rt.zbuf(), steps=rt.steps(), max=rt.max())).items()}


def _record_fields(recs) -> dict:
    return dict(status=recs["status"].astype(np.int64), fail_job=recs["fail_job"].astype(np.int64),
                fail_step=recs["fail_step"].astype(np.int64), extent=recs["extent"])


def _run_set(sar, rt, st) -> dict:
    a = dict(st.args)
    pts = J.point_sets(a["t"], a["jobs"], a["sets"])
    if st.family == "pairs":
        hist, cnt = sar.pair_histogram(rt, pts, samples=a["t"], counts=True)
        return dict(hist=hist, counted=cnt["counted"], skipped=cnt["skipped"])
    if st.family == "plot":
        return dict(plot=sar.recurrence_plot(rt, pts[0], eps2=QK.EPS2))
    if st.family == "boxes":
        rows = sar.box_counts(rt, pts, origin=J.BOX_CUBE[0], size=J.BOX_CUBE[1], levels=16)
        return {f: rows[f] for f in rows.dtype.names}
    if st.family == "spectra":
        power, recs = sar.power_spectra(rt, pts, n=a["n"], hop=a["hop"], window="hann", samples=a["t"], records=True)
        return dict(power=power, energy=recs["energy"], jobs=recs["jobs"], segments=recs["segments"])
    diag, vert, recs = sar.recurrence_lines(rt, pts, eps2=QK.EPS2, samples=a["t"], theiler=a["theiler"], line_bins=a["line_bins"], records=True)
    return dict(diag=diag, vert=vert, **{f: recs[f] for f in Q.COUNTS})


def _run_maps(sar, rt, st) -> dict:
    a = dict(st.args)
    ms, starts = J.maps(a["maps"]), J.map_starts(a["jobs"])
    kw = {k: v for k, v in a.items() if k != "maps"}
    if st.family == "corrdim":
        res = sar.correlation_dimension(rt, ms, starts=starts, points=True, **kw)
        out = dict(hist=res.hist, counted=res.records["counted"], skipped=res.records["skipped"])
    elif st.family == "boxdim":
        res = sar.box_dimension(rt, ms, starts=starts, points=True, l_min=1, min_occupancy=2.0, **kw)
        out = {f: res.levels[f] for f in res.levels.dtype.names}
        out.update(origin=res.records["origin"], size=res.records["size"])
    elif st.family == "spectrum":
        res = sar.power_spectrum(rt, ms, starts=starts, points=True, **kw)
        out = dict(power=res.power, energy=res.records["energy"], segments=res.records["segments"])
    else:
        res = sar.recurrence_analysis(rt, ms, starts=starts, points=True, **kw)
        out = dict(diag=res.diag, vert=res.vert, eps2=res.records["eps2"])
        out.update({f: res.records["counts"][f] for f in Q.COUNTS})
    out.update(_record_fields(res.records), points=res.points)
    return out


def _flow_call(sar, rt, st):
    k = FK.Parity(sar, J.arg(st, "case"))
    return sar.render_flow(k.cfg, rt, jobs=len(k.starts), steps=k.steps, starts=k.starts, stats=True, plot=J.arg(st, "plot"),
                           chunk_steps=J.CHUNK_STEPS, **k.params)


def _section_call(sar, rt, st):
    k = SK.Parity(sar, J.arg(st, "case"))
    cfg, _ = J.section_view(sar, st)
    return sar.flow_section(cfg, rt, k.surface, jobs=len(k.starts), starts=k.starts, plot=bool(J.arg(st, "plot")), chunk_steps=J.CHUNK_STEPS,
                            **k.params)


def _volume_answer(v, stats) -> dict:
    out = {"stats." + f: np.asarray(stats[f]) for f in V.STATS}
    out["slabs"] = v.slabs()
    return out


def _run_scene(sar, rt, st, ctx) -> dict:
    """A step of the flow / section / volume journeys; ctx carries the held volume's Python object from step to step."""
    a = dict(st.args)
    got = {}
    if st.family == "size":
        rt.set_width_height(a["width"], a["height"])          # (resets: the size changes at every such step)
        ctx["size"] = (a["width"], a["height"])
    elif st.family == "flow":
        got = J.flow_stats_dict(_flow_call(sar, rt, st))
    elif st.family == "section":
        fs = _section_call(sar, rt, st)
        got = J.section_dict(fs.points, fs.ret, fs.records, fs.stats)
    elif st.family == "volume":
        k = VK.case(a["case"])
        half = k.jobs // 2
        ctx["volume"] = sar.volume(rt, k.config(sar), jobs=half, iterations=k.iterations, slabs=k.slabs, z_range=k.z_range, starts=k.starts[:half])
        got = _volume_answer(ctx["volume"], ctx["volume"].stats)
    elif st.family == "add":
        k = VK.case(a["case"])
        got = _volume_answer(ctx["volume"], ctx["volume"].add(k.starts[k.jobs // 2:]))
    elif st.family == "refuse":
        v = ctx["volume"]
        for call in (v.section, v.slabs, v.march):
            with pytest.raises(sar.SarError, match="holds no volume|the runtime holds"):
                call()
        with pytest.raises(sar.SarError, match="add needs a held volume|the runtime holds"):
            v.add(VK.case(J.J3_VOLUME).starts[:8])
    elif st.family == "load_volume":
        k, z_range = J.loaded_case(a["case"])
        ctx["volume"] = rt.debug_load_volume(k.config(sar), k.vol, z_range)
        got = _volume_answer(ctx["volume"], ctx["volume"].stats)
    elif st.family == "march":
        k = VE.case(a["case"])
        img, stats = ctx["volume"].march(config=k.config(sar, a["label"], a["transparent"]), stats=True, **k.params(a["label"])[1])
        got = dict(image=img, **{"march." + f: np.int64(v) for f, v in stats.items()})
    elif st.family == "load_section":
        count, nearest = ctx["volume"].load_section()
        got = dict(section_count=count, nearest=nearest)
    elif st.family == "density":
        rt.density_filter(samples=a["samples"])
    elif st.family == "render":
        sar.render_jobs(J.map_config(sar, ctx["size"], a["jobs"], a["iters"]), rt, sar.start_points(a["seed"], 0, a["jobs"]))
    got.update(_frame(rt))
    return got


def _run(sar, rt, st, ctx=None) -> dict:
    if st.family in J.SET_FORMS:
        return _run_set(sar, rt, st)
    if st.family in J.MAP_FORMS:
        return _run_maps(sar, rt, st)
    return _run_scene(sar, rt, st, ctx)


def _hold(journey, i, st, got, want):
    bad = J.differences(got, want)
    assert not bad, f"{journey} step {i} ({st.family} {dict(st.args)}): " + "; ".join(bad[:6])


# ---- J1, J2: point sets and the map forms -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", list(J.J1))
def test_j1_point_sets_through_d_points(sar, gpu, order):
    rt = _runtime(sar)
    for i, st in enumerate(J.J1[order]):
        _hold(f"J1 {order}", i, st, _run(sar, rt, st), J.reference(st))
    rt.close()


@pytest.mark.parametrize("order", list(J.J2))
def test_j2_map_forms_through_the_orbit_buffers(sar, gpu, order):
    rt = _runtime(sar)
    for i, st in enumerate(J.J2[order]):
        _hold(f"J2 {order}", i, st, _run(sar, rt, st), J.reference(st))
    rt.close()


# ---- J3: flows, sections and the volume across sizes -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(J.J3))
def test_j3_flows_sections_and_the_volume_across_sizes(sar, gpu, name):
    rt, ctx = _runtime(sar, (16, 16)), {}
    for i, (st, want) in enumerate(zip(J.J3[name], J.walk(sar, name, J.J3[name]))):
        _hold(f"J3 {name}", i, st, _run(sar, rt, st, ctx), want)
    rt.close()


# ---- J4: held pictures ---------------------------------------------------------------------------------------------------------
def _picture(sar, rt, family, small=False):
    """(the family's picture object computed on rt, its records as the reference names them)."""
    import basin_restatement as BR
    import fate_cases as TK
    import ftle_restatement as L
    import period_cases as EK
    if family == "plane":
        p = J.J4_PLANE_SMALL if small else J.J4_PLANE
        pic = sar.lyapunov_plane(rt, *J.plane_args(p), "l1", transient=p["transient"], steps=p["steps"])
        got = {f: (pic.records[f][..., 0] if pic.records[f].ndim == 3 else pic.records[f]) for f in J.PLANE_RAW}
        got["lyapunov"] = pic.lyapunov
    elif family == "period":
        k = EK.HENON_PLANE
        pic = sar.period_plane(rt, k["base"], k["axes"], k["x_range"], k["y_range"], **J.J4_PERIOD)
        got = {f: pic.records[f] for f in ("status", "period", "transient_done", "steps_done", "residual")}
    elif family == "basin":
        pic = sar.basin_map(rt, BR.pitchfork(TK.PITCHFORK_MU), **(J.J4_BASIN_SMALL if small else J.J4_BASIN))
        got = dict(status=pic.status, escape_step=pic.escape_step, label=pic.label, n_attractors=np.int64(pic.n_attractors),
                   box=np.array([tuple(pic.params.box_lo), tuple(pic.params.box_hi)], dtype=np.float64))
    else:
        pic = sar.ftle_map(rt, L.henon(), **J.J4_FTLE)
        got = {f: pic.records[f] for f in L.RECORD_FIELDS}
    return pic, got


def _fates(sar, rt) -> dict:
    f = sar.basin_fates(rt, J.probe_points())
    return {n: f[n] for n in J.probe_reference()}


@pytest.mark.parametrize("name", list(J.J4))
def test_j4_held_pictures_keep_their_records_images_and_probes(sar, gpu, name):
    """Four pictures, each colourised right after it is computed; the four again in reverse order; the basin probes after all of
    that, after a second, smaller plane and a point-set call, on a second basin picture, and after set_width_height to (1, 1) and
    back — which leaves the held pictures, their images and the probes as they were (include/sar.h). Every image is held to the
    restated colorize of the restated records, and is byte for byte the first image of its picture."""
    rt = _runtime(sar, J.J4_SIZE)
    cfg = sar.Config.poisson_saturne()
    palette = cfg.palette_rgb[:cfg.palette_len]
    pics, first = {}, {}
    for i, (st, held) in enumerate(zip(J.J4[name], J.j4_held(J.J4[name]))):
        want = J.j4_reference(st, held, palette)
        what = f"J4 {name} step {i} ({st.family} {dict(st.args)})"
        if st.family == "picture":
            pics[J.arg(st, "of")], got = _picture(sar, rt, J.arg(st, "of"), held[J.arg(st, "of")])
            _hold(f"J4 {name}", i, st, got, want)
        elif st.family == "colorize":
            key = (J.arg(st, "of"), held[J.arg(st, "of")])
            img = pics[key[0]].colorize(cfg)
            bad = J.image_differences(img, *want)
            assert not bad, what + ": " + "; ".join(bad)
            assert img.tobytes() == first.setdefault(key, img).tobytes(), what + ": not the bytes of this picture's first image"
        elif st.family == "fates":
            _hold(f"J4 {name}", i, st, _fates(sar, rt), want)
        elif st.family == "size":
            rt.set_width_height(J.arg(st, "width"), J.arg(st, "height"))
        else:
            _hold(f"J4 {name}", i, st, _run(sar, rt, st), want)
    rt.close()


# ---- J5: frame writers under the modes -------------------------------------------------------------------------------------------
def _moded(sar, size):
    rt = _runtime(sar, size)
    rt.set_exposure()
    rt.set_color_range()
    return rt


@pytest.mark.parametrize("name", list(J.J5))
def test_j5_frame_writers_under_exposure_and_colour_range(sar, gpu, name):
    """After every writer the Gas image equals that of a fresh runtime under the same modes, loaded with the restated frame."""
    rt, ctx = _moded(sar, (16, 16)), {}
    gas = FK.Parity(sar, J.J5_FLOW).cfg.replace(render_kind=sar.SAR_RENDER_GAS)
    for i, (st, want) in enumerate(zip(J.J5[name], J.walk_modes(sar))):
        _run_scene(sar, rt, st, ctx)
        _hold(f"J5 {name}", i, st, _frame(rt), want)
        if st.family in ("size", "load_volume"):
            continue
        fresh = _moded(sar, J.J5_SIZE)
        fresh.load(np.ascontiguousarray(want["frame.count"]), np.ascontiguousarray(want["frame.steps"]), np.ascontiguousarray(want["frame.zbuf"]),
                   int(want["frame.max"]))
        _hold(f"J5 {name}", i, st, dict(image=sar.colorize(gas, rt)), dict(image=sar.colorize(gas, fresh)))
        fresh.close()
    rt.close()


def _launches(rt, call):
    rt.enable_timing(True)
    try:
        call()
        return rt.last_timing().iterate_launches
    finally:
        rt.enable_timing(False)


# ---- J6: a member of a frame group ---------------------------------------------------------------------------------------------
def test_j6_a_member_of_a_frame_group_between_its_neighbours_renders(sar, gpu):
    cfg = sar.Config.poisson_saturne(width=J.J6_SIZE[0], height=J.J6_SIZE[1], iterations=J.J6_NEIGHBOUR["jobs"] * J.J6_NEIGHBOUR["iters"],
                                     jobs_total=J.J6_NEIGHBOUR["jobs"], scale=1.0)
    rts = sar.Runtime.group(cfg, 3)
    wants = [J.reference(st) for st in J.J1_STEPS[:4]] + J.walk(sar, "J3 head", J.J3_HEAD)
    ctx = {}
    for i, (st, want) in enumerate(zip(J.J6_STEPS, wants)):
        _hold("J6", i, st, _run(sar, rts[1], st, ctx), want)
        if st in J.J6_TIMED:                           # the member's spans start afresh: the launches of the same call on a fresh runtime
            fresh = _runtime(sar, ctx.get("size", J.J6_SIZE))
            call = (lambda r: _section_call(sar, r, st)) if st.family == "section" else (lambda r: _run(sar, r, st))
            n = _launches(rts[1], lambda: call(rts[1]))
            assert n >= 1 and n == _launches(fresh, lambda: call(fresh)), f"J6 step {i} ({st.family}): iterate_launches {n}"
            fresh.close()
        for member in (0, 2):
            sar.render_jobs(cfg, rts[member], sar.start_points(100 * member + i, 0, J.J6_NEIGHBOUR["jobs"]))
            _hold(f"J6 member {member}", i, st, _frame(rts[member]), {"frame." + f: v for f, v in J.neighbour_frame(member, i + 1).items()})
    for rt in rts:
        rt.close()


# ---- the timing spans after other families' calls --------------------------------------------------------------------------------
def test_timing_spans_start_afresh_after_other_families(sar, gpu):
    """analysis_begin starts the spans afresh: a timed call at the end of a journey counts the launches it counts on a fresh runtime."""
    timed = J.J1_STEPS[-1]
    used, fresh = _runtime(sar), _runtime(sar)
    for st in J.J1_STEPS[:-1]:
        _run(sar, used, st)
    n = _launches(used, lambda: _run(sar, used, timed))
    assert n >= 1 and n == _launches(fresh, lambda: _run(sar, fresh, timed)), "J1: " + str(timed)
    ctx = {}
    for st in J.J3_STEPS[:3]:
        _run(sar, used, st, ctx)
    fresh.set_width_height(*ctx["size"])
    timed = J.J3_STEPS[3]
    n = _launches(used, lambda: _section_call(sar, used, timed))
    assert n >= 1 and n == _launches(fresh, lambda: _section_call(sar, fresh, timed)), "J3: " + str(timed)
    used.close()
    fresh.close()
