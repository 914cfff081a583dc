"""Journeys of ONE runtime through the analysis families that share its device scratch, and their references
(tests/test_family_journeys_host.py holds the conditions they rely on, tests/test_gpu_family_journeys.py walks them on the device).

Every family's own device test makes a runtime and runs that family alone on it. The families do not own their device memory that
separately (csrc/sar_runtime_impl.hpp), and DevBuf::grow only ever grows: after a shrink a buffer holds what its last owner left,
whichever family that was. The sharing groups, and the journey that walks each:

  d_points                     the staging buffer of pairs, boxes, spectra, recurrence lines and the recurrence plot, and the orbit
                               buffer of their four map forms (read back with points=True)                                J1, J2
  d_state, d_coeffs, d_starts  the four map forms                                                                         J2
  flow scratch, d_keys         render_flow and flow_section; d_keys has the runtime's pixel count and is grown and zeroed by a
                               plotting call only                                                                         J3
  the held volume              dropped by set_width_height; load_section writes the frame the next render's hints meet    J3
  the held pictures            plane, period, basin and FTLE each keep one, with an image buffer; the basin probes read the held
                               basin picture and upload its label table lazily                                           J4
  the frame under the modes    flows, sections, density and a loaded section write what exposure and colour range measure J5

A journey is an ordered list of steps (family, arguments); every step that leaves something observable has a reference — a dict
name -> array — computed here once (functools.lru_cache), shared and read-only, from the families' restatements and case modules
alone. `differences` compares a step's answer with its reference bit for bit and names the first element that differs.

Sizes: at most 2048 points per set, 6 maps, 257 jobs, 3000 steps, images up to 96 x 64."""
import functools
from collections import namedtuple

import numpy as np

import basin_restatement as BR
import box_restatement as B
import corr_restatement as X
import density_restatement as D
import fate_cases as TK
import fate_restatement as T
import flow_cases as FK
import flow_restatement as FR
import ftle_cases as LK
import ftle_restatement as L
import oracle_lib as O
import period_cases as EK
import period_restatement as E
import plane_restatement as N
import rqa_cases as QK
import rqa_restatement as Q
import section_cases as SK
import section_restatement as P
import spectrum_cases as WK
import spectrum_restatement as W
import volume_cases as VK
import volume_edge_cases as VE
import volume_restatement as V
from orbit_cases import logistic

Step = namedtuple("Step", "family args")          # args: a sorted tuple of (name, value), hashable


def step(family, **args) -> Step:
    return Step(family, tuple(sorted(args.items())))


def arg(st: Step, name, default=None):
    return dict(st.args).get(name, default)


SET_FORMS = ("pairs", "plot", "boxes", "spectra", "lines")
MAP_FORMS = ("corrdim", "boxdim", "spectrum", "rqa")
BY_VALUE = ("extent",)                             # of -0.0 and +0.0 a minimum may report either


def _frozen(d: dict) -> dict:
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _first(name, g, w, bad) -> str:
    at = np.argwhere(bad)
    first = tuple(at[0])
    return f"{name}: {len(at)} differ, first at {[int(i) for i in first]}: got {g[first]!r}, want {w[first]!r}"


def differences(got: dict, want: dict) -> list:
    """What differs between a step's answer and its reference: 'name: n differ, first at [index]: got .., want ..'. The names are the
    same on both sides. Floats have the reference's dtype and are compared by their bits (NaN with NaN), the names of BY_VALUE by
    value; integers are compared as integers whatever their width and signedness. One set may answer without the sets' axis."""
    out = [f"{name}: not in the reference" for name in got if name not in want]
    for name, w in want.items():
        if name not in got:
            out.append(f"{name}: missing")
            continue
        g, w = np.asarray(got[name]), np.asarray(w)
        if w.ndim == g.ndim + 1 and w.shape[0] == 1 and w.shape[1:] == g.shape:
            g = g[None]                             # (one set answers without the sets' axis)
        if g.shape != w.shape:
            out.append(f"{name}: shape {g.shape}, want {w.shape}")
            continue
        if w.dtype.kind == "f":
            if g.dtype != w.dtype:
                out.append(f"{name}: dtype {g.dtype}, want {w.dtype}")
                continue
            if name in BY_VALUE:
                bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
            else:
                bits = np.uint64 if w.dtype == np.float64 else np.uint32
                bad = (np.ascontiguousarray(g).view(bits) != np.ascontiguousarray(w).view(bits)) & ~(np.isnan(g) & np.isnan(w))
        elif w.dtype.kind in "iub" and g.dtype.kind in "iub":
            neg_g = g < 0 if g.dtype.kind == "i" else np.zeros(g.shape, dtype=bool)
            neg_w = w < 0 if w.dtype.kind == "i" else np.zeros(w.shape, dtype=bool)
            bad = (neg_g != neg_w) | (g.astype(np.uint64) != w.astype(np.uint64))     # (equal negatives wrap alike)
        else:
            out.append(f"{name}: dtype {g.dtype}, want {w.dtype}")
            continue
        if np.any(bad):
            out.append(_first(name, g, w, bad))
    return out


def image_differences(img, want, exact) -> list:
    """An RGBA16 image against its restatement: bit for bit on the pixels of `exact`, within one unit a channel elsewhere (what
    include/sar.h states for the pixels that pass through the device's logarithm)."""
    img, want = np.asarray(img), np.asarray(want)
    if img.shape != want.shape or img.dtype != np.uint16 or want.dtype != np.uint16:
        return [f"image: {img.dtype} {img.shape}, want {want.dtype} {want.shape}"]
    out = []
    bad = (img != want).any(axis=-1) & exact
    if bad.any():
        out.append(_first("image on the exact pixels", img, want, bad[..., None] & (img != want)))
    far = (np.abs(img.astype(np.int64) - want.astype(np.int64)) > 1) & ~exact[..., None]
    if far.any():
        out.append(_first("image beyond one unit", img, want, far))
    return out


# ---- J1: point sets through d_points ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def point_sets(t, jobs, sets) -> np.ndarray:
    """rqa_cases.noisy_cycle: (sets, jobs * t, 3), points of the unit cube; another stream for every shape."""
    p = QK.noisy_cycle(t, jobs, sets)
    p.setflags(write=False)
    return p


BOX_CUBE = ((-0.25, -0.25, -0.25), 1.5)            # holds the noisy cycle; the multiply by 2^L / 1.5 rounds

J1_STEPS = (
    step("pairs", t=700, jobs=1, sets=3),
    step("plot", t=65, jobs=1, sets=1),
    step("boxes", t=257, jobs=1, sets=1),
    step("spectra", t=2048, jobs=1, sets=2, n=256, hop=128),
    step("lines", t=513, jobs=3, sets=1, theiler=1, line_bins=64),
    step("pairs", t=65, jobs=1, sets=1),
    step("boxes", t=2048, jobs=1, sets=3),
    step("spectra", t=512, jobs=1, sets=1, n=64, hop=32),
    step("lines", t=700, jobs=3, sets=3, theiler=0, line_bins=32),
)
J1 = {"forward": J1_STEPS, "reversed": J1_STEPS[::-1]}


def staged(st: Step):
    """The doubles a set-form step stages in d_points, in the order they lie there; None for another family."""
    if st.family not in SET_FORMS:
        return None
    return point_sets(arg(st, "t"), arg(st, "jobs"), arg(st, "sets")).reshape(-1)


@functools.lru_cache(maxsize=None)
def set_reference(st: Step) -> dict:
    pts = point_sets(arg(st, "t"), arg(st, "jobs"), arg(st, "sets"))
    t = arg(st, "t")
    if st.family == "pairs":
        rows = [X.pair_hist(p, t, 0) for p in pts]
        return _frozen(dict(hist=np.stack([r[0] for r in rows]), counted=np.array([r[1] for r in rows], dtype=np.uint64),
                            skipped=np.array([r[2] for r in rows], dtype=np.uint64)))
    if st.family == "plot":
        return _frozen(dict(plot=Q.matrix(pts[0], QK.EPS2)))
    if st.family == "boxes":
        rows = np.stack([B.level_rows(p, BOX_CUBE[0], BOX_CUBE[1], 16) for p in pts])
        return _frozen({f: rows[f] for f in B.LEVEL_DTYPE.names})
    if st.family == "spectra":
        power, energy, jobs, segs = W.spectra(pts, arg(st, "n"), arg(st, "hop"), W.HANN, t)
        return _frozen(dict(power=power, energy=np.asarray(energy), jobs=np.full(len(pts), jobs, dtype=np.uint32),
                            segments=np.full(len(pts), segs, dtype=np.uint32)))
    assert st.family == "lines"
    rows = [Q.lines(p, QK.EPS2, t, arg(st, "theiler"), arg(st, "line_bins")) for p in pts]
    out = dict(diag=np.stack([r[0] for r in rows]), vert=np.stack([r[1] for r in rows]))
    out.update({f: np.array([r[2][f] for r in rows], dtype=np.uint64) for f in Q.COUNTS})
    return _frozen(out)


# ---- J2: the map forms through d_state / d_coeffs / d_starts / d_points -----------------------------------------------------------
def _henon(a):
    c = WK.henon().copy()
    c[2] = -a
    return c


@functools.lru_cache(maxsize=None)
def maps(n_maps) -> np.ndarray:
    """1: Henon. 4: poisson-saturne, solar-sail (loses jobs that are not the first: DIVERGED), Henon, the logistic map at r = 4.4 (leaves
    from every start point: DIVERGED, fail_job 0). 6: those, the rotation and Henon at a = 1.2."""
    def rows(c):
        return np.concatenate([np.array(list(c.coeff_x)), np.array(list(c.coeff_y)), np.array(list(c.coeff_z))])
    four = [rows(O.poisson_saturne()), rows(O.solar_sail()), WK.henon(), logistic(4.4, 4.4)[0]]
    m = np.stack({1: [WK.henon()], 4: four, 6: four + [WK.rotation(), _henon(1.2)]}[n_maps])
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def map_starts(jobs) -> np.ndarray:
    s = O.start_points(0, 0, jobs)
    s.setflags(write=False)
    return s


J2_STEPS = (
    step("boxdim", maps=1, jobs=5, samples=16, stride=1, transient=200),
    step("corrdim", maps=4, jobs=70, samples=8, stride=3, transient=200, theiler=2),
    J1_STEPS[0],
    step("spectrum", maps=6, jobs=24, segments=3, n=32, hop=16, transient=200),
    step("rqa", maps=6, jobs=20, samples=100, transient=200, theiler=1, line_bins=64),
    J1_STEPS[2],
    step("boxdim", maps=4, jobs=70, samples=8, stride=3, transient=200),
    step("rqa", maps=1, jobs=3, samples=65, transient=50, theiler=0, line_bins=8),
    step("spectrum", maps=4, jobs=20, segments=2, n=16, hop=8, transient=100),
    step("corrdim", maps=1, jobs=5, samples=16, stride=1, transient=200, theiler=0),
)
J2 = {"grow_then_shrink": J2_STEPS, "shrink_then_grow": J2_STEPS[::-1]}


def samples_of(st: Step) -> int:
    if st.family == "spectrum":
        return arg(st, "n") + (arg(st, "segments") - 1) * arg(st, "hop")
    return arg(st, "samples")


@functools.lru_cache(maxsize=None)
def map_reference(st: Step) -> dict:
    a = dict(st.args)
    ms, starts = maps(a["maps"]), map_starts(a["jobs"])
    if st.family == "corrdim":
        rows = [X.corrdim(c, starts, a["samples"], a["stride"], a["transient"], theiler=a["theiler"]) for c in ms]
        out = dict(hist=np.stack([r["hist"] for r in rows]), counted=np.array([r["counted"] for r in rows], dtype=np.uint64),
                   skipped=np.array([r["skipped"] for r in rows], dtype=np.uint64))
    elif st.family == "boxdim":
        rows = [B.boxdim(c, starts, a["samples"], a["stride"], a["transient"], l_min=1, min_occupancy=2.0) for c in ms]
        lv = np.stack([r["levels"] for r in rows])
        out = {f: lv[f] for f in B.LEVEL_DTYPE.names}
        ok = [r["status"] == B.BOUNDED for r in rows]
        out["origin"] = np.stack([np.asarray(r["origin"], dtype=np.float64) if k else np.full(3, np.nan) for r, k in zip(rows, ok)])
        out["size"] = np.array([r["size"] if k else np.nan for r, k in zip(rows, ok)], dtype=np.float64)
    elif st.family == "spectrum":
        rows = [W.spectrum(c, starts, segments=a["segments"], n=a["n"], hop=a["hop"], transient=a["transient"]) for c in ms]
        out = dict(power=np.stack([r["power"] for r in rows]), energy=np.array([r["energy"] for r in rows], dtype=np.float64),
                   segments=np.array([r["segments"] for r in rows], dtype=np.uint32))
    else:
        assert st.family == "rqa"
        rows = [Q.rqa(c, starts, a["samples"], transient=a["transient"], theiler=a["theiler"], line_bins=a["line_bins"]) for c in ms]
        out = dict(diag=np.stack([r["diag"] for r in rows]), vert=np.stack([r["vert"] for r in rows]),
                   eps2=np.array([r["eps2"] for r in rows], dtype=np.float64))
        out.update({f: np.array([r["counts"][f] for r in rows], dtype=np.uint64) for f in Q.COUNTS})
    out.update(status=np.array([r["status"] for r in rows], dtype=np.int64), fail_job=np.array([r["fail_job"] for r in rows], dtype=np.int64),
               fail_step=np.array([r["fail_step"] for r in rows], dtype=np.int64), extent=np.stack([np.asarray(r["extent"]) for r in rows]),
               points=np.stack([r["points"] for r in rows]))
    return _frozen(out)


def reference(st: Step) -> dict:
    return set_reference(st) if st.family in SET_FORMS else map_reference(st)


def footprint(st: Step) -> dict:
    """What a step of J1 / J2 asks of each sharing group, in elements: d_points in points, d_state (with d_starts and d_coeffs) in
    trajectories."""
    if st.family in SET_FORMS:
        return dict(d_points=arg(st, "t") * arg(st, "jobs") * arg(st, "sets"))
    return dict(d_points=arg(st, "maps") * arg(st, "jobs") * samples_of(st), d_state=arg(st, "maps") * arg(st, "jobs"))


def transitions(footprints, families) -> dict:
    """group -> the kinds of change between successive users of the group: 'grow', 'shrink', and 'hand_over' where the user before
    was another family (as reuse_cases.transitions, by sharing group)."""
    kinds, last = {}, {}
    for fp, fam in zip(footprints, families):
        for group, size in fp.items():
            k = kinds.setdefault(group, set())
            if group in last:
                before, who = last[group]
                if size > before:
                    k.add("grow")
                elif size < before:
                    k.add("shrink")
                if who != fam:
                    k.add("hand_over")
            last[group] = (size, fam)
    return kinds


# ---- J3: flows, sections and the volume across sizes ---------------------------------------------------------------------------
CHUNK_STEPS = 64
J3_FLOW_SMALL, J3_SECTION = "lorenz-7x5-j64-s37-k7", "lorenz-z27-64x48-j257-s3-up-t1000"
J3_FLOW_MEASURE, J3_SECTION_MEASURE = "rossler-64x48-j65-s300-k3", "rossler-y0-64x48-j65-s3-up-t200"
J3_FLOW_ONE, J3_SECTION_ONE = "rossler-1x1-j257-s300-k7", "lorenz-z27-1x1-j1-s1-both-t0"
J3_VOLUME, J3_LOADED = "shrink_alt_tiny", "wrap_to_zero"
J3_RENDER = dict(jobs=2048, iters=200, seed=3)

J3_STEPS = (
    step("size", width=7, height=5),
    step("flow", case=J3_FLOW_SMALL, plot=1),
    step("size", width=64, height=48),
    step("section", case=J3_SECTION, plot=1, view="face_on"),
    step("flow", case=J3_FLOW_MEASURE, plot=0),
    step("section", case=J3_SECTION_MEASURE, plot=0),
    step("size", width=1, height=1),
    step("flow", case=J3_FLOW_ONE, plot=1),
    step("section", case=J3_SECTION_ONE, plot=1),
    step("size", width=96, height=64),
    step("volume", case=J3_VOLUME),
    step("add", case=J3_VOLUME),
    step("size", width=64, height=48),
    step("refuse"),
    step("size", width=VE.SMALL[0], height=VE.SMALL[1]),
    step("load_volume", case=J3_LOADED),
    step("march", case=J3_LOADED, label="default", transparent=1),
    step("load_section", case=J3_LOADED),
    step("render", **J3_RENDER),
)
J3 = {"across_sizes": J3_STEPS}
J3_HEAD = J3_STEPS[:6]                              # steps 1-5 of the issue's list: what a member of a frame group also walks


def section_view(sar, st: Step):
    """(config, view) of a section step: the case's own, or — 'face_on' — the plane z = 27 seen squarely (identity rotation, angle 0)
    at a scale that fills the image past its edges, so that crossings land in the first row: below pixel 35, where the 7 x 5 image
    before the resize left its keys, and far beyond it."""
    k = SK.Parity(sar, arg(st, "case"))
    if arg(st, "view") != "face_on":
        return k.cfg, k.view
    cfg = FK.rows_config(sar, sar.flow_coefficients(k.system), k.size, rotation_axis=(0.0, 0.0, 1.0), rotation_angle=0.0,
                         center_camera=(0.0, -30.0, 0.0), scale=1.0 / 48.0, angle=0.0)
    return cfg, FR.view_of(cfg.c)


def frame_dict(f) -> dict:
    return dict(count=np.asarray(f["count"]), zbuf=np.asarray(f["zbuf"]), steps=np.asarray(f["steps"]), max=np.int64(int(f["max"])))


def flow_stats_dict(s) -> dict:
    out = {"stats." + f: np.int64(int(s[f])) for f in FR.COUNTERS}
    out["extent"] = np.asarray(s["extent"], dtype=np.float64)
    return out


def section_dict(points, ret, records, stats) -> dict:
    out = dict(points=np.asarray(points), ret=np.asarray(ret))
    out.update({"records." + f: np.asarray(records[f]) for f in P.RECORD_DTYPE.names})
    out.update({"stats." + f: np.int64(int(stats[f])) for f in P.COUNTERS})
    out["extent"] = np.asarray(stats["extent"], dtype=np.float64)
    for f in ("ret_min", "ret_max", "residual_max"):
        out["value." + f] = np.asarray(stats[f], dtype=np.float64)
    return out


def section_frame(vol, z_range) -> dict:
    """Volume.load_section's docstring in numpy (tests/test_gpu_volume_edges.py): the frame the whole volume's section leaves."""
    count, nearest = V.section(vol)
    lo, hi = z_range
    slabs = vol.shape[0]
    centre = (lo + (nearest.astype(np.float64) + 0.5) * ((hi - lo) / slabs)).astype(np.float32)
    return dict(count=count, zbuf=np.where(nearest >= 0, centre, np.float32(-1.0)).astype(np.float32),
                steps=np.where(nearest >= 0, (nearest.astype(np.float64) + 0.5) / slabs, 0.0), max=int(count.max()))


def loaded_case(name):
    """(case, z_range) of a volume that goes in through debug_load_volume: one of volume_edge_cases, or volume_cases' own result."""
    return (VE.case(name), VE.Z_RANGE) if name in VE.NAMES else (VK.case(name), VK.case(name).z_range)


def map_config(sar, size, jobs, iters):
    return sar.Config.poisson_saturne(width=size[0], height=size[1], iterations=jobs * iters, jobs_total=jobs, scale=1.0)


def oracle_continued(sar, frame, size, jobs, iters, seed) -> dict:
    """The oracle's render of `jobs` x `iters` of poisson-saturne on top of `frame`."""
    ort = O.Runtime(*size)
    ort.count[...], ort.zbuf[...], ort.steps[...] = frame["count"], frame["zbuf"], frame["steps"]
    ort.set_max(int(frame["max"]))
    O.render_jobs(map_config(sar, size, jobs, iters).c, ort, O.start_points(seed, 0, jobs), iters)
    return dict(count=ort.count.copy(), zbuf=ort.zbuf.copy(), steps=ort.steps.copy(), max=int(ort.max))


_WALKED = {}


def walk(sar, name, steps) -> list:
    """The references of a flow / section / volume journey, step by step: every step's dict holds what the call answers and, under
    'frame.*', the runtime's frame after it. A resize leaves a reset frame (the device test resets after it, as the families' own
    tests do)."""
    if name in _WALKED:
        return _WALKED[name]
    out, frame, size, vol = [], None, None, None
    for st in steps:
        a = dict(st.args)
        want = {}
        if st.family == "size":
            size = (a["width"], a["height"])
            frame, vol = FR.empty_frame(*size), None
        elif st.family == "flow":
            k = FK.Parity(sar, a["case"])
            assert k.size == size
            frame, s = FR.flow(k.view, k.starts, k.steps, frame=frame, plot=a["plot"], chunk_steps=CHUNK_STEPS, **k.params)
            want = flow_stats_dict(s)
        elif st.family == "section":
            k = SK.Parity(sar, a["case"])
            assert k.size == size
            points, ret, records, stats, frame = P.section(section_view(sar, st)[1], k.surface, k.starts, frame=frame, plot=a["plot"], **k.params)
            want = section_dict(points, ret, records, stats)
        elif st.family in ("volume", "add"):
            k = VK.case(a["case"])
            assert (k.width, k.height) == size
            half = k.jobs // 2
            if st.family == "volume":
                vol, stats = V.volume(k.view, k.starts[:half], k.iterations, k.slabs, *k.z_range)
            else:
                vol, stats = k.vol, k.stats
            want = {"stats." + f: np.asarray(stats[f]) for f in V.STATS}
            want["slabs"] = vol
        elif st.family == "load_volume":
            k = VE.case(a["case"])
            assert (k.width, k.height) == size
            want = {"stats." + f: np.asarray(k.stats[f]) for f in V.STATS}
            want["slabs"] = k.vol
        elif st.family == "march":
            k = VE.case(a["case"])
            img, stats = k.march(a["label"], a["transparent"])
            want = dict(image=img, **{"march." + f: np.int64(v) for f, v in stats.items()})
        elif st.family == "load_section":
            k = VE.case(a["case"])
            count, nearest = k.section()
            frame = section_frame(k.vol, VE.Z_RANGE)
            want = dict(section_count=count, nearest=nearest)
        elif st.family == "render":
            frame = oracle_continued(sar, frame, size, a["jobs"], a["iters"], a["seed"])
        else:
            assert st.family == "refuse"
        want.update({"frame." + f: v for f, v in frame_dict(frame).items()})
        out.append(_frozen(want))
    _WALKED[name] = out
    return out


def keys_of(frame) -> np.ndarray:
    """The 64-bit depth-and-hue key per pixel that left `frame` on a reset runtime (flow_restatement.resolve, inverted): 0 where no
    key won."""
    zbuf, steps = np.asarray(frame["zbuf"]).reshape(-1), np.asarray(frame["steps"]).reshape(-1)
    key = (FR.sortable32(zbuf) << np.uint64(32)) | FR.sortable32(steps.astype(np.float32))
    return np.where(zbuf != np.float32(-1.0), key, np.uint64(0))


def j3_footprints(steps):
    """(footprints, families) of the flow scratch (trajectories) and d_keys (pixels, plotting calls only) along a journey."""
    fps, fams, size = [], [], None
    for st in steps:
        if st.family == "size":
            size = (arg(st, "width"), arg(st, "height"))
        if st.family in ("flow", "section"):
            jobs = (FK.PARITY[arg(st, "case")][2] if st.family == "flow" else SK.PARITY[arg(st, "case")][3])
            fp = dict(flow_scratch=jobs)
            if arg(st, "plot"):
                fp["d_keys"] = size[0] * size[1]
            fps.append(fp)
            fams.append(st.family)
    return fps, fams


# ---- J4: held pictures ---------------------------------------------------------------------------------------------------------
# the Henon plane of period_cases (a along the columns, b along the rows): beside its BOUNDED pixels it holds DIVERGED ones and, where
# a = 0 exactly, a DEGENERATE one, so the pixels whose colour is bit for bit the restatement's show two colours
J4_PLANE = dict(EK.HENON_PLANE, width=37, height=21, transient=200, steps=300)
J4_PLANE_SMALL = dict(EK.HENON_PLANE, x_range=(-1.45, -0.9), width=8, height=8, transient=50, steps=60)
J4_PERIOD = dict(width=16, height=16, transient=300, max_period=64, eps=1e-9)
J4_BASIN = TK.pitchfork_kw(1)                      # 33 x 17, the pitchfork case of tests/test_gpu_fate.py
# a window that cuts the right basin short: the left one is the larger and takes label 0, so most probes' labels swap; a coarser grid
J4_BASIN_SMALL = dict(origin=(-2.0, -0.5, 0.05), du=(3.0, 0.0, 0.0), dv=(0.0, 3.0, 0.0), width=16, height=9, transient=300, steps=16, grid=4)
J4_FTLE = dict(LK.HENON_GEOMETRY, width=24, height=24, steps=12)
J4_PROBES = dict(n=65, seed=2)                     # fate_cases.LADDER's base points
J4_ORDER = ("plane", "period", "basin", "ftle")
PLANE_RAW = ("status", "transient_done", "steps_done", "log2_exp", "mant")


def plane_args(p) -> tuple:
    """(base, axes, x_range, y_range, width, height) of lyapunov_plane / plane_restatement.plane."""
    return p["base"], p["axes"], p["x_range"], p["y_range"], p["width"], p["height"]


@functools.lru_cache(maxsize=None)
def picture_reference(family, small=False) -> dict:
    """The records of a held picture, by the family's restatement."""
    if family == "plane":
        p = J4_PLANE_SMALL if small else J4_PLANE
        want = N.plane(*plane_args(p), "l1", transient_steps=p["transient"], steps=p["steps"])
        out = {f: (want[f][..., 0] if want[f].ndim == 3 else want[f]) for f in PLANE_RAW}
        out["lyapunov"] = want["lyapunov"][..., 0]
    elif family == "period":
        want = E.period_plane(width=J4_PERIOD["width"], height=J4_PERIOD["height"], **EK.HENON_PLANE,
                              **{k: v for k, v in J4_PERIOD.items() if k not in ("width", "height")})
        out = {f: want[f] for f in ("status", "period", "transient_done", "steps_done", "residual")}
    elif family == "basin":
        want = BR.basin_auto(BR.pitchfork(TK.PITCHFORK_MU), **(J4_BASIN_SMALL if small else J4_BASIN))
        out = {f: want[f] for f in ("status", "escape_step", "label")}
        out["n_attractors"] = np.int64(want["stats"]["attractors"])
        out["box"] = np.array(want["box"], dtype=np.float64)
    else:
        assert family == "ftle"
        want = L.ftle(L.henon(), **J4_FTLE)
        out = {f: want[f] for f in L.RECORD_FIELDS}
    return _frozen(out)


def picture_image(family, palette, small=False):
    """(image, exact) of a held picture's colorize by the family's restatement, from the restated records. `exact` marks the pixels
    that are bit for bit the device's: all of them for period and basin; for the plane those that are not BOUNDED, for FTLE the
    DIVERGED, the EDGE and those without a finite ftle — the others pass through the device's logarithm and may differ by one unit
    (include/sar.h)."""
    want = picture_reference(family, small)
    everywhere = np.ones(want["status"].shape, dtype=bool)
    if family == "plane":
        return N.colorize(want["status"], want["steps_done"], want["lyapunov"], palette), want["status"] != N.BOUNDED
    if family == "period":
        return E.colorize(want["status"], want["period"], palette), everywhere
    if family == "basin":
        return BR.colorize(want["status"], want["escape_step"], want["label"], int(want["n_attractors"]), palette), everywhere
    assert family == "ftle"
    lo, hi = L.window(want["ftle"])
    img = L.colorize(want["status"], want["escape_step"], want["flags"], want["ftle"], palette, lo, hi)
    return img, (want["status"] == L.DIVERGED) | ((want["flags"] & L.EDGE) != 0) | ~np.isfinite(want["ftle"])


@functools.lru_cache(maxsize=None)
def probe_points() -> np.ndarray:
    p = TK.window_points(TK.PITCHFORK_WINDOW, J4_PROBES["n"], J4_PROBES["seed"])
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def probe_reference(small=False) -> dict:
    """fate_restatement.fates of the probe points on the restated held picture."""
    want = picture_reference("basin", small)
    box = (tuple(want["box"][0]), tuple(want["box"][1]))
    pic = T.picture(BR.pitchfork(TK.PITCHFORK_MU), box=box, status=want["status"], label=want["label"], **(J4_BASIN_SMALL if small else J4_BASIN))
    f = T.fates(pic, probe_points())
    return _frozen({n: f[n] for n in T.FATE_DTYPE.names})


J4_SIZE = (48, 40)
J4_STEPS = (
    tuple(st for f in J4_ORDER for st in (step("picture", of=f), step("colorize", of=f)))
    + tuple(step("colorize", of=f) for f in J4_ORDER[::-1])
    + (step("fates"),
       step("picture", of="plane", small=1), step("colorize", of="plane"), J1_STEPS[0], step("fates"),
       step("picture", of="basin", small=1), step("colorize", of="basin"), step("fates"),
       step("size", width=1, height=1), step("size", width=J4_SIZE[0], height=J4_SIZE[1]))
    + tuple(step("colorize", of=f) for f in J4_ORDER)
    + (step("fates"),)
)
J4 = {"held_pictures": J4_STEPS}


def j4_held(steps):
    """Per step, which picture of each family the runtime holds after it: {family: small}."""
    out, held = [], {}
    for st in steps:
        if st.family == "picture":
            held = dict(held, **{arg(st, "of"): bool(arg(st, "small"))})
        out.append(held)
    return out


def j4_reference(st: Step, held: dict, palette):
    """What a step of J4 is held to: a picture's records, (image, exact) of a colorize, the probes' fates, a point-set answer; None
    for a resize."""
    if st.family == "picture":
        return picture_reference(arg(st, "of"), held[arg(st, "of")])
    if st.family == "colorize":
        return picture_image(arg(st, "of"), palette, held[arg(st, "of")])
    if st.family == "fates":
        return probe_reference(held["basin"])
    return reference(st) if st.family in SET_FORMS else None


def j4_footprints(steps):
    """(footprints, users) of the four held pictures along J4, in pixels: a picture call writes its family's, a colorize reads it, the
    probes read the basin's."""
    fps, users = [], []
    for st, held in zip(steps, j4_held(steps)):
        fam = "basin" if st.family == "fates" else arg(st, "of")
        if st.family in ("picture", "colorize", "fates"):
            fps.append({"held_" + fam: picture_reference(fam, held[fam])["status"].size})
            users.append(st.family)
    return fps, users


# ---- J5: frame writers under the modes -----------------------------------------------------------------------------------------
J5_SIZE = (64, 48)
J5_FLOW, J5_SECTION, J5_VOLUME = "lorenz-64x48-j257-s300", "lorenz-z27-64x48-j63-s3-both-t1000", "ps_small"
J5_STEPS = (
    step("size", width=J5_SIZE[0], height=J5_SIZE[1]),
    step("flow", case=J5_FLOW, plot=1),
    step("section", case=J5_SECTION, plot=1, view="face_on"),
    step("density", samples=64),
    step("load_volume", case=J5_VOLUME),
    step("load_section", case=J5_VOLUME),
)
J5 = {"under_the_modes": J5_STEPS}


def walk_modes(sar) -> list:
    """The restated frame after every step of J5 ('frame.*'); the images are compared on the device with a fresh runtime under the
    same modes, loaded with that frame. The volume is volume_cases' own, loaded as the hooks build loads one."""
    if "J5" in _WALKED:
        return _WALKED["J5"]
    out, frame = [], None
    for st in J5_STEPS:
        a = dict(st.args)
        if st.family == "size":
            frame = FR.empty_frame(a["width"], a["height"])
        elif st.family == "flow":
            k = FK.Parity(sar, a["case"])
            frame, _ = FR.flow(k.view, k.starts, k.steps, frame=frame, plot=1, chunk_steps=CHUNK_STEPS, **k.params)
        elif st.family == "section":
            k = SK.Parity(sar, a["case"])
            frame = P.section(section_view(sar, st)[1], k.surface, k.starts, frame=frame, plot=1, **k.params)[4]
        elif st.family == "density":
            c, s, m, _ = D.filter(np.asarray(frame["count"]), np.asarray(frame["steps"]), a["samples"])
            frame = dict(count=c, steps=s, zbuf=frame["zbuf"], max=m)
        elif st.family == "load_section":
            k = VK.case(a["case"])
            frame = section_frame(k.vol, k.z_range)
        out.append(_frozen({"frame." + f: v for f, v in frame_dict(frame).items()}))
    _WALKED["J5"] = out
    return out


def j5_footprints(steps):
    """(footprints, users) of the frame under the modes along J5, in pixels: every writer is another family."""
    writers = [st.family for st in steps if st.family in ("flow", "section", "density", "load_section")]
    return [dict(frame=J5_SIZE[0] * J5_SIZE[1]) for _ in writers], writers


# ---- J6: a member of a frame group -----------------------------------------------------------------------------------------------
J6_SIZE = (64, 48)
J6_STEPS = J1_STEPS[:4] + J3_HEAD
J6_NEIGHBOUR = dict(jobs=640, iters=257)
J6_TIMED = (J1_STEPS[3], J3_HEAD[5])              # one step of each: run again with timing on, after the step and the neighbours' renders


@functools.lru_cache(maxsize=None)
def neighbour_frame(member, visits) -> dict:
    """The frame of member 0 or 2 of the group after `visits` renders without a reset: poisson-saturne at J6_SIZE, the start points of
    seed 100 * member + visit."""
    ort = O.Runtime(*J6_SIZE)
    for v in range(visits):
        c = O.poisson_saturne()
        c.width, c.height, c.jobs_total, c.iterations = J6_SIZE[0], J6_SIZE[1], J6_NEIGHBOUR["jobs"], J6_NEIGHBOUR["jobs"] * J6_NEIGHBOUR["iters"]
        c.scale = 1.0
        O.render_jobs(c, ort, O.start_points(100 * member + v, 0, J6_NEIGHBOUR["jobs"]), J6_NEIGHBOUR["iters"])
    return _frozen(frame_dict(dict(count=ort.count.copy(), zbuf=ort.zbuf.copy(), steps=ort.steps.copy(), max=ort.max)))
