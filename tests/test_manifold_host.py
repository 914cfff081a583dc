"""CPU: the host half of the unstable-manifold family (include/sar.h: sar_manifold_params_default, sar_manifold_pixel, and what
sar_runtime_manifold refuses before it touches a device) — the defaults and the struct layouts against the C header, every refusal
text of sar_manifold.cpp, sar_manifold_pixel against the numpy restatement bit for bit — and the restatement itself: the raster rule
on every small segment, a linear saddle whose manifold is the x axis, and the Henon attractor inside the closure of its saddle's W^u."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import manifold_cases as K
import manifold_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN, INF = math.nan, math.inf


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- defaults and layouts -----------------------------------------------------------------------------------------------------------
def test_defaults_and_layouts(sar):
    from strange_attractor_renderer_amd import _abi
    p = sar.manifold_params()
    assert {f: getattr(p, f) for f, _ in p._fields_ if f != "_pad"} == R.DEFAULTS
    structs = {"sar_manifold_params": _abi.SarManifoldParams, "sar_manifold_branch": _abi.SarManifoldBranch,
               "sar_manifold_record": _abi.SarManifoldRecord}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for cname, cls in structs.items():
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        for f, _ in cls._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
    prog += 'printf("%d %d\\n", SAR_MANIFOLD_OK, SAR_MANIFOLD_DOMAIN_ESCAPED);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    k = 0
    for cls in structs.values():
        assert int(out[k]) == C.sizeof(cls)
        k += 1
        for f, _ in cls._fields_:
            assert int(out[k]) == getattr(cls, f).offset, f
            k += 1
    assert [int(v) for v in out[k:]] == [R.OK, R.DOMAIN_ESCAPED] == [_abi.SAR_MANIFOLD_OK, _abi.SAR_MANIFOLD_DOMAIN_ESCAPED]
    assert [C.sizeof(c) for c in structs.values()] == [24, 64, 112]
    for mine, theirs in ((sar.MANIFOLD_BRANCH_DTYPE, R.BRANCH_DTYPE), (sar.MANIFOLD_RECORD_DTYPE, R.RECORD_DTYPE)):
        assert mine.itemsize == theirs.itemsize and mine.names == theirs.names
        assert [mine.fields[f][1] for f in mine.names] == [theirs.fields[f][1] for f in theirs.names]
    assert sar.MANIFOLD_NONE == R.NONE
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for cls in structs.values():
        body = rs[rs.index(f"pub struct {cls.__name__} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in cls._fields_]
    with pytest.raises(AttributeError):
        sar.manifold_params(chunk=1)   # there is none: nothing is stored per lane


# ---- every refusal, with its text --------------------------------------------------------------------------------------------------
W = "sar_runtime_manifold: "
GOOD = (K.BASE_R, K.DIR_R, 1e-6, 2)
NULLS = W + "the runtime, the branches or an output buffer of the manifold is NULL"
# name, parameters, branches, text
REFUSALS = [
    ("samples_0", dict(samples=0), [GOOD], W + "samples must be 2 to 2^20 points of a fundamental domain (0)"),
    ("samples_1", dict(samples=1), [GOOD], W + "samples must be 2 to 2^20 points of a fundamental domain (1)"),
    ("samples_above", dict(samples=2 ** 20 + 1), [GOOD], W + "samples must be 2 to 2^20 points of a fundamental domain (1048577)"),
    ("steps_65536", dict(steps=65536), [GOOD], W + "steps must be at most 65535 for a manifold (65536)"),
    ("max_span_0", dict(max_span=0), [GOOD], W + "max_span must be 1 to 4096 pixels (0)"),
    ("max_span_4097", dict(max_span=4097), [GOOD], W + "max_span must be 1 to 4096 pixels (4097)"),
    ("bound_0", dict(bound=0.0), [GOOD], W + "bound must be positive and finite"),
    ("bound_nan", dict(bound=NAN), [GOOD], W + "bound must be positive and finite"),
    ("bound_inf", dict(bound=INF), [GOOD], W + "bound must be positive and finite"),
    ("branches_4097", dict(samples=2, steps=0), [GOOD] * 4097, W + "a call takes at most 4096 branches (4097)"),
    ("segments_2_32", dict(samples=2 ** 16 + 1, steps=65535), [GOOD],
     W + "branches * (samples - 1) * (steps + 1) must stay below 2^32 segments (4294967296)"),
    ("lanes_above", dict(samples=2 ** 20, steps=0), [GOOD] * 63, W + "a call takes at most 2^26 lanes, 64 per 63 segments of a branch (67112640)"),
    ("base_nan", {}, [GOOD, ((0.0, NAN, 0.0), K.DIR_R, 1e-6, 2)], W + "branch 1: base, dir and delta must be finite"),
    ("base_inf", {}, [((INF, 0.0, 0.0), K.DIR_R, 1e-6, 2)], W + "branch 0: base, dir and delta must be finite"),
    ("dir_nan", {}, [(K.BASE_R, (1.0, 0.0, NAN), 1e-6, 2)], W + "branch 0: base, dir and delta must be finite"),
    ("dir_inf", {}, [(K.BASE_R, (-INF, 0.0, 0.0), 1e-6, 2)], W + "branch 0: base, dir and delta must be finite"),
    ("delta_nan", {}, [(K.BASE_R, K.DIR_R, NAN, 2)], W + "branch 0: base, dir and delta must be finite"),
    ("delta_inf", {}, [(K.BASE_R, K.DIR_R, INF, 2)], W + "branch 0: base, dir and delta must be finite"),
    ("delta_0", {}, [(K.BASE_R, K.DIR_R, 0.0, 2)], W + "branch 0: delta and dir must not be zero"),
    ("dir_0", {}, [GOOD, GOOD, (K.BASE_R, (0.0, -0.0, 0.0), 1e-6, 2)], W + "branch 2: delta and dir must not be zero"),
    ("period_0", {}, [(K.BASE_R, K.DIR_R, 1e-6, 0)], W + "branch 0: period must be 1 to 128 map steps per return (0)"),
    ("period_129", {}, [(K.BASE_R, K.DIR_R, 1e-6, 129)], W + "branch 0: period must be 1 to 128 map steps per return (129)"),
    ("no_runtime", {}, [GOOD], NULLS),
]


def _call(sar, params, rows, view=None, buffers=True, n=None):
    lib = sar.load_library()
    cfg = K.config_of(sar, view or K.henon_view(64, 48))
    p = sar.manifold_params(**params)
    br = np.ascontiguousarray(R.branches_array(rows))
    npix = min(int(cfg.c.width) * int(cfg.c.height), 1 << 16)   # (a refused call writes nothing)
    count, first = np.zeros(npix, np.uint32), np.zeros(npix, np.uint32)
    recs = np.zeros(max(len(rows), 1), dtype=sar.MANIFOLD_RECORD_DTYPE)
    from strange_attractor_renderer_amd import _abi
    u32 = C.POINTER(C.c_uint32)
    status = lib.sar_runtime_manifold(None, C.byref(cfg.c), C.byref(p), len(rows) if n is None else n,
                                      br.ctypes.data_as(C.POINTER(_abi.SarManifoldBranch)) if buffers else None,
                                      count.ctypes.data_as(u32) if buffers else None, first.ctypes.data_as(u32) if buffers else None,
                                      recs.ctypes.data_as(C.POINTER(_abi.SarManifoldRecord)) if buffers else None)
    return status, lib.sar_last_error().decode()


@pytest.mark.parametrize("name,params,rows,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusal(sar, name, params, rows, text):
    assert _call(sar, params, rows) == (1, text)


def test_every_refusal_text_of_the_family_has_a_row():
    """Each set_error format of sar_manifold.cpp, with its conversions filled in by one of the rows above."""
    text = open(os.path.join(ROOT, "strange_attractor_renderer_amd", "csrc", "sar_manifold.cpp")).read()
    formats = re.findall(r'set_error\(\s*"((?:[^"\\]|\\.)*)"', text)
    assert len(formats) == 10
    rows = [r[3] for r in REFUSALS]
    for f in formats:
        pattern = "^" + re.sub(r"%(?:llu|u|s)", lambda m: r"[0-9]+" if m.group(0) != "%s" else "sar_runtime_manifold", re.escape(f).replace("\\%", "%")) + "$"
        assert any(re.match(pattern, r) for r in rows), f


def test_the_image_the_limits_and_the_empty_call(sar):
    assert _call(sar, {}, [GOOD], view=K.henon_view(4097, 4096)) == (1, W + "the plane must hold 1 to 2^24 pixels (4097 x 4096)")
    assert _call(sar, {}, [GOOD], view=K.henon_view(0, 4))[0] != 0                    # sar_config_validate's refusal, with its status
    assert _call(sar, {}, [], n=0)[0] == 0                                              # no branches: nothing to do, no device needed
    assert _call(sar, {}, [], n=0, buffers=False)[0] == 0
    assert _call(sar, dict(samples=1), [], n=0)[0] == 1                                 # the parameters are checked first
    assert _call(sar, {}, [GOOD], buffers=False) == (1, NULLS)
    # the limits themselves pass the checks: what is left to refuse is the NULL runtime
    assert _call(sar, dict(samples=2 ** 16 + 1, steps=65534), [GOOD]) == (1, NULLS)
    assert _call(sar, dict(samples=2 ** 20, steps=0), [GOOD] * 62) == (1, NULLS)
    assert _call(sar, dict(samples=2, steps=65535, max_span=4096), [(K.BASE_R, K.DIR_R, -1e-300, 128)]) == (1, NULLS)
    lib = sar.load_library()
    assert lib.sar_manifold_params_default(None) == 1
    assert lib.sar_manifold_pixel(None, None, None) == 1
    cfg = sar.Config.solar_sail()
    assert lib.sar_manifold_pixel(C.byref(cfg.c), None, None) == 1


# ---- sar_manifold_pixel against the restatement ---------------------------------------------------------------------------------------
POINTS = [(0.0, 0.0, 0.0), (0.05, 0.02, -0.03), (-0.1, 0.05, 0.1), (0.02, -0.08, 0.04), (0.12, 0.1, -0.1), (-0.2, -0.1, 0.15), (0.1, -0.2, 0.3), (-0.7, 0.4, 0.05), (0.33, 0.33, -0.9), (1e-300, -1e-300, 0.0), (-0.0, 0.0, -0.0),
          (25.0, -40.0, 3.0), (-1e9, 2e12, 7.0), (1e300, 1e300, -1e300), (INF, 0.0, 0.0), (0.0, -INF, 1.0),
          (NAN, 0.0, 0.0), (0.2, NAN, 0.1), (0.2, 0.1, NAN)]


@pytest.mark.parametrize("preset", ["poisson_saturne", "solar_sail"])
@pytest.mark.parametrize("angle", [0.0, 0.7, -2.5])
def test_pixel_equals_the_restatement(sar, preset, angle):
    view = dict(R.G.POISSON if preset == "poisson_saturne" else R.G.SOLAR, angle=angle, width=96, height=64)
    cfg = getattr(sar.Config, preset)(width=96, height=64, angle=angle)
    inside = outside = 0
    on_attractor, q = [], (0.05, 0.05, 0.05)
    for i in range(1016):            # points of the preset's own attractor: the view was made for them
        q = R.G.next_point(view, q)
        if i >= 1000:
            on_attractor.append(q)
    for p in POINTS + on_attractor:
        got, want = sar.manifold_pixel(cfg, p), R.pixel(view, p)
        assert np.array_equal(_bits(got), _bits(want)), (p, got, want)
        placed, X, Y = R.place(want[0:1], want[1:2])
        if placed[0] and 0 <= X[0] < 96 and 0 <= Y[0] < 64:
            inside += 1
        else:
            outside += 1
        if any(v != v for v in p):
            assert not placed[0] and np.isnan(got).any()      # NaN is not placed
    assert inside >= 3 and outside >= 6


def test_pixel_of_the_henon_window_is_the_affine_window(sar):
    """The view of tests/manifold_cases.py is the window its docstring states: x = 1.5 - 3 i / 128, y / KY = (48 - j) 0.9 / 96."""
    cfg = K.config_of(sar, K.henon_view())
    for i, j in ((0, 0), (127, 95), (64, 48), (17, 80)):
        x, y = 1.5 - 3.0 * (i + 0.5) / 128.0, K.KY * (48.0 - (j + 0.5)) * 0.9 / 96.0
        fi, fj = sar.manifold_pixel(cfg, (x, y, 0.123))
        assert (math.floor(fi), math.floor(fj)) == (i, j) and abs(fi - (i + 0.5)) < 1e-9 and abs(fj - (j + 0.5)) < 1e-9


# ---- the restatement itself -----------------------------------------------------------------------------------------------------------
def test_raster_rule_on_every_small_segment():
    """All (dX, dY) with |.| <= 6 from a start off the origin: the plots begin at (X0, Y0); there are max(L, 1) of them, distinct and
    in steps of one along the major axis; no step moves more than 1 in either axis; the end pixel is never reached (L >= 1) — the
    next segment, which starts there, plots it."""
    d = np.arange(-6, 7, dtype=np.int64)
    dX, dY = (g.reshape(-1) for g in np.meshgrid(d, d, indexing="ij"))
    X0, Y0 = np.full(dX.shape, -3, dtype=np.int64), np.full(dX.shape, 5, dtype=np.int64)
    seg, xs, ys = R.raster(X0, Y0, dX, dY)
    for s in range(dX.size):
        pts = sorted(zip(xs[seg == s].tolist(), ys[seg == s].tolist()), key=lambda p: ((p[0] + 3) * int(np.sign(dX[s])), (p[1] - 5) * int(np.sign(dY[s]))))
        L = max(abs(int(dX[s])), abs(int(dY[s])))
        assert len(pts) == max(L, 1) and pts[0] == (-3, 5), (dX[s], dY[s])
        if L == 0:
            continue
        end = (-3 + int(dX[s]), 5 + int(dY[s]))
        assert end not in pts
        major = 0 if abs(int(dX[s])) == L else 1
        assert [p[major] for p in pts] == [(-3, 5)[major] + k * int(np.sign((dX[s], dY[s])[major])) for k in range(L)]
        for p, q in zip(pts, pts[1:] + [end]):
            assert max(abs(q[0] - p[0]), abs(q[1] - p[1])) == 1
        # the exact rule, in Python's integers (// floors)
        assert set(pts) == {(-3 + (2 * k * int(dX[s]) + L) // (2 * L), 5 + (2 * k * int(dY[s]) + L) // (2 * L)) for k in range(L)}
    # the division floors: one plot of a segment going left or up lies at a negative offset that truncation would pull to zero
    seg, xs, ys = R.raster(np.array([0]), np.array([0]), np.array([-1]), np.array([-3]))
    assert sorted(zip(xs.tolist(), ys.tolist())) == [(-1, -2), (0, -1), (0, 0)]


def test_linear_saddle_draws_the_x_axis_and_doubles():
    """x' = 2 x, y' = y / 2, z' = z / 2: W^u of the origin is the x axis. With 16 pixels per unit and the domain [2^-6, 2^-5] every
    coordinate is exact: at step n the curve spans x = 2^(n-6) .. 2^(n-5), fi = 32 - 16 x, so it is floor(32 - 2^(n-2)) -
    floor(32 - 2^(n-1)) pixels long — 0, 0, 1, 2, 4, 8, 16, 32: it doubles — and every plot lies in the row of y = 0."""
    view = dict(x=[0, 2.0, 0, 0, 0, 0, 0, 0, 0, 0], y=[0, 0, 0, 0, 0, 0.5, 0, 0, 0, 0], z=[0, 0, 0, 0, 0, 0, 0, 0, 0.5, 0],
                center_camera=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 1.0), rotation=0.0, scale=0.25, angle=0.0, width=64, height=48)
    branch = R.branches_array([((0.0, 0.0, 0.0), (1.0, 0.0, 0.0), 2.0 ** -6, 1)])
    lengths = []
    for steps in range(8):
        count, first, rec = R.manifold(view, branch, samples=257, steps=steps, max_span=16)
        r = rec[0]
        assert r["status"] == R.OK and r["n_long"] == r["n_dead"] == r["n_far"] == 0 and r["n_drawn"] == 256 * (steps + 1)
        assert tuple(r["a"]) == (2.0 ** -6, 0.0, 0.0) and tuple(r["b"]) == (2.0 ** -5, 0.0, 0.0) and r["alive_end"] == 257
        rows = np.flatnonzero(count.any(axis=1))
        assert rows.tolist() == [24] and np.array_equal(count > 0, first != R.NONE)
        lengths.append(int(r["length_px"]))
    assert np.diff([0] + lengths).tolist() == [0, 0, 1, 2, 4, 8, 16, 32]
    # step 7 reaches x = 4, fi = -32: drawn (placed) and counted in the length, but its plots left of the image are not pixels
    assert int(r["pixels"]) < int(r["n_drawn"]) and count[24, 0] > 0 and first[24, 0] // 4096 == 6


def test_henon_attractor_lies_inside_the_manifold():
    """a = 1.4, b = 0.3, the saddle inside the attractor, period 2 (its multiplier is -1.92), delta 1e-6, 4096 samples, 32 steps,
    max_span 16, in the 128 x 96 window: every pixel that 200 000 points of the attractor visit is a manifold pixel — the closure of
    W^u is the attractor. 0 uncovered of 743 visited; 911 manifold pixels; one long segment, at step 32."""
    count, first, rec = K.reference("image_128x96")
    visited = K.attractor_pixels(K.HENON["view"])
    print("visited", visited.size, "uncovered", int((count.reshape(-1)[visited] == 0).sum()), "manifold pixels", int((count > 0).sum()),
          "long", int(rec[0]["n_long"]), "first long step", int(rec[0]["first_long_step"]))
    assert visited.size > 700
    assert int((count.reshape(-1)[visited] == 0).sum()) == 0
    assert rec[0]["status"] == R.OK and rec[0]["alive_end"] == 4096 and rec[0]["n_dead"] == 0 and rec[0]["first_long_step"] >= 30
    assert abs(K.LAMBDA_R - (-1.9237388581534067)) < 1e-12 and K.RIGHT[3] == 2


def test_manifold_branches_from_cycles(sar):
    """manifold_branches on a Cycles made by hand (no device): the two Henon saddles of the stretched map — the left one gives two
    branches of period 1, the right one a single branch of period 2 — with unit eigenvectors, the largest component positive; a
    sink, a source and a saddle with a complex pair outside the unit circle give none."""
    a, b, k = K.A, K.B, K.KY
    slots = np.zeros((1, 8), dtype=sar.CYCLE_ORBIT_DTYPE)
    for i, base in enumerate((K.BASE_L, K.BASE_R)):
        slots[0, i]["rep"], slots[0, i]["period"] = base, 1
        slots[0, i]["M"] = [-2 * a * base[0], 1.0 / k, 0, k * b, 0, 0, 0, 0, 0]
    slots[0, 2]["period"], slots[0, 2]["M"] = 3, np.diag([0.5, -0.5, 0.1]).reshape(9)                         # a sink
    slots[0, 3]["period"], slots[0, 3]["M"] = 1, np.diag([2.0, -3.0, 1.5]).reshape(9)                         # a source
    slots[0, 4]["period"], slots[0, 4]["M"] = 1, [0, -2.0, 0, 2.0, 0, 0, 0, 0, 0.5]                            # a complex pair outside
    slots[0, 5]["period"], slots[0, 5]["M"], slots[0, 5]["rep"] = 4, [0.5, 0, 0, 0, 0.25, 0, 0, 7.0, -3.0], (1.0, 2.0, 3.0)
    recs = np.zeros(1, dtype=sar.CYCLES_RECORD_DTYPE)
    recs["n_orbits"] = 6
    cyc = sar.Cycles(None, np.zeros((1, 30)), np.zeros((1, 3)), recs, slots)
    br, index = sar.manifold_branches(cyc, delta=1e-5)
    assert br.dtype == sar.MANIFOLD_BRANCH_DTYPE and index.tolist() == [0, 0, 1, 5]
    assert br["period"].tolist() == [1, 1, 2, 8] and br["delta"].tolist() == [1e-5, -1e-5, 1e-5, 1e-5]
    assert np.allclose(br["dir"][0], K.DIR_L, atol=1e-12) and np.allclose(br["dir"][1], K.DIR_L, atol=1e-12)
    assert np.allclose(br["dir"][2], K.DIR_R, atol=1e-12) and np.allclose(br["dir"][3], (0.0, 0.0, 1.0), atol=1e-12)
    assert np.allclose(np.sqrt((br["dir"] ** 2).sum(axis=1)), 1.0, atol=1e-15)
    assert tuple(br["base"][2]) == K.BASE_R and tuple(br["base"][3]) == (1.0, 2.0, 3.0)
    empty, none = sar.manifold_branches(sar.Cycles(None, np.zeros((1, 30)), np.zeros((1, 3)), np.zeros(1, dtype=sar.CYCLES_RECORD_DTYPE), slots))
    assert empty.shape == (0,) and empty.dtype == sar.MANIFOLD_BRANCH_DTYPE and none.shape == (0,)
