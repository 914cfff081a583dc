"""CPU: the host half of the FTLE maps (include/sar.h: sar_ftle_*) and their reference. The numpy restatement is what the GPU tests
hold the library to, so it is itself held to analysis here: a linear map, whose stretching is a generalised eigenvalue, and the two
fixed points of the Henon map, whose unstable multipliers are known in closed form. Then the classes of pixel on the Henon plane,
the degenerate shapes' finish, the defaults, sar_ftle_start against sar_basin_start bit for bit, the struct layouts in C, ctypes
and the Rust crate, and every refusal with its exact text. No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import ftle_restatement as F
from ftle_cases import ACCEPTED, DEGENERATE, HENON_SMALL, REFUSED, refused_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_ftle_params": "SarFtleParams", "sar_ftle_pixel": "SarFtlePixel", "sar_ftle_stats": "SarFtleStats",
           "sar_ftle_colors": "SarFtleColors"}
INVALID = 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the reference against analysis ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 4, 8])
def test_restated_linear_map_has_the_generalised_eigenvalue(steps):
    """For p' = A p every difference quotient is A^N applied to the plane's steps, one-sided or not: every pixel's stretch2 is the
    largest generalised eigenvalue of (A^N H)^T (A^N H) against H^T H, H = [hu hv]. Tolerance 1e-12 relative: the restatement's own
    error is the cancellation in e_R - e_L, some 1e-14 at these sizes; the factor 100 is for numpy.linalg's eigenvalue routine."""
    A = np.random.default_rng(1).uniform(-1.2, 1.2, (3, 3))
    origin, du, dv, w, h = (-0.3, 0.2, 0.1), (0.5, 0.1, 0.0), (-0.1, 0.4, 0.2), 9, 7
    r = F.ftle(F.linear(A), origin, du, dv, w, h, steps)
    assert np.all(r["status"] == F.BOUNDED) and not (r["flags"] & (F.EDGE | F.NO_U | F.NO_V)).any()
    assert ((r["flags"] & F.ONE_SIDED_U) != 0).sum() == 2 * h and ((r["flags"] & F.ONE_SIDED_V) != 0).sum() == 2 * w
    H = np.stack([np.array(du) / (w - 1), np.array(dv) / (h - 1)], axis=1)
    P = np.linalg.matrix_power(A, steps) @ H
    want = np.linalg.eigvals(np.linalg.solve(H.T @ H, P.T @ P)).real.max()
    err = np.abs(r["stretch2"] - want) / want
    print("linear map, N =", steps, ": largest relative error of stretch2", err.max())
    assert err.max() <= 1e-12
    assert np.allclose(r["ftle"], math.log(want) / (2 * steps), rtol=0, atol=1e-12)


@pytest.mark.parametrize("x_star,ln_mu", [(0.6313544770895047, 0.65427061), (-1.1313544770895048, 1.18167262)])
def test_restated_henon_fixed_points_grow_by_their_unstable_multiplier(x_star, ln_mu):
    """A 3 x 3 plane of spacing 1e-6 centred on a fixed point of the Henon map: between N = 4 and N = 8 the centre pixel's stretch2
    grows by mu_u^8, mu_u = -a x* -+ sqrt(a^2 x*^2 + b). Tolerance 1e-5, set by the nonlinearity at this spacing."""
    a, b, d = 1.4, 0.3, 1e-6
    mu = max(abs(-a * x_star + math.sqrt(a * a * x_star * x_star + b)), abs(-a * x_star - math.sqrt(a * a * x_star * x_star + b)))
    assert abs(math.log(mu) - ln_mu) < 1e-8                                          # the closed form is the recorded figure
    assert abs(1.0 - a * x_star * x_star + b * x_star - x_star) < 1e-15              # and x* a fixed point
    geo = dict(origin=(x_star - d, b * x_star - d, 0.0), du=(2 * d, 0.0, 0.0), dv=(0.0, 2 * d, 0.0), width=3, height=3)
    s = {n: F.ftle(F.henon(a, b), steps=n, **geo) for n in (4, 8)}
    assert all(np.all(r["status"] == F.BOUNDED) and r["flags"][1, 1] == 0 for r in s.values())
    rate = (math.log(s[8]["stretch2"][1, 1]) - math.log(s[4]["stretch2"][1, 1])) / 8.0
    print("Henon fixed point", x_star, ": rate", rate, "ln|mu_u|", math.log(mu), "difference", abs(rate - math.log(mu)))
    assert abs(rate - ln_mu) <= 1e-5


@pytest.fixture(scope="module")
def henon_small():
    return F.ftle(F.henon(), **HENON_SMALL)


def test_restated_henon_plane_holds_every_class_of_pixel(henon_small):
    r = henon_small
    fl, bounded = r["flags"], r["status"] == F.BOUNDED
    assert bounded.any() and (~bounded).any()
    two_u, two_v = bounded & ((fl & (F.ONE_SIDED_U | F.NO_U)) == 0), bounded & ((fl & (F.ONE_SIDED_V | F.NO_V)) == 0)
    for name, mask in (("edge", (fl & F.EDGE) != 0), ("two-sided in both axes", two_u & two_v), ("one-sided u", (fl & F.ONE_SIDED_U) != 0),
                       ("one-sided v", (fl & F.ONE_SIDED_V) != 0), ("NO_U", (fl & F.NO_U) != 0), ("NO_V", (fl & F.NO_V) != 0),
                       ("isolated", ((fl & F.NO_U) != 0) & ((fl & F.NO_V) != 0)), ("NO_U alone", ((fl & F.NO_U) != 0) & ((fl & F.NO_V) == 0)),
                       ("NO_V alone", ((fl & F.NO_V) != 0) & ((fl & F.NO_U) == 0))):
        print(name, int(mask.sum()))
        assert mask.any(), name
    # what a DIVERGED pixel holds, and what the flags exclude
    assert not fl[~bounded].any() and not r["end"][~bounded].any() and not r["g11"][~bounded].any() and not r["g22"][~bounded].any()
    assert np.isnan(r["stretch2"][~bounded]).all() and np.isnan(r["ftle"][~bounded]).all()
    assert not ((fl & F.ONE_SIDED_U) != 0)[(fl & F.NO_U) != 0].any() and not ((fl & F.ONE_SIDED_V) != 0)[(fl & F.NO_V) != 0].any()
    esc = r["escape_step"]
    assert not esc[bounded].any() and esc[~bounded].min() >= 1 and esc[~bounded].max() <= HENON_SMALL["steps"]
    st = r["stats"]
    assert st["escaped"] + st["bounded"] == st["pixels"] == 37 * 29 and st["isolated"] >= 1 and st["ftle_min"] <= st["ftle_max"]
    # a pixel with both axes has the larger root: at least either axis' own quotient
    m11, _, m22, _ = F.metric(HENON_SMALL["du"], HENON_SMALL["dv"], 37, 29)
    both = two_u & two_v
    assert np.all(r["stretch2"][both] >= np.maximum(r["g11"][both] / m11, r["g22"][both] / m22) * (1 - 1e-12))
    # an isolated pixel: no axis, no number
    iso = ((fl & F.NO_U) != 0) & ((fl & F.NO_V) != 0)
    assert np.isnan(r["stretch2"][iso]).all() and not r["g11"][iso].any() and not r["g22"][iso].any()


def test_restated_edge_is_the_basin_boundary(henon_small):
    """EDGE by its definition, pixel by pixel: a BOUNDED pixel with a DIVERGED 4-neighbour inside the picture."""
    st, fl = henon_small["status"], henon_small["flags"]
    h, w = st.shape
    for y in range(h):
        for x in range(w):
            near = [st[j, i] for j, i in ((y, x + 1), (y, x - 1), (y - 1, x), (y + 1, x)) if 0 <= j < h and 0 <= i < w]
            assert bool(fl[y, x] & F.EDGE) == (st[y, x] == F.BOUNDED and F.DIVERGED in near), (x, y)


def test_restated_differences_are_the_definition(henon_small):
    """a and b written out per pixel from the definition, against the vectorised restatement's Gram entries, bit for bit."""
    r = henon_small
    st, e = r["status"], r["end"]
    h, w = st.shape

    def diff(y, x, plus, minus):
        ok = [0 <= j < h and 0 <= i < w and st[j, i] == F.BOUNDED for j, i in (plus, minus)]
        if ok[0] and ok[1]:
            return (e[plus] - e[minus]) * 0.5
        if ok[0]:
            return e[plus] - e[y, x]
        if ok[1]:
            return e[y, x] - e[minus]
        return np.zeros(3)
    for y in range(h):
        for x in range(w):
            if st[y, x] != F.BOUNDED:
                continue
            a, b = diff(y, x, (y, x + 1), (y, x - 1)), diff(y, x, (y - 1, x), (y + 1, x))
            want = [(a[0] * a[0] + a[1] * a[1]) + a[2] * a[2], (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2], (b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]]
            assert np.array_equal(_bits([r["g11"][y, x], r["g12"][y, x], r["g22"][y, x]]), _bits(want)), (x, y)


@pytest.mark.parametrize("case", range(len(DEGENERATE)))
def test_restated_degenerate_shapes_take_the_1d_or_nan_finish(case):
    kw = DEGENERATE[case]
    r = F.ftle(F.henon(), **kw)
    w, h = kw["width"], kw["height"]
    bounded = r["status"] == F.BOUNDED
    assert bounded.any()
    m11, _, m22, _ = F.metric(kw["du"], kw["dv"], w, h)
    if w == 1:
        assert np.all((r["flags"][bounded] & F.NO_U) != 0) and not r["g11"].any() and not r["g12"].any()
    if h == 1:
        assert np.all((r["flags"][bounded] & F.NO_V) != 0) and not r["g22"].any() and not r["g12"].any()
    if w == 1 and h == 1:
        assert np.isnan(r["stretch2"]).all() and np.isnan(r["ftle"]).all() and r["stats"]["isolated"] == 1
        assert r["stats"]["ftle_min"] == math.inf and r["stats"]["ftle_max"] == -math.inf
        return
    g, m, none = (r["g22"], m22, F.NO_V) if w == 1 else (r["g11"], m11, F.NO_U)
    line = bounded & ((r["flags"] & none) == 0)
    assert line.any() and np.array_equal(_bits(r["stretch2"][line]), _bits(g[line] / m))
    assert np.array_equal(_bits(r["ftle"][line]), _bits([F._log(float(s)) / (2.0 * kw["steps"]) for s in r["stretch2"][line]]))
    assert np.isnan(r["stretch2"][bounded & ~line]).all()


def test_restated_colours():
    status = np.array([[F.DIVERGED, F.BOUNDED, F.BOUNDED, F.BOUNDED, F.BOUNDED]], dtype=np.int32)
    esc = np.array([[32, 0, 0, 0, 0]], dtype=np.uint32)
    flags = np.array([[0, F.EDGE, 0, 0, F.NO_U | F.NO_V]], dtype=np.uint32)
    f = np.array([[math.nan, 0.3, 0.25, -math.inf, math.nan]])
    img = F.colorize(status, esc, flags, f, [(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)], 0.0, 1.0, fade=32.0)
    half = int(np.sqrt(0.5) * 65535.0)
    assert [list(p) for p in img[0]] == [[int(0.25 * 65535.0)] * 3 + [65535], [65535] * 4, [half, 0, half, 65535], [0, 0, 0, 65535], [0, 0, 0, 65535]]


# ---- the library's host side -------------------------------------------------------------------------------------------------
def test_defaults(sar):
    from strange_attractor_renderer_amd import _abi
    lib = sar.load_library()
    p, b = _abi.SarFtleParams(), _abi.SarBasinParams()
    assert lib.sar_ftle_params_default(C.byref(p)) == 0 and lib.sar_basin_params_default(C.byref(b)) == 0
    for f in ("coeffs", "origin", "du", "dv"):
        assert list(getattr(p, f)) == list(getattr(b, f)), f
    assert (p.width, p.height, p.bound) == (b.width, b.height, b.bound) == (256, 256, 1e6) and (p.steps, p.chunk) == (16, 0)
    assert lib.sar_ftle_params_default(None) == INVALID
    c = _abi.SarFtleColors()
    assert lib.sar_ftle_colors_default(C.byref(c)) == 0 and (c.lo, c.hi, c.fade) == (0.0, 1.0, 32.0)
    assert lib.sar_ftle_colors_default(None) == INVALID
    # the defaults are a valid map: they get as far as the NULL runtime
    assert lib.sar_runtime_ftle(None, C.byref(p), None, None) == INVALID
    assert lib.sar_last_error().decode() == "sar_runtime_ftle: the runtime or the pixel buffer is NULL"
    assert lib.sar_runtime_ftle_colorize(None, None, None, None) == INVALID
    assert (sar.SAR_FTLE_EDGE, sar.SAR_FTLE_ONE_SIDED_U, sar.SAR_FTLE_ONE_SIDED_V, sar.SAR_FTLE_NO_U, sar.SAR_FTLE_NO_V) == \
        (F.EDGE, F.ONE_SIDED_U, F.ONE_SIDED_V, F.NO_U, F.NO_V) == (1, 2, 4, 8, 16)


def test_chunk_is_a_parameter_and_no_runtime_option(sar):
    from strange_attractor_renderer_amd import _abi
    assert "chunk" in [f for f, _ in _abi.SarFtleParams._fields_] and not [o for o in _abi.STABLE_OPTIONS if "ftle" in o]


@pytest.mark.parametrize("width,height", [(1, 1), (1, 7), (7, 1), (5, 3), (37, 29), (1000, 3), (4096, 4096)])
def test_start_is_the_basins_bit_for_bit(sar, width, height):
    rng = np.random.default_rng(width * 7 + height)
    origin, du, dv = rng.uniform(-2, 2, 3), rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
    origin[1], du[1] = 0.1, 1e-9           # a span far below the value
    p = sar.ftle_params(np.zeros(30), origin, du, dv, width, height)
    q = sar.basin_params(np.zeros(30), origin, du, dv, width, height)
    lib = sar.load_library()
    got, want = np.empty(3), np.empty(3)
    dp = C.POINTER(C.c_double)
    for x in sorted({0, 1 % width, width // 3, width // 2, width - 1}):
        for y in sorted({0, 1 % height, height // 3, height // 2, height - 1}):
            assert lib.sar_ftle_start(C.byref(p), x, y, got.ctypes.data_as(dp)) == 0
            assert lib.sar_basin_start(C.byref(q), x, y, want.ctypes.data_as(dp)) == 0
            assert np.array_equal(_bits(got), _bits(want)), (x, y)
            if width * height <= 2048:
                assert np.array_equal(_bits(got), _bits(F.start(origin, du, dv, width, height)[y, x]))
    assert lib.sar_ftle_start(C.byref(p), width, 0, got.ctypes.data_as(dp)) == INVALID
    assert lib.sar_ftle_start(C.byref(p), 0, height, got.ctypes.data_as(dp)) == INVALID
    assert lib.sar_ftle_start(C.byref(p), 0, 0, None) == INVALID
    m = sar.FtleMap(None, p, np.zeros((height, width), dtype=sar.FTLE_PIXEL_DTYPE), {})
    assert lib.sar_ftle_start(C.byref(p), width - 1, 0, got.ctypes.data_as(dp)) == 0 and np.array_equal(_bits(m.start(width - 1, 0)), _bits(got))


def test_params_shorthands(sar):
    cfg = sar.Config.poisson_saturne()
    rows = np.stack([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    p = sar.ftle_params(cfg, (0, 0, 0), (1, 0, 0), (0, 1, 0), 9, 8, steps=5, bound=50, chunk=128)
    q = sar.ftle_params(rows, (0, 0, 0), (1, 0, 0), (0, 1, 0), 9, 8)
    assert list(p.coeffs) == list(q.coeffs) == list(rows.reshape(30))
    assert (p.width, p.height, p.steps, p.bound, p.chunk) == (9, 8, 5, 50.0, 128) and (q.steps, q.chunk) == (16, 0)
    rec = np.zeros(1, dtype=sar.SEARCH_RECORD_DTYPE)
    rec["candidate"] = 12
    r = sar.ftle_params(rec[0], (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, search_seed=5)
    assert list(r.coeffs) == list(sar.search_candidate(5, 12).reshape(30))
    with pytest.raises(ValueError):
        sar.ftle_params(np.zeros(29), (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2)
    with pytest.raises(ValueError):
        sar.ftle_params(cfg, (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, steps=-1)
    with pytest.raises(AttributeError):
        sar.ftle_params(cfg, (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, transient=1)


@pytest.mark.parametrize("change,text", REFUSED, ids=[str(k) for k in range(len(REFUSED))])
def test_refusals_need_no_device(sar, change, text):
    p = refused_params(sar, change)
    lib = sar.load_library()
    out = np.empty(3)
    pix = np.zeros(64, dtype=sar.FTLE_PIXEL_DTYPE)
    assert lib.sar_runtime_ftle(None, C.byref(p), pix.ctypes.data_as(C.POINTER(sar._abi.SarFtlePixel)), None) == INVALID
    assert lib.sar_last_error().decode() == text
    assert lib.sar_ftle_start(C.byref(p), 0, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert lib.sar_last_error().decode() == text.replace("sar_runtime_ftle", "sar_ftle_start")
    assert not pix.view(np.uint8).any()


def test_params_null_and_what_passes_the_checks(sar):
    lib = sar.load_library()
    assert lib.sar_runtime_ftle(None, None, None, None) == INVALID
    assert lib.sar_last_error().decode() == "sar_runtime_ftle: the FTLE parameters are NULL"
    for change in ACCEPTED:
        p = refused_params(sar, change)
        assert lib.sar_runtime_ftle(None, C.byref(p), None, None) == INVALID
        assert lib.sar_last_error().decode() == "sar_runtime_ftle: the runtime or the pixel buffer is NULL", change


def test_struct_layouts_match_c_ctypes_and_rust(sar):
    from strange_attractor_renderer_amd import _abi
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for cname, pyname in STRUCTS.items():
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        for f, _ in getattr(_abi, pyname)._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
    prog += 'printf("%u %u %u %u %u\\n", SAR_FTLE_EDGE, SAR_FTLE_ONE_SIDED_U, SAR_FTLE_ONE_SIDED_V, SAR_FTLE_NO_U, SAR_FTLE_NO_V);\nreturn 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    k = 0
    for cname, pyname in STRUCTS.items():
        cls = getattr(_abi, pyname)
        assert int(out[k]) == C.sizeof(cls), cname
        k += 1
        for f, _ in cls._fields_:
            assert int(out[k]) == getattr(cls, f).offset, (cname, f)
            k += 1
    assert [int(v) for v in out[k:]] == [1, 2, 4, 8, 16]
    assert [C.sizeof(getattr(_abi, n)) for n in STRUCTS.values()] == [336, 80, 64, 24]
    dtype, cls = sar.FTLE_PIXEL_DTYPE, _abi.SarFtlePixel
    assert dtype.itemsize == C.sizeof(cls) and list(dtype.names) == [f for f, _ in cls._fields_]
    for f, _ in cls._fields_:
        assert dtype.fields[f][1] == getattr(cls, f).offset, f
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    for name in ("sar_ftle_params_default", "sar_ftle_start", "sar_runtime_ftle", "sar_ftle_colors_default", "sar_runtime_ftle_colorize"):
        assert f"{name}(" in hpp and re.search(rf"pub fn {name}\s*\(", rs), name
