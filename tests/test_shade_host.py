"""CPU: the host half of shaded rendering (include/sar.h: sar_shade_*) — the defaults against the restatement's field by field, every
refusal that needs no device by status and message, the struct layouts in C, ctypes and Rust — and the numpy restatement
(tests/shade_restatement.py) held to properties known independently of it: the normal and the occlusion of a dyadic plane, the pit,
the peak and the flat field, the depth step, the frontal light, the background and the statistics. No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import shade_cases as K
import shade_restatement as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_shade_params": "SarShadeParams", "sar_shade_stats": "SarShadeStats"}
INVALID = 1
F = np.float64


# ---- the library's host half -------------------------------------------------------------------------------------------------------
def test_defaults_are_the_restatements(sar):
    p = sar.shade_params()
    d = S.DEFAULTS
    assert tuple(p.light) == d["light"] and tuple(p.background) == d["background"]
    for f in ("ambient", "diffuse", "specular", "shininess_log2", "ao_radius", "ao_strength", "ao_range", "smooth", "smooth_range",
              "min_count"):
        assert getattr(p, f) == d[f], f
    assert p.has_window == 0 and p.window.applied == 0
    # every public field of the struct is one of the restatement's, or the window
    fields = {f for f, _ in type(p)._fields_ if not f.startswith("_")}
    assert fields == set(d) | {"has_window", "window"}
    assert sar.load_library().sar_shade_params_default(None) == INVALID
    assert (S.MAX_RADIUS, S.MAX_SHININESS_LOG2) == (8, 10)


def test_unknown_field_is_refused(sar):
    with pytest.raises(AttributeError):
        sar.shade_params(radius=3)
    with pytest.raises(AttributeError):
        sar.shade_params(has_window=1)
    with pytest.raises(ValueError):
        sar.shade_params(light=(1.0, 2.0))


REFUSED = [
    (dict(light=(0.0, 0.0, 0.0)), "light"),
    (dict(light=(math.nan, 0.0, 1.0)), "light"),
    (dict(light=(0.0, math.inf, 1.0)), "light"),
    (dict(ambient=-0.1), "ambient"),
    (dict(ambient=math.nan), "ambient"),
    (dict(diffuse=-1.0), "diffuse"),
    (dict(diffuse=math.inf), "diffuse"),
    (dict(specular=-1e-300), "specular"),
    (dict(specular=math.nan), "specular"),
    (dict(shininess_log2=11), "shininess_log2"),
    (dict(ao_radius=9), "ao_radius"),
    (dict(ao_strength=-1.0), "ao_strength"),
    (dict(ao_strength=math.inf), "ao_strength"),
    (dict(ao_range=-1.0), "ao_range"),
    (dict(ao_range=math.nan), "ao_range"),
    (dict(smooth=2), "smooth"),
    (dict(smooth=-1), "smooth"),
    (dict(smooth_range=-0.5), "smooth_range"),
    (dict(smooth_range=math.inf), "smooth_range"),
]


@pytest.mark.parametrize("fields,word", REFUSED, ids=[f"{w}-{i}" for i, (_, w) in enumerate(REFUSED)])
def test_bad_parameters_are_refused_before_anything_else(sar, fields, word):
    lib = sar.load_library()
    p = sar.shade_params(**fields)
    cfg = sar.Config.solar_sail(width=8, height=8)
    for entry in (lib.sar_shade, lib.sar_shade_device):
        assert entry(C.byref(cfg.c), None, C.byref(p), None, None) == INVALID
        msg = lib.sar_last_error().decode()
        assert word in msg and "sar_shade" in msg, msg


def _window(sar, **kw):
    return sar.ColorRange(**{**dict(lo=0.0, hi=1.0), **kw})


@pytest.mark.parametrize("kw", [dict(pos_lo=math.nan), dict(pos_hi=math.inf), dict(lo=0.5, hi=0.5), dict(lo=0.7, hi=0.2),
                                dict(lo=math.nan), dict(hi=math.inf), dict(lo=-1e308, hi=1e308)])
def test_a_window_the_hold_would_refuse_is_refused(sar, kw):
    lib = sar.load_library()
    cfg = sar.Config.solar_sail(width=8, height=8)
    p = sar.shade_params(window=_window(sar, **kw))
    assert lib.sar_shade(C.byref(cfg.c), None, C.byref(p), None, None) == INVALID
    assert "colour range" in lib.sar_last_error().decode()
    assert lib.sar_runtime_hold_color_range(None, C.byref(p.window)) == INVALID and "colour range" in lib.sar_last_error().decode()
    p.has_window = 2
    assert lib.sar_shade(C.byref(cfg.c), None, C.byref(p), None, None) == INVALID and "has_window" in lib.sar_last_error().decode()


def test_a_window_that_is_not_applied_needs_only_finite_positions(sar):
    lib = sar.load_library()
    cfg = sar.Config.solar_sail(width=8, height=8)
    p = sar.shade_params(window=_window(sar, lo=0.7, hi=0.2, applied=False))
    assert lib.sar_shade(C.byref(cfg.c), None, C.byref(p), None, None) == INVALID
    assert "runtime is NULL" in lib.sar_last_error().decode()      # it got past the parameters


def test_null_pointers_and_bad_configs_are_refused(sar):
    lib = sar.load_library()
    cfg = sar.Config.solar_sail(width=8, height=8)
    p = sar.shade_params()
    for entry in (lib.sar_shade, lib.sar_shade_device):
        assert entry(None, None, C.byref(p), None, None) == INVALID and "config is NULL" in lib.sar_last_error().decode()
        assert entry(C.byref(cfg.c), None, C.byref(p), None, None) == INVALID and "runtime is NULL" in lib.sar_last_error().decode()
        assert entry(C.byref(cfg.c), None, None, None, None) == INVALID and "runtime is NULL" in lib.sar_last_error().decode()   # NULL: the defaults
        for scale in (0.0, -1.0, math.nan, math.inf):
            bad = cfg.replace(scale=scale)
            assert entry(C.byref(bad.c), None, C.byref(p), None, None) == INVALID
            assert "width * scale" in lib.sar_last_error().decode(), scale
        assert entry(C.byref(cfg.replace(palette_len=0).c), None, C.byref(p), None, None) == INVALID
        assert "palette_len" in lib.sar_last_error().decode()
    assert sar.load_library().sar_config_validate(C.byref(cfg.replace(render_kind=2).c)) == INVALID      # no new render kind


def test_struct_layouts_match_c_ctypes_and_rust(sar):
    from strange_attractor_renderer_amd import _abi
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for cname, pyname in STRUCTS.items():
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        for f, _ in getattr(_abi, pyname)._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
    prog += 'printf("%d\\n", SAR_ABI_VERSION);\nreturn 0;}\n'
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
    assert k + 1 == len(out) and int(out[k]) == sar.load_library().sar_abi_version() == 12
    assert (C.sizeof(_abi.SarShadeParams), C.sizeof(_abi.SarShadeStats)) == (144, 24)
    assert _abi.SarShadeParams.window.offset == 104 and C.sizeof(_abi.SarColorRange) == 40
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    rust_types = {"c_double": "f64", "c_uint": "u32", "c_int": "i32", "c_ushort": "u16"}
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname
        for (f, t), rt in zip(getattr(_abi, pyname)._fields_, re.findall(r"pub \w+: ([^,]+),", body)):
            if issubclass(t, C.Array):
                want = f"[{rust_types[t._type_.__name__]}; {t._length_}]"
            elif issubclass(t, C.Structure):
                want = t.__name__
            else:
                want = rust_types[t.__name__]
            assert rt == want, (pyname, f, rt, want)
    for fn in ("sar_shade_params_default", "sar_shade", "sar_shade_device"):
        assert f"pub fn {fn}(" in rs, fn


# ---- the restatement itself ----------------------------------------------------------------------------------------------------
def test_host_constants():
    c = S.constants(S.params(light=(0.0, 0.0, 2.0), ao_radius=2), 64, 0.5)
    assert c["k"] == 32.0 and c["L"].tolist() == [0.0, 0.0, 1.0] and c["H"].tolist() == [0.0, 0.0, 1.0]
    assert c["N"] == 12 and c["inv_d"][1] == 1.0 and c["inv_d"][4] == 0.5 and set(c["inv_d"]) == {1, 2, 3, 4}
    assert S.constants(S.params(light=(0.0, 0.0, -1.0)), 64, 0.5)["H"] is None
    assert [S.constants(S.params(ao_radius=R), 1, 1.0)["N"] for R in (0, 1, 3, 8)] == [0, 4, 28, 196]


def _interior(k, R):
    m = R + 2            # beyond the reach of the border: the 3 x 3 mean of a window the border cuts is not its centre, and the
                         # differences and the disc must see none of those
    return slice(m, k.height - m), slice(m, k.width - m)


@pytest.mark.parametrize("name", K.select("plane_dyadic", "70x40") + K.select("plane_dyadic", "96x80"))
def test_dyadic_plane_has_the_formulas_normal_and_the_direct_occlusion(name):
    k = K.case(name)
    p = S.params(**k.params)
    _, stats, d = K.shade(k, detail=True)
    kk = d["constants"]["k"]
    assert kk == 64.0
    a, b = F(2.0 ** -7), F(-(2.0 ** -8))
    sx, sy = a * kk, b * kk
    length = np.sqrt((sx * sx + sy * sy) + F(1.0))
    want = (-sx / length, -sy / length, F(1.0) / length)
    ys, xs = _interior(k, p["ao_radius"])
    assert ys.start < ys.stop and xs.start < xs.stop
    for got, w in zip(d["normal"], want):
        assert np.all(got[ys, xs] == w)
    assert np.array_equal(d["zt"][ys, xs], k.zbuf.astype(F)[ys, xs])          # the mean of a plane's 3 x 3 window is its centre, exactly
    occ = F(0.0)
    for dx, dy, d2 in S.taps(p["ao_radius"]):
        h = (a * dx + b * dy) * kk
        if h > 0 and h <= p["ao_range"]:
            t = h * (F(1.0) / np.sqrt(F(d2)))
            occ = occ + (t if t < 1 else F(1.0))
    assert np.all(d["occ"][ys, xs] == occ)
    assert stats["surface"] == k.width * k.height and stats["isolated"] == 0


@pytest.mark.parametrize("name", K.select("pit_in_flat", "R8") + K.select("pit_in_flat", "R3") + K.select("pit_in_flat", "R1"))
def test_pit_is_occluded(name):
    k = K.case(name)
    _, stats, d = K.shade(k, detail=True)
    y, x = k.height // 2, k.width // 2
    assert d["ao"][y, x] < 1.0 and d["occ"][y, x] > 0.0 and stats["occluded"] >= 1
    if not k.params["smooth"]:
        assert stats["occluded"] == 1 and np.count_nonzero(d["ao"] != 1.0) == 1


@pytest.mark.parametrize("name", K.select("peak_in_flat", "-s0") + tuple(n for n in K.NAMES if n.startswith("flat-")))
def test_peak_and_flat_field_are_not_occluded_where_they_stand(name):
    k = K.case(name)
    _, stats, d = K.shade(k, detail=True)
    y, x = k.height // 2, k.width // 2
    assert d["ao"][y, x] == 1.0 and d["occ"][y, x] == 0.0
    if name.startswith("flat"):
        assert np.all(d["ao"] == 1.0) and stats["occluded"] == 0 and stats["surface"] == k.width * k.height


@pytest.mark.parametrize("name", K.select("two_planes_far_apart", "70x40") + K.select("two_planes_far_apart", "96x80"))
def test_depth_step_keeps_each_sides_normal_and_occludes_nothing_across(name):
    k = K.case(name)
    p = S.params(**k.params)
    _, _, d = K.shade(k, detail=True)
    kk, half, R = d["constants"]["k"], k.width // 2, p["ao_radius"]
    m = max(R, 2)

    def normal(a, b):
        sx, sy = F(a) * kk, F(b) * kk
        length = np.sqrt((sx * sx + sy * sy) + F(1.0))
        return -sx / length, -sy / length, F(1.0) / length

    ys = slice(m, k.height - m)
    e = 2 if p["smooth"] else 0      # (the 3 x 3 mean of a window cut by the step or the border is not its centre: two columns feel it)
    for xs, want in ((slice(e, half - e), normal(2.0 ** -7, 0.0)), (slice(half + e, k.width - e), normal(2.0 ** -7, -(2.0 ** -6)))):
        for got, w in zip(d["normal"], want):
            assert np.all(got[ys, xs] == w), (name, xs)
    # the other side is 8 units (512 pixels of height) away: beyond ao_range, so each side's occlusion is its own plane's
    alone_l, alone_r = k.zbuf.copy(), k.zbuf.copy()
    alone_l[:, half:] = -1.0
    alone_r[:, :half] = -1.0
    occ_l = K.shade(k, zbuf=alone_l, detail=True)[2]["occ"]
    occ_r = K.shade(k, zbuf=alone_r, detail=True)[2]["occ"]
    assert np.array_equal(d["occ"][:, :half], occ_l[:, :half]) and np.array_equal(d["occ"][:, half:], occ_r[:, half:])
    assert np.array_equal(d["zt"][:, :half], K.shade(k, zbuf=alone_l, detail=True)[2]["zt"][:, :half])


@pytest.mark.parametrize("name", K.select("light_ahead_on_flat"))
def test_frontal_light_on_a_flat_field(name):
    k = K.case(name)
    p = S.params(**k.params)
    rgba, _ = K.reference(name)
    r, g, b = S.palette_blend(k.steps, K.PALETTE)
    for ch, col in enumerate((r, g, b)):
        want = S.as_u16(np.minimum(col * F(p["ambient"] + p["diffuse"]) + F(p["specular"]), 1.0) * F(65535.0))
        assert np.array_equal(rgba[..., ch], want), ch
    assert np.all(rgba[..., 3] == 65535)


@pytest.mark.parametrize("name", K.NAMES)
def test_background_and_statistics(name):
    k = K.case(name)
    rgba, stats = K.reference(name)
    p = S.params(**k.params)
    surface = S.surface_mask(k.count, k.zbuf, p["min_count"])
    bgpx = rgba[~surface]
    assert np.all(bgpx[:, :3] == np.array(p["background"], dtype=np.uint16))
    assert np.all(bgpx[:, 3] == (0 if k.cfg["transparent"] else 65535)) and np.all(rgba[surface][:, 3] == 65535)
    assert stats["surface"] + stats["background"] == k.width * k.height and stats["surface"] == int(surface.sum())
    assert stats["isolated"] <= stats["surface"] and stats["occluded"] <= stats["surface"] and stats["smoothed"] <= stats["surface"]
    if not p["smooth"]:
        assert stats["smoothed"] == 0
    if p["ao_radius"] == 0 or p["ao_range"] == 0:
        assert stats["occluded"] == 0


def test_named_surface_rules():
    """What is and what is not surface: the sentinel, the depths that are not numbers, a zero count, min_count."""
    z = np.array([[0.5, -1.0, np.inf, -np.inf, np.nan, -0.0, 1e-42, 0.5, 0.5]], dtype=np.float32)
    c = np.array([[1, 1, 1, 1, 1, 1, 1, 0, 2]], dtype=np.uint32)
    assert S.surface_mask(c, z, 1).tolist() == [[True, False, False, False, False, True, True, False, True]]
    assert S.surface_mask(c, z, 2).tolist() == [[False] * 8 + [True]]
    assert S.surface_mask(c, z, 0).tolist() == [[True, False, False, False, False, True, True, True, True]]


def test_lone_pixels_are_isolated_and_lit_from_the_front():
    for name in K.select("lone_", "33x17", "R8"):
        k = K.case(name)
        _, stats, d = K.shade(k, detail=True)
        assert (stats["surface"], stats["isolated"], stats["occluded"], stats["smoothed"]) == (1, 1, 0, 0), name
        y, x = np.argwhere(d["surface"])[0]
        assert (d["normal"][0][y, x], d["normal"][1][y, x], d["normal"][2][y, x]) == (0.0, 0.0, 1.0)
