"""CPU: the host half of the basins of attraction (include/sar.h: sar_basin_*) — the defaults, sar_basin_start against the numpy
expression bit for bit, the struct layouts in C, ctypes and the Rust crates, every refusal that needs no device, and the restatement
on the pitchfork fixture and on the preset windows the GPU tests use. No device needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import basin_restatement as B
from basin_cases import (PITCHFORK, PITCHFORK_MU, PITCHFORK_WINDOW, PRESET_COUNTS, PRESET_SHAPE, PRESET_STEPS, PRESET_WINDOW, REFUSED,
                         preset_coeffs, refused_params)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_basin_params": "SarBasinParams", "sar_basin_pixel": "SarBasinPixel", "sar_basin_attractor": "SarBasinAttractor",
           "sar_basin_stats": "SarBasinStats", "sar_basin_colors": "SarBasinColors"}
INVALID = 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_defaults(sar):
    from strange_attractor_renderer_amd import _abi
    p = _abi.SarBasinParams()
    lib = sar.load_library()
    assert lib.sar_basin_params_default(C.byref(p)) == 0
    assert list(p.coeffs) == [0.0] * 30
    assert (p.transient, p.steps, p.bound, p.grid) == (1000, 256, 1e6, 32)
    assert (p.width, p.height) == (256, 256) and p.width * p.height <= 2 ** 24
    assert list(p.origin) == [-1.0, -1.0, 0.0] and list(p.du) == [2.0, 0.0, 0.0] and list(p.dv) == [0.0, 2.0, 0.0]
    assert list(p.box_lo) == [-1.0] * 3 and list(p.box_hi) == [1.0] * 3
    assert lib.sar_basin_params_default(None) == INVALID
    c = _abi.SarBasinColors()
    assert lib.sar_basin_colors_default(C.byref(c)) == 0 and c.fade == 32.0
    assert lib.sar_basin_colors_default(None) == INVALID
    # the defaults are a valid picture: they get as far as the NULL runtime
    assert lib.sar_runtime_basin(None, C.byref(p), None, None, 0, None, None) == INVALID and b"runtime" in lib.sar_last_error()
    assert lib.sar_runtime_basin_colorize(None, None, None, None) == INVALID


def test_basin_chunk_is_a_stable_option(sar):
    from strange_attractor_renderer_amd import _abi
    assert "basin_chunk" in _abi.STABLE_OPTIONS


def _start(sar, p, x, y):
    out = np.empty(3)
    assert sar.load_library().sar_basin_start(C.byref(p), x, y, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out


@pytest.mark.parametrize("width,height", [(1, 1), (1, 7), (7, 1), (2, 2), (5, 3), (33, 17), (1000, 3), (4096, 4096)])
def test_start_matches_the_expression(sar, width, height):
    rng = np.random.default_rng(width * 7 + height)
    origin, du, dv = rng.uniform(-2, 2, 3), rng.uniform(-3, 3, 3), rng.uniform(-3, 3, 3)
    du[2] = dv[2] = 0.0                    # an entry that does not move: stays origin's, exactly
    origin[1], du[1] = 0.1, 1e-9           # a span far below the value
    p = sar.basin_params(np.zeros(30), origin, du, dv, width, height)
    xs = sorted({0, 1 % width, width // 3, width // 2, width - 1})
    ys = sorted({0, 1 % height, height // 3, height // 2, height - 1})
    for x in xs:
        tu = np.float64(x) / np.float64(width - 1) if width > 1 else np.float64(0.0)
        for y in ys:
            tv = np.float64(height - 1 - y) / np.float64(height - 1) if height > 1 else np.float64(0.0)
            got = _start(sar, p, x, y)
            assert np.array_equal(_bits(got), _bits((origin + du * tu) + dv * tv)), (x, y)
            assert _bits(got[2:3])[0] == _bits(origin[2:3])[0]
    assert np.array_equal(_bits(_start(sar, p, 0, height - 1)), _bits((origin + du * 0.0) + dv * 0.0))   # the low corner is the origin
    if width * height <= 2048:             # and the vectorised restatement is the same expression
        want = B.start(origin, du, dv, width, height)
        for x in xs:
            for y in ys:
                assert np.array_equal(_bits(_start(sar, p, x, y)), _bits(want[y, x]))
    out = np.empty(3)
    lib = sar.load_library()
    assert lib.sar_basin_start(C.byref(p), width, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert lib.sar_basin_start(C.byref(p), 0, height, out.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert lib.sar_basin_start(C.byref(p), 0, 0, None) == INVALID
    m = sar.BasinMap(None, p, np.zeros((height, width), dtype=sar.BASIN_PIXEL_DTYPE), np.zeros(0, dtype=sar.BASIN_ATTRACTOR_DTYPE), 0, {})
    assert np.array_equal(_bits(m.start(width - 1, 0)), _bits(_start(sar, p, width - 1, 0)))


def test_params_shorthands(sar):
    cfg = sar.Config.poisson_saturne()
    rows = np.stack([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    p = sar.basin_params(cfg, (0, 0, 0), (1, 0, 0), (0, 1, 0), 9, 8, box=((-2, -3, -4), (2, 3, 4)), transient=7, steps=5, grid=3, bound=50)
    q = sar.basin_params(rows, (0, 0, 0), (1, 0, 0), (0, 1, 0), 9, 8)
    assert list(p.coeffs) == list(q.coeffs) == list(rows.reshape(30))
    assert (p.width, p.height, p.transient, p.steps, p.grid, p.bound) == (9, 8, 7, 5, 3, 50.0)
    assert list(p.box_lo) == [-2.0, -3.0, -4.0] and list(p.box_hi) == [2.0, 3.0, 4.0]
    rec = np.zeros(1, dtype=sar.SEARCH_RECORD_DTYPE)
    rec["candidate"] = 12
    r = sar.basin_params(rec[0], (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, search_seed=5)
    assert list(r.coeffs) == list(sar.search_candidate(5, 12).reshape(30))
    with pytest.raises(ValueError):
        sar.basin_params(np.zeros(29), (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2)
    with pytest.raises(ValueError):
        sar.basin_params(cfg, (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, steps=-1)
    with pytest.raises(AttributeError):
        sar.basin_params(cfg, (0, 0, 0), (1, 0, 0), (0, 1, 0), 2, 2, no_such_field=1)


@pytest.mark.parametrize("change,text", REFUSED)
def test_refusals_need_no_device(sar, change, text):
    p = refused_params(sar, change)
    lib = sar.load_library()
    out = np.empty(3)
    pix = np.zeros(64, dtype=sar.BASIN_PIXEL_DTYPE)
    assert lib.sar_runtime_basin(None, C.byref(p), pix.ctypes.data_as(C.POINTER(sar._abi.SarBasinPixel)), None, 0, None, None) == INVALID
    assert text in lib.sar_last_error().decode(), lib.sar_last_error()
    assert lib.sar_basin_start(C.byref(p), 0, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert lib.sar_runtime_basin(None, None, None, None, 0, None, None) == INVALID


def test_limits_pass_the_checks(sar):
    """The largest sizes and step counts are accepted: they get as far as the NULL runtime."""
    lib = sar.load_library()
    for change in (dict(width=4096, height=4096), dict(width=2 ** 24, height=1), dict(transient=2 ** 31, steps=2 ** 31 - 1), dict(grid=128),
                   dict(grid=1), dict(transient=0, steps=0), dict(box_lo=(0, -1e308), box_hi=(0, 1e308))):   # (hi - lo overflows: scale 0)
        p = refused_params(sar, change)
        assert lib.sar_runtime_basin(None, C.byref(p), None, None, 0, None, None) == INVALID
        assert "runtime" in lib.sar_last_error().decode(), change


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
    assert k + 1 == len(out) and int(out[k]) == sar.load_library().sar_abi_version()
    assert [C.sizeof(getattr(_abi, n)) for n in STRUCTS.values()] == [392, 16, 40, 96, 8]
    for dtype, cls in ((sar.BASIN_PIXEL_DTYPE, _abi.SarBasinPixel), (sar.BASIN_ATTRACTOR_DTYPE, _abi.SarBasinAttractor)):
        assert dtype.itemsize == C.sizeof(cls) and list(dtype.names) == [f for f, _ in cls._fields_]
        for f, _ in cls._fields_:
            assert dtype.fields[f][1] == getattr(cls, f).offset, f
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname
    safe = open(os.path.join(ROOT, "bindings", "rust-safe", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    for name in ("sar_basin_params_default", "sar_basin_start", "sar_runtime_basin", "sar_basin_colors_default", "sar_runtime_basin_colorize"):
        assert f"sys::{name}(" in safe, name
        assert f"{name}(" in hpp, name


@pytest.fixture(scope="module")
def pitchfork_restated():
    c = B.pitchfork(PITCHFORK_MU)
    return [B.basin_auto(c, width=shape["width"], height=shape["height"], **PITCHFORK_WINDOW, **steps) for shape, steps, _, _ in PITCHFORK]


def test_the_pitchfork_map_is_what_it_says():
    c = B.pitchfork(2.0)
    import search_restatement as R
    rows = [[c[10 * r + k] for k in range(10)] for r in range(3)]
    x, y, z = R.next_point(rows, np.float64(0.3), np.float64(0.7), np.float64(0.2))
    assert (x, y, z) == (2.0 * 0.3 - 0.3 * 0.7, 0.3 * 0.3, 0.5 * 0.2)
    assert np.count_nonzero(c) == 4


def test_restated_pitchfork_has_the_recorded_basins(pitchfork_restated):
    for r, (shape, steps, sizes, escaped) in zip(pitchfork_restated, PITCHFORK):
        w, h = shape["width"], shape["height"]
        s, a = r["stats"], r["attractors"]
        assert s["attractors"] == 3 and list(a["pixels"]) == sizes
        assert s["escaped_transient"] + s["escaped_tail"] == escaped and s["bounded"] == w * h - escaped == sum(sizes)
        assert s["cells"] == a["cells"].sum() and s["pixels"] == w * h
        esc = r["escape_step"][r["status"] == B.DIVERGED]
        assert esc.min() >= 1 and esc.max() <= steps["transient"] and not r["escape_step"][r["status"] == B.BOUNDED].any()
        if (w, h) == (48, 40):
            assert (esc.min(), esc.max()) == (5, 13)
        # the two large basins mirror each other and settle on x = +-sqrt(mu - 1): their cells lie in opposite halves of the box
        G = steps["grid"]
        assert a["root"][0] < a["root"][1]                                   # equal sizes: sorted by root
        assert a["cell_hi"][0][0] < G // 2 <= a["cell_lo"][1][0]
        assert np.array_equal(r["label"] == 0, (r["label"] == 1)[:, ::-1])
        # the third attractor is the origin: the row y0 = mu (x1 = 0 exactly) and, where the width is odd, the column x0 = 0
        third = r["label"] == 2
        want = np.zeros((h, w), dtype=bool)
        if (h - 1) * 2 % 3 == 0:
            want[h - 1 - (h - 1) * 2 // 3] = True                            # tv = 2/3: y0 = -0.5 + 3 * 2/3 = 1.5
        if w % 2:
            want[:, w // 2] = True                                           # tu = 1/2: x0 = -2 + 4 / 2 = 0
        assert want.any() and np.array_equal(third, want)
        assert np.all(r["root"][r["status"] == B.DIVERGED] == B.NONE) and np.all(r["label"][r["status"] == B.DIVERGED] == B.NONE)
        for k in range(3):
            assert a["first_pixel"][k] == np.flatnonzero(r["label"].reshape(-1) == k)[0]
            assert np.all(r["root"][r["label"] == k] == a["root"][k])


def test_restated_partition_does_not_depend_on_the_order_of_the_pixels(pitchfork_restated):
    """The plane flipped in both axes: the flipped fates and the same set of (root, pixels, cells)."""
    r = pitchfork_restated[1]
    shape, steps, _, _ = PITCHFORK[1]
    o, du, dv = (np.array(PITCHFORK_WINDOW[k]) for k in ("origin", "du", "dv"))
    f = B.basin(B.pitchfork(PITCHFORK_MU), (o + du) + dv, -du, -dv, shape["width"], shape["height"], steps["transient"], steps["steps"],
                steps["grid"], r["box"])
    assert np.array_equal(f["status"], r["status"][::-1, ::-1])
    assert sorted(zip(*(f["attractors"][k].tolist() for k in ("root", "pixels", "cells")))) == \
        sorted(zip(*(r["attractors"][k].tolist() for k in ("root", "pixels", "cells"))))


@pytest.mark.parametrize("name", sorted(PRESET_COUNTS))
def test_preset_windows_hold_both_fates(sar, name):
    r = B.basin_auto(preset_coeffs(sar, name), width=PRESET_SHAPE["width"], height=PRESET_SHAPE["height"], **PRESET_WINDOW, **PRESET_STEPS)
    s = r["stats"]
    escaped = s["escaped_transient"] + s["escaped_tail"]
    assert (escaped, s["bounded"]) == PRESET_COUNTS[name]
    assert escaped >= 0.05 * s["pixels"] and s["bounded"] >= 0.05 * s["pixels"]
    assert s["attractors"] >= 1 and s["cells"] > 8                       # a strange attractor spreads over many cells


def test_colours_restated():
    status = np.array([[B.DIVERGED, B.DIVERGED, B.BOUNDED, B.BOUNDED]], dtype=np.int32)
    esc = np.array([[1, 32, 0, 0]], dtype=np.uint32)
    label = np.array([[B.NONE, B.NONE, 0, 1]], dtype=np.uint32)
    pal = [(1.0, 0.0, 0.0), (0.0, 0.0, 1.0)]
    img = B.colorize(status, esc, label, 2, pal, fade=32.0)
    assert img.shape == (1, 4, 4) and np.all(img[..., 3] == 65535)
    assert list(img[0, 0, :3]) == [int(0.5 * (1.0 / 33.0) * 65535.0)] * 3 and list(img[0, 1, :3]) == [int(0.25 * 65535.0)] * 3
    # v = 0.25 and 0.75 of a two-entry palette (the last one duplicated): n = 0 at t = 0.5, then n = 1 at t = 0.5 between equal entries
    half = int(np.sqrt(0.5) * 65535.0)
    assert list(img[0, 2, :3]) == [half, 0, half] and list(img[0, 3, :3]) == [0, 0, 65535]
