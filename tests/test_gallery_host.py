"""CPU: the host half of the gallery (include/sar.h: sar_gallery_* / sar_frame_view_box) — the default parameters, the layouts of
the three structs in C, ctypes and the Rust sys crate, the ABI version, sar_frame_view_box against a numpy restatement (bit for
bit), the refusals that need no device, and the atlas geometry. No device needed."""
import ctypes as C
import itertools
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from gallery_cases import EXTENT, SEED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_gallery_item": "SarGalleryItem", "sar_gallery_params": "SarGalleryParams", "sar_gallery_stats": "SarGalleryStats"}
INVALID = 1


def test_gallery_params_default(sar):
    p = sar.gallery_params()
    assert (p.tile_width, p.tile_height, p.cols, p.jobs, p.iterations, p.seed) == (128, 128, 8, 1024, 1 << 20, 0)
    q = sar.gallery_params(tile_width=40, tile_height=24, cols=2, seed=9)
    assert (q.tile_width, q.tile_height, q.cols, q.jobs, q.iterations, q.seed) == (40, 24, 2, 1024, 1 << 20, 9)
    with pytest.raises(AttributeError):
        sar.gallery_params(no_such_field=1)
    with pytest.raises(ValueError):
        sar.gallery_params(jobs=-1)
    assert sar.load_library().sar_gallery_params_default(None) == INVALID
    assert "gallery_chunk" in sar._abi.STABLE_OPTIONS


def test_gallery_struct_layouts_match_c_ctypes_and_rust(sar):
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
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()
    k = 0
    for cname, pyname in STRUCTS.items():
        cls = getattr(_abi, pyname)
        assert int(out[k]) == C.sizeof(cls), cname
        k += 1
        for f, _ in cls._fields_:
            assert int(out[k]) == getattr(cls, f).offset, (cname, f)
            k += 1
    # the ABI version of the header is the library's, and it knows the gallery
    assert k + 1 == len(out) and int(out[k]) == sar.load_library().sar_abi_version() and int(out[k]) >= 11
    assert (C.sizeof(_abi.SarGalleryItem), C.sizeof(_abi.SarGalleryParams), C.sizeof(_abi.SarGalleryStats)) == (272, 32, 24)
    assert sar.GALLERY_ITEM_DTYPE.itemsize == 272 and sar.GALLERY_STATS_DTYPE.itemsize == 24
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname


def _box_restatement(sar, cfg, box, margin, sweep):
    """The definition: the box's 8 corners through rotation_matrix() (row . corner, left to right, no fused op), componentwise
    min / max, then sar_frame_view. Returns (status, config)."""
    m = [[float(v) for v in row] for row in cfg.rotation_matrix()]
    pts = []
    for x, y, z in itertools.product(box[0:2], box[2:4], box[4:6]):
        pts.append([m[r][0] * x + m[r][1] * y + m[r][2] * z for r in range(3)])
    ext = []
    for k in range(3):
        ext += [min(p[k] for p in pts), max(p[k] for p in pts)]
    out = cfg.copy()
    st = sar.load_library().sar_frame_view(C.byref(out.c), (C.c_double * 6)(*ext), margin, int(sweep))
    return st, out


def _same_config(a, b):
    return C.string_at(C.byref(a.c), C.sizeof(a.c)) == C.string_at(C.byref(b.c), C.sizeof(b.c))


@pytest.mark.parametrize("preset", ["poisson_saturne", "solar_sail"])
@pytest.mark.parametrize("cand", [545, 2573, 6377])
def test_frame_view_box_equals_its_restatement(sar, preset, cand):
    box = [float(v) for v in EXTENT[cand]]
    for angle, sweep, size in itertools.product((0.0, 0.7), (False, True), ((1920, 1080), (40, 24))):
        cfg = sar.Config.from_coefficients(sar.search_candidate(SEED, cand), base=getattr(sar.Config, preset)())
        cfg = cfg.replace(angle=angle, width=size[0], height=size[1])
        st, want = _box_restatement(sar, cfg, box, 0.05, sweep)
        assert st == 0
        got = sar.frame_view_box(cfg, box, margin=0.05, sweep=sweep)
        assert _same_config(got, want), (preset, cand, angle, sweep, size)
        assert got.scale > 0 and not _same_config(got, cfg)


def test_frame_view_box_of_degenerate_boxes(sar):
    lib = sar.load_library()
    cfg = sar.Config.solar_sail(width=64, height=64)
    flat = [-0.5, 0.75, 0.25, 0.25, -1.0, 0.5]          # zero range in y: what sar_frame_view gives for its rotated extent
    st, want = _box_restatement(sar, cfg, flat, 0.1, False)
    assert st == 0 and _same_config(sar.frame_view_box(cfg, flat, margin=0.1), want)
    point = [0.3, 0.3, -0.2, -0.2, 0.1, 0.1]              # a single point: refused, as sar_frame_view refuses it
    c = cfg.copy()
    assert _box_restatement(sar, cfg, point, 0.05, False)[0] == INVALID
    assert lib.sar_frame_view_box(C.byref(c.c), (C.c_double * 6)(*point), 0.05, 0) == INVALID and _same_config(c, cfg)
    nan = [0.0, 1.0, 0.0, float("nan"), 0.0, 1.0]
    assert lib.sar_frame_view_box(C.byref(c.c), (C.c_double * 6)(*nan), 0.05, 0) == INVALID
    assert lib.sar_frame_view_box(None, (C.c_double * 6)(*flat), 0.05, 0) == INVALID
    assert lib.sar_frame_view_box(C.byref(c.c), None, 0.05, 0) == INVALID


def test_gallery_parameters_are_refused_without_a_device(sar):
    """The parameters are checked before the handles: with a NULL runtime the message tells which check refused the call."""
    lib = sar.load_library()
    base = sar.Config.solar_sail()
    item = (sar._abi.SarGalleryItem * 1)()
    bad_base = base.replace(palette_len=0)
    cases = [(dict(tile_width=0), base, item, "tile side"), (dict(tile_height=0), base, item, "tile side"),
             (dict(tile_width=129, tile_height=128), base, item, "at most 16384 pixels"),
             (dict(tile_width=1, tile_height=16385), base, item, "at most 16384 pixels"), (dict(cols=0), base, item, "cols is 0"),
             (dict(jobs=0), base, item, "jobs is 0"), (dict(jobs=2, iterations=1 << 32), base, item, "below 2^32"),
             (dict(jobs=1, iterations=1 << 40), base, item, "below 2^32"), (dict(), bad_base, item, "palette"),
             (dict(), base, None, "items_host is NULL")]
    for kw, b, it, text in cases:
        p = sar.gallery_params(**kw)
        assert lib.sar_runtime_gallery(None, C.byref(b.c), C.byref(p), 1, it, None, None, None, None, None, None) == INVALID, kw
        assert text in lib.sar_last_error().decode(), (kw, lib.sar_last_error())
    p = sar.gallery_params()
    assert lib.sar_runtime_gallery(None, None, C.byref(p), 1, item, None, None, None, None, None, None) == INVALID
    assert lib.sar_runtime_gallery(None, C.byref(base.c), None, 1, item, None, None, None, None, None, None) == INVALID
    # n == 0 succeeds and writes nothing, whatever the handles; good parameters get as far as the NULL runtime — 129 x 127 is
    # 16 383 pixels and passes, as 128 x 128 and 16384 x 1 do
    assert lib.sar_runtime_gallery(None, C.byref(base.c), C.byref(p), 0, None, None, None, None, None, None, None) == 0
    for size in ((128, 128), (129, 127), (16384, 1)):
        q = sar.gallery_params(tile_width=size[0], tile_height=size[1])
        assert lib.sar_runtime_gallery(None, C.byref(base.c), C.byref(q), 1, item, None, None, None, None, None, None) == INVALID
        assert "runtime" in lib.sar_last_error().decode(), size


def test_gallery_items_and_atlas_geometry(sar):
    base = sar.Config.solar_sail()
    cands = (545, 2573, 6377)
    coeffs = np.stack([sar.search_candidate(SEED, c) for c in cands])            # (3, 3, 10)
    views = [((0.1 * i, -0.2, 0.3), 1.0 + i) for i in range(3)]
    items = sar.gallery_items(coeffs, views, base=base)
    assert items.dtype == sar.GALLERY_ITEM_DTYPE and items.shape == (3,)
    assert np.array_equal(items["coeff"], coeffs.reshape(3, 30))
    assert np.array_equal(items["center_camera"][1], [0.1, -0.2, 0.3]) and list(items["scale"]) == [1.0, 2.0, 3.0]
    records = np.zeros(3, dtype=sar.SEARCH_RECORD_DTYPE)
    for i, c in enumerate(cands):
        records["extent"][i] = EXTENT[c]
    framed = sar.gallery_items(coeffs, base=base, records=records, margin=0.07, sweep=True, tile=(40, 24))
    for i in range(3):
        want = sar.frame_view_box(base.replace(width=40, height=24), EXTENT[cands[i]], margin=0.07, sweep=True)
        assert np.array_equal(framed["center_camera"][i], want.center_camera) and framed["scale"][i] == want.scale
    with pytest.raises(ValueError):
        sar.gallery_items(coeffs, base=base)
    with pytest.raises(ValueError):
        sar.gallery_items(coeffs, views[:2], base=base)
    # n = 5, cols = 2: three rows of two cells
    assert sar.gallery_atlas_shape(5, (40, 24), 2) == (72, 80, 4)
    assert sar.gallery_atlas_shape(6, (40, 24), 2) == (72, 80, 4) and sar.gallery_atlas_shape(7, (40, 24), 2) == (96, 80, 4)
    assert sar.gallery_atlas_shape(0, (40, 24), 2) == (0, 80, 4) and sar.gallery_atlas_shape(3) == (128, 1024, 4)
    g = sar.Gallery(base, sar.gallery_params(tile_width=40, tile_height=24, cols=2), np.zeros(5, dtype=sar.GALLERY_ITEM_DTYPE),
                    np.arange(72 * 80 * 4, dtype=np.uint16).reshape(72, 80, 4), np.zeros(5, dtype=sar.GALLERY_STATS_DTYPE))
    assert g.tile(3).shape == (24, 40, 4) and np.array_equal(g.tile(3), g.image[24:48, 40:80]) and len(g) == 5
    with pytest.raises(IndexError):
        g.tile(5)
    c3 = sar.Gallery(base, sar.gallery_params(tile_width=40, tile_height=24, jobs=7, iterations=99), items, None, None).config(2)
    assert (c3.width, c3.height, c3.iterations, c3.jobs_total, c3.scale) == (40, 24, 99, 7, 3.0)
    assert np.array_equal(c3.coeff_y, coeffs[2, 1]) and np.array_equal(c3.center_camera, [0.2, -0.2, 0.3])
