"""CPU: the host half of the basin probes (include/sar.h: sar_runtime_basin_fates, sar_runtime_basin_uncertainty) — the struct
layouts in C, ctypes and the Rust crate, the defaults, every refusal that needs no device, and the restatement: the identity (a pixel's
own start point has the pixel's fate, hit 0), the closed form (uncertain = 2^(10 - k), alpha = 1), the figures recorded for the
pitchfork, and the conditions that keep the GPU tests' exact inputs honest (fate_cases says which cases they bind). No device needed."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import basin_restatement as B
import fate_cases as K
import fate_restatement as F
from basin_cases import PITCHFORK, PITCHFORK_MU, PITCHFORK_WINDOW, preset_coeffs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_basin_fate": "SarBasinFate", "sar_basin_fate_counts": "SarBasinFateCounts", "sar_basin_ladder_params": "SarBasinLadderParams",
           "sar_basin_uncertainty_level": "SarBasinUncertaintyLevel", "sar_basin_ladder_mask": "SarBasinLadderMask"}
ENTRIES = ("sar_basin_ladder_params_default", "sar_runtime_basin_fates", "sar_runtime_basin_uncertainty")
INVALID = 1


def test_struct_layouts_match_c_ctypes_and_rust(sar):
    from strange_attractor_renderer_amd import _abi
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for cname, pyname in STRUCTS.items():
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        for f, _ in getattr(_abi, pyname)._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
    prog += 'printf("%u %d\\n", SAR_BASIN_UNKNOWN, SAR_BASIN_MAX_LEVELS);\nreturn 0;}\n'
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
    assert [int(v) for v in out[k:]] == [sar.SAR_BASIN_UNKNOWN, sar.SAR_BASIN_MAX_LEVELS] == [0xFFFFFFFE, 31]
    assert sar.BASIN_UNKNOWN == F.UNKNOWN == 0xFFFFFFFE and sar.BASIN_NONE == F.NONE
    assert [C.sizeof(getattr(_abi, n)) for n in STRUCTS.values()] == [16, 32, 40, 32, 8]
    for dtype, cls, mine in ((sar.BASIN_FATE_DTYPE, _abi.SarBasinFate, F.FATE_DTYPE), (sar.BASIN_LEVEL_DTYPE, _abi.SarBasinUncertaintyLevel, F.LEVEL_DTYPE),
                             (sar.BASIN_LADDER_MASK_DTYPE, _abi.SarBasinLadderMask, F.MASK_DTYPE)):
        assert dtype.itemsize == C.sizeof(cls) == mine.itemsize and list(dtype.names) == [f for f, _ in cls._fields_] == list(mine.names)
        for f, _ in cls._fields_:
            assert dtype.fields[f][1] == getattr(cls, f).offset == mine.fields[f][1], f
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    for name in ENTRIES:
        assert f"pub fn {name}(" in rs, name
        assert f"{name}(" in hpp, name


def test_defaults(sar):
    from strange_attractor_renderer_amd import _abi
    lib = sar.load_library()
    p = _abi.SarBasinLadderParams()
    assert lib.sar_basin_ladder_params_default(C.byref(p)) == 0
    assert (list(p.dir), p.eps0, p.levels, p.chunk) == ([1.0, 0.0, 0.0], 0.125, 24, 0)
    assert lib.sar_basin_ladder_params_default(None) == INVALID
    q = sar.basin_ladder_params(dir=(0, 1, 0), eps0=0.5, levels=3, chunk=7)
    assert (list(q.dir), q.eps0, q.levels, q.chunk) == ([0.0, 1.0, 0.0], 0.5, 3, 7)
    with pytest.raises(ValueError):
        sar.basin_ladder_params(levels=-1)
    with pytest.raises(AttributeError):
        sar.basin_ladder_params(no_such_field=1)


def _fates(lib, sar, n, pts, out=True, rt=None):
    buf = np.zeros(4, dtype=sar.BASIN_FATE_DTYPE)
    return lib.sar_runtime_basin_fates(rt, n, None if pts is None else pts.ctypes.data_as(C.POINTER(C.c_double)),
                                       buf.ctypes.data_as(C.POINTER(sar._abi.SarBasinFate)) if out else None, None), buf


def test_fates_refusals_need_no_device(sar):
    lib = sar.load_library()
    pts = np.zeros((4, 3))
    for n, p, out, text in ((0, pts, True, "1 to 2^24 points"), (2 ** 24 + 1, pts, True, "1 to 2^24 points"), (4, None, True, "NULL"),
                            (4, pts, False, "NULL")):
        status, buf = _fates(lib, sar, n, p, out)
        assert status == INVALID and text in lib.sar_last_error().decode(), (n, lib.sar_last_error())
    for bad in (np.nan, np.inf, -np.inf):
        q = pts.copy()
        q[2, 1] = bad
        status, buf = _fates(lib, sar, 4, q)
        assert status == INVALID and "must be finite (point 2)" in lib.sar_last_error().decode()
        assert not buf.view(np.uint8).any()                 # refused before anything is written
    # valid arguments get as far as the NULL runtime; the limit itself passes the count's check
    status, _ = _fates(lib, sar, 4, pts)
    assert status == INVALID and "runtime is NULL" in lib.sar_last_error().decode()
    assert lib.sar_runtime_basin_fates(None, 2 ** 24, None, None, None) == INVALID and "NULL" in lib.sar_last_error().decode()


def _ladder(lib, sar, p, n, pts, levels=True, rt=None):
    out = np.zeros(31, dtype=sar.BASIN_LEVEL_DTYPE)
    return lib.sar_runtime_basin_uncertainty(rt, None if p is None else C.byref(p), n, None if pts is None else pts.ctypes.data_as(C.POINTER(C.c_double)),
                                             out.ctypes.data_as(C.POINTER(sar._abi.SarBasinUncertaintyLevel)) if levels else None, None, None), out


@pytest.mark.parametrize("change,text", K.LADDER_REFUSED)
def test_ladder_parameter_refusals_need_no_device(sar, change, text):
    lib = sar.load_library()
    p = sar.basin_ladder_params()
    for k, v in change.items():
        if isinstance(v, tuple):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    status, out = _ladder(lib, sar, p, 4, np.zeros((4, 3)))
    assert status == INVALID and text in lib.sar_last_error().decode(), lib.sar_last_error()
    assert not out.view(np.uint8).any()


def test_ladder_argument_refusals_need_no_device(sar):
    lib = sar.load_library()
    pts = np.zeros((4, 3))
    p = sar.basin_ladder_params()
    for n, q, levels, text in ((0, pts, True, "1 to 2^20 points"), (2 ** 20 + 1, pts, True, "1 to 2^20 points"), (4, None, True, "NULL"),
                               (4, pts, False, "NULL")):
        status, _ = _ladder(lib, sar, p, n, q, levels)
        assert status == INVALID and text in lib.sar_last_error().decode(), (n, lib.sar_last_error())
    q = pts.copy()
    q[3, 0] = np.nan
    status, _ = _ladder(lib, sar, p, 4, q)
    assert status == INVALID and "must be finite (point 3)" in lib.sar_last_error().decode()
    # the limits pass, and NULL parameters are the defaults: as far as the NULL runtime
    for params in (p, None, sar.basin_ladder_params(levels=31), sar.basin_ladder_params(levels=1, eps0=5e-324, chunk=2 ** 32 - 1)):
        status, _ = _ladder(lib, sar, params, 4, pts)
        assert status == INVALID and "runtime is NULL" in lib.sar_last_error().decode(), lib.sar_last_error()
    with pytest.raises(ValueError):
        sar.basin_fates(None, np.zeros((4, 2)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pitchfork_pictures():
    """Both pitchfork pictures restated, with their held pictures: computed once and left unchanged."""
    c = B.pitchfork(PITCHFORK_MU)
    out = []
    for case in range(len(PITCHFORK)):
        kw = K.pitchfork_kw(case)
        r = B.basin_auto(c, **kw)
        out.append((r, F.picture(c, box=r["box"], status=r["status"], label=r["label"], **kw)))
    return out


@pytest.mark.parametrize("case", range(len(PITCHFORK)))
def test_identity_a_pixels_own_start_point_has_the_pixels_fate(pitchfork_pictures, case):
    r, pic = pitchfork_pictures[case]
    kw = K.pitchfork_kw(case)
    starts = B.start(kw["origin"], kw["du"], kw["dv"], kw["width"], kw["height"]).reshape(-1, 3)
    f = F.fates(pic, starts)
    assert np.array_equal(f["status"], r["status"].reshape(-1)) and np.array_equal(f["escape_step"], r["escape_step"].reshape(-1))
    assert np.array_equal(f["label"], r["label"].reshape(-1)) and not f["hit"].any()
    assert (f["status"] == F.DIVERGED).sum() == PITCHFORK[case][3]
    # the table holds exactly the picture's cells, each with the label of its attractor
    assert (pic.table != F.NONE).sum() == r["stats"]["cells"]
    assert np.array_equal(np.bincount(pic.table[pic.table != F.NONE]), r["attractors"]["cells"])


def test_a_point_off_the_plane_and_an_unknown_one(pitchfork_pictures):
    r, pic = pitchfork_pictures[0]
    # off the plane, between pixels: the pitchfork's fixed points attract it
    f = F.fates(pic, [(0.7, 0.4, 0.3), (-0.7, 0.4, -0.3), (5.0, 5.0, 0.0)])
    assert list(f["status"]) == [F.BOUNDED, F.BOUNDED, F.DIVERGED] and set(f["label"][:2]) == {0, 1} and f["label"][2] == F.NONE
    assert list(f["hit"]) == [0, 0, 0] and f["escape_step"][2] >= 1 and not f["escape_step"][:2].any()
    # a table without a label anywhere: every bounded probe is UNKNOWN with hit = steps + 1
    blank = F.Picture(pic.coeffs, pic.transient, pic.steps, pic.grid, pic.box, pic.bound, np.full_like(pic.table, F.NONE))
    g = F.fates(blank, [(0.7, 0.4, 0.3), (5.0, 5.0, 0.0)])
    assert (g["label"][0], g["hit"][0], g["label"][1], g["hit"][1]) == (F.UNKNOWN, pic.steps + 1, F.NONE, 0)
    L = F.ladder(blank, [(0.7, 0.4, 0.3)], (1, 0, 0), 0.25, 3)
    assert list(L["levels"]["unknown"]) == [1, 1, 1] and not L["levels"]["uncertain"].any() and not L["levels"]["tested"].any()
    assert (L["masks"]["unknown_bits"][0], L["masks"]["uncertain_bits"][0]) == (7, 0)


def _closed_picture():
    return F.picture(K.closed_map(), box=K.CLOSED_BOX, **K.CLOSED_KW)


def test_closed_form(sar):
    pic = _closed_picture()
    assert (pic.table != F.NONE).sum() == 1 and pic.table[(2 * 4 + 2) * 4 + 2] == 0            # the origin's cell, label 0
    L = F.ladder(pic, K.closed_base(), K.CLOSED["dir"], K.CLOSED["eps0"], K.CLOSED["levels"])
    lv = L["levels"]
    assert list(lv["uncertain"]) == K.CLOSED_UNCERTAIN == [512, 256, 128, 64, 32, 16, 8, 4, 2, 1]
    assert not lv["unknown"].any() and np.all(lv["tested"] == 1024)
    assert np.array_equal(lv["eps"], 2.0 ** -np.arange(2, 12))
    assert np.all(L["fate0"]["status"] == F.BOUNDED) and not L["fate0"]["label"].any() and not L["fate0"]["hit"].any()
    # base point i is uncertain at the levels with e_k > delta_i = (2 i + 1) 2^-12: a run of low bits
    delta = (2.0 * np.arange(1024) + 1.0) * 2.0 ** -12
    want = (lv["eps"][None, :] > delta[:, None])
    assert np.array_equal(L["masks"]["uncertain_bits"], (want * (1 << np.arange(10))[None, :]).sum(1)) and not L["masks"]["unknown_bits"].any()
    # the fit over all ten levels: f = 2^-k on e = 2^-(k + 1), alpha = 1 — through the package's own fit
    u = sar.BasinUncertainty(sar.basin_ladder_params(**K.CLOSED), K.closed_base(), lv.astype(sar.BASIN_LEVEL_DTYPE), L["fate0"], L["masks"])
    fit = u.fit(min_uncertain=1, f_max=1.0)
    assert abs(fit.alpha - 1.0) < 1e-12 and list(fit.levels) == list(range(1, 11)) and abs(fit.boundary_dimension(1) - 0.0) < 1e-12
    assert fit.alpha_err < 1e-12 and abs(u.boundary_dimension(2, min_uncertain=1, f_max=1.0) - 1.0) < 1e-12
    assert np.array_equal(u.f, 2.0 ** -np.arange(1, 11))
    assert list(u.fit().levels) == [1, 2, 3, 4, 5, 6] and abs(u.fit().alpha - 1.0) < 1e-12      # the defaults: uncertain >= 16, f <= 0.5
    assert list(u.fit(f_max=0.4).levels) == [2, 3, 4, 5, 6]
    alpha, used = F.fit(lv, 1, 1.0)
    assert abs(alpha - 1.0) < 1e-12 and list(used) == list(range(1, 11))
    with pytest.raises(ValueError):
        u.fit(min_uncertain=512)


def _summary(L):
    cls = F.classes(L["fate0"])
    labelled = cls[(cls != F.NONE) & (cls != F.UNKNOWN)]
    return dict(escaped=int((cls == F.NONE).sum()), labels=np.bincount(labelled).tolist(), unknown=int((cls == F.UNKNOWN).sum()))


def _unknown_share(pic, base, case):
    """UNKNOWN probes among all the probes of a ladder case: the base points and both sides of every level."""
    b = np.asarray(base)
    d = np.asarray(case["dir"])
    eps = np.ldexp(case["eps0"], -np.arange(case["levels"]))
    step = d[None, None, :] * eps[None, :, None]
    probes = np.concatenate([b, (b[:, None, :] + step).reshape(-1, 3), (b[:, None, :] - step).reshape(-1, 3)])
    return float((F.classes(F.fates(pic, probes)) == F.UNKNOWN).mean())


def test_recorded_pitchfork_figures(pitchfork_pictures):
    _, pic = pitchfork_pictures[K.RECORDED["case"]]
    base = K.window_points(PITCHFORK_WINDOW, K.RECORDED["n"], K.RECORDED["seed"])
    L = F.ladder(pic, base, K.RECORDED["dir"], K.RECORDED["eps0"], K.RECORDED["levels"])
    assert _summary(L) == K.RECORDED_BASE_FATES
    assert list(L["levels"]["uncertain"][::2]) == K.RECORDED_UNCERTAIN_EVERY_SECOND and not L["levels"]["unknown"].any()
    assert _unknown_share(pic, base, K.RECORDED) <= 0.05


def test_conditions_of_the_sweeps_ladder(pitchfork_pictures):
    _, pic = pitchfork_pictures[K.LADDER["case"]]
    base = K.window_points(PITCHFORK_WINDOW, K.LADDER["n"], K.LADDER["seed"])
    L = F.ladder(pic, base, K.LADDER["dir"], K.LADDER["eps0"], K.LADDER["levels"])
    s = _summary(L)
    assert s == K.LADDER_BASE_FATES and list(L["levels"]["uncertain"]) == K.LADDER_UNCERTAIN
    assert s["escaped"] > 0 and sum(1 for v in s["labels"] if v) >= 2                        # two bounded classes and DIVERGED
    assert (L["levels"]["uncertain"] > 0).sum() >= 3 and (L["levels"]["uncertain"] == 0).sum() >= 1
    assert _unknown_share(pic, base, K.LADDER) <= 0.05
    # the fates' own point sets: prefixes of 700 plane points
    f = F.fates(pic, K.window_points(PITCHFORK_WINDOW, max(K.FATE_NS), 3))
    assert (f["label"] == F.UNKNOWN).mean() <= 0.05 and (f["status"] == F.DIVERGED).any() and {0, 1} <= set(f["label"].tolist())


def test_conditions_of_the_other_cases(sar):
    c = preset_coeffs(sar, "solar_sail")
    r = B.basin_auto(c, **K.SOLAR_KW)
    pic = F.picture(c, box=r["box"], status=r["status"], label=r["label"], **K.SOLAR_KW)
    base = K.window_points(K.SOLAR_KW, K.SOLAR["n"], K.SOLAR["seed"])
    L = F.ladder(pic, base, K.SOLAR["dir"], K.SOLAR["eps0"], K.SOLAR["levels"])
    s = _summary(L)
    assert r["stats"]["attractors"] == 1 and s["escaped"] > 0 and s["labels"][0] > 0           # one attractor: one bounded class
    assert (L["levels"]["uncertain"] > 0).sum() >= 3 and (L["levels"]["uncertain"] == 0).sum() >= 1
    assert _unknown_share(pic, base, K.SOLAR) <= 0.05
    assert _unknown_share(_closed_picture(), K.closed_base(), K.CLOSED) == 0.0
    pk = F.picture(B.pitchfork(PITCHFORK_MU), box=B.UNIT_BOX, **K.GRID1_KW)
    assert (pk.table != F.NONE).sum() == 1 and pk.table[0] == 0
    g = F.ladder(pk, K.window_points(PITCHFORK_WINDOW, K.GRID1["n"], K.GRID1["seed"]), K.GRID1["dir"], K.GRID1["eps0"], K.GRID1["levels"])
    cls = F.classes(g["fate0"])
    assert set(cls.tolist()) == {0, F.NONE} and not g["levels"]["unknown"].any() and g["levels"]["uncertain"][0] > 0   # escape versus stay
