"""Host: box counting without a device (include/sar.h: sar_box_*, sar_boxdim_*) — the fixed-point logarithm against the restatement,
its exact values and its distance from log2; sar_boxdim_fit against the restatement, on a uniform lattice and without a window; the
restatement itself against closed-form lattices; the defaults and every refusal that needs no device."""
import ctypes as C
import math

import numpy as np
import pytest

import box_cases as K
import box_restatement as B
from corr_cases import henon


def test_log2_equals_the_restatement(sar):
    ns = set(range(1, 4097))
    for k in range(21):
        ns |= {2 ** k - 1, 2 ** k, 2 ** k + 1}
    for n in sorted(ns - {0}):
        if n > 2 ** 20 + 1:
            continue
        assert sar.box_log2_q32(n) == B.lg32(n), n
    assert sar.box_log2_q32(2 ** 32 - 1) == B.lg32(2 ** 32 - 1)


def test_log2_is_exact_at_powers_of_two_and_truncated_elsewhere(sar):
    for k in range(32):
        assert sar.box_log2_q32(2 ** k) == k << 32
    # v / 2^32 is exact in a double (37 bits); math.log2 is within an ulp or two, 2^-47 at these magnitudes
    for n in list(range(1, 4097)) + [2 ** k + d for k in range(2, 21) for d in (-1, 1)] + [999_983, 2 ** 20 - 3]:
        gap = math.log2(n) - sar.box_log2_q32(n) / 2.0 ** 32
        assert -2.0 ** -46 <= gap < 2.0 ** -32 + 2.0 ** -46, (n, gap)


def test_log2_refuses_zero(sar):
    lib = sar.load_library()
    out = C.c_uint64(7)
    assert lib.sar_box_log2_q32(0, C.byref(out)) == 1 and out.value == 7
    assert lib.sar_box_log2_q32(5, None) == 1
    with pytest.raises(sar.SarError):
        sar.box_log2_q32(0)


def test_restatement_rows_of_the_lattices():
    rows = B.level_rows(K.cube_lattice(), levels=6)
    for l in range(7):
        assert tuple(int(v) for v in rows[l]) == K.cube_lattice_row(l), l
    n = 300
    rows = B.level_rows(K.line_lattice(n), levels=16)
    for l in range(11):
        assert int(rows[l]["cells"]) == -(-n // 2 ** (10 - l)), l
    assert all(int(rows[l]["cells"]) == n and int(rows[l]["singles"]) == n for l in range(10, 17))
    assert tuple(int(v) for v in rows[0]) == (1, 0, n * n, n * B.lg32(n))      # level 0 is the whole cube
    assert tuple(int(v) for v in B.level_rows(np.zeros((1, 3)), levels=2)[0]) == (1, 1, 1, 0)


def test_restatement_cells_at_the_edges():
    o, s = K.CUBE_EXACT
    o = np.asarray(o)
    pts = np.array([o, o + s, np.nextafter(o, -np.inf), np.nextafter(o + s, -np.inf), [math.inf, -math.inf, o[2] + 0.5 * s], o + s * 2.0 ** -16,
                    o + 3.0 * s])
    c = B.cells(pts, o, s, 16)
    assert c.tolist() == [[0, 0, 0], [65535] * 3, [0, 0, 0], [65535] * 3, [65535, 0, 32768], [1, 1, 1], [65535] * 3]
    assert B.cells(np.array([[-0.0, 0.0, -0.0]]), (0.0, 0.0, 0.0), 1.0, 4).tolist() == [[0, 0, 0]]
    assert B.cube([1.0, 3.0, -2.0, -1.5, 0.0, 0.0])[1] == 2.0 and B.cube([1.0, 1.0, 2.0, 2.0, 3.0, 3.0])[1] == 1.0
    assert B.cube([1.0, 3.0, -2.0, -1.5, 0.0, 0.0])[0].tolist() == [1.0, -2.0, 0.0]


def test_defaults(sar):
    p = sar.box_params()
    assert (p.levels, list(p.origin), p.size) == (16, [0.0, 0.0, 0.0], 1.0)
    q = sar.boxdim_params()
    assert (q.jobs, q.samples, q.stride, q.transient, q.levels, q.l_min) == (256, 128, 4, 1000, 16, 3)
    assert (q.seed, q.bound, q.min_occupancy) == (0, 1e6, 16.0)
    c = sar.corrdim_params()
    assert (q.jobs, q.samples, q.stride, q.transient, q.seed, q.bound) == (c.jobs, c.samples, c.stride, c.transient, c.seed, c.bound)
    p = sar.box_params(levels=5, origin=(1.0, 2.0, 3.0), size=0.5)
    assert (p.levels, list(p.origin), p.size) == (5, [1.0, 2.0, 3.0], 0.5)
    assert "box_chunk" in sar.api._abi.STABLE_OPTIONS and "box_slots" in sar.api._abi.STABLE_OPTIONS
    lib = sar.load_library()
    assert lib.sar_box_params_default(None) == 1 and lib.sar_boxdim_params_default(None) == 1
    with pytest.raises(ValueError):
        sar.box_params(levels=-1)
    with pytest.raises(ValueError):
        sar.box_params(origin=(1.0, 2.0))
    with pytest.raises(AttributeError):
        sar.boxdim_params(theiler=3)
    assert sar.BOX_LEVEL_DTYPE == B.LEVEL_DTYPE


def _same_lines(got, want):
    assert (int(got["status"]), int(got["first_level"]), int(got["last_level"]), int(got["used"])) == \
        (want["status"], want["first_level"], want["last_level"], want["used"])
    for d in ("d0", "d1", "d2"):
        for f in ("slope", "intercept", "rms"):
            if math.isnan(want[d][f]):
                assert math.isnan(got[d][f]), (d, f)
            else:
                # 1e-9 relative: libm and summation differences over at most 14 terms of order 1 — the fit's conditioning
                assert abs(got[d][f] - want[d][f]) <= 1e-9 * max(abs(want[d][f]), 1.0), (d, f, got[d][f], want[d][f])


def _sets():
    rng = np.random.default_rng(3)
    yield rng.random((5000, 3))                                              # a cloud: D near 3 over a short window
    yield np.stack([rng.random(4000), rng.random(4000), np.zeros(4000)], axis=1)   # a sheet
    yield K.line_lattice(300)
    yield K.planted_sets(700)[0]


def test_fit_equals_the_restatement(sar):
    for pts in _sets():
        rows, n = B.level_rows(pts), len(pts)
        for l_min, occ in ((3, 16.0), (0, 1.0), (2, 4.0), (5, 0.5), (1, 100.0)):
            _same_lines(sar.box_fit(rows, n, l_min, occ), B.fit(rows, n, l_min, occ))
    rows = B.level_rows(K.cube_lattice(), levels=5)
    _same_lines(sar.box_fit(rows, 512, 0, 1.0), B.fit(rows, 512, 0, 1.0))


def test_fit_gives_three_on_a_uniform_lattice(sar):
    rows = np.array(K.uniform_rows(), dtype=sar.BOX_LEVEL_DTYPE)
    assert rows.size == 7
    lines = sar.box_fit(rows, 2 ** 20, 0, 1.0)
    assert (int(lines["status"]), int(lines["first_level"]), int(lines["last_level"]), int(lines["used"])) == (sar.SAR_BOXDIM_FIT_OK, 0, 6, 7)
    for d in ("d0", "d1", "d2"):
        assert abs(lines[d]["slope"] - 3.0) <= 1e-12 and lines[d]["rms"] <= 1e-12, d
    lines = sar.box_fit(rows, 2 ** 20)                         # the default window: 2^20 >= 16 * 8^l up to l = 5
    assert (int(lines["first_level"]), int(lines["last_level"]), int(lines["used"])) == (3, 5, 3)
    assert abs(lines["d1"]["slope"] - 3.0) <= 1e-12


def test_no_window(sar):
    rows = B.level_rows(K.line_lattice(300))                   # 3, 5, 10 cells at levels 3, 4, 5: 300 >= 32 cells at 3 and 4 only
    lines = sar.box_fit(rows, 300, 3, 32.0)
    assert lines["status"] == sar.SAR_BOXDIM_NO_WINDOW and lines["used"] == 0 and lines["first_level"] == 0 and lines["last_level"] == 0
    assert all(math.isnan(lines[d][f]) for d in ("d0", "d1", "d2") for f in ("slope", "intercept", "rms"))
    _same_lines(lines, B.fit(rows, 300, 3, 32.0))
    lines = sar.box_fit(rows, 300, 2, 32.0)                    # ... and level 2: three levels
    assert lines["status"] == sar.SAR_BOXDIM_FIT_OK and (int(lines["first_level"]), int(lines["last_level"])) == (2, 4)
    assert sar.box_fit(rows, 300, 17)["status"] == sar.SAR_BOXDIM_NO_WINDOW      # l_min past the last level
    zero = np.zeros(17, dtype=sar.BOX_LEVEL_DTYPE)             # a DIVERGED map's rows
    assert sar.box_fit(zero, 300, 0, 1.0)["status"] == sar.SAR_BOXDIM_NO_WINDOW


def test_fit_refusals(sar):
    rows = B.level_rows(K.line_lattice(300))
    lib = sar.load_library()
    for n, l_min, occ, text in ((0, 3, 16.0, "points"), (2 ** 20 + 1, 3, 16.0, "points"), (300, 3, 0.0, "min_occupancy"),
                                (300, 3, math.nan, "min_occupancy")):
        with pytest.raises(sar.SarError):
            sar.box_fit(rows, n, l_min, occ)
        assert text in lib.sar_last_error().decode()
    with pytest.raises(sar.SarError):
        sar.box_fit(np.zeros(18, dtype=sar.BOX_LEVEL_DTYPE), 300)        # L = 17
    assert "levels" in lib.sar_last_error().decode()
    with pytest.raises(ValueError):
        sar.box_fit(rows[:1], 300)
    out = sar.api._abi.SarBoxdimLines()
    assert lib.sar_boxdim_fit(None, 16, 300, 3, 16.0, C.byref(out)) == 1


@pytest.mark.parametrize("change,text", K.BOXES_REFUSED)
def test_boxes_refusals_need_no_device(sar, change, text):
    change = dict(change)
    n = change.pop("n", 10)
    p = sar.box_params(**change)
    pts = np.zeros((min(max(n, 1), 16), 3))                    # (refused before the points are read)
    rows = np.zeros(17, dtype=sar.BOX_LEVEL_DTYPE)
    lib = sar.load_library()
    assert lib.sar_runtime_boxes(None, C.byref(p), 1, n, pts.ctypes.data_as(C.POINTER(C.c_double)),
                                 rows.ctypes.data_as(C.POINTER(sar.api._abi.SarBoxLevel))) == 1
    assert text in lib.sar_last_error().decode()
    assert not rows.view(np.uint64).any()


def test_a_nan_coordinate_is_refused_without_a_device(sar):
    pts = np.zeros((2, 5, 3))
    pts[1, 3, 2] = math.nan
    rows = np.zeros((2, 17), dtype=sar.BOX_LEVEL_DTYPE)
    lib = sar.load_library()
    assert lib.sar_runtime_boxes(None, None, 2, 5, pts.ctypes.data_as(C.POINTER(C.c_double)),
                                 rows.ctypes.data_as(C.POINTER(sar.api._abi.SarBoxLevel))) == 1
    assert "coordinate 2 of point 3 of set 1 is NaN" in lib.sar_last_error().decode()
    pts[1, 3, 2] = math.inf                                    # an infinity is taken: the next refusal is the missing runtime
    assert lib.sar_runtime_boxes(None, None, 2, 5, pts.ctypes.data_as(C.POINTER(C.c_double)),
                                 rows.ctypes.data_as(C.POINTER(sar.api._abi.SarBoxLevel))) == 1
    assert "runtime is NULL" in lib.sar_last_error().decode()
    assert lib.sar_runtime_boxes(None, None, 0, 5, None, None) == 0      # no set: nothing to do


@pytest.mark.parametrize("change,text", K.BOXDIM_REFUSED)
def test_boxdim_refusals_need_no_device(sar, change, text):
    p = sar.boxdim_params(**dict(dict(jobs=4, samples=4, stride=1, transient=10), **change))
    lib = sar.load_library()
    rows = np.zeros(17, dtype=sar.BOX_LEVEL_DTYPE)
    rec = np.zeros(1, dtype=sar.BOXDIM_RECORD_DTYPE)
    co = henon()
    assert lib.sar_runtime_boxdim(None, C.byref(p), 1, co.ctypes.data_as(C.POINTER(C.c_double)), None,
                                  rows.ctypes.data_as(C.POINTER(sar.api._abi.SarBoxLevel)),
                                  rec.ctypes.data_as(C.POINTER(sar.api._abi.SarBoxdimRecord)), None) == 1
    assert text in lib.sar_last_error().decode()


def test_boxdim_refuses_coefficients_and_starts_that_are_not_finite(sar):
    p = sar.boxdim_params(jobs=2, samples=2, stride=1, transient=1)
    lib = sar.load_library()
    rows = np.zeros(17, dtype=sar.BOX_LEVEL_DTYPE)
    rec = np.zeros(1, dtype=sar.BOXDIM_RECORD_DTYPE)
    args = (rows.ctypes.data_as(C.POINTER(sar.api._abi.SarBoxLevel)), rec.ctypes.data_as(C.POINTER(sar.api._abi.SarBoxdimRecord)), None)
    co = henon()
    co[7] = math.inf
    assert lib.sar_runtime_boxdim(None, C.byref(p), 1, co.ctypes.data_as(C.POINTER(C.c_double)), None, *args) == 1
    assert "coefficients must be finite (map 0, entry 7)" in lib.sar_last_error().decode()
    st = np.zeros((2, 3))
    st[1, 0] = math.nan
    co = henon()
    assert lib.sar_runtime_boxdim(None, C.byref(p), 1, co.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_double)), *args) == 1
    assert "start points must be finite (job 1)" in lib.sar_last_error().decode()
    assert lib.sar_runtime_boxdim(None, C.byref(p), 0, None, None, None, None, None) == 0     # no map: nothing to do


def test_struct_layouts_match_c_and_rust(sar):
    import os
    import re
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    abi = sar.api._abi
    pairs = [("sar_box_params", abi.SarBoxParams), ("sar_box_level", abi.SarBoxLevel), ("sar_boxdim_line", abi.SarBoxdimLine),
             ("sar_boxdim_lines", abi.SarBoxdimLines), ("sar_boxdim_params", abi.SarBoxdimParams), ("sar_boxdim_record", abi.SarBoxdimRecord)]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for cname, cls in pairs:
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        for f, _ in cls._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), src, "-o", exe], check=True)
        out = iter(int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    rs = open(os.path.join(root, "bindings", "rust", "src", "lib.rs")).read()
    for cname, cls in pairs:
        assert next(out) == C.sizeof(cls), cname
        for f, _ in cls._fields_:
            assert next(out) == getattr(cls, f).offset, (cname, f)
        body = rs[rs.index(f"pub struct {cls.__name__} {{"):]
        assert re.findall(r"pub (\w+):", body[:body.index("}")]) == [f for f, _ in cls._fields_], cname
