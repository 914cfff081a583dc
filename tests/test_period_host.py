"""CPU: the host half of the period planes (include/sar.h: sar_period_*) — the defaults, every refusal, sar_period_coeffs against the
planes' formula, the record layouts in C, ctypes and Rust — and the numpy restatement (tests/period_restatement.py) held to periods
known independently of it: the logistic family's bifurcation points and period-3 window, Hénon's cascade, linear maps that are exact
cycles, and the pixel counts of two Hénon planes (tests/period_cases.py). No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import period_cases as K
import period_restatement as Q
import plane_restatement as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the restatement against known answers ---------------------------------------------------------------------------------
def test_logistic_periods():
    r = Q.period_list(np.stack([K.logistic(v) for v, _, _ in K.LOGISTIC]), **K.LOGISTIC_PARAMS)
    for i, (v, status, period) in enumerate(K.LOGISTIC):
        assert (int(r["status"][i]), int(r["period"][i])) == (status, period), v
        if status == K.BOUNDED:
            assert r["transient_done"][i] == K.LOGISTIC_PARAMS["transient"]
            assert r["steps_done"][i] == (period if period else K.LOGISTIC_PARAMS["max_period"])
            assert (r["residual"][i] <= K.LOGISTIC_PARAMS["eps"]) if period else math.isnan(r["residual"][i])
        else:
            assert (int(r["transient_done"][i]), int(r["steps_done"][i])) == (K.LOGISTIC_DIVERGED_AT, 0) and math.isnan(r["residual"][i])


def test_henon_periods():
    r = Q.period_list(np.stack([K.henon(a) for a, _ in K.HENON]), **K.HENON_PARAMS)
    assert np.all(r["status"] == K.BOUNDED)
    assert [int(p) for p in r["period"]] == [p for _, p in K.HENON]


def test_exact_cycles():
    cs = np.stack([K.linear(m) for _, m, _ in K.CYCLES])
    r = Q.period_list(cs, **K.CYCLE_PARAMS)
    assert [int(p) for p in r["period"]] == [p for _, _, p in K.CYCLES] == [int(s) for s in r["steps_done"]]
    assert np.all(r["status"] == K.BOUNDED) and np.array_equal(_bits(r["residual"]), _bits(np.zeros(len(K.CYCLES))))
    short = Q.period_list(cs, **{**K.CYCLE_PARAMS, "max_period": 5})
    assert [int(p) for p in short["period"]] == [1, 2, 3, 4, 0] and int(short["steps_done"][-1]) == 5
    assert short["status"][-1] == K.BOUNDED and math.isnan(short["residual"][-1])


@pytest.mark.parametrize("case", K.HENON_PLANES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_henon_plane_counts(case):
    w, h, params, diverged, zero, counts, distinct = case
    r = Q.period_plane(width=w, height=h, **K.HENON_PLANE, **params)
    bounded = r["status"] == K.BOUNDED
    assert np.count_nonzero(~bounded) == diverged
    assert np.count_nonzero(bounded & (r["period"] == 0)) == zero
    for p, n in counts.items():
        assert np.count_nonzero(bounded & (r["period"] == p)) == n, p
    if distinct is not None:
        assert len(set(r["period"][bounded & (r["period"] != 0)].tolist())) == distinct
    st = Q.stats(r)
    assert st["pixels"] == w * h == st["diverged_transient"] + st["diverged_late"] + st["periodic"] + st["aperiodic"]
    assert st["aperiodic"] == zero and st["diverged_transient"] + st["diverged_late"] == diverged
    assert np.all(r["period"][~bounded] == 0) and np.all(np.isnan(r["residual"][r["period"] == 0]))


def test_logistic_line_stays_within_the_cap_of_zero_columns():
    """What tests/test_gpu_period.py asks of OrbitDiagram.period holds for the restatement alone at the default transient: along
    r in [2.8, 3.56] the periods 1, 2, 4, 8 appear in order, and at most 6 columns read 0 (slow convergence at the bifurcations)."""
    line = K.LOGISTIC_LINE
    rr = P.sweep(*line["r_range"], line["width"])
    r = Q.period_list(np.stack([K.logistic(v) for v in rr]), start=line["start"])
    assert np.all(r["status"] == K.BOUNDED)
    per = r["period"].astype(np.int64)
    assert {1, 2, 4, 8} <= set(per.tolist())
    assert np.count_nonzero(per == 0) <= line["max_zero_columns"]
    assert np.all(np.diff(per[per != 0]) >= 0)


def test_colorize_restatement_on_a_hand_made_plane():
    status = np.array([[K.DIVERGED, K.BOUNDED, K.BOUNDED, K.BOUNDED], [K.BOUNDED, K.BOUNDED, K.BOUNDED, K.DIVERGED]], dtype=np.int32)
    period = np.array([[0, 0, 1, 2], [3, 4, 5, 0]], dtype=np.uint32)
    pal = [[0.0, 0.0, 0.0], [1.0, 0.25, 0.0], [0.0, 1.0, 0.5]]   # three entries: v * 3 selects the pair to blend
    img = Q.colorize(status, period, pal, colours=4)
    assert img.shape == (2, 4, 4) and img.dtype == np.uint16
    assert img[0, 0].tolist() == [0, 0, 0, 0] == img[1, 3].tolist()          # DIVERGED: transparent
    assert img[0, 1].tolist() == [0, 0, 0, 65535]                            # bounded, no period: the black sea
    assert np.array_equal(img[0, 2], img[1, 2])                              # periods 1 and 5 share a slot of 4
    assert len({tuple(img[y, x]) for y, x in ((0, 2), (0, 3), (1, 0), (1, 1))}) == 4
    # period 1 of 4 colours: v = 0.125, v * 3 = 0.375: between entries 0 and 1 at t = 0.375
    want = [int(math.sqrt(c * 0.375 + 0.0 * 0.625) * 65535.0) for c in pal[1]]
    assert img[0, 2].tolist() == want + [65535]
    # period 4: v = 0.875, v * 3 = 2.625: entry 2 against its duplicate
    assert img[1, 1].tolist() == [int(math.sqrt(c * 0.625 + c * 0.375) * 65535.0) for c in pal[2]] + [65535]
    one = Q.colorize(status, period, pal, colours=1)
    assert np.array_equal(one[0, 2], one[0, 3]) and np.array_equal(one[0, 2], one[1, 1])


# ---- the ABI ---------------------------------------------------------------------------------------------------------------
def test_defaults(sar):
    from strange_attractor_renderer_amd import _abi
    p = _abi.SarPeriodParams()
    assert sar.load_library().sar_period_params_default(C.byref(p)) == 0
    q = sar.plane_params(np.zeros(30), (0, 1), (-1.2, 1.2), (-1.2, 1.2), 256, 256)
    d = _abi.SarPlaneParams()
    assert sar.load_library().sar_plane_params_default(C.byref(d)) == 0
    for f in ("base", "axis", "lo", "hi", "start"):
        assert list(getattr(p, f)) == list(getattr(d, f)) == list(getattr(q, f)), f
    assert (p.width, p.height, p.bound) == (d.width, d.height, d.bound) == (256, 256, 1e6)
    assert list(p.start) == [0.05] * 3 and (p.transient, p.max_period, p.eps) == (2000, 256, 1e-9)
    assert sar.period_colors().colours == 16 and sar.period_colors(5).colours == 5


def _params(sar, **kw):
    base = kw.pop("base", np.zeros(30))
    axes = kw.pop("axes", (1, 15))
    xr, yr = kw.pop("x_range", (-1.0, 1.0)), kw.pop("y_range", (-0.5, 0.5))
    w, h = kw.pop("width", 8), kw.pop("height", 6)
    return sar.period_params(base, axes, xr, yr, w, h, **kw)


PLANE_REFUSALS = [dict(axes=(3, 3)), dict(axes=(30, 1)), dict(axes=(0, 31)), dict(x_range=(math.nan, 1.0)), dict(x_range=(0.0, math.inf)),
                  dict(y_range=(-math.inf, 0.0)), dict(y_range=(0.0, math.nan))]
RUN_REFUSALS = [dict(width=0), dict(height=0), dict(width=4097, height=4096), dict(bound=math.inf), dict(bound=math.nan),
                dict(bound=0.0), dict(transient=2 ** 31 + 1), dict(max_period=0), dict(max_period=2 ** 31 + 1), dict(eps=-1e-300),
                dict(eps=math.nan), dict(eps=math.inf)]


@pytest.mark.parametrize("change", PLANE_REFUSALS + RUN_REFUSALS)
def test_refusals(sar, change):
    p = _params(sar, **change)
    lib = sar.load_library()
    out = np.empty(30)
    assert lib.sar_period_coeffs(C.byref(p), 0, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert lib.sar_runtime_period(None, C.byref(p), None, None, None) == 1   # refused before any device is needed
    assert lib.sar_last_error()


def test_the_list_form_ignores_the_plane_but_not_the_run(sar):
    """With a coefficient list a bad axis or range is no refusal — the call then fails only for want of a runtime, with another
    message —, a bad size, bound, step count or eps still is."""
    lib = sar.load_library()
    cs = np.zeros((8 * 6, 30))
    ptr = cs.ctypes.data_as(C.POINTER(C.c_double))
    for change in PLANE_REFUSALS:
        assert lib.sar_runtime_period(None, C.byref(_params(sar, **change)), ptr, None, None) == 1
        assert b"NULL" in lib.sar_last_error(), change
    for change in RUN_REFUSALS:
        assert lib.sar_runtime_period(None, C.byref(_params(sar, **change)), ptr, None, None) == 1
        assert b"NULL" not in lib.sar_last_error(), change


def test_limits_are_accepted(sar):
    p = _params(sar, width=4096, height=4096, transient=2 ** 31, max_period=2 ** 31, eps=0.0)
    out = np.empty(30)
    lib = sar.load_library()
    assert lib.sar_period_coeffs(C.byref(p), 4095, 4095, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert lib.sar_period_coeffs(C.byref(p), 4096, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert lib.sar_runtime_period(None, C.byref(p), None, None, None) == 1 and b"NULL" in lib.sar_last_error()


def test_python_parameter_checks(sar):
    with pytest.raises(AttributeError):
        _params(sar, steps=5)
    with pytest.raises(ValueError):
        _params(sar, max_period=2 ** 32)
    with pytest.raises(ValueError):
        sar.period_plane(None, width=4, height=4)                              # neither a plane nor a list
    with pytest.raises(ValueError):
        sar.period_plane(None, width=4, height=4, coeffs=np.zeros((15, 30)))   # a list of the wrong length


class _Plane:   # PeriodPlane.coeffs without a runtime
    def __init__(self, sar, p, cs=None):
        self.params, self.list_coeffs = p, cs
        self.coeffs = lambda x, y: sar.PeriodPlane.coeffs(self, x, y)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (9, 1), (7, 5), (64, 33)])
def test_coeffs_match_the_planes_formula(sar, w, h):
    rng = np.random.default_rng(w * 100 + h)
    base = rng.uniform(-1.2, 1.2, 30)
    base[[4, 11, 29]] = -0.0
    axes, xr, yr = (17, 2), (-1.2, 1.2), (-0.3, 0.9)
    want = P.coeffs(base, axes, xr, yr, w, h)
    pl = _Plane(sar, sar.period_params(base, axes, xr, yr, w, h))
    lya = sar.plane_params(base, axes, xr, yr, w, h)
    out = np.empty(30)
    for x in sorted({0, w // 2, w - 1}):
        for y in sorted({0, h // 2, h - 1}):
            got = pl.coeffs(x, y).reshape(30)
            assert np.array_equal(_bits(got), _bits(want[y, x])), (x, y)
            assert sar.load_library().sar_plane_coeffs(C.byref(lya), x, y, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
            assert np.array_equal(_bits(got), _bits(out))                     # sar_runtime_plane's pixel, to the bit
            assert not np.any(np.signbit(got) & (got == 0.0))
    listed = _Plane(sar, None, want.copy())
    assert np.array_equal(_bits(listed.coeffs(w - 1, 0)), _bits(want[0, w - 1].reshape(3, 10)))


def test_record_layout_in_c_ctypes_and_rust(sar):
    from strange_attractor_renderer_amd import _abi
    structs = {"sar_period_params": _abi.SarPeriodParams, "sar_period_record": _abi.SarPeriodRecord,
               "sar_period_stats": _abi.SarPeriodStats, "sar_period_colors": _abi.SarPeriodColors}
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for name, cls in structs.items():
        prog += f'printf("{name} %zu\\n", sizeof({name}));\n'
        for f, _ in cls._fields_:
            prog += f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));\n'
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "t.c")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"), src, "-o",
                        os.path.join(d, "t")], check=True)
        out = subprocess.run([os.path.join(d, "t")], capture_output=True, text=True, check=True).stdout.split("\n")
    got = dict(line.rsplit(" ", 1) for line in out if line)
    for name, cls in structs.items():
        assert int(got[name]) == C.sizeof(cls), name
        for f, _ in cls._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(cls, f).offset, (name, f)
    assert sar.PERIOD_RECORD_DTYPE.itemsize == C.sizeof(_abi.SarPeriodRecord) == 24
    for f in sar.PERIOD_RECORD_DTYPE.names:
        assert sar.PERIOD_RECORD_DTYPE.fields[f][1] == getattr(_abi.SarPeriodRecord, f).offset, f
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for rname, cls in (("SarPeriodParams", _abi.SarPeriodParams), ("SarPeriodRecord", _abi.SarPeriodRecord),
                       ("SarPeriodStats", _abi.SarPeriodStats), ("SarPeriodColors", _abi.SarPeriodColors)):
        body = rs[rs.index(f"pub struct {rname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in cls._fields_], rname


def test_period_chunk_is_a_stable_option(sar):
    from strange_attractor_renderer_amd import _abi
    assert "period_chunk" in _abi.STABLE_OPTIONS
