"""CPU: the host half of the Lyapunov planes (include/sar.h: sar_plane_*) — the defaults, every refusal, sar_plane_coeffs against the
numpy formula bit for bit, the record layouts in C, ctypes and Rust, and the restatement's L1 recurrence against the search's
restatement (first Gram-Schmidt column) and the decimal references of tests/lyapunov_reference.py. No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import lyapunov_reference as L
import plane_restatement as P
import search_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-12   # the search tests' tolerance against the decimal references


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_defaults(sar):
    from strange_attractor_renderer_amd import _abi
    p = _abi.SarPlaneParams()
    assert sar.load_library().sar_plane_params_default(C.byref(p)) == 0
    assert list(p.start) == [0.05] * 3 and (p.transient, p.steps, p.bound) == (1000, 20000, 1e6)
    assert p.mode == sar.SAR_PLANE_L1 and list(p.axis) == [0, 1] and p.width > 0 and p.height > 0
    c = sar.plane_colors()
    assert (c.threshold, c.chaos_scale, c.order_scale) == (0.0, 0.25, 1.0)
    assert (sar.SAR_PLANE_L1, sar.SAR_PLANE_SPECTRUM) == (1, 3)


def _params(sar, **kw):
    base = kw.pop("base", np.zeros(30))
    axes = kw.pop("axes", (1, 15))
    xr, yr = kw.pop("x_range", (-1.0, 1.0)), kw.pop("y_range", (-0.5, 0.5))
    w, h = kw.pop("width", 8), kw.pop("height", 6)
    mode = kw.pop("mode", "l1")
    return sar.plane_params(base, axes, xr, yr, w, h, mode, **kw)


@pytest.mark.parametrize("change", [
    dict(axes=(3, 3)), dict(axes=(30, 1)), dict(axes=(0, 31)), dict(width=0), dict(height=0), dict(width=4097, height=4096),
    dict(x_range=(math.nan, 1.0)), dict(x_range=(0.0, math.inf)), dict(y_range=(-math.inf, 0.0)), dict(y_range=(0.0, math.nan)),
    dict(bound=math.inf), dict(bound=math.nan), dict(bound=0.0), dict(transient=2 ** 31 + 1), dict(steps=2 ** 31 + 1),
])
def test_refusals(sar, change):
    p = _params(sar, **change)
    lib = sar.load_library()
    out = np.empty(30)
    assert lib.sar_plane_coeffs(C.byref(p), 0, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == 1
    assert lib.sar_runtime_plane(None, C.byref(p), None, None) == 1   # refused before any device is needed
    assert lib.sar_last_error()


@pytest.mark.parametrize("mode", [0, 2, 4, -1])
def test_bad_mode_is_refused(sar, mode):
    p = _params(sar)
    p.mode = mode
    lib = sar.load_library()
    assert lib.sar_runtime_plane(None, C.byref(p), None, None) == 1
    assert b"mode" in lib.sar_last_error()
    with pytest.raises(ValueError):
        _params(sar, mode="lambda")


def test_limits_are_accepted(sar):
    """2^24 pixels and 2^31 steps are the largest plane and run; the parameters pass the checks (coefficients at the corner)."""
    p = _params(sar, width=4096, height=4096, transient=2 ** 31, steps=2 ** 31)
    out = np.empty(30)
    assert sar.load_library().sar_plane_coeffs(C.byref(p), 4095, 4095, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert sar.load_library().sar_plane_coeffs(C.byref(p), 4096, 0, out.ctypes.data_as(C.POINTER(C.c_double))) == 1


class _Plane:   # LyapunovPlane.coeffs without a runtime
    def __init__(self, sar, p):
        self.params = p
        self.coeffs = lambda x, y: sar.LyapunovPlane.coeffs(self, x, y)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (9, 1), (8, 8), (7, 5), (64, 33), (2, 2)])
@pytest.mark.parametrize("xr,yr", [((-1.2, 1.2), (-0.3, 0.9)), ((0.1, 0.1 + 1e-9), (1e-300, -1e-300)), ((-0.0, 0.0), (2.5, -7.25))])
def test_coeffs_match_the_formula(sar, w, h, xr, yr):
    rng = np.random.default_rng(w * 100 + h)
    base = rng.uniform(-1.2, 1.2, 30)
    base[[4, 11, 29]] = -0.0
    axes = (17, 2)
    p = sar.plane_params(base, axes, xr, yr, w, h)
    want = P.coeffs(base, axes, xr, yr, w, h)
    pl = _Plane(sar, p)
    for x in sorted({0, w // 2, w - 1}):
        for y in sorted({0, h // 2, h - 1}):
            got = pl.coeffs(x, y).reshape(30)
            assert np.array_equal(_bits(got), _bits(want[y, x])), (x, y)
            fixed = [j for j in range(30) if j not in axes]
            assert np.array_equal(_bits(got[fixed]), _bits(0.0 + 1.0 * base[fixed]))   # copies, -0.0 made +0.0
            assert not np.any(np.signbit(got) & (got == 0.0))
    assert pl.coeffs(0, 0)[1, 7] == xr[0]                    # column 0 is exactly lo0 (axis 17: row y, index 7)
    assert pl.coeffs(w - 1, h - 1)[0, 2] == yr[0]            # row H-1 is exactly lo1
    if h > 1:
        assert pl.coeffs(0, 0)[0, 2] == yr[0] + (yr[1] - yr[0]) * 1.0   # row 0 is the high end


def test_coeffs_from_a_config_and_from_rows(sar):
    cfg = sar.Config.poisson_saturne()
    rows = np.stack([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    a = sar.plane_params(cfg, (0, 1), (-1, 1), (-1, 1), 5, 5)
    b = sar.plane_params(rows, (0, 1), (-1, 1), (-1, 1), 5, 5)
    assert list(a.base) == list(b.base) == list(rows.reshape(30))
    with pytest.raises(ValueError):
        sar.plane_params(np.zeros(29), (0, 1), (-1, 1), (-1, 1), 5, 5)


def test_record_layout_in_c_ctypes_and_rust(sar):
    from strange_attractor_renderer_amd import _abi
    structs = {"sar_plane_params": _abi.SarPlaneParams, "sar_plane_record": _abi.SarPlaneRecord,
               "sar_plane_stats": _abi.SarPlaneStats, "sar_plane_colors": _abi.SarPlaneColors}
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
    assert sar.PLANE_RECORD_DTYPE.itemsize == C.sizeof(_abi.SarPlaneRecord) == 96
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for rname, cls in (("SarPlaneParams", _abi.SarPlaneParams), ("SarPlaneRecord", _abi.SarPlaneRecord),
                       ("SarPlaneStats", _abi.SarPlaneStats), ("SarPlaneColors", _abi.SarPlaneColors)):
        body = rs[rs.index(f"pub struct {rname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in cls._fields_], rname


def test_plane_chunk_is_a_stable_option(sar):
    from strange_attractor_renderer_amd import _abi
    assert "plane_chunk" in _abi.STABLE_OPTIONS


# ---- the restatement's L1 recurrence ------------------------------------------------------------------------------------
def test_l1_is_the_first_column_of_the_search_restatement():
    cs = np.concatenate([R.candidates(1, k, 1) for k in (545, 1791, 2513, 2573, 2617)] + [R.candidates(3, 0, 64)])
    alive, x, y, z = R.screen(cs, (0.05,) * 3, 1000, 1e6)
    idx = np.nonzero(alive)[0]
    assert idx.size >= 5
    full = R.lyapunov(cs[idx], x[idx], y[idx], z[idx], 3000, 1e6)
    one = P.l1(cs[idx], x[idx], y[idx], z[idx], 3000, 1e6)
    bounded = full["status"] == R.BOUNDED
    assert bounded.sum() >= 5
    assert np.array_equal(one["status"][bounded], full["status"][bounded])
    assert np.array_equal(one["steps_done"][bounded], full["steps_done"][bounded])
    assert np.array_equal(_bits(one["mant"][bounded]), _bits(full["mant"][bounded, 0]))
    assert np.array_equal(one["log2_exp"][bounded], full["log2_exp"][bounded, 0])


@pytest.mark.parametrize("name", sorted(L.AFFINE_MAPS))
def test_l1_meets_the_decimal_first_column_on_affine_maps(name):
    A, b = L.AFFINE_MAPS[name]
    c = np.array([L.affine_coeffs(A, b)])
    steps, transient = 1000, 200
    alive, x, y, z = R.screen(c, (0.05,) * 3, transient, L.AFFINE_BOUND)
    assert alive[0]
    r = P.l1(c, x, y, z, steps, L.AFFINE_BOUND)
    assert (int(r["status"][0]), int(r["steps_done"][0])) == (L.BOUNDED, steps)
    prod, _ = L.affine_gram_schmidt(A, steps)
    want = float(L._CTX.divide(L._CTX.ln(prod[0]), steps))
    got = (float(r["log2_exp"][0]) * P.LN2 + math.log(float(r["mant"][0]))) / steps
    assert abs(got - want) <= TOL, (got, want)


def test_restated_plane_transient_and_l1_on_a_diagonal_map():
    """A diagonal affine plane in the restatement alone: a = 0 is DEGENERATE at step 1, |a| > 1 leaves the box in the transient
    at the step a plain loop predicts, L1 is ln|a| (the growth of e1) while the spectrum's maximum is max(ln|a|, ln|b|, ln|c|)."""
    base = L.affine_coeffs([[0.5, 0, 0], [0, 0.7, 0], [0, 0, 0.3]], (0.01, 0.02, 0.03))
    pl = P.plane(base, (1, 15), (-1.5, 1.5), (0.2, 0.9), 7, 3, "l1", transient_steps=100, steps=200, bound=1e3)
    a = P.sweep(-1.5, 1.5, 7)
    assert a[3] == 0.0
    assert np.all(pl["status"][:, 3] == P.DEGENERATE) and np.all(pl["steps_done"][:, 3] == 1)
    big = np.abs(a) > 1
    assert np.all(pl["status"][:, big] == P.DIVERGED) and np.all(pl["steps_done"][:, big] == 0)
    for xi in np.nonzero(big)[0]:
        c = list(P.coeffs(base, (1, 15), (-1.5, 1.5), (0.2, 0.9), 7, 3)[0, xi])
        p, step = [0.05] * 3, None
        for t in range(100):
            p = L.next_point(c, *p)
            if not all(abs(v) <= 1e3 for v in p):
                step = t + 1
                break
        assert step is not None and np.all(pl["transient_done"][:, xi] == step)
    ok = (np.abs(a) < 1) & (a != 0)
    assert np.allclose(pl["lyapunov"][:, ok, 0], np.log(np.abs(a[ok]))[None, :], rtol=0, atol=1e-12)
