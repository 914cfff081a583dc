"""CPU: the host half of the orbit diagrams (include/sar.h: sar_orbit_*) — the defaults, sar_orbit_coeffs against the numpy formula
bit for bit, the struct layouts in C, ctypes and the Rust crates, every refusal that needs no device, the Python shorthand for
a line, and the restatement on the analytic logistic columns. No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import orbit_restatement as O
from orbit_cases import REFUSED, logistic as _logistic, refused_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_orbit_params": "SarOrbitParams", "sar_orbit_column": "SarOrbitColumn"}
INVALID = 1


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_defaults(sar):
    from strange_attractor_renderer_amd import _abi
    p = _abi.SarOrbitParams()
    lib = sar.load_library()
    assert lib.sar_orbit_params_default(C.byref(p)) == 0
    assert list(p.a) == [0.0] * 30 and list(p.b) == [0.0] * 30
    assert (p.width, p.height, p.jobs, p.transient, p.steps, p.seed, p.bound) == (1024, 512, 256, 1000, 4096, 0, 1e6)
    assert list(p.proj) == [1.0, 0.0, 0.0] and (p.v_lo, p.v_hi) == (-1.0, 1.0)
    assert lib.sar_orbit_params_default(None) == INVALID
    # the defaults are a valid diagram: they get as far as the NULL runtime
    assert lib.sar_runtime_orbit(None, C.byref(p), None, None, None, None) == INVALID and b"runtime" in lib.sar_last_error()
    assert lib.sar_abi_version() >= 12


def test_orbit_chunk_is_a_stable_option(sar):
    from strange_attractor_renderer_amd import _abi
    assert "orbit_chunk" in _abi.STABLE_OPTIONS


def _coeffs(sar, p, c):
    out = np.empty(30)
    assert sar.load_library().sar_orbit_coeffs(C.byref(p), c, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    return out


@pytest.mark.parametrize("width", [1, 2, 5, 7, 64, 1000, 65536])
def test_coeffs_match_the_formula(sar, width):
    rng = np.random.default_rng(width)
    a, b = rng.uniform(-1.2, 1.2, 30), rng.uniform(-1.2, 1.2, 30)
    same = [3, 12, 13, 29]
    b[same] = a[same]                    # entries that do not move
    a[[4, 17]] = -0.0                    # a -0.0 end, moving (4) ...
    a[21] = b[21] = -0.0                 # ... and fixed
    a[8], b[8] = 0.1, 0.1 + 1e-9         # a span far below the value
    a[9], b[9] = 1e-300, -1e-300
    p = sar.orbit_params(a, b, width=width)
    want = O.coeffs(a, b, width)
    for c in sorted({0, 1 % width, width // 3, width // 2, width - 1}):
        got = _coeffs(sar, p, c)
        assert np.array_equal(_bits(got), _bits(want[c])), c
        assert np.array_equal(_bits(got[same]), _bits(a[same])), c          # a == b entries stay exactly a_k
        assert not np.any(np.signbit(got) & (got == 0.0))                   # -0.0 made +0.0
        assert _bits(got[21:22])[0] == 0
    assert np.array_equal(_bits(_coeffs(sar, p, 0)), _bits(0.0 + 1.0 * a))   # column 0 is a
    if width == 1:
        assert np.array_equal(_bits(want[0]), _bits(0.0 + 1.0 * a))          # t = 0
    else:
        last = _coeffs(sar, p, width - 1)                                    # t = 1: a + (b - a), which may differ from b by an ulp
        assert np.array_equal(_bits(last), _bits(0.0 + 1.0 * (a + (b - a) * 1.0)))
        assert np.allclose(last, b, rtol=0, atol=1e-15)
    out = np.empty(30)
    assert sar.load_library().sar_orbit_coeffs(C.byref(p), width, out.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert sar.load_library().sar_orbit_coeffs(C.byref(p), 0, None) == INVALID
    d = sar.OrbitDiagram(p, np.zeros((1, 1), np.uint32), None, 0)
    assert d.coeffs(width - 1).shape == (3, 10) and np.array_equal(_bits(d.coeffs(width - 1).reshape(30)), _bits(want[width - 1]))


def test_line_shorthands(sar):
    cfg = sar.Config.poisson_saturne()
    rows = np.stack([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    p = sar.orbit_params(cfg, axis=13, range=(-0.5, 0.25), width=9)
    q = sar.orbit_params(rows, rows.reshape(30), axis=13, range=(-0.5, 0.25), width=9)
    assert list(p.a) == list(q.a) and list(p.b) == list(q.b)
    flat = rows.reshape(30)
    assert p.a[13] == -0.5 and p.b[13] == 0.25
    assert [p.a[k] for k in range(30) if k != 13] == [p.b[k] for k in range(30) if k != 13] == [flat[k] for k in range(30) if k != 13]
    two = sar.orbit_params(cfg, sar.Config.solar_sail(), v_range=(-2, 3), proj=(0.6, -0.3, 0.7), height=77, jobs=5, seed=9, bound=50)
    assert list(two.b[:10]) == list(sar.Config.solar_sail().coeff_x) and (two.v_lo, two.v_hi) == (-2.0, 3.0)
    assert list(two.proj) == [0.6, -0.3, 0.7] and (two.height, two.jobs, two.seed, two.bound) == (77, 5, 9, 50.0)
    for bad in (dict(), dict(axis=3), dict(range=(0, 1)), dict(axis=30, range=(0, 1))):
        with pytest.raises(ValueError):
            sar.orbit_params(cfg, **bad)
    with pytest.raises(ValueError):
        sar.orbit_params(np.zeros(29), np.zeros(30))
    with pytest.raises(ValueError):
        sar.orbit_params(cfg, cfg, steps=-1)
    with pytest.raises(AttributeError):
        sar.orbit_params(cfg, cfg, no_such_field=1)


@pytest.mark.parametrize("change,text", REFUSED)
def test_refusals_need_no_device(sar, change, text):
    p = refused_params(sar, change)
    lib = sar.load_library()
    out = np.empty(30)
    count = np.zeros(8, dtype=np.uint32)
    assert lib.sar_runtime_orbit(None, C.byref(p), None, count.ctypes.data_as(C.POINTER(C.c_uint32)), None, None) == INVALID
    assert text in lib.sar_last_error().decode(), lib.sar_last_error()
    assert lib.sar_orbit_coeffs(C.byref(p), 0, out.ctypes.data_as(C.POINTER(C.c_double))) == INVALID
    assert lib.sar_runtime_orbit(None, None, None, None, None, None) == INVALID


def test_limits_pass_the_checks(sar):
    """The largest sizes and step counts are accepted: they get as far as the NULL runtime."""
    lib = sar.load_library()
    for change in (dict(width=65536, height=32768), dict(jobs=1024, steps=2 ** 22 - 1), dict(jobs=1, transient=2 ** 31, steps=2 ** 31),
                   dict(v_lo=-1e308, v_hi=1e308)):   # (v_hi - v_lo overflows: the scale is 0, which is finite)
        p = refused_params(sar, change)
        assert lib.sar_runtime_orbit(None, C.byref(p), None, None, None, None) == INVALID
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
    assert k + 1 == len(out) and int(out[k]) == sar.load_library().sar_abi_version() == 12
    assert (C.sizeof(_abi.SarOrbitParams), C.sizeof(_abi.SarOrbitColumn)) == (560, 56)
    assert sar.ORBIT_COLUMN_DTYPE.itemsize == 56
    assert [n for n in sar.ORBIT_COLUMN_DTYPE.names] == [f for f, _ in _abi.SarOrbitColumn._fields_]
    for f, _ in _abi.SarOrbitColumn._fields_:
        assert sar.ORBIT_COLUMN_DTYPE.fields[f][1] == getattr(_abi.SarOrbitColumn, f).offset, f
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname
    safe = open(os.path.join(ROOT, "bindings", "rust-safe", "src", "lib.rs")).read()
    assert "sys::sar_runtime_orbit(" in safe and "sys::sar_orbit_params_default(" in safe and "sys::sar_orbit_coeffs(" in safe
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    assert "sar_runtime_orbit(" in hpp and "sar_orbit_params_default(" in hpp and "sar_orbit_coeffs(" in hpp


def test_restated_logistic_columns_are_the_analytic_ones():
    """The restatement alone against the closed forms: the fixed point 1 - 1/r at r = 2.8, the 2-cycle at r = 3.2, escape at 4.4."""
    a, b = _logistic()
    jobs, steps, height = 6, 100, 64
    starts = np.linspace(0.01, 0.09, jobs * 3).reshape(jobs, 3)
    d = O.diagram(a, b, 5, height, starts, 1000, steps, (0.0, 1.0))
    s = d["stats"]
    r = O.coeffs(a, b, 5)[:, 1]
    assert np.allclose(r, [2.8, 3.2, 3.6, 4.0, 4.4], rtol=0, atol=1e-15)
    assert np.array_equal(np.nonzero(d["count"][:, 0])[0], [height - 1 - int(height * (1 - 1 / r[0]))])
    root = math.sqrt((r[1] - 3) * (r[1] + 1))
    rows = sorted(height - 1 - int(height * (r[1] + 1 + sgn * root) / (2 * r[1])) for sgn in (1, -1))
    assert np.array_equal(np.nonzero(d["count"][:, 1])[0], rows) and np.all(d["count"][rows, 1] == jobs * steps // 2)
    assert s["dead_transient"][4] == jobs and not d["count"][:, 4].any() and s["vmin"][4] == math.inf and s["vmax"][4] == -math.inf
    assert np.array_equal(s["dead_transient"] + s["dead_late"] + s["alive"], [jobs] * 5)
    assert np.array_equal(s["hits"], d["count"].sum(0)) and d["max"] == d["count"].max() == jobs * steps
