"""CPU: the host half of the auto colour range (include/sar.h: sar_color_range_params / sar_color_range) — the layouts of both
structs in C, ctypes and the Rust sys crate, the default parameters, their validation through the mode switches, the hold's
validation, sar_color_range_to_velocity, the numpy restatement of the definition, and the bindings' methods. No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import color_range_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_color_range_params": "SarColorRangeParams", "sar_color_range": "SarColorRange"}
INVALID = 1


def test_color_range_struct_layouts_match_c_ctypes_and_rust():
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
    assert int(out[k]) >= 10 and k + 1 == len(out)
    assert C.sizeof(_abi.SarColorRangeParams) == 32 and C.sizeof(_abi.SarColorRange) == 40
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname


def test_color_range_params_default(sar):
    p = sar.color_range_params()
    assert (p.q_lo, p.q_hi, p.pos_lo, p.pos_hi) == (0.01, 0.99, 0.0, 1.0)
    q = sar.color_range_params(q_hi=0.9, pos_lo=1.0, pos_hi=0.0)   # a reversed palette is allowed
    assert (q.q_lo, q.q_hi, q.pos_lo, q.pos_hi) == (0.01, 0.9, 1.0, 0.0)
    with pytest.raises(AttributeError):
        sar.color_range_params(no_such_field=1)
    assert sar.load_library().sar_color_range_params_default(None) == INVALID
    assert sar.load_library().sar_abi_version() >= 10


@pytest.mark.parametrize("bad", [dict(q_lo=-0.1), dict(q_hi=1.5), dict(q_lo=0.6, q_hi=0.5), dict(q_lo=math.nan), dict(q_hi=math.nan),
                                 dict(pos_lo=math.inf), dict(pos_hi=-math.inf), dict(pos_lo=math.nan), dict(pos_hi=math.nan)])
def test_color_range_parameters_are_validated_without_a_device(sar, bad):
    # the parameters are checked before the handles: with NULL handles the message tells which check refused the call
    lib = sar.load_library()
    p = sar.color_range_params(**bad)
    for fn in (lib.sar_runtime_set_color_range, lib.sar_renderer_set_color_range):
        assert fn(None, C.byref(p)) == INVALID
        assert lib.sar_last_error().decode().startswith("colour range: need"), lib.sar_last_error()
        assert fn(None, C.byref(sar.color_range_params())) == INVALID   # good parameters: the NULL handle is refused
        assert "is NULL" in lib.sar_last_error().decode(), lib.sar_last_error()
        assert fn(None, None) == INVALID
    from strange_attractor_renderer_amd import _abi
    cfg, out = sar.Config.solar_sail(), _abi.SarColorRange()
    assert lib.sar_runtime_color_range(C.byref(cfg.c), None, C.byref(p), C.byref(out)) == INVALID
    assert lib.sar_last_error().decode().startswith("colour range: need"), lib.sar_last_error()


@pytest.mark.parametrize("bad", [dict(lo=0.0, hi=1.0, pos_lo=math.nan), dict(lo=0.0, hi=1.0, pos_hi=math.inf), dict(lo=1.0, hi=1.0),
                                 dict(lo=2.0, hi=1.0), dict(lo=-math.inf, hi=1.0), dict(lo=0.0, hi=math.inf), dict(lo=math.nan, hi=1.0),
                                 dict(lo=-1.7e308, hi=1.7e308)])
def test_a_held_window_is_validated_without_a_device(sar, bad):
    lib = sar.load_library()
    assert lib.sar_runtime_hold_color_range(None, C.byref(sar.ColorRange(**bad).c)) == INVALID
    assert lib.sar_last_error().decode().startswith("colour range: a held window needs"), lib.sar_last_error()
    assert lib.sar_runtime_hold_color_range(None, C.byref(sar.ColorRange(0.0, 1.0).c)) == INVALID
    assert "is NULL" in lib.sar_last_error().decode()
    assert lib.sar_runtime_hold_color_range(None, None) == INVALID


def test_to_velocity_formulas_and_refusals(sar):
    cfg = sar.Config.solar_sail()
    assert (cfg.ct_offset, cfg.ct_factor) == (0.8, -0.2)
    w = sar.ColorRange(-0.5, -0.25)
    out = sar.color_range_to_velocity(cfg, w)
    assert out.ct_offset == 0.8 - (-0.5) / -0.2 and out.ct_factor == -0.2 / (-0.25 - -0.5)
    back = out.replace(ct_offset=cfg.ct_offset, ct_factor=cfg.ct_factor)   # nothing else changed
    assert C.string_at(C.byref(back.c), C.sizeof(cfg.c)) == C.string_at(C.byref(cfg.c), C.sizeof(cfg.c))
    assert C.string_at(C.byref(sar.color_range_to_velocity(cfg, sar.ColorRange(3.0, 1.0, applied=False)).c), C.sizeof(cfg.c)) == \
        C.string_at(C.byref(cfg.c), C.sizeof(cfg.c))                       # a window that is not applied: the config as it is
    for bad_cfg, bad_w in ((sar.Config.poisson_saturne(), w),              # another transform
                           (cfg, sar.ColorRange(-0.5, -0.25, pos_lo=0.1)), (cfg, sar.ColorRange(-0.5, -0.25, pos_hi=0.5)),
                           (cfg, sar.ColorRange(-0.5, -0.25, pos_lo=1.0, pos_hi=0.0)),
                           (cfg.replace(ct_factor=0.0), w), (cfg, sar.ColorRange(1.0, 1.0)), (cfg, sar.ColorRange(0.0, math.inf)),
                           (cfg.replace(ct_factor=1e-300), sar.ColorRange(1e100, 2e100))):   # lo / ct_factor overflows
        with pytest.raises(sar.SarError) as ex:
            sar.color_range_to_velocity(bad_cfg, bad_w)
        assert ex.value.status == INVALID
    lib = sar.load_library()
    assert lib.sar_color_range_to_velocity(None, C.byref(w.c), C.byref(cfg.c)) == INVALID
    assert lib.sar_color_range_to_velocity(C.byref(cfg.c), None, C.byref(cfg.c)) == INVALID
    assert lib.sar_color_range_to_velocity(C.byref(cfg.c), C.byref(w.c), None) == INVALID


def test_to_velocity_is_the_same_window_within_the_rounding_of_four_operations(sar):
    """steps = (m + offset) * factor; the position from the new constants, (m + offset') * factor', against the windowed position
    ((steps - lo) / span): within 8 * 2^-53 * max(|lo|, |hi|, |steps|) / span — the rounding of four operations amplified by the
    cancellation."""
    rng = np.random.default_rng(7)
    cfg = sar.Config.solar_sail()
    for _ in range(2000):
        # (offset >= 0, as |dp| + offset of the reference's presets: a negative one could cancel |dp| and leave |offset * factor|,
        # which the bound does not name, as the largest term)
        offset, factor = float(rng.uniform(0.0, 1.0)), float(rng.choice([-1, 1]) * np.exp(rng.uniform(-3.0, 1.0)))
        m = float(np.exp(rng.uniform(math.log(1e-3), math.log(2.0))))
        s_all = (np.exp(rng.uniform(math.log(1e-3), math.log(2.0), size=2)) + offset) * factor
        lo, hi = float(s_all.min()), float(s_all.max())
        if not hi - lo > 0.0:
            continue
        out = sar.color_range_to_velocity(cfg.replace(ct_offset=offset, ct_factor=factor), sar.ColorRange(lo, hi))
        steps = (m + offset) * factor
        windowed = float(R.positions(np.float64(steps), R.Window(lo, hi, 0.0, 1.0, 1, 1)))
        direct = (m + out.ct_offset) * out.ct_factor
        assert abs(direct - windowed) <= 8 * 2.0 ** -53 * max(abs(lo), abs(hi), abs(steps)) / (hi - lo), (m, offset, factor, lo, hi)


def test_the_restatement_states_the_definition():
    neg0, nan = -0.0, math.nan
    vals = np.array([3.0, -math.inf, neg0, 0.0, 5e-324, -5e-324, math.inf, -2.0, 1.0, nan])
    keys = R.sortable(vals[:-1])
    order = np.argsort(keys)
    assert np.array_equal(vals[:-1][order].view(np.uint64),
                          np.array([-math.inf, -2.0, -5e-324, neg0, 0.0, 5e-324, 1.0, 3.0, math.inf]).view(np.uint64))
    assert np.array_equal(R.unsortable(keys).view(np.uint64), vals[:-1].view(np.uint64))
    count = np.ones(10, dtype=np.uint32)
    w = R.window(count, vals, 0.0, 1.0)
    assert (w.lo, w.hi, w.covered, w.applied) == (-math.inf, math.inf, 9, 0)          # NaN is not in the population; infinite ends
    w = R.window(count, vals, 0.2, 0.8)                                                # k = floor(1.8) = 1, floor(7.2) = 7
    assert (w.lo, w.hi, w.covered, w.applied) == (-2.0, 3.0, 9, 1)
    assert R.window(count, vals, 1.0, 1.0)[:2] == (math.inf, math.inf)                 # k clamps to n - 1
    count[1] = count[6] = 0
    assert R.window(count, vals, 0.0, 1.0) == R.Window(-2.0, 3.0, 0.0, 1.0, 7, 1)      # uncovered pixels are not in it either
    assert R.window(np.zeros(10), vals) == R.Window(0.0, 0.0, 0.0, 1.0, 0, 0)
    assert R.window(np.ones(4), np.full(4, 0.25)).applied == 0                         # span 0
    w = R.Window(-2.0, 3.0, 1.0, 0.25, 7, 1)
    assert R.positions(np.array([0.5]), w)[0] == 1.0 + ((0.5 - -2.0) / 5.0) * (0.25 - 1.0)
    assert np.array_equal(R.positions(vals, w._replace(applied=0)).view(np.uint64), vals.view(np.uint64))
    assert list(R.segments(np.array([-1.0, 0.0, 0.5, 0.999, 1.0, 7.0]), 6)) == [0, 0, 3, 5, 5, 5]


def test_bindings_expose_the_color_range():
    safe = open(os.path.join(ROOT, "bindings", "rust-safe", "src", "lib.rs")).read()
    assert "pub fn color_range<T: Mi355xTransform>(&mut self" in safe
    assert safe.count("pub fn set_color_range(&mut self, params: Option<&sys::SarColorRangeParams>)") == 2   # runtime and renderer
    assert "pub fn hold_color_range(&mut self, range: Option<&sys::SarColorRange>)" in safe
    assert "pub fn color_range_params_default()" in safe and "pub fn color_range_to_velocity(" in safe
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    sys_rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for name in ("sar_color_range_params_default", "sar_runtime_color_range", "sar_runtime_set_color_range", "sar_runtime_hold_color_range",
                 "sar_renderer_set_color_range", "sar_color_range_to_velocity"):
        assert name + "(" in hpp, name
        assert f"pub fn {name}(" in sys_rs, name


def test_c_program_builds_and_reports_a_missing_device_as_a_status(sar, tmp_path):
    pkg = os.path.join(ROOT, "strange_attractor_renderer_amd")
    exe = str(tmp_path / "sar_color_range")
    subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "c", "sar_color_range.c"), "-o", exe, "-L", pkg, "-l:libsar_hip.so",
                    f"-Wl,-rpath,{pkg}", "-Wl,-rpath,/opt/rocm/lib"], check=True)
    out = subprocess.run([exe, str(tmp_path), "64", "48", "8", "100", "5"], capture_output=True, text=True)
    if sar.device_count() > 0:
        assert out.returncode == 0, out.stderr
    else:
        assert out.returncode == 3 and "no HIP device" in out.stderr, (out.returncode, out.stderr)
