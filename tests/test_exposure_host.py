"""CPU: the host half of auto exposure (include/sar.h: sar_exposure_params / sar_exposure) — the layouts of both structs in C,
ctypes and the Rust sys crate, the default parameters, their validation through the mode switch, and the bindings' methods.
No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRUCTS = {"sar_exposure_params": "SarExposureParams", "sar_exposure": "SarExposure"}


def test_exposure_struct_layouts_match_c_ctypes_and_rust():
    from strange_attractor_renderer_amd import _abi
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for cname, pyname in STRUCTS.items():
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        for f, _ in getattr(_abi, pyname)._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
    prog += 'return 0;}\n'
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
    assert k == len(out)
    assert C.sizeof(_abi.SarExposureParams) == 32 and C.sizeof(_abi.SarExposure) == 40
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname


def test_exposure_params_default(sar):
    p = sar.exposure_params()
    assert (p.q_black, p.q_white, p.level_black, p.level_white) == (0.0, 0.995, 0.0, 1.0)
    q = sar.exposure_params(q_white=0.9, level_black=0.1)
    assert (q.q_black, q.q_white, q.level_black, q.level_white) == (0.0, 0.9, 0.1, 1.0)
    with pytest.raises(AttributeError):
        sar.exposure_params(no_such_field=1)
    assert sar.load_library().sar_exposure_params_default(None) == 1   # SAR_ERR_INVALID


@pytest.mark.parametrize("bad", [dict(q_black=-0.1), dict(q_white=1.5), dict(q_black=0.6, q_white=0.5), dict(q_black=math.nan),
                                 dict(q_white=math.nan), dict(level_black=1.0), dict(level_black=2.0), dict(level_white=math.inf),
                                 dict(level_black=-math.inf), dict(level_white=math.nan)])
def test_exposure_parameters_are_validated_without_a_device(sar, bad):
    # the parameters are checked before the handle: with NULL handles the message tells which check refused the call
    from strange_attractor_renderer_amd import _abi
    lib = sar.load_library()
    p = sar.exposure_params(**bad)
    for fn in (lib.sar_runtime_set_exposure, lib.sar_renderer_set_exposure):
        assert fn(None, C.byref(p)) == _abi.SAR_ERR_INVALID
        assert lib.sar_last_error().decode().startswith("exposure: need"), lib.sar_last_error()
        assert fn(None, C.byref(sar.exposure_params())) == _abi.SAR_ERR_INVALID   # good parameters: the NULL handle is refused
        assert "is NULL" in lib.sar_last_error().decode(), lib.sar_last_error()
        assert fn(None, None) == _abi.SAR_ERR_INVALID


def test_bindings_expose_the_exposure():
    safe = open(os.path.join(ROOT, "bindings", "rust-safe", "src", "lib.rs")).read()
    assert "pub fn exposure<T: Mi355xTransform>(&mut self" in safe
    assert safe.count("pub fn set_exposure(&mut self, params: Option<&sys::SarExposureParams>)") == 2   # runtime and renderer
    assert "pub fn exposure_params_default()" in safe
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    for name in ("sar_exposure_params_default", "sar_runtime_exposure", "sar_runtime_set_exposure", "sar_renderer_set_exposure"):
        assert name + "(" in hpp, name
