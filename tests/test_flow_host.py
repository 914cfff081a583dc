"""CPU: flow rendering without a device (include/sar.h: sar_flow_*, sar_runtime_render_flow) — the numpy restatement held to facts
that do not come from this code (the exact RK4 factor of p' = -p, Lorenz's fixed point, fourth-order convergence on Roessler, the
blow-up time of x' = 1 + x^2, Lorenz's known box); sar_flow_step against the restatement bit for bit; the defaults, the layouts and
every refusal that needs no device; flow_coefficients against the published equations; the mirrors of the ABI."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import flow_restatement as R
import manifold_restatement as M
from test_abi_and_host import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _view(rows, **kw):
    """A view of the field `rows` (3, 10): the identity rotation, a 64 x 48 image."""
    rows = np.asarray(rows, dtype=np.float64).reshape(3, 10)
    v = dict(x=list(rows[0]), y=list(rows[1]), z=list(rows[2]), center_camera=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 1.0), rotation=0.0, scale=1.0,
             angle=0.0, width=64, height=48, transform=("adjusted_velocity", 0.8, -0.2))
    v.update(kw)
    return v


def _rows(**terms):
    """Rows from {"x": {index: value}, ...}."""
    out = np.zeros((3, 10))
    for r, name in enumerate("xyz"):
        for k, v in terms.get(name, {}).items():
            out[r, k] = v
    return out


LORENZ = _rows(x={1: -10.0, 5: 10.0}, y={1: 28.0, 4: -1.0, 5: -1.0}, z={3: 1.0, 8: -8.0 / 3.0})
ROSSLER = _rows(x={5: -1.0, 8: -1.0}, y={1: 1.0, 5: 0.2}, z={0: 0.2, 4: 1.0, 8: -5.7})


# ---- 1. the restatement against facts from elsewhere ------------------------------------------------------------------------------
def test_linear_decay_is_the_exact_rk4_factor():
    c = M.coefficients(_view(_rows(x={1: -1.0}, y={5: -1.0}, z={8: -1.0})))
    h = Fraction(0.1)                                          # the double 0.1, exactly
    factor = 1 - h + h ** 2 / 2 - h ** 3 / 6 + h ** 4 / 24
    p = (1.0, -2.0, 0.5)
    q = R.step(c, 0.1, *(np.float64(v) for v in p))
    for got, start in zip(q, p):
        want = Fraction(start) * factor
        assert abs(Fraction(float(got)) - want) <= abs(want) * Fraction(1, 10 ** 14)


def test_lorenz_fixed_point_stays():
    c = M.coefficients(_view(LORENZ))
    r = math.sqrt(8.0 / 3.0 * 27.0)
    p0 = (np.float64(r), np.float64(r), np.float64(27.0))
    p = p0
    for _ in range(1000):
        p = R.step(c, 0.01, *p)
    assert max(abs(float(a) - float(b)) for a, b in zip(p, p0)) <= 1e-9


def test_fourth_order_on_rossler():
    c = M.coefficients(_view(ROSSLER))

    def at_one(n):
        p = (np.float64(1.0),) * 3
        for _ in range(n):
            p = R.step(c, 1.0 / n, *p)
        return np.array(p)

    ref = at_one(4096)
    e32, e64 = np.abs(at_one(32) - ref).max(), np.abs(at_one(64) - ref).max()
    assert 14.0 <= e32 / e64 <= 18.0, e32 / e64


def test_blow_up_escapes_at_step_158():
    """x' = 1 + x^2 from 0 is tan t, with its pole at pi / 2 = 157.08 steps of 0.01: 157 counted steps stay within the bound
    (tan 1.57 = 1256), and the job escapes with the 158th, the one that steps over the pole."""
    v = _view(_rows(x={0: 1.0, 2: 1.0}))
    for steps, escaped in ((157, 0), (158, 1), (300, 1)):
        _, s = R.flow(v, [[0.0, 0.0, 0.0]], steps, dt=0.01, bound=1e6, transient=0)
        assert (s["steps"], s["escaped"], s["alive"], s["escaped_transient"]) == (157, escaped, 1 - escaped, 0), (steps, s)
    p = np.zeros(3)
    for nth in range(1, 200):
        p, within = R.flow_step(v, p, 0.01, 1e6)
        if not within:
            break
    assert nth == 158
    _, s = R.flow(v, [[0.0, 0.0, 0.0]], 10, dt=0.01, bound=1e6, transient=200)
    assert (s["escaped_transient"], s["steps"], s["visits"], s["alive"]) == (1, 0, 0, 0)


def test_lorenz_stays_in_its_box():
    """One job from (1, 1, 1) at h = 0.005 as the feature runs a job — the default transient of 1000 uncounted steps, then 20 000
    counted ones: the extent of the counted points, the restatement's own statistic, lies in |x| < 20, |y| < 27, 0 < z < 50
    (x in [-18.67, 17.92], y in [-25.45, 24.03], z in [3.78, 46.04]). The box is the attractor's; the swing that carries the start
    point onto it is not part of it — with transient = 0 the 60th step (t = 0.30) reaches y = 27.18, which is the equation's own
    value there (RK4 at a tenth and a hundredth of the step gives 27.184) and lies in the transient here."""
    _, s = R.flow(_view(LORENZ), [[1.0, 1.0, 1.0]], 20000, dt=0.005, plot=0)
    assert R.DEFAULTS["transient"] == 1000 and (s["steps"], s["alive"], s["escaped"], s["escaped_transient"]) == (20000, 1, 0, 0)
    lo, hi = s["extent"][0::2], s["extent"][1::2]
    assert -20 < lo[0] and hi[0] < 20 and -27 < lo[1] and hi[1] < 27 and 0 < lo[2] and hi[2] < 50, (lo, hi)


# ---- 2. sar_flow_step is the restatement's step -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("lorenz", "rossler", "chen", "sprott_m"))
def test_flow_step_equals_the_restatement(sar, name):
    cfg = sar.Config.from_coefficients(sar.flow_coefficients(name)).replace(width=64, height=48)
    c = M.coefficients(R.view_of(cfg.c))
    rng = np.random.default_rng(20240 + len(name))
    pts = rng.uniform(-30.0, 30.0, size=(1000, 3))
    pts[:8] *= 1e5                                             # a few that leave the default bound
    for dt, bound in ((0.01, 1e6), (0.003, 50.0)):
        with np.errstate(all="ignore"):
            want = np.stack(R.step(c, dt, pts[:, 0], pts[:, 1], pts[:, 2]), axis=1)
            inside = M.within(want[:, 0], want[:, 1], want[:, 2], bound)
        assert 0 < inside.sum() < len(pts)
        for p, w, ok in zip(pts, want, inside):
            got, within = sar.flow_step(cfg, p, dt=dt, bound=bound, within=True)
            assert np.array_equal(got.view(np.uint64), w.view(np.uint64)) and within == bool(ok), (name, p)
    one, ok = R.flow_step(R.view_of(cfg.c), pts[100], 0.01, 1e6)
    assert np.array_equal(one, sar.flow_step(cfg, pts[100])) and ok


# ---- 3. defaults, layouts, refusals -----------------------------------------------------------------------------------------------
def test_defaults_and_layouts(sar):
    from strange_attractor_renderer_amd import _abi
    p = sar.flow_params()
    assert (p.dt, p.bound, p.transient, p.stride, p.plot, p.chunk_jobs, p.chunk_steps) == (0.01, 1e6, 1000, 1, 1, 0, 0)
    assert {f: getattr(p, f) for f in R.DEFAULTS} == R.DEFAULTS
    fields = ["dt", "bound", "transient", "stride", "plot", "chunk_jobs", "chunk_steps"]
    sfields = ["steps", "visits", "outside", "escaped_transient", "escaped", "alive", "count_atomics", "key_atomics", "extent", "max"]
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    prog += 'printf("%zu %zu\\n", sizeof(sar_flow_params), sizeof(sar_flow_stats));\n'
    prog += "".join(f'printf("%zu\\n", offsetof(sar_flow_params, {f}));\n' for f in fields)
    prog += "".join(f'printf("%zu\\n", offsetof(sar_flow_stats, {f}));\n' for f in sfields)
    prog += "return 0;}\n"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "t.c"), os.path.join(d, "t")
        open(src, "w").write(prog)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out[:2] == [C.sizeof(_abi.SarFlowParams), C.sizeof(_abi.SarFlowStats)] == [40, 120]
    assert out[2:] == [getattr(_abi.SarFlowParams, f).offset for f in fields] + [getattr(_abi.SarFlowStats, f).offset for f in sfields]
    # the launch bounds are fields of the parameters, not runtime options
    assert not [o for o in _abi.STABLE_OPTIONS if "flow" in o]


def test_refusals_that_need_no_device(sar):
    from strange_attractor_renderer_amd import _abi
    lib = sar.load_library()
    cfg = sar.Config.from_coefficients(sar.flow_coefficients("lorenz")).replace(width=64, height=48)
    starts = np.full((4, 3), 0.1)
    st = _abi.SarFlowStats()
    sp = starts.ctypes.data_as(C.POINTER(C.c_double))

    def call(cfg_=cfg, jobs=4, steps=16, s=sp, stats=st, **fields):
        p = sar.flow_params(**fields)
        status = lib.sar_runtime_render_flow(C.byref(cfg_.c) if cfg_ is not None else None, None, C.byref(p), jobs, steps, s,
                                             C.byref(stats) if stats is not None else None)
        return status, lib.sar_last_error().decode()

    for fields, text in ((dict(dt=0.0), "dt must be finite and positive"), (dict(dt=-0.01), "dt must be finite and positive"),
                         (dict(dt=math.nan), "dt must be finite and positive"), (dict(dt=math.inf), "dt must be finite and positive"),
                         (dict(bound=0.0), "bound must be finite and positive"), (dict(bound=-1.0), "bound must be finite and positive"),
                         (dict(bound=math.inf), "bound must be finite and positive"), (dict(bound=math.nan), "bound must be finite and positive"),
                         (dict(stride=0), "stride must be at least 1"), (dict(plot=2), "plot must be 0 or 1"), (dict(plot=-1), "plot must be 0 or 1"),
                         (dict(chunk_jobs=(1 << 24) + 1), "at most 2^24"), (dict(chunk_steps=(1 << 24) + 1), "at most 2^24")):
        status, msg = call(**fields)
        assert status == _abi.SAR_ERR_INVALID and text in msg, (fields, status, msg)
    assert call(cfg_=None)[0] == _abi.SAR_ERR_INVALID
    assert call(cfg_=cfg.replace(width=0))[0] == _abi.SAR_ERR_INVALID
    status, msg = call(jobs=0)
    assert status == _abi.SAR_ERR_INVALID and "n_jobs must be at least 1" in msg
    status, msg = call(steps=1 << 32)
    assert status == _abi.SAR_ERR_INVALID and "2^32 - 1" in msg
    status, msg = call(steps=3 * (1 << 32), stride=3)
    assert status == _abi.SAR_ERR_INVALID and "2^32 - 1" in msg
    status, msg = call(steps=3 * (1 << 32) - 1, stride=3)      # 2^32 - 1 plots: passes that check and stops at the runtime
    assert status == _abi.SAR_ERR_INVALID and "NULL" in msg
    for bad in (math.nan, math.inf, -math.inf):
        s2 = starts.copy()
        s2[2, 1] = bad
        status, msg = call(s=s2.ctypes.data_as(C.POINTER(C.c_double)))
        assert status == _abi.SAR_ERR_INVALID and "start point 2 is not finite" in msg
    for kw in (dict(), dict(s=None), dict(stats=None)):          # everything right but the runtime / the starts / the output
        status, msg = call(**kw)
        assert status == _abi.SAR_ERR_INVALID and "NULL" in msg
    assert lib.sar_flow_params_default(None) == _abi.SAR_ERR_INVALID
    xyz = np.zeros(3)
    xp = xyz.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.sar_flow_step(None, None, xp, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_flow_step(C.byref(cfg.c), None, None, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_flow_step(C.byref(cfg.c), C.byref(sar.flow_params(dt=0.0)), xp, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_flow_step(C.byref(cfg.c), C.byref(sar.flow_params(bound=math.nan)), xp, None) == _abi.SAR_ERR_INVALID
    assert lib.sar_flow_step(C.byref(cfg.c), None, xp, None) == _abi.SAR_OK and xyz[0] == 0.0      # Lorenz's origin is a fixed point
    with pytest.raises(ValueError):
        sar.flow_params(stride=-1)
    with pytest.raises(AttributeError):
        sar.flow_params(tolerance=1e-6)
    with pytest.raises(ValueError):
        sar.render_flow(cfg, None, jobs=4, starts=np.zeros((3, 3)))


# ---- 4. the named systems ---------------------------------------------------------------------------------------------------------
PUBLISHED = {
    "lorenz": lambda x, y, z: (10.0 * (y - x), x * (28.0 - z) - y, x * y - 8.0 / 3.0 * z),
    "rossler": lambda x, y, z: (-y - z, x + 0.2 * y, 0.2 + z * (x - 5.7)),
    "chen": lambda x, y, z: (35.0 * (y - x), (28.0 - 35.0) * x - x * z + 28.0 * y, x * y - 3.0 * z),
    "nose_hoover": lambda x, y, z: (y, -x + y * z, 1.0 - y * y),
    "sprott_a": lambda x, y, z: (y, -x + y * z, 1.0 - y * y),
    "sprott_b": lambda x, y, z: (y * z, x - y, 1.0 - x * y),
    "sprott_c": lambda x, y, z: (y * z, x - y, 1.0 - x * x),
    "sprott_d": lambda x, y, z: (-y, x + z, x * z + 3.0 * y * y),
    "sprott_e": lambda x, y, z: (y * z, x * x - y, 1.0 - 4.0 * x),
    "sprott_f": lambda x, y, z: (y + z, -x + 0.5 * y, x * x - z),
    "sprott_g": lambda x, y, z: (0.4 * x + z, x * z - y, -x + y),
    "sprott_h": lambda x, y, z: (-y + z * z, x + 0.5 * y, x - z),
    "sprott_i": lambda x, y, z: (-0.2 * y, x + z, x + y * y - z),
    "sprott_j": lambda x, y, z: (2.0 * z, -2.0 * y + z, -x + y + y * y),
    "sprott_k": lambda x, y, z: (x * y - z, x - y, x + 0.3 * z),
    "sprott_l": lambda x, y, z: (y + 3.9 * z, 0.9 * x * x - y, 1.0 - x),
    "sprott_m": lambda x, y, z: (-z, -x * x - y, 1.7 + 1.7 * x + y),
    "sprott_n": lambda x, y, z: (-2.0 * y, x + z * z, 1.0 + y - 2.0 * z),
    "sprott_o": lambda x, y, z: (y, x - z, x + x * z + 2.7 * y),
    "sprott_p": lambda x, y, z: (2.7 * y + z, -x + y * y, x + y),
    "sprott_q": lambda x, y, z: (-z, x - y, 3.1 * x + y * y + 0.5 * z),
    "sprott_r": lambda x, y, z: (0.9 - y, 0.4 + z, x * y - z),
    "sprott_s": lambda x, y, z: (-x - 4.0 * y, x + z * z, 1.0 + x),
}


def test_named_systems(sar):
    assert set(sar.FLOW_SYSTEMS) == set(PUBLISHED) and len(sar.FLOW_SYSTEMS) == 23
    assert np.array_equal(sar.flow_coefficients("lorenz"), LORENZ)
    assert np.array_equal(sar.flow_coefficients("rossler"), ROSSLER)
    assert np.array_equal(sar.flow_coefficients("lorenz", rho=99.5, sigma=3.0, beta=1.25),
                          _rows(x={1: -3.0, 5: 3.0}, y={1: 99.5, 4: -1.0, 5: -1.0}, z={3: 1.0, 8: -1.25}))
    assert np.array_equal(sar.flow_coefficients("rossler", a=0.1, b=0.3, c=14.0), _rows(x={5: -1.0, 8: -1.0}, y={1: 1.0, 5: 0.1}, z={0: 0.3, 4: 1.0, 8: -14.0}))
    assert np.array_equal(sar.flow_coefficients("nose_hoover", a=2.0)[2], _rows(z={0: 2.0, 6: -1.0})[2])
    for name, rhs in PUBLISHED.items():
        c = sar.flow_coefficients(name)
        assert c.shape == (3, 10) and c.dtype == np.float64
        for p in ((0.3, -1.7, 2.9), (-4.0, 0.25, -0.6), (1.5, 2.5, 3.5)):
            got = M.next_point(c, *(np.float64(v) for v in p))
            assert np.allclose([float(g) for g in got], rhs(*p), rtol=1e-13, atol=1e-13), (name, p)
    with pytest.raises(ValueError):
        sar.flow_coefficients("lorentz")
    with pytest.raises(ValueError):
        sar.flow_coefficients("sprott_a", a=1.0)
    with pytest.raises(ValueError):
        sar.flow_coefficients("lorenz", r=28.0)


# ---- 5. the mirrors ---------------------------------------------------------------------------------------------------------------
def test_mirrors_name_the_new_entries(sar):
    from strange_attractor_renderer_amd import _abi
    names = [n for n in declared_functions() if "flow" in n and "ftle" not in n]
    assert names == ["sar_flow_params_default", "sar_flow_step", "sar_runtime_render_flow"]
    lib = sar.load_library()
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    hpp = open(os.path.join(ROOT, "include", "sar.hpp")).read()
    for n in names:
        assert n in _abi.PROTOTYPES and hasattr(lib, n) and re.search(rf"pub fn {n}\s*\(", rs) and f"{n}(" in hpp, n
    for struct, mirror in (("SarFlowParams", _abi.SarFlowParams), ("SarFlowStats", _abi.SarFlowStats)):
        body = rs[rs.index(f"pub struct {struct} {{"):]
        assert re.findall(r"pub (\w+):", body[:body.index("}")]) == [f for f, _ in mirror._fields_]
    header = open(os.path.join(ROOT, "include", "sar.h")).read()
    for word in ("h6 * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)", "max(|x'|, |y'|, |z'|) <= bound", "(sortable(zf) << 32) | sortable((float)c)",
                 "Not here:"):
        assert word in header, word
    for fn in ("flow_params", "flow_step", "render_flow", "flow_extent", "flow_view", "flow_coefficients"):
        assert callable(getattr(sar, fn))
