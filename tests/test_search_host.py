"""CPU: the host half of the chaotic-map search (include/sar.h: sar_search_*, sar_frame_view) — the random-access candidate
generator against a numpy SplitMix64 restatement, the layouts of the three search structs in C, ctypes and Rust, and the
framing arithmetic against the reference's projection (src/lib.rs:774-789). No device needed."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import search_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("seed,index", [(0, 0), (1, 0), (1, 1), (1, 4095), (7, 123456), (0xDEADBEEF, 2**40 - 1), (3, 2**40 + 17),
                                        (2**64 - 1, 2**33)])
def test_candidate_is_the_splitmix64_restatement(sar, seed, index):
    got = sar.search_candidate(seed, index)
    want = R.candidates(seed, index, 1)[0].reshape(3, 10)
    assert got.shape == (3, 10)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert np.all(got >= -1.2) and np.all(got < 1.2)
    assert not np.any(np.signbit(got) & (got == 0.0))


def test_candidate_box_and_draw_order(sar):
    # draw k of the stream is mix64(seed + (k+1) * golden): candidate c holds draws 30c .. 30c+29 — consecutive candidates
    # continue one stream, whatever the box
    lo, hi = -0.5, 2.0
    c0 = sar.search_candidate(42, 5, lo, hi).ravel()
    d = R.mix64(np.uint64(42) + (np.arange(150, 180, dtype=np.uint64) + np.uint64(1)) * R.GOLDEN)
    u = (d >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
    assert np.array_equal(c0, lo + (hi - lo) * u)
    assert np.all((c0 >= lo) & (c0 < hi))
    # a box at zero: lo + span * 0 is +0.0, never -0.0
    z = sar.search_candidate(1, 0, -0.0, 0.0).ravel()
    assert np.all(z == 0.0) and not np.any(np.signbit(z))


def test_search_params_default(sar):
    p = sar.search_params()
    assert (p.seed, p.lo, p.hi, list(p.start), p.transient, p.steps, p.bound, p.min_lyapunov, p.min_ky_dim, p.keep_rejected) == \
        (0, -1.2, 1.2, [0.05] * 3, 1000, 20000, 1e6, 0.005, 0.0, 0)
    q = sar.search_params(seed=9, start=(0.1, 0.2, 0.3), keep_rejected=1, min_ky_dim=-math.inf)
    assert q.seed == 9 and list(q.start) == [0.1, 0.2, 0.3] and q.keep_rejected == 1 and q.min_ky_dim == -math.inf
    with pytest.raises(AttributeError):
        sar.search_params(no_such_field=1)


STRUCTS = {"sar_search_params": "SarSearchParams", "sar_search_record": "SarSearchRecord", "sar_search_stats": "SarSearchStats"}


def test_search_struct_layouts_match_c_ctypes_and_rust():
    from strange_attractor_renderer_amd import _abi
    prog = '#include <stdio.h>\n#include <stddef.h>\n#include "sar.h"\nint main(void){\n'
    for cname, pyname in STRUCTS.items():
        prog += f'printf("%zu\\n", sizeof({cname}));\n'
        for f, _ in getattr(_abi, pyname)._fields_:
            prog += f'printf("%zu\\n", offsetof({cname}, {f}));\n'
    prog += 'printf("%d %d %d\\n", SAR_SEARCH_BOUNDED, SAR_SEARCH_DIVERGED, SAR_SEARCH_DEGENERATE);\nreturn 0;}\n'
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
    assert out[k:] == [str(_abi.SAR_SEARCH_BOUNDED), str(_abi.SAR_SEARCH_DIVERGED), str(_abi.SAR_SEARCH_DEGENERATE)]
    assert C.sizeof(_abi.SarSearchRecord) == 144
    from strange_attractor_renderer_amd import api
    assert api.SEARCH_RECORD_DTYPE.names == tuple(f for f, _ in _abi.SarSearchRecord._fields_)
    assert [api.SEARCH_RECORD_DTYPE.fields[f][1] for f in api.SEARCH_RECORD_DTYPE.names] == \
        [getattr(_abi.SarSearchRecord, f).offset for f, _ in _abi.SarSearchRecord._fields_]
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    for pyname in STRUCTS.values():
        body = rs[rs.index(f"pub struct {pyname} {{"):]
        body = body[:body.index("}")]
        assert re.findall(r"pub (\w+):", body) == [f for f, _ in getattr(_abi, pyname)._fields_], pyname
    safe = open(os.path.join(ROOT, "bindings", "rust-safe", "src", "lib.rs")).read()
    assert "pub fn search(&mut self" in safe


def _project(cfg, corners, angle):
    """The reference's projection of screen-space points (src/lib.rs:774-789) -> (i, j) as f64."""
    cc = cfg.center_camera
    sin_v, cos_v = math.sin(angle), math.cos(angle)
    w, h = float(cfg.width), float(cfg.height)
    width_scaled, mid = w * cfg.scale, 0.5 / cfg.scale
    out = []
    for sx, sy, sz in corners:
        x2 = (sx + cc[0]) * cos_v + (sz + cc[1]) * sin_v
        out.append(((mid - x2) * width_scaled, h / 2. - (sy + cc[2]) * width_scaled))
    return np.array(out)


EXTENTS = [(-1.0, 1.0, -0.5, 0.5, -0.2, 0.3), (0.3, 0.9, -2.0, 1.5, 0.0, 4.0), (-3.0, -2.9, 1.0, 1.0001, -5.0, 5.0),
           (10.0, 12.0, -1.0, 1.0, -1.0, 1.0)]


@pytest.mark.parametrize("ext", EXTENTS)
@pytest.mark.parametrize("size", [(256, 256), (1920, 1080), (300, 800)])
def test_frame_view_still_keeps_the_box_inside_with_margin(sar, ext, size):
    margin = 0.05
    base = sar.Config.solar_sail(width=size[0], height=size[1])
    cfg = base.copy()
    assert sar.load_library().sar_frame_view(C.byref(cfg.c), (C.c_double * 6)(*ext), margin, 0) == 0
    assert list(cfg.rotation_axis) == list(base.rotation_axis) and cfg.angle == base.angle and cfg.width == size[0]
    corners = [(x, y, z) for x in ext[0:2] for y in ext[2:4] for z in ext[4:6]]
    ij = _project(cfg, corners, 0.0)
    w, h = size
    tol = 1e-9 * max(w, h)
    assert np.all(ij[:, 0] >= w * margin / 2 - tol) and np.all(ij[:, 0] <= w * (1 - margin / 2) + tol)
    assert np.all(ij[:, 1] >= h * margin / 2 - tol) and np.all(ij[:, 1] <= h * (1 - margin / 2) + tol)
    # the largest such scale: one axis touches the margin
    slack_i = min(ij[:, 0].min(), w - ij[:, 0].max()) / w
    slack_j = min(ij[:, 1].min(), h - ij[:, 1].max()) / h
    assert min(abs(slack_i - margin / 2), abs(slack_j - margin / 2)) < 1e-9


@pytest.mark.parametrize("ext", EXTENTS)
def test_frame_view_sweep_keeps_the_box_inside_at_every_angle(sar, ext):
    margin, w, h = 0.05, 512, 384
    cfg = sar.Config.poisson_saturne(width=w, height=h)
    assert sar.load_library().sar_frame_view(C.byref(cfg.c), (C.c_double * 6)(*ext), margin, 1) == 0
    corners = [(x, y, z) for x in ext[0:2] for y in ext[2:4] for z in ext[4:6]]
    tol = 1e-9 * w
    for angle in np.arange(64) * (2 * math.pi / 64):
        ij = _project(cfg, corners, float(angle))
        assert np.all(ij[:, 0] >= w * margin / 2 - tol) and np.all(ij[:, 0] <= w * (1 - margin / 2) + tol), angle
        assert np.all(ij[:, 1] >= h * margin / 2 - tol) and np.all(ij[:, 1] <= h * (1 - margin / 2) + tol), angle
    # a still of the same extent may zoom closer than the sweep
    still = sar.Config.poisson_saturne(width=w, height=h)
    sar.load_library().sar_frame_view(C.byref(still.c), (C.c_double * 6)(*ext), margin, 0)
    assert still.scale >= cfg.scale


def test_frame_view_rejects_what_cannot_be_framed(sar):
    lib = sar.load_library()
    cfg = sar.Config.solar_sail()
    for ext, margin in (((-math.inf, 1, 0, 1, 0, 1), 0.05), ((0, 1, 0, math.nan, 0, 1), 0.05), ((1, 1, 2, 2, 3, 3), 0.05),
                        ((0, 1, 0, 1, 0, 1), 1.0), ((0, 1, 0, 1, 0, 1), -0.1)):
        assert lib.sar_frame_view(C.byref(cfg.c), (C.c_double * 6)(*ext), margin, 0) == sar._abi.SAR_ERR_INVALID
    assert bytes(cfg.c) == bytes(sar.Config.solar_sail().c)


def test_search_refuses_step_counts_that_would_wrap(sar):
    """transient / steps above 2^31 are refused before anything touches a device (the kernels count steps in 32 bits); from
    Python they cannot even wrap into range (ctypes would turn steps=-1 into 2^32-1 silently)."""
    lib = sar.load_library()
    n_out = C.c_uint32()
    for field in ("steps", "transient"):
        for bad in (2**31 + 1, 2**32 - 1):
            p = sar.search_params()
            setattr(p, field, bad)
            assert lib.sar_runtime_search(None, C.byref(p), 0, 1, None, None, 0, C.byref(n_out), None) == sar._abi.SAR_ERR_INVALID
            assert b"at most 2^31" in lib.sar_last_error()
        for bad in (-1, 2**32):
            with pytest.raises(ValueError):
                sar.search_params(**{field: bad})
    with pytest.raises(ValueError):
        sar.search_params(seed=-1)


def test_restatement_self_check_kaplan_yorke():
    """A self-check of the test oracle (search_restatement.finish), not of the library: the GPU parity test holds the library's
    finish to it."""
    # lambda = (0.5, 0, -1): j = 2, D = 2 + 0.5 / 1; all negative: 0; sum of all positive: 3
    def rec(lams):
        e = [0, 0, 0]
        m = [math.exp(l) for l in lams]   # steps_done = 1: lambda_i = ln M_i
        return R.finish(R.BOUNDED, 1, e, m)
    lam, ky = rec([0.5, -1.0, 0.0])
    assert lam == pytest.approx([0.5, 0.0, -1.0]) and ky == pytest.approx(2.5)
    assert rec([-0.1, -0.2, -0.3])[1] == 0.0
    assert rec([0.1, 0.2, 0.3])[1] == 3.0
    assert rec([0.3, -0.1, -0.4])[1] == pytest.approx(2 + 0.2 / 0.4)
    lam, ky = R.finish(R.DEGENERATE, 1, [0, 0, 0], [1.0, 1.0, 1.0])   # no folded step: NaN
    assert all(math.isnan(v) for v in lam) and math.isnan(ky)
