"""CPU: the cases of tests/volume_edge_cases.py without a device — every case still reaches what it is for, and the numpy restatement's
march and section (tests/volume_restatement.py: whole images at once, np.where masks for the pixels that have stopped or see an empty
voxel) are held to a SECOND reading of include/sar.h's contract on every case: one pixel at a time, Python floats (IEEE doubles, one
operation per expression, never contracted), a loop that leaves at the slab where the march stops, math.sqrt, and integers for
everything behind the fp64 steps. Image bytes, the three march statistics, count and nearest must be equal."""
import math

import numpy as np
import pytest

import volume_edge_cases as E
import volume_restatement as R


# ---- the second reading -----------------------------------------------------------------------------------------------------------
def scalar_colour(v: float, palette) -> tuple:
    """Palette::interpolate as colorize applies it: v clamped to [0, 0.999999], the two rows around v * len (the last row repeated),
    c2 * t + c1 * (1 - t) and the square root."""
    rows = list(palette) + [palette[-1]]
    if v < 0.0:
        v = 0.0
    elif v >= 1.0:
        v = 0.999999
    v = v * float(len(palette))
    fl = math.floor(v)
    n = min(int(fl), len(palette) - 1)
    t = v - fl
    t1 = 1.0 - t
    return tuple(math.sqrt(rows[n + 1][ch] * t + rows[n][ch] * t1) for ch in range(3))


def scalar_u16(c: float) -> int:
    """c > 0 ? c : 0, c < 1 ? c : 1, then `as u16` of c * 65535.0 (saturating, NaN -> 0, truncation)."""
    c = c if c > 0.0 else 0.0
    c = c if c < 1.0 else 1.0
    e = c * 65535.0
    if e != e or e <= 0.0:
        return 0
    return 65535 if e >= 65535.0 else int(e)


def scalar_march(vol, vmax, palette, transparent, half_count=0.0, t_min=0.0, pos_lo=0.0, pos_hi=1.0, k0=0, k1=None, background=(0, 0, 0)):
    D, height, width = vol.shape
    k1 = D if k1 is None else k1
    half = float(half_count) if half_count != 0 else (float(vmax) * 0.125 if vmax else 1.0)
    colours = {}
    out = np.zeros((height, width, 4), dtype=np.uint16)
    slabs_seen = covered = n_stopped = 0
    for j in range(height):
        for i in range(width):
            column = vol[:, j, i].tolist()
            T, R_, G_, B_, seen, stopped = 1.0, 0.0, 0.0, 0.0, 0, False
            for k in range(k1 - 1, k0 - 1, -1):
                n = column[k]
                if n == 0:
                    continue
                if k not in colours:
                    colours[k] = scalar_colour(float(pos_lo) + ((float(k) + 0.5) / float(D)) * (float(pos_hi) - float(pos_lo)), palette)
                r_k, g_k, b_k = colours[k]
                seen += 1
                nd = float(n)
                a = nd / (nd + half)
                w = T * a
                R_ = R_ + w * r_k
                G_ = G_ + w * g_k
                B_ = B_ + w * b_k
                T = T * (1.0 - a)
                if T < t_min:
                    stopped = True
                    break
            if transparent:
                chans = [X / (1.0 - T) if T < 1.0 else 0.0 for X in (R_, G_, B_)] + [1.0 - T]
            else:
                chans = [X + T * (float(background[c]) / 65535.0) for c, X in enumerate((R_, G_, B_))] + [1.0]
            out[j, i] = [scalar_u16(c) for c in chans]
            slabs_seen += seen
            covered += seen > 0
            n_stopped += stopped
    return out, dict(slabs_seen=slabs_seen, covered=covered, stopped=n_stopped)


def scalar_section(vol, k0=0, k1=None):
    D, height, width = vol.shape
    k1 = D if k1 is None else k1
    count, nearest = np.zeros((height, width), dtype=np.uint32), np.zeros((height, width), dtype=np.int32)
    for j in range(height):
        for i in range(width):
            total, near = 0, -1
            for k, n in enumerate(vol[k0:k1, j, i].tolist(), start=k0):
                total = (total + n) & 0xFFFFFFFF                # wraps as count does
                if n:
                    near = k
            count[j, i], nearest[j, i] = total, near
    return count, nearest


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", E.NAMES)
def test_edge_case_reaches_what_it_was_built_for(name):
    E.check_condition(name)


@pytest.mark.parametrize("name", E.NAMES)
def test_restated_march_equals_the_scalar_reading(name):
    k = E.case(name)
    for label, pal, p in k.marches:
        for transparent in (0, 1):
            img, st = k.march(label, transparent)
            want_img, want_st = scalar_march(k.vol, k.stats["vmax"], E.PALETTES[pal], transparent, **p)
            bad = (img != want_img).any(axis=-1)
            assert not bad.any(), (name, label, transparent, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert st == want_st, (name, label, transparent)


@pytest.mark.parametrize("name", E.NAMES)
def test_restated_section_equals_the_scalar_reading(name):
    k = E.case(name)
    windows = k.windows if name != "big_reduce" else []            # (big_reduce is the reduction's case: statistics only)
    for k0, k1 in windows:
        count, nearest = k.section(k0, k1)
        want = scalar_section(k.vol, k0, k1)
        assert count.dtype == np.uint32 and nearest.dtype == np.int32
        assert np.array_equal(count, want[0]) and np.array_equal(nearest, want[1]), (name, k0, k1)


def test_the_scalar_colour_is_the_restated_blend():
    """The two readings of the palette alone, at the positions the cases reach and at the clamp's edges."""
    from shade_restatement import palette_blend
    vs = [-0.5, -0.0, 0.0, 5e-324, 0.3, 0.999998, 0.999999, float(np.nextafter(1.0, 0.0)), 1.0, 1.5, 0.2, 0.4, 0.6, 0.8, 1.0 / 15.0, 14.0 / 15.0]
    vs += E.positions(E.case("positions"), "outside").tolist()
    for pal in E.PALETTES.values():
        want = np.stack(palette_blend(np.array(vs), pal), axis=-1)
        got = np.array([scalar_colour(v, pal) for v in vs])
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_the_load_hook_is_in_the_hooks_build_alone(sar):
    """The door the GPU tests use (include/sar_test_hooks.h) is no part of the product: libsar_hip.so exports neither hook, include/sar.h
    names neither, the hooks build has both, and without a runtime or voxels the load is refused before any device call."""
    import ctypes as C
    import os
    from strange_attractor_renderer_amd import _abi
    product, hooks = C.CDLL(_abi.LIB_PATH), C.CDLL(_abi.HOOKS_PATH)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sar.h")).read()
    for hook in ("sar_runtime_debug_volume_load", "sar_runtime_debug_volume_stats"):
        assert not hasattr(product, hook) and hasattr(hooks, hook) and hook not in header and hook in _abi.OPTIONAL_PROTOTYPES
        assert hook not in _abi.PROTOTYPES
    lib = sar.load_library()
    one = np.ones(1, dtype=np.uint32)
    ptr = one.ctypes.data_as(C.POINTER(C.c_uint32))
    assert lib.sar_runtime_debug_volume_load(None, 1, -1.0, 1.0, ptr) == _abi.SAR_ERR_INVALID and "NULL" in lib.sar_last_error().decode()
    assert lib.sar_runtime_debug_volume_stats(None, None) == _abi.SAR_ERR_INVALID
    assert callable(sar.Runtime.debug_load_volume) and callable(sar.Volume.march_device)


def test_loaded_statistics_are_the_voxels():
    k = E.case("max_counts")
    assert k.stats["stored"] == k.stats["visits"] == sum(int(n) for n in k.vol.reshape(-1).tolist()) > 1 << 40
    assert E.stats_of(E.case("empty").vol) == dict(visits=0, stored=0, below=0, above=0, nan=0, nonempty=0, vmax=0, z_min=math.inf, z_max=-math.inf)
