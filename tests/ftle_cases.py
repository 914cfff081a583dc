"""What the FTLE tests share (tests/test_ftle_host.py, tests/test_gpu_ftle.py): the Henon plane that holds every class of pixel, the
degenerate shapes, the basins' fixtures as further maps, and every parameter set sar_runtime_ftle must refuse with the exact text it
leaves."""
import numpy as np

import basin_restatement as B
import ftle_restatement as F
from basin_cases import PITCHFORK, PITCHFORK_MU, PITCHFORK_WINDOW, PRESET_COUNTS, PRESET_SHAPE, PRESET_WINDOW, preset_coeffs

# Henon, a = 1.4, b = 0.3, on a window around the attractor's basin: by a numpy run 232 bounded and 841 diverged pixels (escape steps
# 4 .. 10), 118 edge pixels, 113 two-sided in both axes, 88 one-sided along u and 82 along v, 17 NO_U, 3 NO_V and 1 isolated
HENON_GEOMETRY = dict(origin=(-2.5, -3.0, 0.0), du=(5.0, 0.0, 0.0), dv=(0.0, 9.0, 0.0))
HENON_SMALL = dict(HENON_GEOMETRY, width=37, height=29, steps=12)
DEGENERATE = [dict(HENON_GEOMETRY, width=1, height=29, steps=12), dict(HENON_GEOMETRY, width=37, height=1, steps=12),
              dict(HENON_GEOMETRY, width=1, height=1, steps=12)]
# a column and a row that hold bounded pixels: the one-pixel-wide shapes start on origin, the low corner
DEGENERATE[0]["origin"] = (0.0, -3.0, 0.0)
DEGENERATE[1]["origin"] = (-2.5, 0.0, 0.0)
DEGENERATE[2]["origin"] = (0.0, 0.0, 0.0)
FTLE_STEPS = 12


def maps(sar):
    """(name, coeffs, keyword arguments of ftle_map / F.ftle) of every picture the GPU tests hold to the restatement."""
    out = [("henon_small", F.henon(), HENON_SMALL)]
    out += [(f"degenerate_{k['width']}x{k['height']}", F.henon(), k) for k in DEGENERATE]
    out += [(f"pitchfork_{shape['width']}x{shape['height']}", B.pitchfork(PITCHFORK_MU), dict(PITCHFORK_WINDOW, **shape, steps=FTLE_STEPS))
            for shape, _, _, _ in PITCHFORK]
    out += [(name, preset_coeffs(sar, name), dict(PRESET_WINDOW, **PRESET_SHAPE, steps=FTLE_STEPS)) for name in sorted(PRESET_COUNTS)]
    return out


NAN, INF = float("nan"), float("inf")
W = "sar_runtime_ftle"
# (a change to a small valid picture, the exact text sar_runtime_ftle leaves)
REFUSED = [
    (dict(width=0), f"{W}: the plane must hold 1 to 2^24 pixels (0 x 4)"),
    (dict(height=0), f"{W}: the plane must hold 1 to 2^24 pixels (5 x 0)"),
    (dict(width=4097, height=4096), f"{W}: the plane must hold 1 to 2^24 pixels (4097 x 4096)"),
    (dict(steps=2 ** 31 + 1), f"{W}: transient and steps must be at most 2^31 (0, 2147483649)"),
    (dict(steps=0), f"{W}: steps must be 1 to 2^31 (0)"),
    (dict(chunk=2 ** 30 + 1), f"{W}: chunk must be at most 2^30 pixels (1073741825)"),
    (dict(coeffs=(7, NAN)), f"{W}: the map's coefficients must be finite (entry 7)"),
    (dict(coeffs=(29, INF)), f"{W}: the map's coefficients must be finite (entry 29)"),
    (dict(origin=(0, NAN)), f"{W}: the plane's origin, du and dv must be finite"),
    (dict(du=(1, INF)), f"{W}: the plane's origin, du and dv must be finite"),
    (dict(dv=(2, -INF)), f"{W}: the plane's origin, du and dv must be finite"),
    (dict(bound=0.0), f"{W}: bound must be positive and finite"),
    (dict(bound=-1.0), f"{W}: bound must be positive and finite"),
    (dict(bound=INF), f"{W}: bound must be positive and finite"),
    (dict(bound=NAN), f"{W}: bound must be positive and finite"),
    (dict(du=(0, 0.0)), f"{W}: du is zero (or its square underflows) over 5 columns"),
    (dict(dv=(1, 0.0)), f"{W}: dv is zero (or its square underflows) over 4 rows"),
    (dict(du=(0, 1e-170)), f"{W}: du is zero (or its square underflows) over 5 columns"),
    (dict(height=1, du=(0, 0.0)), f"{W}: du is zero (or its square underflows) over 5 columns"),
    (dict(width=1, dv=(1, 0.0)), f"{W}: dv is zero (or its square underflows) over 4 rows"),
    (dict(du=(0, 0.0), dv=(1, 0.0)), f"{W}: du is zero (or its square underflows) over 5 columns"),       # du is reported first
    (dict(dv=[(0, 8.0), (1, 0.0)]), f"{W}: du and dv must span a plane (the determinant of their Gram matrix is not positive and finite)"),
    (dict(du=(0, 1e160), dv=(1, 1e160)), f"{W}: du and dv must span a plane (the determinant of their Gram matrix is not positive and finite)"),
    (dict(steps=0, chunk=2 ** 30 + 1), f"{W}: steps must be 1 to 2^31 (0)"),                              # the order of the checks
    (dict(chunk=2 ** 30 + 1, bound=0.0), f"{W}: chunk must be at most 2^30 pixels (1073741825)"),
    (dict(bound=0.0, du=(0, 0.0)), f"{W}: bound must be positive and finite"),
]
# shapes with one axis absent accept what the absent axis would refuse
ACCEPTED = [dict(width=1, du=(0, 0.0)), dict(height=1, dv=(1, 0.0)), dict(width=1, height=1, du=(0, 0.0), dv=(1, 0.0)),
            dict(steps=2 ** 31), dict(steps=1), dict(chunk=2 ** 30), dict(width=4096, height=4096)]


def refused_params(sar, change):
    """A small valid FTLE map — 5 x 4 pixels, du = (4, 0, 0), dv = (0, 3, 0) — with one thing wrong (a scalar field, or (index, value) of
    an array field, or a list of those)."""
    p = sar.ftle_params(F.henon(), (-2.0, -0.5, 0.0), (4.0, 0.0, 0.0), (0.0, 3.0, 0.0), 5, 4, steps=8)
    for k, v in change.items():
        if isinstance(v, (tuple, list)):
            for i, x in v if isinstance(v, list) else [v]:
                getattr(p, k)[i] = x
        else:
            setattr(p, k, v)
    return p
