"""The views, the branches and the cases of the manifold tests (tests/test_manifold_host.py, tests/test_gpu_manifold.py).

The Henon map is taken in its classic form x' = 1 - a x^2 + y, y' = b x (its inverse is quadratic: x = y' / b, y = x' - 1 + a (y' / b)^2)
with the y coordinate stretched by KY = 2.5: x' = 1 - a x^2 + y / KY, y' = KY b x. The camera has one scale for both axes, so the
stretch is what lets a 128 x 96 image be the window x in [-1.5, 1.5], y / KY in [-0.45, 0.45]: pixel (i, j) holds
x = 1.5 - 3 i / 128 and y / KY = (48 - j) 0.9 / 96."""
import math

import numpy as np

import manifold_restatement as R

A, B, KY = 1.4, 0.3, 2.5


def _row(**entries):
    row = [0.0] * 10
    for name, v in entries.items():
        row[int(name[1:])] = v
    return row


def henon_view(width=128, height=96, a=A, b=B, **over) -> dict:
    """The window of the module's docstring at any size: x in [-1.5, 1.5] over the width, the rows centred on y = 0. The rotation is
    0 (the matrix is the identity), the angle 0: fi = (1.5 - x) width / 3, fj = height / 2 - y width / 3."""
    view = dict(x=_row(c0=1.0, c2=-a, c5=1.0 / KY), y=_row(c1=KY * b), z=_row(), center_camera=(0.0, 0.0, 0.0), axis=(0.0, 0.0, 1.0),
                rotation=0.0, scale=1.0 / 3.0, angle=0.0, width=width, height=height)
    view.update(over)
    return view


def henon_saddle(right=True, a=A, b=B):
    """A fixed point of the map, its unstable multiplier and that multiplier's unit eigenvector, in closed form: x* = (-(1 - b) +-
    sqrt((1 - b)^2 + 4 a)) / 2 a, y* = KY b x*; lambda solves l^2 + 2 a x* l - b = 0 and its eigenvector is (lambda, KY b, 0). The
    right point's multiplier is below -1, the left one's above 1."""
    xs = (-(1.0 - b) + (1.0 if right else -1.0) * math.sqrt((1.0 - b) ** 2 + 4.0 * a)) / (2.0 * a)
    root = math.sqrt(a * a * xs * xs + b)
    lam = -a * xs - root if right else -a * xs + root
    v = np.array([lam, KY * b, 0.0])
    v = v / math.sqrt(float(v @ v))
    return (xs, KY * b * xs, 0.0), lam, tuple(-v if v[np.argmax(np.abs(v))] < 0 else v)


BASE_R, LAMBDA_R, DIR_R = henon_saddle(True)
BASE_L, LAMBDA_L, DIR_L = henon_saddle(False)
RIGHT = (BASE_R, DIR_R, 1e-6, 2)           # the saddle inside the attractor: one branch, two steps per return
RIGHT_MINUS = (BASE_R, DIR_R, -1e-6, 2)
LEFT_IN = (BASE_L, DIR_L, 1e-6, 1)         # the saddle on the basin boundary: its two sides, one step per return
LEFT_OUT = (BASE_L, DIR_L, -1e-6, 1)
FAR_AWAY = ((50.0, 0.0, 0.0), (1.0, 0.0, 0.0), 1e-3, 2)   # x' = 1 - 1.4 * 2500, then beyond 1e6: its domain escapes

HENON = dict(view=henon_view(), branches=[RIGHT], samples=4096, steps=32, max_span=16)   # the case of the covering test

ROTATED = henon_view(64, 48, center_camera=(0.1, -0.05, 0.02), axis=(0.3, 0.5, -0.4), rotation=0.9, scale=0.3, angle=0.6)
MINUS_ZERO = henon_view(64, 48)
for _r in "xyz":
    MINUS_ZERO[_r] = [(-0.0 if v == 0.0 else v) for v in MINUS_ZERO[_r]]

# name -> dict(view, branches, and the parameters): one call each, all held bit for bit against the restatement on the GPU
CASES = {f"samples_{s}": dict(view=henon_view(64, 48), branches=[RIGHT], samples=s) for s in (2, 63, 64, 65, 127)}
CASES.update({
    "samples_4096": dict(view=henon_view(64, 48), branches=[RIGHT], samples=4096),
    "samples_64_late": dict(view=henon_view(64, 48), branches=[(BASE_R, DIR_R, 1e-2, 2)], samples=64, steps=6),   # the seam spread over pixels
    "samples_127_late": dict(view=henon_view(67, 45), branches=[(BASE_R, DIR_R, 1e-2, 2)], samples=127, steps=8),
    "steps_0": dict(view=henon_view(64, 48), branches=[RIGHT], samples=127, steps=0),
    "steps_1": dict(view=henon_view(64, 48), branches=[RIGHT], samples=127, steps=1),
    "branches_3_two_equal": dict(view=henon_view(64, 48), branches=[RIGHT, RIGHT, RIGHT_MINUS], samples=1000),
    "period_1": dict(view=henon_view(64, 48), branches=[LEFT_IN], samples=1000),
    "max_span_1": dict(view=henon_view(64, 48), branches=[RIGHT], samples=1000, max_span=1),
    "max_span_4096": dict(view=henon_view(64, 48), branches=[RIGHT], samples=127, max_span=4096),
    "image_1x1": dict(view=henon_view(1, 1), branches=[RIGHT], samples=127),
    "image_67x45": dict(view=henon_view(67, 45), branches=[RIGHT, LEFT_IN], samples=1000),
    "image_128x96": HENON,
    "rotated": dict(view=ROTATED, branches=[RIGHT, LEFT_IN], samples=1000),
    "minus_zero": dict(view=MINUS_ZERO, branches=[RIGHT], samples=1000),
    "domain_escaped_among_good": dict(view=henon_view(64, 48), branches=[RIGHT, FAR_AWAY, LEFT_IN], samples=127),
    "dies_midway": dict(view=henon_view(64, 48), branches=[LEFT_OUT, LEFT_IN], samples=1000),   # the outer side leaves for infinity
    "dies_midway_small_bound": dict(view=henon_view(64, 48), branches=[RIGHT], samples=1000, bound=1.2),
    "far_endpoints": dict(view=henon_view(64, 48, scale=2e7), branches=[RIGHT, LEFT_IN], samples=127, max_span=4096),
})


def parameters(case) -> dict:
    return {k: case.get(k, v) for k, v in R.DEFAULTS.items()}


_REFERENCES = {}


def reference(name):
    """The restatement of a case, computed once: (count, first, records). Callers leave it unchanged."""
    if name not in _REFERENCES:
        case = CASES[name]
        _REFERENCES[name] = R.manifold(case["view"], R.branches_array(case["branches"]), **parameters(case))
    return _REFERENCES[name]


def config_of(sar, view):
    """The view as the library's Config (the colours are solar_sail's; the manifolds do not read them)."""
    return sar.Config.solar_sail().replace(coeff_x=view["x"], coeff_y=view["y"], coeff_z=view["z"], center_camera=view["center_camera"],
                                           rotation_axis=view["axis"], rotation_angle=view["rotation"], scale=view["scale"],
                                           angle=view["angle"], width=view["width"], height=view["height"])


def attractor_pixels(view, n=200_000, transient=1000, start=(0.1, 0.1, 0.0)) -> np.ndarray:
    """The sorted pixel indices inside the image that an n-point orbit of the view's map visits after a transient."""
    p = tuple(float(v) for v in start)
    pts = np.empty((n, 3))
    for i in range(transient + n):
        p = R.G.next_point(view, p)   # (plain Python floats: the orbit need not equal anyone's bit for bit)
        if i >= transient:
            pts[i - transient] = p
    _, X, Y = R.place(*R.project(R.constants(view), pts[:, 0], pts[:, 1], pts[:, 2]))
    inside = (X >= 0) & (X < view["width"]) & (Y >= 0) & (Y < view["height"])
    return np.unique(Y[inside] * view["width"] + X[inside])
