"""What tests/test_gpu_device_log.py runs and tests/test_log_brackets_host.py checks the conditions of, from fixed seeds: the probe's
arguments, the two loaded Gas states, the exposure state whose maximum alone lies beyond the table, the gallery tile of two piled
pixels, and the parameters of the planes and FTLE maps the existing tests colour."""
import math

import numpy as np

from log_brackets import TABLE

W, H = 67, 31                      # 2077 pixels: nine blocks of 256 less 227, no multiple of a wave
RANGE_SLICE = (100, 1500)          # colorize_range_device's (first_px, n_px): neither a multiple of 64


# ---- the probe's arguments ----------------------------------------------------------------------------------------------------------
def probe_u32() -> np.ndarray:
    """kind 1: both sides of the table's end, the powers of two and their neighbours, the wrap, and random values on both sides."""
    rng = np.random.default_rng(20)
    planted = [TABLE - 1, TABLE, TABLE + 1, TABLE + 2]
    planted += [v for k in range(21, 32) for v in ((1 << k) - 1, 1 << k, (1 << k) + 1)]
    planted += [(1 << 32) - 1, 0, 1]
    above = rng.integers(TABLE + 1, 1 << 32, size=4096, dtype=np.uint64)
    below = rng.integers(1, TABLE + 1, size=256, dtype=np.uint64)
    return np.concatenate([np.array(planted, dtype=np.uint64), above, below]).astype(np.uint32)


PROBE_F64_CLASSES = [0.0, -0.0, -1.0, math.inf, -math.inf, math.nan, 1.7976931348623157e308]


def probe_f64() -> np.ndarray:
    """kind 0: around 1, the plane's mantissas in [0.5, 1), the FTLE's stretch2 over every binade, subnormals and the classes."""
    rng = np.random.default_rng(21)
    planted = [0.5, math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0)]
    mant = 0.5 + 0.5 * rng.random(2048)
    wide = np.ldexp(1.0 + rng.random(2048), rng.integers(-1022, 1024, size=2048).astype(np.int32))
    sub = [5e-324, 2.0 ** -1050]
    return np.concatenate([np.array(planted), mant, wide, np.array(sub), np.array(PROBE_F64_CLASSES)])


# ---- the loaded Gas states ------------------------------------------------------------------------------------------------------------
GAS_MAX = {"max_in_table": TABLE - 1, "max_beyond": 3_000_000_019}     # max + 1 = 2^20, the table's last entry / far beyond it


def gas_state(name: str):
    """(count, steps, zbuf, max) of W x H pixels: a quarter unvisited (count 0: with the reset state's steps they take colorize's
    short way, a few with other steps and with NaN), counts random on both sides of the table's end, count + 1 planted on 2^20 - 1,
    2^20, 2^20 + 1 and on the u32 wrap, steps outside [0, 1) and not finite."""
    rng = np.random.default_rng({"max_in_table": 30, "max_beyond": 31}[name])
    n = W * H
    count = np.zeros(n, dtype=np.uint64)
    kind = rng.random(n)
    inside = (kind >= 0.25) & (kind < 0.6)
    beyond = kind >= 0.6
    count[inside] = np.exp(rng.uniform(0.0, math.log(TABLE - 1), size=int(inside.sum()))).astype(np.uint64)          # 1 .. 2^20 - 2
    count[beyond] = np.exp(rng.uniform(math.log(TABLE + 1), math.log(2.0 ** 32 - 2), size=int(beyond.sum()))).astype(np.uint64)
    visited = np.nonzero(count)[0]
    planted = [TABLE - 2, TABLE - 1, TABLE] * 8 + [(1 << 32) - 1] * 3 + [1, GAS_MAX[name]]
    count[rng.choice(visited, len(planted), replace=False)] = planted
    steps = np.zeros(n)
    steps[count != 0] = rng.uniform(-0.2, 1.2, size=int((count != 0).sum()))
    odd = [math.nan, math.inf, -math.inf, -0.0, 1.0, 0.999999, 1.5, -2.0, 5e-324, 1.0 / 3.0]
    for k, p in enumerate(rng.choice(n, 4 * len(odd), replace=False)):       # on visited and unvisited pixels alike
        steps[p] = odd[k % len(odd)]
    zbuf = np.where(count != 0, rng.uniform(-0.5, 1.0, size=n), -1.0).astype(np.float32)
    return count.astype(np.uint32).reshape(H, W), steps.reshape(H, W), zbuf.reshape(H, W), GAS_MAX[name]


GAS_STATES = ("max_in_table", "max_beyond")


# ---- exposure: M + 1 beyond the table, both selected counts inside it ------------------------------------------------------------------
EXPOSURE_INSIDE_MAX = 5_000_034     # (log2(M + 1) * ln 2 lies a double outside ln(M + 1)'s bracket: stand-in (c) shows in this record)


def exposure_inside_state() -> np.ndarray:
    """Lognormal counts of a few thousand at most and one pixel of five million: the maximum."""
    rng = np.random.default_rng(40)
    c = np.exp(rng.normal(2.0, 1.6, size=(41, 53))).astype(np.uint64) + 1
    c[rng.random(c.shape) < 0.8] = 0
    c[17, 29] = EXPOSURE_INSIDE_MAX
    return c.astype(np.uint32)


# ---- the gallery tile -------------------------------------------------------------------------------------------------------------------
GALLERY_JOBS, GALLERY_ITERATIONS = 2048, 1100
GALLERY_SPLIT = 1000                                  # jobs on pixel 0; the other 1048 on pixel 1
GALLERY_COUNTS = (GALLERY_SPLIT * GALLERY_ITERATIONS, (GALLERY_JOBS - GALLERY_SPLIT) * GALLERY_ITERATIONS)    # 1 100 000 and 1 152 800
IDENTITY = np.zeros(30)
IDENTITY[1] = IDENTITY[10 + 5] = IDENTITY[20 + 8] = 1.0   # x' = x, y' = y, z' = z: every start point is a fixed point


def gallery_view() -> dict:
    """The fields of the base config that make the 2 x 1 tile's screen the plane itself: no rotation, no sweep angle, the camera on the
    origin, scale 1 — i = 1 - 2 x and j = 0.5 - 2 y, so x in (0, 0.5] is pixel 0 and x in (-0.5, 0] pixel 1."""
    return dict(rotation_angle=0.0, angle=0.0, center_camera=(0.0, 0.0, 0.0), scale=1.0)


def gallery_starts() -> np.ndarray:
    """Start points on both sides of the edge x = 0 between the two pixels, depths in front of the reset state's."""
    rng = np.random.default_rng(50)
    s = np.zeros((GALLERY_JOBS, 3))
    s[:, 0] = rng.uniform(0.001, 0.2, size=GALLERY_JOBS)
    s[GALLERY_SPLIT:, 0] *= -1.0
    s[:, 1] = rng.uniform(-0.1, 0.1, size=GALLERY_JOBS)
    s[:, 2] = rng.uniform(-0.4, -0.1, size=GALLERY_JOBS)
    return rng.permutation(s)                         # (the two sides mixed over the waves)


# ---- the planes and FTLE maps the existing tests colour -----------------------------------------------------------------------------------
PLANES = {   # tests/test_gpu_plane.py: test_l1_parity_with_the_restatement's first plane, test_spectrum_equals_the_search's
    "l1_48x40": dict(preset="poisson_saturne", axes=(0, 13), d=0.08, width=48, height=40, mode="l1", transient=1000, steps=2000, colors={}),
    "spectrum_24x20": dict(preset="poisson_saturne", axes=(3, 27), d=0.15, width=24, height=20, mode="spectrum", transient=1000, steps=2000,
                           colors=dict(threshold=0.05, chaos_scale=0.1, order_scale=0.5)),
}
FTLE_MAPS = ("henon_small", "poisson_saturne", "degenerate_1x1")        # tests/test_gpu_ftle.py: test_colours
FTLE_WINDOWS = ((None, None), ((-0.1, 0.35), 3.5))


# ---- stand-in logarithms: what the sets can and cannot tell ---------------------------------------------------------------------------------
def _c_log(x: float) -> float:
    return math.nan if x != x or x < 0.0 else -math.inf if x == 0.0 else math.log(x)


def log_two_ulps(x: float) -> float:
    """(a) host libm's value moved by two doubles."""
    y = _c_log(x)
    return math.nextafter(math.nextafter(y, math.inf), math.inf) if math.isfinite(y) and y != 0.0 else y


def log_float32(x: float) -> float:
    """(b) rounded through float32."""
    return float(np.float32(_c_log(x)))


def log_via_log2(x: float) -> float:
    """(c) log2(x) * ln 2."""
    return math.log2(x) * 0.6931471805599453 if x == x and 0.0 < x < math.inf else _c_log(x)


STAND_INS = {"two_ulps": log_two_ulps, "float32": log_float32, "log2_times_ln2": log_via_log2}
