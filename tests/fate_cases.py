"""What the basin-probe tests share (tests/test_fate_host.py, tests/test_gpu_fate.py): the pictures, the point sets and the ladders
the GPU tests run — the host test shows on the restatement that these exact inputs keep the GPU cases honest —, the closed-form case
and every argument the two entries must refuse, with a piece of the message they leave.

Which cases the conditions bind. The ladder conditions — two bounded classes and DIVERGED among the base fates, three levels with
uncertain > 0 and one with uncertain = 0 — are held by LADDER, the input behind the K x n sweep: the sweep runs prefixes of its base
points and of its levels. The closed-form map, a grid = 1 picture and the solar-sail window each have ONE bounded class by construction
(x' = x^2 has one attractor, grid = 1 has one cell, and solar-sail's picture has one attractor at every grid and tail length tried), so
for them the condition that can fail, and is checked, is the share of UNKNOWN probes."""
import numpy as np

import basin_restatement as B
import fate_restatement as F
from basin_cases import PITCHFORK, PITCHFORK_MU, PITCHFORK_WINDOW, PRESET_SHAPE, PRESET_STEPS, PRESET_WINDOW

FATE_NS = (1, 2, 63, 64, 65, 255, 256, 257, 700)    # partial waves, workgroup edges
LADDER_KS = (1, 2, 10, 21, 31)                      # g = 3, 5, 21, 43, 63: many groups per wave, one group with idle lanes, a full wave
LADDER_NS = (1, 2, 3, 21, 22, 65)                   # at K = 10, three groups a wave: a last wave with one group, a count that is no multiple


def pitchfork_kw(case: int) -> dict:
    shape, steps, _, _ = PITCHFORK[case]
    return dict(PITCHFORK_WINDOW, **shape, **steps)


def window_points(window: dict, n: int, seed: int) -> np.ndarray:
    return F.plane_points(window["origin"], window["du"], window["dv"], n, seed)


# the sweep's input, on the 33 x 17 pitchfork picture: by the restatement its 65 base points hold 12 escaped, 25 of label 0 and 28 of
# label 1, levels 1..10 hold 55, 32, 24, 14, 9, 6, 3, 2, 1, 1 uncertain base points and levels 11..31 none; no probe is UNKNOWN
LADDER = dict(case=1, n=65, seed=2, dir=(1.0, 0.0, 0.0), eps0=0.5, levels=31)
LADDER_BASE_FATES = dict(escaped=12, labels=[25, 28], unknown=0)
LADDER_UNCERTAIN = [55, 32, 24, 14, 9, 6, 3, 2, 1, 1] + [0] * 21

# the issue's own figures: the 48 x 40 pitchfork picture, 512 plane points of default_rng(1), dir x, e = 0.25 * 2^-k at k = 0, 2, .., 18
RECORDED = dict(case=0, n=512, seed=1, dir=(1.0, 0.0, 0.0), eps0=0.25, levels=19)
RECORDED_BASE_FATES = dict(escaped=77, labels=[203, 232], unknown=0)
RECORDED_UNCERTAIN_EVERY_SECOND = [286, 109, 45, 13, 7, 0, 0, 0, 0, 0]

# solar-sail over basin_cases' preset window: 64 plane points, 24 levels from 1/8
SOLAR = dict(n=64, seed=1, dir=(1.0, 0.0, 0.0), eps0=0.125, levels=24)
SOLAR_KW = dict(PRESET_WINDOW, **PRESET_SHAPE, **PRESET_STEPS)

# the closed form: x' = x^2, y' = 0.5 y, z' = 0.5 z. Start points with |x| < 1 fall to the origin, |x| > 1 escape. Base points
# x0 = 1 - (2 i + 1) 2^-12 lie delta_i below the boundary x = 1, so level k is uncertain exactly where e_k > delta_i: 2^(10 - k) of
# the 1024 base points for e_k = 2^-(k + 1). No probe lands on x = 1: delta is an odd multiple of 2^-12, the coarsest e_k is 2^-2.
CLOSED_KW = dict(origin=(-1.5, 0.0, 0.0), du=(3.0, 0.0, 0.0), dv=(0.0, 0.0, 0.0), width=33, height=1, transient=64, steps=8, grid=4)
CLOSED_BOX = ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0))
CLOSED = dict(dir=(1.0, 0.0, 0.0), eps0=0.25, levels=10)
CLOSED_UNCERTAIN = [2 ** (10 - k) for k in range(1, 11)]


def closed_map() -> np.ndarray:
    c = np.zeros(30)
    c[2], c[10 + 5], c[20 + 8] = 1.0, 0.5, 0.5
    return c


def closed_base() -> np.ndarray:
    i = np.arange(1024, dtype=np.float64)
    return np.stack([1.0 - (2.0 * i + 1.0) * 2.0 ** -12, np.zeros(1024), np.zeros(1024)], axis=1)


# the grid = 1 picture: the 33 x 17 pitchfork in the unit box
GRID1_KW = dict(pitchfork_kw(1), grid=1)
GRID1 = dict(n=65, seed=2, dir=(1.0, 0.0, 0.0), eps0=0.5, levels=10)

NAN, INF = float("nan"), float("inf")
# (field changes of the ladder's parameters, a piece of the message)
LADDER_REFUSED = [
    (dict(levels=0), "levels must be"),
    (dict(levels=32), "levels must be"),
    (dict(eps0=0.0), "eps0"),
    (dict(eps0=-0.125), "eps0"),
    (dict(eps0=NAN), "eps0"),
    (dict(eps0=INF), "eps0"),
    (dict(dir=(0.0, 0.0, 0.0)), "all zero"),
    (dict(dir=(1.0, NAN, 0.0)), "dir must be finite"),
    (dict(dir=(INF, 0.0, 0.0)), "dir must be finite"),
]
