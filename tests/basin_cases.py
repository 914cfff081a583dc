"""What the basin tests share (tests/test_basin_host.py, tests/test_gpu_basin.py): the pitchfork window with the figures a numpy run
gave, the preset windows, and every parameter set sar_runtime_basin must refuse, with a piece of the message it leaves."""
import numpy as np

# the pitchfork x' = mu x - x y, y' = x^2, z' = 0.5 z at mu = 1.5: the mirror pair of fixed points (+-sqrt(0.5), 0.5, 0) and the origin,
# which is reached only from the row y0 = mu (x1 = 0 exactly) and the column x0 = 0
PITCHFORK_MU = 1.5
PITCHFORK_WINDOW = dict(origin=(-2.0, -0.5, 0.05), du=(4.0, 0.0, 0.0), dv=(0.0, 3.0, 0.0))
#            shape                  steps                              sizes of the basins      escaped
PITCHFORK = [
    (dict(width=48, height=40), dict(transient=1000, steps=64, grid=16), [773, 773, 48], 326),
    (dict(width=33, height=17), dict(transient=300, steps=32, grid=8), [221, 221, 17], 102),   # partial tiles; the column x0 = 0 exists
]

# a window inside [-1, 1]^2 around the start box, at z = 0.05, for both presets; by the restatement at 48 x 40, 1000 + 64 steps it
# holds (escaped, bounded) = solar-sail (1301, 619), poisson-saturne (584, 1336): both fates above 5 % of the 1920 pixels
PRESET_WINDOW = dict(origin=(-0.5, -0.5, 0.05), du=(1.0, 0.0, 0.0), dv=(0.0, 1.0, 0.0))
PRESET_SHAPE = dict(width=48, height=40)
PRESET_STEPS = dict(transient=1000, steps=64, grid=16)
PRESET_COUNTS = {"solar_sail": (1301, 619), "poisson_saturne": (584, 1336)}


def preset_coeffs(sar, name: str) -> np.ndarray:
    cfg = getattr(sar.Config, name)()
    return np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])


REFUSED = [
    (dict(width=0), "2^24 pixels"),
    (dict(height=0), "2^24 pixels"),
    (dict(width=4097, height=4096), "2^24 pixels"),
    (dict(transient=2 ** 31 + 1), "at most 2^31"),
    (dict(steps=2 ** 31 + 1), "at most 2^31"),
    (dict(transient=2 ** 31, steps=2 ** 31), "below 2^32"),
    (dict(grid=0), "grid must be"),
    (dict(grid=129), "grid must be"),
    (dict(bound=0.0), "bound"),
    (dict(bound=-1.0), "bound"),
    (dict(bound=float("inf")), "bound"),
    (dict(bound=float("nan")), "bound"),
    (dict(coeffs=(7, float("nan"))), "coefficients must be finite"),
    (dict(coeffs=(29, float("inf"))), "coefficients must be finite"),
    (dict(origin=(0, float("nan"))), "origin, du and dv"),
    (dict(du=(1, float("inf"))), "origin, du and dv"),
    (dict(dv=(2, float("-inf"))), "origin, du and dv"),
    (dict(box_lo=(0, float("nan"))), "box_lo < box_hi"),
    (dict(box_hi=(1, float("inf"))), "box_lo < box_hi"),
    (dict(box_lo=(2, 1.0)), "box_lo < box_hi"),            # lo == hi
    (dict(box_lo=(0, 2.0)), "box_lo < box_hi"),            # lo > hi
    (dict(box_lo=(1, 0.0), box_hi=(1, 5e-324)), "not finite"),   # grid / (hi - lo) overflows
]


def refused_params(sar, change):
    """A small valid basin picture with one thing wrong (a scalar field, or (index, value) of an array field)."""
    import basin_restatement as B
    p = sar.basin_params(B.pitchfork(PITCHFORK_MU), width=5, height=4, transient=10, steps=8, grid=4, **PITCHFORK_WINDOW)
    for k, v in change.items():
        if isinstance(v, tuple):
            getattr(p, k)[v[0]] = v[1]
        else:
            setattr(p, k, v)
    return p
