"""What the orbit-diagram tests share (tests/test_orbit_host.py, tests/test_gpu_orbit.py): the logistic line and every parameter
set sar_runtime_orbit must refuse, with a piece of the message it leaves."""
import math
import re

import numpy as np


def logistic(lo=2.8, hi=4.4):
    """The line of x' = r x - r x^2 from r = lo to r = hi: entries 1 and 2 of the x row move together."""
    a, b = np.zeros(30), np.zeros(30)
    a[1], a[2], b[1], b[2] = lo, -lo, hi, -hi
    return a, b


REFUSED = [
    (dict(width=0), "columns"), (dict(height=0), "columns"), (dict(width=65537), "columns"), (dict(height=32769), "columns"),
    (dict(jobs=0), "jobs must be"), (dict(jobs=1025), "jobs must be"),
    (dict(jobs=2, steps=2 ** 31), "below 2^32"), (dict(jobs=1024, steps=2 ** 22), "below 2^32"),
    (dict(transient=2 ** 31 + 1), "at most 2^31"), (dict(jobs=1, steps=2 ** 31 + 1), "at most 2^31"),
    (dict(a7=math.nan), "a and b"), (dict(a0=math.inf), "a and b"), (dict(b29=-math.inf), "a and b"), (dict(b3=math.nan), "a and b"),
    (dict(proj=(1.0, math.nan, 0.0)), "proj"), (dict(proj=(math.inf, 0.0, 0.0)), "proj"),
    (dict(v_lo=math.nan), "v_lo"), (dict(v_hi=math.inf), "v_lo"), (dict(v_lo=-math.inf), "v_lo"),
    (dict(v_lo=1.0, v_hi=1.0), "v_lo"), (dict(v_lo=2.0, v_hi=1.0), "v_lo"),
    (dict(bound=0.0), "bound"), (dict(bound=-1.0), "bound"), (dict(bound=math.inf), "bound"), (dict(bound=math.nan), "bound"),
    (dict(v_lo=0.0, v_hi=5e-324), "not finite"),         # scale = height / 5e-324 = inf
]


def refused_params(sar, change):
    """A small valid diagram with one thing wrong (shared with tests/test_gpu_orbit.py)."""
    a, b = logistic()
    p = sar.orbit_params(a, b, width=5, height=64, jobs=8, transient=10, steps=20, v_range=(0.0, 1.0))
    for k, v in change.items():
        m = re.fullmatch(r"([ab])(\d+)", k)
        if m:
            getattr(p, m.group(1))[int(m.group(2))] = v
        elif k == "proj":
            for i in range(3):
                p.proj[i] = v[i]
        else:
            setattr(p, k, v)
    return p
