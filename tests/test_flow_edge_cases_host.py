"""CPU: the flow edge cases (tests/flow_edge_cases.py) without a device — every case's condition on the restatement's result, and
the restatement held to a second, independent reading of the header on the edge cases: job by job in plain Python, each step through
sar_flow_step, the projection, the f32 depth, the colour transform, the key's order and the final rule written out from
include/sar.h's flow section in Python floats and numpy.float32 scalars. The two must give count, zbuf, steps and max bit for bit, so
that the only reference the device's flows have does not share a misreading with the kernel on +-inf, NaN, subnormal and -0.0."""
import math
import struct

import numpy as np
import pytest

import flow_cases as K
import flow_edge_cases as E
import flow_restatement as R
import manifold_restatement as M


@pytest.mark.parametrize("name", E.NAMES + E.SHAPE_NAMES)
def test_the_restatement_reaches_the_cases_state(sar, name):
    case = E.Case(sar, name)
    E.check_condition(case)
    if name in E.NAMES:                                                     # and no launch shape changes a bit of the frame
        (_, a), (_, b) = case.shapes
        assert a != b and not K.same_frame(case.want(a)[0], case.want(b)[0])
        assert not K.same_stats(case.want(a)[1], case.want(b)[1], atomics=False)


def _sortable(v) -> int:
    """The order-preserving u32 image of an f32: negative values with every bit inverted, the others with the sign bit set."""
    b, = struct.unpack("<I", struct.pack("<f", v))
    return (~b & 0xFFFFFFFF) if b >> 31 else (b | 0x80000000)


def scalar_flow(sar, case) -> dict:
    """The frame after the case's call, one job and one step at a time."""
    width, height = case.size
    k = M.constants(case.view)                                              # the constants render hoists: no arithmetic of the flow's
    m = [[float(v) for v in row] for row in k["m"]]
    sin_v, cos_v, (ccx, ccy, ccz) = float(k["sin_v"]), float(k["cos_v"]), (float(v) for v in k["cc"])
    width_scaled, mid, half_height = float(k["width_scaled"]), float(k["scale_adjusted_mid"]), float(k["half_height"])
    kind, offset, factor = case.view["transform"]
    assert kind == "adjusted_velocity"
    dt, bound, stride = case.params["dt"], case.params["bound"], case.params["stride"]
    assert case.params["transient"] == 0
    best = {}                                                               # pixel -> [visits, (sortable depth, sortable hue), depth, hue]
    with np.errstate(all="ignore"):
        for start in case.starts:
            p = [float(v) for v in start]
            for t in range(case.steps):
                q, within = sar.flow_step(case.cfg, p, dt=dt, bound=bound, within=True)
                if not within:
                    break
                x, y, z = (float(v) for v in q)
                d = (x - p[0], y - p[1], z - p[2])
                p = [x, y, z]
                if (t + 1) % stride:
                    continue
                sx = m[0][0] * x + m[0][1] * y + m[0][2] * z
                sy = m[1][0] * x + m[1][1] * y + m[1][2] * z
                sz = m[2][0] * x + m[2][1] * y + m[2][2] * z
                ax, az = sx + ccx, sz + ccy
                x2, z2 = ax * cos_v + az * sin_v, ax * sin_v - az * cos_v
                fi, fj = (mid - x2) * width_scaled, half_height - (sy + ccz) * width_scaled
                if fi >= width or fj >= height or fi < 0.0 or fj < 0.0:    # (a NaN passes)
                    continue
                pix = (0 if fj != fj else int(fj)) * width + (0 if fi != fi else int(fi))
                slot = best.setdefault(pix, [0, None, None, None])
                slot[0] += 1
                zf = np.float32(z2) + np.float32(0.0)
                if zf != zf:                                                # counted, and offers no key
                    continue
                hue = np.float32((math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + offset) * factor)
                key = (_sortable(zf), _sortable(hue))
                if slot[1] is None or key > slot[1]:
                    slot[1:] = [key, zf, hue]
    out = R.empty_frame(width, height) if case.before is None else {f: (v.copy() if f != "max" else v) for f, v in case.before.items()}
    count, zbuf, steps = out["count"].reshape(-1), out["zbuf"].reshape(-1), out["steps"].reshape(-1)
    for pix, (visits, key, zf, hue) in best.items():
        count[pix] = (int(count[pix]) + visits) % (1 << 32)
        if key is not None and zf > zbuf[pix]:                              # render's strict test, IEEE: false against a NaN
            zbuf[pix], steps[pix] = zf, float(hue)
    out["max"] = max(int(out["max"]), int(count.max()))
    return out


@pytest.mark.parametrize("name", E.NAMES)
def test_a_scalar_reading_of_the_header_gives_the_restatements_frame(sar, name):
    case = E.Case(sar, name)
    want, _ = case.want(case.shapes[0][1])
    got = scalar_flow(sar, case)
    bad = K.same_frame(got, want)
    assert not bad, (name, bad, {f: int(np.count_nonzero(K.bits(got[f]) != K.bits(want[f]))) for f in bad if f != "max"})
