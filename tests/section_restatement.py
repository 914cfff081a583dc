"""Poincare sections of flows (include/sar.h: sar_section_step, sar_runtime_section) restated in numpy — test infrastructure.

Every floating-point operation is one numpy float64 operation (numpy never contracts a multiply and an add), in the order the header
gives; everything behind the fp64 steps is integers. The RK4 step, the projection, the sortable images and the resolve are
tests/flow_restatement.py's (step, project, sortable32, resolve), the polynomial and the bound test tests/manifold_restatement.py's.

A `view` is flow_restatement's. A surface is ten float64 in the monomial order [1, x, x^2, xy, xz, y, y^2, yz, z, z^2]. The field's
coefficients `c` are (3, 10) — or (3, 10, n), one field per job, which the library does not offer and the host tests use to run a
family of fields in one pass."""
import numpy as np

import flow_restatement as R
import manifold_restatement as M

F = np.float64
FULL, SHORT, ESCAPED, ESCAPED_TRANSIENT = 0, 1, 2, 3
NONE = 0xFFFFFFFF
DEFAULTS = dict(dt=0.01, bound=1e6, transient=1000, direction=1, samples=1024, max_steps=1 << 20, plot=0, chunk_jobs=0, chunk_steps=0)
RECORD_DTYPE = np.dtype([(f, "<u4") for f in ("status", "found", "rough", "steps", "clock_step", "_pad")])
COUNTERS = ("steps", "crossings", "rough", "clocked", "full", "short_jobs", "escaped", "escaped_transient", "visits", "outside", "max")


def plane(normal, offset=0.0):
    s = np.zeros(10)
    s[0], s[1], s[5], s[8] = -offset, normal[0], normal[1], normal[2]
    return s


def g(s, x, y, z):
    """g = s0, then g = g + t[k] * s[k + 1], left to right."""
    acc = s[0]
    for k, t in enumerate((x, x * x, x * y, x * z, y, y * y, y * z, z, z * z)):
        acc = acc + t * s[k + 1]
    return acc


def rate(c, s, d, x, y, z):
    """Henon's right-hand side at p: (P * w, w), w = 1.0 / gdot."""
    px, py, pz = M.next_point(c, x, y, z)
    gx = ((s[1] + d[0] * x) + s[3] * y) + s[4] * z
    gy = ((s[5] + s[3] * x) + d[1] * y) + s[7] * z
    gz = ((s[8] + s[4] * x) + s[7] * y) + d[2] * z
    gdot = (gx * px + gy * py) + gz * pz
    w = F(1.0) / gdot
    return px * w, py * w, pz * w, w


def henon(c, s, h, bound, g0, x, y, z):
    """One RK4 step of Henon's system from (p, t = 0) with the step -g0: (q, dt, accepted)."""
    d = (F(2.0) * s[2], F(2.0) * s[6], F(2.0) * s[9])
    D = -g0
    D2, D6 = D * F(0.5), D / F(6.0)
    p = (x, y, z)
    k1 = rate(c, s, d, *p)
    k2 = rate(c, s, d, *(p[i] + D2 * k1[i] for i in range(3)))
    k3 = rate(c, s, d, *(p[i] + D2 * k2[i] for i in range(3)))
    k4 = rate(c, s, d, *(p[i] + D * k3[i] for i in range(3)))
    q = tuple(p[i] + D6 * (((k1[i] + F(2.0) * k2[i]) + F(2.0) * k3[i]) + k4[i]) for i in range(3))
    dt = F(0.0) + D6 * (((k1[3] + F(2.0) * k2[3]) + F(2.0) * k3[3]) + k4[3])
    ok = (F(0.0) <= dt) & (dt <= h) & M.within(*q, bound)
    return q, dt, ok


def refine(c, s, h, bound, g0, g1, p0, p1):
    """The crossing of a step whose ends lie on two sides: (q (3 arrays), dt, rough)."""
    q, dt, ok = henon(c, s, h, bound, g0, *p0)
    theta = g0 / (g0 - g1)
    rq = tuple(p0[i] + theta * (p1[i] - p0[i]) for i in range(3))
    return tuple(np.where(ok, q[i], rq[i]) for i in range(3)), np.where(ok, dt, theta * h), ~ok


def crossing(direction, g0, g1):
    """Which steps hold a crossing that `direction` takes."""
    side0, side1 = g0 >= 0.0, g1 >= 0.0
    up, down = ~side0 & side1, side0 & ~side1
    return ((up & (direction >= 0)) | (down & (direction <= 0))) & np.isfinite(g0) & np.isfinite(g1)


def section_step(view, surface, p, dt=0.01, bound=1e6, direction=1):
    """What sar_section_step gives: (p1, kind, q or None, dt or None)."""
    c, s = M.coefficients(view), np.asarray(surface, dtype=F)
    h, bound = F(dt), F(bound)
    with np.errstate(all="ignore"):
        p0 = tuple(np.array([v], dtype=F) for v in p)
        p1 = R.step(c, h, *p0)
        if not M.within(*p1, bound)[0]:
            return np.array([v[0] for v in p1]), -1, None, None
        g0, g1 = g(s, *p0), g(s, *p1)
        if not crossing(direction, g0, g1)[0]:
            return np.array([v[0] for v in p1]), 0, None, None
        q, t, rough = refine(c, s, h, bound, g0, g1, p0, p1)
    return np.array([v[0] for v in p1]), 2 if rough[0] else 1, np.array([v[0] for v in q]), F(t[0])


def run(c, surface, starts, **params):
    """The jobs alone: (points (n, samples, 3), ret (n, samples), records, stats without the picture's fields)."""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = {**DEFAULTS, **params}
    s = np.asarray(surface, dtype=F)
    h, bound, direction, samples, max_steps = F(p["dt"]), F(p["bound"]), int(p["direction"]), int(p["samples"]), int(p["max_steps"])
    st = np.asarray(starts, dtype=F).reshape(-1, 3)
    n = st.shape[0]
    x, y, z = st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy()
    status = np.full(n, -1, dtype=np.int64)                                   # -1: running
    found, rough, steps = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    clock, t_prev, dt_prev = np.full(n, NONE, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=F)
    points, ret = np.full((n, samples, 3), np.nan), np.full((n, samples), np.nan)
    total_steps = 0
    with np.errstate(all="ignore"):
        for _ in range(int(p["transient"])):
            nx, ny, nz = R.step(c, h, x, y, z)
            live = status == -1
            status[live & ~M.within(nx, ny, nz, bound)] = ESCAPED_TRANSIENT
            live = status == -1
            x, y, z = np.where(live, nx, x), np.where(live, ny, y), np.where(live, nz, z)
            if not live.any():
                break
        g0 = g(s, x, y, z)
        for t in range(max_steps):
            running = status == -1
            if not running.any():
                break
            nx, ny, nz = R.step(c, h, x, y, z)
            gone = running & ~M.within(nx, ny, nz, bound)
            status[gone], steps[gone] = ESCAPED, t
            live = running & ~gone
            total_steps += int(live.sum())
            g1 = g(s, nx, ny, nz)
            at = np.flatnonzero(live & crossing(direction, g0, g1))
            if at.size:
                ca = c[:, :, at] if np.ndim(c) == 3 else c
                q, dtc, rgh = refine(ca, s, h, bound, g0[at], g1[at], (x[at], y[at], z[at]), (nx[at], ny[at], nz[at]))
                rec = clock[at] != NONE
                j, k = at[rec], found[at[rec]]
                ret[j, k] = ((t - t_prev[j]).astype(F) * h + dtc[rec]) - dt_prev[j]
                for a in range(3):
                    points[j, k, a] = q[a][rec]
                found[j] += 1
                rough[j] += rgh[rec]
                clock[at[~rec]] = t
                t_prev[at], dt_prev[at] = t, dtc
                done = j[found[j] == samples]
                status[done], steps[done] = FULL, t + 1
            x, y, z, g0 = np.where(live, nx, x), np.where(live, ny, y), np.where(live, nz, z), np.where(live, g1, g0)
    left = status == -1
    status[left], steps[left] = SHORT, max_steps
    steps[status == ESCAPED_TRANSIENT] = 0
    records = np.zeros(n, dtype=RECORD_DTYPE)
    records["status"], records["found"], records["rough"], records["steps"], records["clock_step"] = status, found, rough, steps, clock
    have = ~np.isnan(ret)
    qs = points[have]
    with np.errstate(all="ignore"):
        res = np.abs(g(s, qs[:, 0], qs[:, 1], qs[:, 2])) if qs.size else np.zeros(0)
    stats = dict(steps=total_steps, crossings=int(found.sum()), rough=int(rough.sum()), clocked=int((clock != NONE).sum()),
                 full=int((status == FULL).sum()), short_jobs=int((status == SHORT).sum()), escaped=int((status == ESCAPED).sum()),
                 escaped_transient=int((status == ESCAPED_TRANSIENT).sum()), visits=0, outside=0,
                 extent=np.array([v for a in range(3) for v in ((qs[:, a].min(), qs[:, a].max()) if qs.size else (np.inf, -np.inf))]),
                 ret_min=F(ret[have].min()) if qs.size else F(np.inf), ret_max=F(ret[have].max()) if qs.size else F(-np.inf),
                 residual_max=F(np.fmax.reduce(res, initial=0.0)))
    assert stats["steps"] == int(steps.sum())
    return points, ret, records, stats


def section(view, surface, starts, frame=None, **params):
    """(points, ret, records, stats, frame) of sar_runtime_section on `frame` (None: a reset runtime's). params: DEFAULTS' fields."""
    width, height = int(view["width"]), int(view["height"])
    frame = R.empty_frame(width, height) if frame is None else frame
    points, ret, records, stats = run(M.coefficients(view), surface, starts, **params)
    if {**DEFAULTS, **params}["plot"]:
        have = ~np.isnan(ret)
        q, r = points[have], ret[have]
        count_add, keys = np.zeros(width * height, dtype=np.int64), np.zeros(width * height, dtype=np.uint64)
        if len(r):
            with np.errstate(all="ignore"):
                inb, idx, zf, _ = R.project(view, M.constants(view), q[:, 0], q[:, 1], q[:, 2])
            stats["visits"], stats["outside"] = int(inb.sum()), int((~inb).sum())
            np.add.at(count_add, idx[inb], 1)
            deep = inb & (zf == zf)
            key = (R.sortable32(zf) << np.uint64(32)) | R.sortable32(r.astype(np.float32))
            np.maximum.at(keys, idx[deep], key[deep])
        frame = R.resolve(frame, count_add, keys)
    stats["max"] = int(frame["max"])
    return points, ret, records, stats, frame
