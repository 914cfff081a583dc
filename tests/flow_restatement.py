"""Flow rendering (include/sar.h: sar_flow_step, sar_runtime_render_flow) restated in numpy — test infrastructure.

Every floating-point operation is one numpy float64 operation (numpy never contracts a multiply and an add), in the order the header
gives; everything behind the fp64 steps is integers. The polynomial and the projection's constants are tests/manifold_restatement.py's
(coefficients, constants, next_point, project, within); the depth z2 is written out next to project's x2 as tests/volume_restatement.py
does, and goes through astype(float32) as render's `z2 as f32`. The colour transform is tests/golden/second_restatement.py's, on arrays.

A `view` is manifold_restatement's dict — the rows "x", "y", "z" of the field's coefficients, "center_camera", "axis", "rotation",
"scale", "angle", "width", "height" — plus "transform": ("adjusted_velocity", offset, factor) or ("poisson_saturne",).

A `frame` is what a runtime holds: dict(count (H, W) u32, zbuf (H, W) f32, steps (H, W) f64, max int)."""
import numpy as np

import manifold_restatement as M
import volume_restatement as V

F = np.float64
DEFAULTS = dict(dt=0.01, bound=1e6, transient=1000, stride=1, plot=1, chunk_jobs=0, chunk_steps=0)
DEFAULT_CHUNK_JOBS, DEFAULT_CHUNK_STEPS = 1 << 17, 1 << 12
COUNTERS = ("steps", "visits", "outside", "escaped_transient", "escaped", "alive", "count_atomics", "key_atomics", "max")


def view_of(cfg, angle=None) -> dict:
    """A sar_config (the oracle's structure, or Config.c) as a view."""
    v = V.view_of(cfg, angle)
    v["transform"] = ("adjusted_velocity", cfg.ct_offset, cfg.ct_factor) if cfg.color_transform == 1 else ("poisson_saturne",)
    return v


def empty_frame(width, height) -> dict:
    """Runtime::reset."""
    return dict(count=np.zeros((height, width), dtype=np.uint32), zbuf=np.full((height, width), -1.0, dtype=np.float32),
                steps=np.zeros((height, width), dtype=F), max=0)


def step(c, h, x, y, z):
    """One RK4 step of p' = P(p), P the polynomial of the rows c, on arrays (or scalars) of float64."""
    h, h2, h6 = F(h), F(h) * F(0.5), F(h) / F(6.0)
    p = (x, y, z)
    k1 = M.next_point(c, *p)
    k2 = M.next_point(c, *(p[i] + h2 * k1[i] for i in range(3)))
    k3 = M.next_point(c, *(p[i] + h2 * k2[i] for i in range(3)))
    k4 = M.next_point(c, *(p[i] + h * k3[i] for i in range(3)))
    return tuple(p[i] + h6 * (((k1[i] + F(2.0) * k2[i]) + F(2.0) * k3[i]) + k4[i]) for i in range(3))


def flow_step(view, p, dt=0.01, bound=1e6):
    """What sar_flow_step gives: (the new point, whether it stayed within bound)."""
    with np.errstate(all="ignore"):
        q = step(M.coefficients(view), dt, F(p[0]), F(p[1]), F(p[2]))
        return np.array(q, dtype=F), bool(M.within(*q, F(bound)))


def sortable32(f) -> np.ndarray:
    """The order-preserving u32 image of f32 values, as uint64 (room for the shift)."""
    b = np.asarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b >> np.uint64(31), ~b & np.uint64(0xFFFFFFFF), b | np.uint64(0x80000000))


def unsortable32(s) -> np.ndarray:
    s = np.asarray(s, dtype=np.uint64)
    b = np.where(s >> np.uint64(31), s & np.uint64(0x7FFFFFFF), ~s & np.uint64(0xFFFFFFFF))
    return b.astype(np.uint32).view(np.float32)


def project(view, k, x, y, z):
    """(in bounds, pixel index, f32 depth with -0.0 -> +0.0, screen-space point) of points: render's lines :773-802."""
    width, height = F(view["width"]), F(view["height"])
    m, cc = k["m"], k["cc"]
    fi, fj = M.project(k, x, y, z)
    sx = m[0][0] * x + m[0][1] * y + m[0][2] * z
    sy = m[1][0] * x + m[1][1] * y + m[1][2] * z
    sz = m[2][0] * x + m[2][1] * y + m[2][2] * z
    ax, az = sx + cc[0], sz + cc[1]
    z2 = ax * k["sin_v"] - az * k["cos_v"]
    inb = ~((fi >= width) | (fj >= height) | (fi < 0.0) | (fj < 0.0))          # NaN passes
    i = np.where(inb & (fi == fi), fi, 0.0).astype(np.int64)                  # `as u32`: truncation, NaN -> 0
    j = np.where(inb & (fj == fj), fj, 0.0).astype(np.int64)
    return inb, j * int(view["width"]) + i, z2.astype(np.float32) + np.float32(0.0), (sx, sy, sz)


def color_transform(view, d, ss):
    """render's colour transform of the displacement d at the screen-space point ss, on arrays."""
    t = view["transform"]
    mag = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    if t[0] == "adjusted_velocity":
        return (mag + F(t[1])) * F(t[2])
    COS, SIN = F(0.7009092642998509), F(0.7132504491541816)
    cc = view["center_camera"]
    x2 = (ss[0] + cc[0]) * COS + (ss[2] + cc[1]) * SIN
    out = (x2 < -0.0839) | (10.55 * x2 + ss[1] < 0.46 - 1.0941) | (1.0426 * x2 + ss[1] < 0.179 - 0.1576) | (0.5139 * x2 - ss[1] > -0.04 - 0.04092)
    color = (np.where(out, 0.0, 1.0) + mag) / 2.0
    return (color - 0.1) / 0.9


def resolve(frame, count_add, keys) -> dict:
    """The frame after a call: count_add (npix,) int64 visits per pixel, keys (npix,) uint64, against the incoming frame."""
    height, width = frame["count"].shape
    count = ((frame["count"].astype(np.int64).reshape(-1) + count_add) % (1 << 32)).astype(np.uint32)
    zbuf, steps = frame["zbuf"].reshape(-1).copy(), frame["steps"].reshape(-1).copy()
    zf = unsortable32(keys >> np.uint64(32))
    hue = unsortable32(keys & np.uint64(0xFFFFFFFF))
    with np.errstate(all="ignore"):
        win = (keys != 0) & (zf > zbuf)                                         # render's strict test
    zbuf[win] = zf[win]
    steps[win] = hue[win].astype(F)
    return dict(count=count.reshape(height, width), zbuf=zbuf.reshape(height, width), steps=steps.reshape(height, width),
                max=max(int(frame["max"]), int(count.max(initial=0))))


def flow(view, starts, steps_per_job, frame=None, **params):
    """(frame, stats) of sar_runtime_render_flow on `frame` (None: a reset runtime's). params: DEFAULTS' fields."""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = {**DEFAULTS, **params}
    width, height = int(view["width"]), int(view["height"])
    npix = width * height
    frame = empty_frame(width, height) if frame is None else frame
    c, k = M.coefficients(view), M.constants(view)
    h, bound, stride, plot = F(p["dt"]), F(p["bound"]), int(p["stride"]), bool(p["plot"])
    chunk_steps = int(p["chunk_steps"]) or DEFAULT_CHUNK_STEPS
    st = np.asarray(starts, dtype=F).reshape(-1, 3)
    n = st.shape[0]
    x, y, z = st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy()
    alive = np.ones(n, dtype=bool)
    s = dict.fromkeys(COUNTERS, 0)
    lo, hi = np.full(3, np.inf), np.full(3, -np.inf)
    count_add = np.zeros(npix, dtype=np.int64)
    keys = np.zeros(npix, dtype=np.uint64)
    run_idx, run_n, run_depth = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)

    def flush(which):
        which = which & (run_n > 0)
        s["count_atomics"] += int(which.sum())
        s["key_atomics"] += int((which & run_depth).sum())
        run_n[which] = 0
        run_depth[which] = False

    def advance():
        """One step of the jobs alive: the new points, and which of the jobs escaped with it."""
        nx, ny, nz = step(c, h, x, y, z)
        gone = alive & ~M.within(nx, ny, nz, bound)
        alive[gone] = False
        return nx, ny, nz, gone

    with np.errstate(all="ignore"):
        for _ in range(int(p["transient"])):
            nx, ny, nz, gone = advance()
            s["escaped_transient"] += int(gone.sum())
            x, y, z = np.where(alive, nx, x), np.where(alive, ny, y), np.where(alive, nz, z)
        for t in range(int(steps_per_job)):
            nx, ny, nz, gone = advance()
            s["escaped"] += int(gone.sum())
            s["steps"] += int(alive.sum())
            if alive.any():
                for a, v in enumerate((nx, ny, nz)):
                    lo[a], hi[a] = min(lo[a], v[alive].min()), max(hi[a], v[alive].max())
            if (t + 1) % stride == 0:
                inb, idx, zf, ss = project(view, k, nx, ny, nz)
                visit, out = alive & inb, alive & ~inb
                s["visits"] += int(visit.sum())
                s["outside"] += int(out.sum())
                if plot:
                    flush(out | (visit & (idx != run_idx)))
                    run_idx[visit] = idx[visit]
                    run_n[visit] += 1
                    deep = visit & (zf == zf)
                    run_depth |= deep
                    np.add.at(count_add, idx[visit], 1)
                    hue = color_transform(view, (nx - x, ny - y, nz - z), ss).astype(np.float32)
                    key = (sortable32(zf) << np.uint64(32)) | sortable32(hue)
                    np.maximum.at(keys, idx[deep], key[deep])
            x, y, z = np.where(alive, nx, x), np.where(alive, ny, y), np.where(alive, nz, z)
            if (t + 1) % chunk_steps == 0 or t + 1 == steps_per_job:
                flush(np.ones(n, dtype=bool))                                  # the end of a launch
    s["alive"] = int(alive.sum())
    assert s["alive"] + s["escaped"] + s["escaped_transient"] == n
    s["extent"] = np.array([lo[0], hi[0], lo[1], hi[1], lo[2], hi[2]])
    out_frame = resolve(frame, count_add, keys) if plot else frame
    s["max"] = int(out_frame["max"])
    return out_frame, s
