"""Volume rendering (include/sar.h: sar_runtime_volume*, sar_volume_slab) restated in numpy — test infrastructure.

Every floating-point operation is one numpy float64 operation (numpy never contracts a multiply and an add), in the order the header
gives; everything behind the fp64 steps is integers. The map step and the projection's constants are tests/manifold_restatement.py's
(coefficients, constants, next_point, project); the depth z2 is written out next to project's x2, and goes through astype(float32)
as render's `z2 as f32` does. The palette blend and `as u16` are tests/shade_restatement.py's.

A `view` is manifold_restatement's dict: the rows "x", "y", "z" of the map's coefficients, "center_camera", "axis", "rotation",
"scale", "angle", "width", "height"."""
import numpy as np

import manifold_restatement as M
from shade_restatement import as_u16, palette_blend

F = np.float64
BELOW, ABOVE, NAN = -1, -2, -3
WARMUP = 1000
STATS = ("visits", "stored", "below", "above", "nan", "nonempty", "vmax", "z_min", "z_max")
MARCH_DEFAULTS = dict(half_count=0.0, t_min=0.0, pos_lo=0.0, pos_hi=1.0, k0=0, k1=None, background=(0, 0, 0))


def view_of(cfg, angle=None) -> dict:
    """A sar_config (the oracle's structure, or Config.c) as a view."""
    return dict(x=list(cfg.coeff_x), y=list(cfg.coeff_y), z=list(cfg.coeff_z), center_camera=tuple(cfg.center_camera),
                axis=tuple(cfg.rotation_axis), rotation=cfg.rotation_angle, scale=cfg.scale, angle=cfg.angle if angle is None else angle,
                width=int(cfg.width), height=int(cfg.height))


def palette_of(cfg) -> list:
    return [tuple(cfg.palette_rgb[k]) for k in range(cfg.palette_len)]


def dscale(slabs, z_lo, z_hi):
    return F(slabs) / (F(z_hi) - F(z_lo))


def slab(zf, slabs, z_lo, z_hi) -> np.ndarray:
    """int64 per depth: the slab of the f32 depth zf, or BELOW / ABOVE / NAN."""
    with np.errstate(all="ignore"):
        u = (np.asarray(zf, dtype=np.float32).astype(F) - F(z_lo)) * dscale(slabs, z_lo, z_hi)
        k = np.where((u >= 0.0) & (u < F(slabs)), u, 0.0).astype(np.int64)   # (truncation)
        return np.where(u != u, NAN, np.where(u < 0.0, BELOW, np.where(u >= F(slabs), ABOVE, k)))


def visits(view, starts, iterations):
    """Per counted iteration of every job at once: (in bounds, pixel index, f32 depth), arrays over the jobs. A generator: the
    warm-up's WARMUP uncounted steps, then `iterations` steps of render's loop body up to the visit."""
    c, k = M.coefficients(view), M.constants(view)
    width, height = F(view["width"]), F(view["height"])
    st = np.asarray(starts, dtype=F).reshape(-1, 3)
    x, y, z = st[:, 0].copy(), st[:, 1].copy(), st[:, 2].copy()
    m, cc = k["m"], k["cc"]
    with np.errstate(all="ignore"):
        for _ in range(WARMUP):
            x, y, z = M.next_point(c, x, y, z)
        for _ in range(iterations):
            x, y, z = M.next_point(c, x, y, z)
            fi, fj = M.project(k, x, y, z)
            sx = m[0][0] * x + m[0][1] * y + m[0][2] * z
            sz = m[2][0] * x + m[2][1] * y + m[2][2] * z
            ax, az = sx + cc[0], sz + cc[1]
            z2 = ax * k["sin_v"] - az * k["cos_v"]
            inb = ~((fi >= width) | (fj >= height) | (fi < 0.0) | (fj < 0.0))          # NaN passes
            i = np.where(inb & (fi == fi), fi, 0.0).astype(np.int64)                  # `as u32`: truncation, NaN -> 0
            j = np.where(inb & (fj == fj), fj, 0.0).astype(np.int64)
            yield inb, j * int(view["width"]) + i, z2.astype(np.float32)


def volume(view, starts, iterations, slabs, z_lo, z_hi, into=None):
    """(vol, stats): vol (slabs, height, width) u32 — added to `into`'s (vol, stats) where that is given, as add = 1 does — and the
    statistics as a dict."""
    width, height = int(view["width"]), int(view["height"])
    npix = width * height
    vol = np.zeros(slabs * npix, dtype=np.int64)
    s = dict(visits=0, stored=0, below=0, above=0, nan=0)
    z_min, z_max = np.float32(np.inf), np.float32(-np.inf)
    for inb, idx, zf in visits(view, starts, iterations):
        k = slab(zf, slabs, z_lo, z_hi)
        s["visits"] += int(inb.sum())
        s["below"] += int((inb & (k == BELOW)).sum())
        s["above"] += int((inb & (k == ABOVE)).sum())
        s["nan"] += int((inb & (k == NAN)).sum())
        stored = inb & (k >= 0)
        s["stored"] += int(stored.sum())
        np.add.at(vol, k[stored] * npix + idx[stored], 1)
        seen = zf[inb & np.isfinite(zf)]
        if seen.size:
            z_min, z_max = min(z_min, seen.min()), max(z_max, seen.max())
    if into is not None:
        vol += into[0].astype(np.int64).reshape(-1)
        for name in ("visits", "stored", "below", "above", "nan"):
            s[name] += into[1][name]
        z_min, z_max = min(z_min, np.float32(into[1]["z_min"])), max(z_max, np.float32(into[1]["z_max"]))
    vol = (vol % (1 << 32)).astype(np.uint32).reshape(slabs, height, width)
    s.update(nonempty=int(np.count_nonzero(vol)), vmax=int(vol.max(initial=0)), z_min=float(z_min), z_max=float(z_max))
    assert s["visits"] == s["stored"] + s["below"] + s["above"] + s["nan"]
    return vol, s


def learned_range(z_min, z_max) -> tuple:
    """What volume(z_range=None) makes of a probe's depths."""
    z_min, z_max = F(z_min), F(z_max)
    if not z_min <= z_max:
        return -1.0, 1.0
    span = z_max - z_min
    return (float(z_min - span / 64.0), float(z_max + span / 64.0)) if span > 0.0 else (float(z_min - 0.5), float(z_max + 0.5))


def section(vol, k0=0, k1=None):
    """(count u32, nearest int32) of the slabs k0 <= k < k1."""
    k1 = vol.shape[0] if k1 is None else k1
    part = vol[k0:k1].astype(np.int64)
    count = (part.sum(axis=0) % (1 << 32)).astype(np.uint32)
    ks = np.arange(k0, k1, dtype=np.int64).reshape(-1, 1, 1)
    nearest = np.where(part != 0, ks, -1).max(axis=0).astype(np.int32)
    return count, nearest


def march(vol, vmax, palette, transparent, half_count=0.0, t_min=0.0, pos_lo=0.0, pos_hi=1.0, k0=0, k1=None, background=(0, 0, 0),
          reverse=False):
    """(rgba (height, width, 4) u16, stats): the slabs composited front to back — k1 - 1 down to k0 —, or in the opposite order with
    reverse=True (the tests' wrong direction)."""
    D, height, width = vol.shape
    k1 = D if k1 is None else k1
    half = F(half_count) if half_count != 0 else (F(vmax) * F(0.125) if vmax else F(1.0))
    T = np.ones((height, width), dtype=F)
    R, G, B = (np.zeros((height, width), dtype=F) for _ in range(3))
    seen = np.zeros((height, width), dtype=np.int64)
    live = np.ones((height, width), dtype=bool)
    stopped = np.zeros((height, width), dtype=bool)
    order = range(k0, k1) if reverse else range(k1 - 1, k0 - 1, -1)
    with np.errstate(all="ignore"):
        for k in order:
            v = F(pos_lo) + ((F(k) + F(0.5)) / F(D)) * (F(pos_hi) - F(pos_lo))
            r_k, g_k, b_k = (F(ch) for ch in palette_blend(v, palette))
            n = vol[k]
            on = live & (n != 0)
            seen += on
            nd = n.astype(F)
            a = nd / (nd + half)
            w = T * a
            R = np.where(on, R + w * r_k, R)
            G = np.where(on, G + w * g_k, G)
            B = np.where(on, B + w * b_k, B)
            T = np.where(on, T * (F(1.0) - a), T)
            stop = on & (T < F(t_min))
            stopped |= stop
            live &= ~stop
        if transparent:
            cover = F(1.0) - T
            any_ = T < 1.0
            chans = [np.where(any_, X / cover, 0.0) for X in (R, G, B)] + [cover]
        else:
            chans = [X + T * (F(background[c]) / F(65535.0)) for c, X in enumerate((R, G, B))] + [np.ones_like(T)]
        out = np.empty((height, width, 4), dtype=np.uint16)
        for c, X in enumerate(chans):
            X = np.where(X > 0.0, X, 0.0)
            X = np.where(X < 1.0, X, 1.0)
            out[..., c] = as_u16(X * F(65535.0))
    return out, dict(slabs_seen=int(seen.sum()), covered=int((seen > 0).sum()), stopped=int(stopped.sum()))
