"""Shaded rendering (include/sar.h: sar_shade) restated in numpy: the contract of the header, line for line, vectorised over the pixels
with Python loops over the taps. fp64 throughout, one IEEE operation per numpy call (numpy fuses nothing), the sums in the contract's
order. It never calls into the library: tests/test_shade_host.py holds it to properties known independently of it, and
tests/test_gpu_shade.py holds the device to it bit for bit."""
import numpy as np

MAX_RADIUS = 8
MAX_SHININESS_LOG2 = 10

DEFAULTS = dict(
    light=(-0.5, -0.7, 0.6),
    ambient=0.25, diffuse=0.75, specular=0.25,
    shininess_log2=5,
    ao_radius=6, ao_strength=1.0, ao_range=12.0,
    smooth=1, smooth_range=2.0,
    min_count=1,
    background=(0, 0, 0),
)

F = np.float64


def params(**fields):
    """The defaults with the given fields replaced; an unknown field is an error."""
    p = dict(DEFAULTS)
    for k, v in fields.items():
        if k not in p:
            raise AttributeError(k)
        p[k] = v
    return p


def _normalised(v):
    with np.errstate(all="ignore"):
        x, y, z = (F(c) for c in v)
        length = np.sqrt((x * x + y * y) + z * z)
        return np.array([x / length, y / length, z / length], dtype=F), length


def taps(R):
    """The lattice offsets (dx, dy, d2) with 0 < d2 <= R^2 in the contract's order: dy outside, dx inside."""
    return [(dx, dy, dx * dx + dy * dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if 0 < dx * dx + dy * dy <= R * R]


def constants(p, width, scale):
    """The host constants: k, L, H (None when its length is 0), inv_d by d2, N."""
    k = F(width) * F(scale)
    L, _ = _normalised(p["light"])
    H, hlen = _normalised((L[0], L[1], L[2] + F(1.0)))
    R = int(p["ao_radius"])
    with np.errstate(all="ignore"):
        inv_d = {d2: F(1.0) / np.sqrt(F(d2)) for d2 in range(1, R * R + 1)}
    return dict(k=k, L=L, H=None if hlen == 0.0 else H, inv_d=inv_d, N=len(taps(R)))


def _shift(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` outside the image."""
    h, w = a.shape
    out = np.full((h, w), fill, dtype=a.dtype)
    ys, yd = slice(max(dy, 0), h + min(dy, 0)), slice(max(-dy, 0), h + min(-dy, 0))
    xs, xd = slice(max(dx, 0), w + min(dx, 0)), slice(max(-dx, 0), w + min(-dx, 0))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[yd, xd] = a[ys, xs]
    return out


def as_u16(v):
    """Rust `as u16` of an f64: saturating, NaN -> 0."""
    v = np.asarray(v, dtype=F)
    with np.errstate(all="ignore"):
        t = np.where(v == v, v, 0.0)
        t = np.where(t <= 0.0, 0.0, t)
        t = np.where(t >= 65535.0, 65535.0, t)
    return t.astype(np.uint32).astype(np.uint16)


def palette_blend(v, palette):
    """Palette::interpolate as colorize applies it: the clamp, the blend of two rows and the three square roots."""
    pal = np.asarray(palette, dtype=F)
    n_rows = len(pal)
    rows = np.vstack([pal, pal[-1:]])
    with np.errstate(all="ignore"):
        v = np.asarray(v, dtype=F)
        v = np.where(v < 0.0, 0.0, np.where(v >= 1.0, 0.999999, v))
        v = v * F(n_rows)
        fl = np.floor(v)
        n = np.where(fl == fl, fl, 0.0).astype(np.uint32)
        n = np.minimum(n, n_rows - 1)
        t = v - fl
        t1 = F(1.0) - t
        c1, c2 = rows[n], rows[n + 1]
        return [np.sqrt(c2[..., ch] * t + c1[..., ch] * t1) for ch in range(3)]


def surface_mask(count, zbuf, min_count):
    z = np.asarray(zbuf, dtype=np.float32)
    return np.isfinite(z) & (z != np.float32(-1.0)) & (np.asarray(count, dtype=np.uint32) >= np.uint32(min_count))


def smooth(zbuf, surface, k, p):
    """z~ (NaN off the surface) and the mask of the pixels whose window took in more than the centre."""
    z = np.where(surface, np.asarray(zbuf, dtype=np.float32).astype(F), np.nan)
    if not p["smooth"]:
        return z, np.zeros(z.shape, dtype=bool)
    with np.errstate(all="ignore"):
        total = np.zeros(z.shape, dtype=F)
        n = np.zeros(z.shape, dtype=np.uint32)
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                zq = _shift(z, dx, dy, np.nan)
                take = surface & (np.abs(zq - z) * k <= F(p["smooth_range"]))     # (a NaN neighbour fails the compare)
                total = np.where(take, total + zq, total)
                n = n + take.astype(np.uint32)
        zt = np.where(surface, total / n.astype(F), np.nan)
    return zt, surface & (n > 1)


def _gradient(zt, dx, dy):
    """The smaller of the forward and the backward difference along (dx, dy); the one there is; 0 with neither."""
    with np.errstate(all="ignore"):
        ahead, behind = _shift(zt, dx, dy, np.nan), _shift(zt, -dx, -dy, np.nan)
        a, b = ahead - zt, zt - behind
        has_a, has_b = ahead == ahead, behind == behind
        both = np.where(np.abs(a) <= np.abs(b), a, b)
        return np.where(has_a & has_b, both, np.where(has_a, a, np.where(has_b, b, 0.0)))


def normals(zt, k):
    with np.errstate(all="ignore"):
        sx, sy = _gradient(zt, 1, 0) * k, _gradient(zt, 0, 1) * k
        length = np.sqrt((sx * sx + sy * sy) + F(1.0))
        return -sx / length, -sy / length, F(1.0) / length


def occlusion(zt, k, p, c):
    """occ per pixel, in the tap order."""
    occ = np.zeros(zt.shape, dtype=F)
    with np.errstate(all="ignore"):
        for dx, dy, d2 in taps(int(p["ao_radius"])):
            h = (_shift(zt, dx, dy, np.nan) - zt) * k
            t = h * c["inv_d"][d2]
            occ = np.where((h > 0.0) & (h <= F(p["ao_range"])), occ + np.where(t < 1.0, t, 1.0), occ)
    return occ


def shade(count, steps, zbuf, width, scale, palette, transparent, p=None, window=None, detail=False):
    """The RGBA16 image (H, W, 4) and the statistics; with detail=True also the intermediate fields. window: None or a dict
    lo, hi, pos_lo, pos_hi, applied."""
    p = params() if p is None else p
    c = constants(p, width, scale)
    k = c["k"]
    surface = surface_mask(count, zbuf, p["min_count"])
    zt, smoothed = smooth(zbuf, surface, k, p)
    nx, ny, nz = normals(zt, k)
    L, H = c["L"], c["H"]
    with np.errstate(all="ignore"):
        d = (nx * L[0] + ny * L[1]) + nz * L[2]
        d = np.where(d > 0.0, d, 0.0)
        if H is None:
            s = np.zeros(zt.shape, dtype=F)
        else:
            s = (nx * H[0] + ny * H[1]) + nz * H[2]
            s = np.where(s > 0.0, s, 0.0)
            for _ in range(int(p["shininess_log2"])):
                s = s * s
        occ = occlusion(zt, k, p, c)
        if int(p["ao_radius"]) == 0:
            ao = np.ones(zt.shape, dtype=F)
        else:
            ao = F(1.0) - F(p["ao_strength"]) * (occ / F(c["N"]))
            ao = np.where(ao > 0.0, ao, 0.0)
        v = np.asarray(steps, dtype=F)
        if window is not None and window["applied"]:
            span, dpos = F(window["hi"]) - F(window["lo"]), F(window["pos_hi"]) - F(window["pos_lo"])
            v = F(window["pos_lo"]) + ((v - F(window["lo"])) / span) * dpos
        rgb = palette_blend(v, palette)
        lum = ao * (F(p["ambient"]) + F(p["diffuse"]) * d)
        glint = ao * (F(p["specular"]) * s)
        out = np.empty(zt.shape + (4,), dtype=np.uint16)
        for ch in range(3):
            col = rgb[ch] * lum + glint
            col = np.where(col > 0.0, col, 0.0)
            col = np.where(col < 1.0, col, 1.0)
            out[..., ch] = np.where(surface, as_u16(col * F(65535.0)), np.uint16(p["background"][ch]))
        out[..., 3] = np.where(surface, 65535, 0 if transparent else 65535)
    near = np.zeros(zt.shape, dtype=bool)
    for dx, dy in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        near |= _shift(surface, dx, dy, False)
    stats = dict(surface=int(surface.sum()), background=int((~surface).sum()), isolated=int((surface & ~near).sum()),
                 occluded=int((surface & (occ > 0.0)).sum()), smoothed=int(smoothed.sum()))
    if detail:
        return out, stats, dict(surface=surface, zt=zt, normal=(nx, ny, nz), occ=occ, ao=ao, d=d, s=s, constants=c)
    return out, stats
