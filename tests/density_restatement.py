"""Plain numpy restatement of density estimation (include/sar.h: sar_density_*): the weight tables `plan(S)` and the filter
`filter(count, steps, S) -> (count', steps', max', stats)`. The filter loops over the (2R+1)^2 taps, dy outer and dx inner, with
shifted whole-array operations: every pixel sees its sources in the device's order, so the fp64 hue sum has the device's bits.
Integers are uint64 / int64 throughout; the only floating point is t, u, q of a weight and the hue's multiply, add and division."""
import numpy as np

STATS = ("mass_in", "mass_q16", "covered_in", "covered_out", "spread", "saturated", "max_in", "max_out")


def radius(S: int) -> int:
    """floor(sqrt(S - 1)) in integers."""
    r = 0
    while (r + 1) * (r + 1) < S:
        r += 1
    return r


def row(S: int, c: int) -> np.ndarray:
    """Class c's table W_c[0 .. S) as uint32."""
    if c < 1:
        raise ValueError("class 0 has no table")
    out = np.zeros(S, dtype=np.uint32)
    if c >= S:
        out[0] = 65536
        return out
    R = radius(S)
    q = [0] * S
    for d2 in range(S):
        if d2 * c < S:
            t = np.float64(d2 * c) / np.float64(S)
            u = np.float64(1.0) - t
            q[d2] = int(np.floor((u * u) * np.float64(1048576.0)))
    offsets = [(dx, dy) for dy in range(-R, R + 1) for dx in range(-R, R + 1) if (dx * dx + dy * dy) * c < S]
    N = sum(q[dx * dx + dy * dy] for dx, dy in offsets)
    for d2 in range(1, S):
        if d2 * c < S:
            out[d2] = (q[d2] << 16) // N
    out[0] = 65536 - sum(int(out[dx * dx + dy * dy]) for dx, dy in offsets if dx or dy)
    return out


_PLANS: dict = {}


def plan(S: int) -> np.ndarray:
    """[S + 1][S] uint32: row c is class c's table for c = 1 .. S (row S: the identity every class c >= S shares); row 0 is zeros."""
    if S not in _PLANS:
        p = np.zeros((S + 1, S), dtype=np.uint32)
        for c in range(1, S + 1):
            p[c] = row(S, c)
        p.setflags(write=False)
        _PLANS[S] = p
    return _PLANS[S]


def filter(count: np.ndarray, steps: np.ndarray, S: int):
    """(count', steps', max', stats) of one call of the filter on a [height][width] frame."""
    count = np.ascontiguousarray(count, dtype=np.uint32)
    steps = np.ascontiguousarray(steps, dtype=np.float64)
    H, W = count.shape
    R = radius(S)
    table = plan(S).astype(np.uint64)
    cpad = np.zeros((H + 2 * R, W + 2 * R), dtype=np.uint64)   # outside the image: count 0, a source the contract skips
    cpad[R:R + H, R:R + W] = count
    spad = np.zeros((H + 2 * R, W + 2 * R), dtype=np.float64)
    spad[R:R + H, R:R + W] = steps
    cls = np.minimum(cpad, np.uint64(S)).astype(np.intp)
    fin_pad = np.isfinite(spad)
    acc = np.zeros((H, W), dtype=np.uint64)
    den = np.zeros((H, W), dtype=np.uint64)
    num = np.zeros((H, W), dtype=np.float64)
    others = np.zeros((H, W), dtype=bool)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                d2 = dx * dx + dy * dy
                if d2 >= S:             # dead for every class
                    continue
                win = (slice(R + dy, R + dy + H), slice(R + dx, R + dx + W))
                m = table[cls[win], d2] * cpad[win]     # class 0 (an empty source) has the zero row
                acc += m
                use = fin_pad[win] & (m != 0)
                den += np.where(use, m, np.uint64(0))
                num = num + np.where(use, m.astype(np.float64) * np.where(use, spad[win], 0.0), 0.0)
                if d2:
                    others |= use
        rounded = (acc + np.uint64(32768)) >> np.uint64(16)
        sat = rounded > np.uint64(0xFFFFFFFF)
        out_count = np.where(sat, np.uint64(0xFFFFFFFF), rounded).astype(np.uint32)
        out_steps = steps.copy()
        mean = num / den.astype(np.float64)
        out_steps[others] = mean[others]
    stats = {
        "mass_in": int(count.sum(dtype=np.uint64)),
        "mass_q16": int(acc.sum(dtype=np.uint64)),             # (modulo 2^64, as the device's atomics)
        "covered_in": int(np.count_nonzero(count)),
        "covered_out": int(np.count_nonzero(out_count)),
        "spread": int(np.count_nonzero((count != 0) & (count < S))),
        "saturated": int(np.count_nonzero(sat)),
        "max_in": int(count.max()) if count.size else 0,
        "max_out": int(out_count.max()) if count.size else 0,
    }
    return out_count, out_steps, stats["max_out"], stats
