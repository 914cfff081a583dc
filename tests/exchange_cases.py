"""What the exchange-case tests share (tests/test_exchange_cases_host.py, tests/test_gpu_exchange_cases.py): the exchange context
(sar_exchange_*: flags -> plan -> pack -> merge -> finish, and the rooted form) driven for all ranks inside ONE process, the
collectives done by hand with numpy, on partial states where the ORDER of the fold shows — the depth cases of tests/depth_cases.py
cut over the ranks (exact ties on every pixel, +-inf, the -1 sentinel on visited pixels, frames of negative or equal depths), ranks
that rendered nothing, ranks that touch different granules, and counts whose sum passes 2^32 inside the fold.

ONE driver (`run`) serves the three forms — `dense` (pack without flags), `sparse` (dense_above 2.0, or the threshold given) and
`rooted` — over objects with the methods of api.Exchange and a small memory object: DeviceMemory with api.Exchange on the GPU,
HostMemory with the numpy stand-in of tests/exchange_numpy.py on the CPU. The reference is always oracle.merge folded in rank order
over oracle runtimes that hold the same partial states.

Every partial state is reached by render_job_range on a depth case (`Spec`: the case, the size and every rank's job range); the
wrapped rows (`Plant`) then change ONE pixel's count per rank and `max`, nothing else."""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import depth_cases as DC
from exchange_numpy import unsortable

SEG, RECORD = 64, 64 * 16
FORMS = ("dense", "sparse", "rooted")
SLICED = ("dense", "sparse")
U32 = 0xFFFFFFFF

# ---- the partial states ------------------------------------------------------------------------------------------------------------
# parts: every rank's job range [lo, hi) of the case's start set, lo == hi: the rank renders nothing (a fresh runtime); n: iterations
# per job (None: the case's own)
Spec = namedtuple("Spec", "case size parts n")

CUTS = {"thirds": (0, 107, 214, 320), "halves": (0, 160, 320)}
EMPTY = {"first": ((0, 0), (0, 160), (160, 320)), "middle": ((0, 160), (160, 160), (160, 320)), "last": ((0, 160), (160, 320), (320, 320))}
# few short jobs: the ranks touch DIFFERENT granules. Granules by presence pattern (bit r: rank r touches it), patterns 0..7, as
# measured on the oracle when the cases were made (the (x, y) carrier is the same for every case):
#   SCATTER[3]  96 x 64: 67, 1, 3, 2, 1, 6, 4, 12      256 x 64: 192, 14, 17, 3, 9, 8, 6, 7
# SCATTER[5] at 96 x 64: ranks 3 and 4 own no slice. SCATTER[2] and [4] carry the wrapped rows of two and four ranks.
SCATTER = {2: ((0, 4, 8), 10), 3: ((0, 4, 8, 12), 10), 4: ((0, 4, 8, 12, 16), 10), 5: ((0, 2, 4, 6, 8, 10), 12)}
EDGE_CASES = ("rising", "alt_inf", "falling_sentinel")     # the cases `empty` and `scatter` run over


def cuts_spec(case, size, cuts) -> Spec:
    return Spec(case, tuple(size), tuple(zip(cuts[:-1], cuts[1:])), None)


def empty_spec(case, size, where) -> Spec:
    return Spec(case, tuple(size), EMPTY[where], None)


def scatter_spec(case, size, world) -> Spec:
    jobs, n = SCATTER[world]
    return Spec(case, tuple(size), tuple(zip(jobs[:-1], jobs[1:])), n)


def iterations(spec) -> int:
    return DC.CASES[spec.case]["n"] if spec.n is None else spec.n


# ---- the wrapped rows ---------------------------------------------------------------------------------------------------------------
# Per-rank counts of ONE pixel; every u32 is a count a render reaches (tests/test_gpu_tail.py: test_one_pixel_past_u32).
#   fold_max: what Runtime::merge's running max holds after the fold (rank 0's own max, then every intermediate sum, :721-723) — the
#   other pixels' counts are tiny beside it; rooted_exact: max(rank 0's max, the final sums) — all an unordered SUM can know — is the same.
Row = namedtuple("Row", "counts fold_max rooted_exact what")
ROWS = {
    "wrap_at_1": Row((0xFFFFFFF0, 0x20, 5), 0xFFFFFFF0, True, "the sum wraps at rank 1: only rank 0's own max holds the largest value"),
    "peak_at_1": Row((5, 0xFFFFFFF0, 0x20), 0xFFFFFFF5, False, "0xFFFFFFF5 exists only as the intermediate sum after rank 1"),
    "wrap_to_0": Row((0x80000000, 0x80000000, 0), 0x80000000, True, "the sum wraps to exactly 0; rank 2 adds nothing"),
    "rank0_absent": Row((0, 0xFFFFFFFF, 1), 0xFFFFFFFF, False, "rank 0 holds nothing; u32::MAX after rank 1, 0 after rank 2"),
    "rank0_alone": Row((0xFFFFFFFF, 0, 0), 0xFFFFFFFF, True, "only rank 0 holds a count: u32::MAX, added to twice"),
    "four_ranks": Row((1, 0xFFFFFFFE, 1, 0xFFFFFFFF), 0xFFFFFFFF, True, "u32::MAX after rank 1, 0 after rank 2, u32::MAX again at the end"),
    # the same at two ranks, where the rooted form has nothing to lose: one add, and the final sum is the only intermediate one
    "two_wrap": Row((0xFFFFFFF0, 0x20), 0xFFFFFFF0, True, "two ranks, the sum wraps"),
    "two_peak": Row((5, 0xFFFFFFF0), 0xFFFFFFF5, True, "two ranks, the sum is the peak"),
    "two_to_0": Row((0x80000000, 0x80000000), 0x80000000, True, "two ranks, the sum wraps to 0"),
    "two_absent": Row((0, 0xFFFFFFFF), 0xFFFFFFFF, True, "two ranks, rank 0 holds nothing"),
    "two_alone": Row((0xFFFFFFFF, 0), 0xFFFFFFFF, True, "two ranks, rank 1 holds nothing"),
}
SITES = ("common", "untouched")   # a pixel of a granule every rank touches / of one nobody touched (the planted counts alone decide who sends)
# liar: rank 1 is loaded with max = u32::MAX and no such count — the fold never looks at a later rank's max (:716-724)
Plant = namedtuple("Plant", "row site liar", defaults=(False,))


def prefix_sums(counts) -> list:
    """The sums the fold walks through, rank by rank (wrapping u32, :719)."""
    out, c = [], 0
    for r, v in enumerate(counts):
        c = (c + v) & U32 if r else v
        out.append(c)
    return out


# ---- the oracle's side ---------------------------------------------------------------------------------------------------------------
Partial = namedtuple("Partial", "count zbuf steps max")
_PARTIAL, _FOLD = {}, {}


def partial(oracle, spec, r) -> Partial:
    """Rank r's partial state of `spec` on the oracle, once per module run; read-only."""
    lo, hi = spec.parts[r]
    key = (spec.case, spec.size, lo if hi > lo else 0, hi if hi > lo else 0, iterations(spec))
    if key not in _PARTIAL:
        ort = DC.oracle_runtime(oracle, spec.case, spec.size, lo, hi, n=iterations(spec)) if hi > lo else oracle.Runtime(*spec.size)
        p = Partial(ort.count.copy(), ort.zbuf.copy(), ort.steps.copy(), ort.max)
        for a in p[:3]:
            a.setflags(write=False)
        _PARTIAL[key] = p
    return _PARTIAL[key]


def touched(p: Partial) -> np.ndarray:
    """The granule flags of a partial state: a granule is touched when any of its pixels has a count or a depth."""
    npix = p.count.size
    t = np.zeros(-(-npix // SEG) * SEG, bool)
    t[:npix] = (p.count.ravel() != 0) | (p.zbuf.ravel() != np.float32(-1.0))
    return t.reshape(-1, SEG).any(axis=1)


def presence(oracle, spec) -> np.ndarray:
    """Per granule, the ranks that touch it as a bit mask (bit r: rank r)."""
    return sum((touched(partial(oracle, spec, r)).astype(np.int64) << r) for r in range(len(spec.parts)))


def site_pixel(oracle, spec, site) -> int:
    """Where a row is planted: lane 5 of the first granule every rank touches / of the last granule nobody touched."""
    pat = presence(oracle, spec)
    if site == "common":
        g = np.nonzero(pat == (1 << len(spec.parts)) - 1)[0][0]
    else:
        assert site == "untouched", site
        g = np.nonzero(pat == 0)[0][-1]
    return int(g) * SEG + 5


def planted(oracle, spec, plant) -> list:
    """Every rank's (count, max) under `plant` — or as rendered when plant is None."""
    parts = [partial(oracle, spec, r) for r in range(len(spec.parts))]
    if plant is None:
        return [(p.count, p.max) for p in parts]
    row = ROWS[plant.row]
    assert len(row.counts) == len(parts), (plant, len(parts))
    px, out = site_pixel(oracle, spec, plant.site), []
    for r, p in enumerate(parts):
        c = p.count.copy()
        c.flat[px] = row.counts[r]
        out.append((c, U32 if plant.liar and r == 1 else int(c.max())))      # max: that of the rank's own counts
    return out


def oracle_parts(oracle, spec, plant=None) -> list:
    """Fresh oracle runtimes holding every rank's partial state (the caller may merge into them)."""
    out = []
    for r, (c, mx) in enumerate(planted(oracle, spec, plant)):
        p, ort = partial(oracle, spec, r), oracle.Runtime(*spec.size)
        ort.count[:], ort.zbuf[:], ort.steps[:] = c, p.zbuf, p.steps
        ort.set_max(mx)
        out.append(ort)
    return out


def fold(oracle, spec, plant=None) -> DC.State:
    """Runtime::merge folded in rank order over the partial states (:1068-1076), frozen; once per module run."""
    key = (spec, plant)
    if key not in _FOLD:
        parts = oracle_parts(oracle, spec, plant)
        for other in parts[1:]:
            assert oracle.merge(parts[0], other) == 0
        _FOLD[key] = DC.freeze(oracle, spec.case, spec.size, parts[0])
    return _FOLD[key]


def rooted_max(oracle, spec, plant=None) -> int:
    """What the rooted form states for `max` (api.Exchange.rooted): max(rank 0's max, the final sums)."""
    return max(planted(oracle, spec, plant)[0][1], int(fold(oracle, spec, plant).count.max()))


# ---- memory: the buffers of the collectives ----------------------------------------------------------------------------------------------
class HostMemory:
    """Host buffers for the numpy stand-in (exchange_numpy.NumpyExchange over a NumpyRuntime); `api`: its NumpyApi."""

    def __init__(self, api):
        self.api = api

    def zeros(self, nbytes):
        return np.zeros(max(int(nbytes), 8), np.uint8)

    def upload(self, a):
        b = self.zeros(a.nbytes)
        b[:a.nbytes] = np.ascontiguousarray(a).view(np.uint8).ravel()
        return b

    def ptr(self, b) -> int:
        return b.ctypes.data

    def download(self, b, dtype=np.uint8):
        return b.view(dtype).copy()

    def sync(self, ex):
        pass

    def frame(self, ex):
        rt = ex.runtime
        return rt.count.copy(), unsortable(rt.z).copy(), rt.steps.copy(), (U32 if rt.wrap else int(rt.max))

    def colorize(self, cfg, ex, first, n, b):
        self.api.colorize_range_device(cfg, ex.runtime, first, n, self.ptr(b))


class DeviceMemory:
    """Device buffers (torch) for api.Exchange. Buffers are made on torch's stream and used on the runtimes': both are waited for."""

    def __init__(self, sar):
        import torch
        self.sar, self.torch = sar, torch

    def zeros(self, nbytes):
        b = self.torch.zeros(max(int(nbytes), 8), dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()
        return b

    def upload(self, a):
        h = np.zeros(max(a.nbytes, 8), np.uint8)
        h[:a.nbytes] = np.ascontiguousarray(a).view(np.uint8).ravel()
        b = self.torch.from_numpy(h).cuda()
        self.torch.cuda.synchronize()
        return b

    def ptr(self, b) -> int:
        return b.data_ptr()

    def download(self, b, dtype=np.uint8):
        return b.cpu().numpy().view(dtype)

    def sync(self, ex):
        ex.runtime.synchronize()

    def frame(self, ex):
        rt = ex.runtime
        return rt.count().ravel(), rt.zbuf().ravel(), rt.steps().ravel(), rt.max()

    def colorize(self, cfg, ex, first, n, b):
        self.sar.colorize_range_device(cfg, ex.runtime, first, n, self.ptr(b))


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------
class Result:
    """What an exchange left: the frame put together from every owner's slice (flat count / zbuf / steps), the max every rank reports
    (rooted: the root's alone), the images asked for (H x W x 4, one per config), and — sliced forms — the form pack chose, the split
    sizes (send_bytes[r][d], recv_bytes[d][r]) and the gathered flags (world x granules; None without flags)."""

    def __init__(self):
        self.count, self.zbuf, self.steps, self.maxes, self.images = None, None, None, [], []
        self.sparse, self.send_bytes, self.recv_bytes, self.flags = None, [], [], None


PAD = 0xA5    # what a receive buffer holds behind the bytes that arrived: nothing may read it


def run(mem, exs, form, dense_above=2.0, colorize=(), dims=None) -> Result:
    """Drives the exchange contexts `exs` (rank order; all of one world) through one exchange of `form`. `colorize`: configs whose
    image is put together from colorize_range_device of every owner's slice after finish (sliced forms; `dims` = (W, H))."""
    assert form in FORMS, form
    world = len(exs)
    assert [e.rank for e in exs] == list(range(world)) and all(e.world == world for e in exs)
    npix = sum(e.count for e in exs)
    res = Result()
    if form == "rooted":
        return _run_rooted(mem, exs, npix, res)
    nseg, blk = exs[0].granules, exs[0].block_bytes
    assert nseg == -(-npix // SEG) and blk == world * exs[0].slice_pixels * 16 and exs[0].slice_pixels % SEG == 0
    flags_all = None
    if form == "sparse":
        bufs = [mem.zeros(nseg) for _ in exs]
        for e, b in zip(exs, bufs):
            e.flags(mem.ptr(b))
            mem.sync(e)
        res.flags = np.stack([mem.download(b)[:nseg] for b in bufs])                 # the all-gather
        assert set(np.unique(res.flags)) <= {0, 1}
        flags_all = [mem.upload(res.flags) for _ in exs]                             # (every rank holds its own copy)
    send, forms = [], []
    for r, e in enumerate(exs):
        b = mem.zeros(blk)
        sparse, sb, rb = e.pack(mem.ptr(flags_all[r]) if flags_all else None, dense_above, mem.ptr(b))
        mem.sync(e)
        assert len(sb) == len(rb) == world and sum(sb) <= blk and sum(rb) <= blk, (r, sb, rb)
        send.append(mem.download(b)); res.send_bytes.append(list(sb)); res.recv_bytes.append(list(rb)); forms.append(bool(sparse))
    assert len(set(forms)) == 1, forms                                                # every rank decides alike
    res.sparse = forms[0]
    for r in range(world):
        for d in range(world):
            assert res.send_bytes[r][d] == res.recv_bytes[d][r], (r, d, res.send_bytes[r][d], res.recv_bytes[d][r])
    scalars = []
    for d, e in enumerate(exs):                                                       # the all-to-all: owner d receives, source by source
        recv = np.full(blk, PAD, np.uint8)
        at = 0
        for r in range(world):
            off, n = sum(res.send_bytes[r][:d]), res.send_bytes[r][d]
            recv[at:at + n] = send[r][off:off + n]
            at += n
        rbuf, s4 = mem.upload(recv), mem.zeros(32)
        e.merge(mem.ptr(rbuf), mem.ptr(s4))
        mem.sync(e)
        scalars.append(mem.download(s4, np.int64)[:4])
    red = np.max(np.stack(scalars), axis=0)                                           # the all-reduce MAX of the four scalars
    res.count, res.zbuf, res.steps = np.zeros(npix, np.uint32), np.zeros(npix, np.float32), np.zeros(npix, np.float64)
    for e in exs:
        rbuf = mem.upload(red)
        e.finish(mem.ptr(rbuf))
        mem.sync(e)
        c, z, st, mx = mem.frame(e)
        f, n = e.first, e.count
        res.count[f:f + n], res.zbuf[f:f + n], res.steps[f:f + n] = c[f:f + n], z[f:f + n], st[f:f + n]
        res.maxes.append(mx)
    for cfg in colorize:
        img = np.zeros((npix, 4), np.uint16)
        for e in exs:
            if e.count:
                out = mem.zeros(e.count * 8)
                mem.colorize(cfg, e, e.first, e.count, out)
                mem.sync(e)
                img[e.first:e.first + e.count] = mem.download(out, np.uint16)[:e.count * 4].reshape(-1, 4)
        res.images.append(img.reshape(dims[1], dims[0], 4))
    return res


def _run_rooted(mem, exs, npix, res):
    keys = [mem.zeros(npix * 8) for _ in exs]
    for e, k in zip(exs, keys):
        e.rooted(0, mem.ptr(k))
        mem.sync(e)
    red = np.max(np.stack([mem.download(k, np.int64)[:npix] for k in keys]), axis=0)   # the all-reduce: elementwise MAX of the keys
    sums = []
    for e in exs:
        k, s = mem.upload(red), mem.zeros(3 * npix * 4)
        e.rooted(1, mem.ptr(k), mem.ptr(s))
        mem.sync(e)
        sums.append(mem.download(s, np.uint32)[:3 * npix])
    total = np.stack(sums).sum(axis=0, dtype=np.uint32)                                # the reduce: int32 SUM, wrapping
    k, s = mem.upload(red), mem.upload(total)
    exs[0].rooted(2, mem.ptr(k), mem.ptr(s))
    mem.sync(exs[0])
    c, z, st, mx = mem.frame(exs[0])
    res.count, res.zbuf, res.steps, res.maxes, res.images = c.copy(), z.copy(), st.copy(), [mx], []
    assert res.count.size == npix
    return res


# ---- the comparisons ---------------------------------------------------------------------------------------------------------------------
NEG_ZERO = 0x80000000


def diff(got, want) -> str:
    got, want = np.asarray(got), np.asarray(want)
    bad = np.argwhere(got != want)
    return f"{len(bad)} differ, first at {bad[:4].tolist()}: got {[got[tuple(i)].tolist() for i in bad[:4]]}, " \
           f"want {[want[tuple(i)].tolist() for i in bad[:4]]}"


def assert_frame(res, ref, what):
    """count, zbuf (after + 0.0f, and no -0.0 returned: DESIGN.md section 4) and steps against the fold, bit for bit."""
    assert np.array_equal(res.count, ref.count.ravel()), f"{what}: count: {diff(res.count, ref.count.ravel())}"
    assert not (DC.bits(res.zbuf) == NEG_ZERO).any(), f"{what}: -0.0 returned on {int((DC.bits(res.zbuf) == NEG_ZERO).sum())} pixels"
    z_got, z_want = DC.bits(res.zbuf + np.float32(0.0)), DC.bits(ref.zbuf.ravel() + np.float32(0.0))
    assert np.array_equal(z_got, z_want), f"{what}: zbuf: {diff(z_got, z_want)}"
    s_got, s_want = DC.bits(res.steps), DC.bits(ref.steps.ravel())
    assert np.array_equal(s_got, s_want), f"{what}: steps: {diff(s_got, s_want)}"


def assert_max(res, want, what):
    assert all(m == want for m in res.maxes), f"{what}: max {[hex(m) for m in res.maxes]} vs {hex(want)}"


def assert_plan(res, slice_pixels, what):
    """The split sizes are the flags' own counts: rank r sends owner d one record per granule of d's slice that r touched."""
    world, sps = len(res.send_bytes), slice_pixels // SEG
    padded = np.zeros((world, world * sps), bool)
    padded[:, :res.flags.shape[1]] = res.flags != 0
    for r in range(world):
        own = [int(padded[r, d * sps:(d + 1) * sps].sum()) * RECORD for d in range(world)]
        assert res.send_bytes[r] == own, f"{what}: rank {r} sends {res.send_bytes[r]}, its flags say {own}"
