"""Journeys of ONE long-lived runtime, renderer or frame group through several image sizes, and their references
(tests/test_reuse_cases_host.py holds the conditions they rely on, tests/test_gpu_runtime_reuse.py walks them on the device).

sar_runtime_set_width_height frees six size-dependent buffers and leaves the rest to their owners' next grow(), which only ever
grows: after a shrink, or a change of shape at equal pixel count, the segment flags, the density snapshot, the record arena, the
checkpoints, the warm-up sets, the hints' book-keeping, the survivor share, a pending announcement, the exposure and colour-range
modes, the batch tables, the image tickets and the timing spans are all what the previous size left. A journey is an ordered list of
sizes (and what is done at each); every step that leaves something observable has a reference computed here, once, shared and
read-only:

  render state, merge, colorize   the CPU oracle (oracle_lib) on the same start points, bit for bit
  converted image formats         oracle_lib.convert of the oracle's image
  density                         density_restatement.filter
  shade                           shade_restatement.shade

(The exposure, colour-range and held-window modes are compared on the device with a FRESH runtime of the new size given the same
mode and the oracle's state: tests/test_gpu_exposure.py and tests/test_gpu_color_range.py already hold a fresh runtime to the oracle
with restated constants.)

Sizes, (width, height), the smallest that reach each layout. Narrow (16-bit) depth hints live in 8 x 8 tiles when the width is a
power of two (>= 8) and the height a multiple of eight, row-major otherwise; every size up to 65536 pixels is ONE interleaved bin of
32768 records (sar_bin_geometry), 320 x 200 is two bins dealt in 2048-pixel segments (31.25 of them).

  (256, 64)   tiled narrow hints
  (96, 64)    row-major hints
  (64, 96)    the same 6144 pixels, other shape; tiled (64 is a power of two, 96 a multiple of eight)
  (128, 48)   the same 6144 pixels, a third shape; tiled
  (97, 53)    npix % 4 == 1, ragged everywhere; row-major
  (320, 200)  the largest: two bins, more than one 2048-pixel segment per bin, 1000 exchange granules; row-major
  (1, 1)      the smallest

Jobs are at most 1024, iterations per job at most 300; solar-sail loses 38 % of its jobs in the warm-up and poisson-saturne none,
and the frames alternate between them, so the survivor share that steers the next plan moves from step to step."""
import functools
from collections import namedtuple

import numpy as np

import density_cases as DK
import density_restatement as D
import oracle_lib as O
import shade_cases as SK
import shade_restatement as S

MAX_JOBS, MAX_ITERS = 1024, 300

# (width, height) -> whether the narrow hints are tiled there
SIZES = {(256, 64): True, (96, 64): False, (64, 96): True, (128, 48): True, (97, 53): False, (320, 200): False, (1, 1): False}
EQUAL_NPIX = ((96, 64), (64, 96), (128, 48))
# what sar_bin_geometry answers (default options): (bins, bin_shift, interleaved)
GEOMETRY = {size: ((2, 15, 1) if size == (320, 200) else (1, 15, 1)) for size in SIZES}

# The size orders of a single runtime. Each holds a shrink, a change of shape at equal pixel count, a growth, a shrink to 1 x 1 with the
# growth back, and ends on its first size.
ORDERS = {
    "from_tiled": ((256, 64), (96, 64), (64, 96), (320, 200), (1, 1), (97, 53), (256, 64)),
    "from_row_major": ((96, 64), (128, 48), (320, 200), (97, 53), (1, 1), (128, 48), (96, 64)),
}
# Journeys of three runtimes / one renderer: size A, size B, (and where the journey says so) size A again.
PAIRS = {
    "smaller": ((256, 64), (96, 64)),
    "larger": ((96, 64), (320, 200)),
    "same_npix": ((96, 64), (128, 48)),
}
# density and shade: shrink, shrink to 1 x 1, grow, equal pixel count; (96, 80) and (1, 1) are sizes of density_cases / shade_cases
FILTER_ORDER = ((320, 200), (96, 80), (1, 1), (96, 64), (64, 96), (97, 53))
DENSITY_SAMPLES = (2, 64, 256)
DENSITY_TILES = (8, 16, 32)
SHADE_COMBOS = tuple(dict(ao_radius=R, smooth=sm) for R in (0, 6) for sm in (0, 1))


def npix(size):
    return size[0] * size[1]


def is_tiled(size):
    """The rule of the narrow hints' layout (sar_render.cpp, fill_bin_iter_args), restated."""
    w, h = size
    return w >= 8 and w & (w - 1) == 0 and h % 8 == 0


def transitions(order):
    """The kinds of change between the successive sizes of an order."""
    kinds = set()
    for a, b in zip(order, order[1:]):
        if npix(b) > npix(a):
            kinds.add("grow")
        elif npix(b) < npix(a):
            kinds.add("shrink")
        elif a != b:
            kinds.add("equal_npix")
        if b == (1, 1):
            kinds.add("to_1x1")
        if a == (1, 1):
            kinds.add("from_1x1")
        if is_tiled(a) != is_tiled(b):
            kinds.add("other_hint_layout")
    if len(order) > 2 and order[-1] == order[0]:
        kinds.add("back_to_first")
    return kinds


# ---- rendered frames -------------------------------------------------------------------------------------------------------------
Frame = namedtuple("Frame", "preset width height jobs n seed kind angle transparent")
State = namedtuple("State", "count max zbuf steps")
_SHAPES = ((1024, 300), (640, 257), (1000, 201))       # (jobs, iterations per job): full waves, ragged, an odd iteration count


def frame(size, k, seed=0, kind=0, transparent=0):
    """The k-th frame of a journey at `size`: presets alternate, the job shape rotates, the view turns, the start points are the
    oracle's stream for seed 1000 * seed + k."""
    jobs, n = _SHAPES[k % 3]
    return Frame(("solar_sail", "poisson_saturne")[k % 2], size[0], size[1], jobs, n, 1000 * seed + k, kind, 0.37 * k, transparent)


def config(f: Frame):
    """The oracle's (ctypes) config of a frame; the device takes a copy of the same struct."""
    c = getattr(O, f.preset)()
    c.width, c.height, c.jobs_total, c.iterations = f.width, f.height, f.jobs, f.jobs * f.n
    c.render_kind, c.angle, c.transparent, c.scale, c.seed = f.kind, f.angle, f.transparent, 1.0, f.seed
    return c


@functools.lru_cache(maxsize=None)
def starts(f: Frame) -> np.ndarray:
    s = O.start_points(f.seed, 0, f.jobs)
    s.setflags(write=False)
    return s


def _frozen(ort) -> State:
    out = State(ort.count.copy(), ort.max, ort.zbuf.copy(), ort.steps.copy())
    for a in (out.count, out.zbuf, out.steps):
        a.setflags(write=False)
    return out


def oracle_runtime(state: State):
    h, w = state.count.shape
    ort = O.Runtime(w, h)
    ort.count[:], ort.zbuf[:], ort.steps[:] = state.count, state.zbuf, state.steps
    ort.set_max(state.max)
    return ort


@functools.lru_cache(maxsize=None)
def rendered(*frames) -> State:
    """The frames rendered one after the other into ONE reset oracle runtime (render continues an un-reset runtime)."""
    ort = O.Runtime(frames[0].width, frames[0].height)
    for f in frames:
        O.render_jobs(config(f), ort, starts(f), f.n)
    return _frozen(ort)


def merge_states(into: State, other: State) -> State:
    """Runtime::merge of `other` into `into`, by the oracle."""
    dst, src = oracle_runtime(into), oracle_runtime(other)
    assert O.merge(dst, src) == 0
    return _frozen(dst)


@functools.lru_cache(maxsize=None)
def merged(a: tuple, b: tuple) -> State:
    """Runtime::merge of rendered(*b) into rendered(*a)."""
    return merge_states(rendered(*a), rendered(*b))


@functools.lru_cache(maxsize=None)
def image(state_frames: tuple, view: Frame) -> np.ndarray:
    """colorize of rendered(*state_frames) under the config of `view` (its kind, transparency and colours)."""
    img = O.colorize(config(view), oracle_runtime(rendered(*state_frames)))
    img.setflags(write=False)
    return img


def render_steps(order, seed=0):
    """What the render journey does at the sizes of an order: at each one a frame, a second one without a reset, a reset and a third.
    [(size, (frame, ...) as accumulated since the last reset)] in the order they run."""
    out = []
    for i, size in enumerate(order):
        a, b, c = (frame(size, 3 * i + j, seed) for j in range(3))
        out.append((size, ((a,), (a, b), (c,))))
    return out


def announcement_steps(order):
    """At every size after the first: (the frame announced at the PREVIOUS size, the frame rendered after the resize — the announced
    map, job shape and start points at the new size, so that nothing but the resize stands between the announcement and its call —, the
    frame announced and rendered at the new size)."""
    out = []
    for i in range(1, len(order)):
        announced = frame(order[i - 1], 2 * i, seed=3)
        after = announced._replace(width=order[i][0], height=order[i][1])
        out.append((order[i], announced, after, frame(order[i], 2 * i + 1, seed=3)))
    return out


def all_render_references():
    """Every rendered reference a journey of this module compares with, by what it is for."""
    for name, order in ORDERS.items():
        for size, groups in render_steps(order):
            for g in groups:
                yield f"{name} {size} {[f.seed for f in g]}", rendered(*g)
    for name, order in ORDERS.items():
        for size, _, after, then in announcement_steps(order):
            yield f"{name} {size} announced before the resize", rendered(after)
            yield f"{name} {size} announced after the resize", rendered(then)
    for name in PAIRS:
        for what, groups in list(batch_frames(name).items()) + list(group_frames(name).items()):
            for member, g in enumerate(groups):
                yield f"batch {name} {what} member {member}", rendered(*g)
        for ndev in (1, 3):
            for call, st in enumerate(renderer_references(name, ndev)):
                yield f"renderer {name} x{ndev} call {call}", st


# ---- batches -----------------------------------------------------------------------------------------------------------------------
def batch_frame(size, visit, member):
    """Frame `member` of the `visit`-th set of three frames of a pair journey. One preset, job shape and scale per set — what lets
    frames share a launch —, a view and start points per frame."""
    jobs, n = _SHAPES[visit % 3]
    return Frame(("solar_sail", "poisson_saturne")[visit % 2], size[0], size[1], jobs, n, 5000 + 10 * visit + member, 0,
                 0.21 * member + 0.5 * visit, 0)


def batch_frames(pair_name) -> dict:
    """Three runtimes of their own: a batch at size A, all resized to B and batched again, then a single-frame tail each on the
    un-reset runtimes. name -> per member, the frames accumulated in its runtime when it is compared."""
    a, b = PAIRS[pair_name]
    first = [batch_frame(a, 0, m) for m in range(3)]
    second = [batch_frame(b, 1, m) for m in range(3)]
    tails = [batch_frame(b, 2, m) for m in range(3)]
    return {"first": [(f,) for f in first], "second": [(f,) for f in second], "tails": [(s, t) for s, t in zip(second, tails)]}


def group_frames(pair_name) -> dict:
    """One frame group: a batch at size A, member 1 alone resized to B (the frames can no longer share a launch), member 1 back at A
    and a batch again; a reset before each."""
    a, b = PAIRS[pair_name]
    return {"group together": [(batch_frame(a, 3, m),) for m in range(3)],
            "group apart": [(batch_frame(b if m == 1 else a, 4, m),) for m in range(3)],
            "group again": [(batch_frame(a, 5, m),) for m in range(3)]}


# ---- the multi-device renderer -------------------------------------------------------------------------------------------------
RENDERER = dict(units=96, jobs_per_unit=5, seed=23, iterations=96 * 5 * 250 + 77, preset="solar_sail", kind=1)


def shard_jobs(jobs, world, rank):
    """distributed.shard_jobs restated: contiguous shards, the first jobs % world one longer."""
    base, extra = divmod(jobs, world)
    return rank * base + min(rank, extra), base + (1 if rank < extra else 0)


@functools.lru_cache(maxsize=None)
def renderer_references(pair_name, ndev):
    """The states after the three calls (size A, B, A) of a renderer over `ndev` shards: start points continue across the calls, the
    jobs are sharded like the devices and the shards folded with Runtime::merge in rank order (as tests/test_gpu_dist.py builds it)."""
    a, b = PAIRS[pair_name]
    r = RENDERER
    jobs = r["units"] * r["jobs_per_unit"]
    n = r["iterations"] // jobs
    out = []
    for call, size in enumerate((a, b, a)):
        parts = []
        for rank in range(ndev):
            first, cnt = shard_jobs(jobs, ndev, rank)
            f = Frame(r["preset"], size[0], size[1], cnt, n, r["seed"], r["kind"], 0.0, 0)
            c = config(f)
            c.iterations = r["iterations"]
            ort = O.Runtime(*size)
            O.render_jobs(c, ort, O.start_points(r["seed"], call * jobs + first, cnt), n)
            parts.append(ort)
        for other in parts[1:]:
            assert O.merge(parts[0], other) == 0
        out.append(_frozen(parts[0]))
    return tuple(out)


def renderer_config(size):
    """The oracle config render_parallel is called with at `size` (jobs_total is the renderer's business)."""
    r = RENDERER
    c = config(Frame(r["preset"], size[0], size[1], 1, 1, r["seed"], r["kind"], 0.0, 0))
    c.iterations = r["iterations"]
    return c


# ---- loaded states for density and shade ----------------------------------------------------------------------------------------
Loaded = namedtuple("Loaded", "width height count steps zbuf max")


@functools.lru_cache(maxsize=None)
def density_state(size, samples) -> Loaded:
    """density_cases' sparse random frame where it has the size, the same recipe elsewhere."""
    w, h = size
    if size in DK.SIZES:
        k = DK.case(f"sparse_random-{w}x{h}-S{samples}")
        return Loaded(w, h, k.count, k.steps, k.zbuf, k.max)
    rng = np.random.default_rng([77, w, h, samples])
    count = (rng.integers(0, 2 * samples + 1, size=(h, w)) * (rng.random((h, w)) < 0.30)).astype(np.uint32)
    steps = np.where(count != 0, rng.random((h, w)), 0.0)
    zbuf = np.where(count != 0, rng.random((h, w)) * 2.0 - 0.5, -1.0).astype(np.float32)
    return Loaded(w, h, count, steps, zbuf, int(count.max()))


@functools.lru_cache(maxsize=None)
def density_reference(size, samples):
    """(count, steps, max, stats) of density_restatement.filter on density_state."""
    k = density_state(size, samples)
    c, s, m, st = D.filter(k.count, k.steps, samples)
    c.setflags(write=False)
    s.setflags(write=False)
    return c, s, m, st


@functools.lru_cache(maxsize=None)
def shade_state(size) -> Loaded:
    """shade_cases' random field where it has the size, the same recipe elsewhere."""
    w, h = size
    if size in SK.SIZES:
        k = SK.case(f"random-{w}x{h}-R8-s1")
        return Loaded(w, h, k.count, k.steps, k.zbuf, k.max)
    rng = np.random.default_rng([78, w, h])
    on = rng.random((h, w)) < 0.7
    zbuf = np.where(on, 0.5 + rng.random((h, w)) * 6.0 / (w * SK.SCALE), -1.0).astype(np.float32)
    count = np.where(on, rng.integers(1, 50, size=(h, w)), 0).astype(np.uint32)
    return Loaded(w, h, count, rng.random((h, w)), zbuf, int(count.max()))


def shade_config(size) -> dict:
    return dict(width=size[0], height=size[1], scale=SK.SCALE, transparent=size[0] & 1, palette_rgb=SK.PALETTE)


@functools.lru_cache(maxsize=None)
def shade_reference(size, ao_radius, smooth):
    """(rgba, stats) of shade_restatement.shade on shade_state under shade_config."""
    k, cfg = shade_state(size), shade_config(size)
    rgba, stats = S.shade(k.count, k.steps, k.zbuf, cfg["width"], cfg["scale"], SK.PALETTE, cfg["transparent"],
                          S.params(ao_radius=ao_radius, smooth=smooth))
    rgba.setflags(write=False)
    return rgba, stats
