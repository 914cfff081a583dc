"""GPU: k_iterate_split with ONE iteration per barrier phase (PH = 1) — the form the launchers pick where the LDS staging leaves
1 KiB for the visits in flight between the producer and the consumer wave: 256 .. 270 bins with 64-byte chunks, 132 .. 139 with
128-byte ones (tests/split_phase_cases.py has the table, tests/test_split_phases_host.py holds it to the restated rules). That form
has code of its own — 64-entry hand-over halves, a consumer trip of two one-visit phases with the register copy at the back edge,
its own meeting with the n % 2 tail and with DepthPipe's park windows — and is what every image the default geometry puts into 256
bins runs (above 8.39 Mpx, up to 4096 x 4096). Here every PH = 1 instantiation runs on the smallest images that reach those bin
counts: both chunk sizes x both hint types x the four park windows, and the batched kernel's four; the shapes on either side of
both edges of both windows; the depth cases of tests/depth_cases.py; every way a job is cut; and the one shape the product plans
into that form with no test option at all.

Every render asserts — with no skip — on what the launch says of itself (sar_runtime_describe_last_launch: kernel, R=, bins=, hint
type, park=, and phase=, which is the launcher's own report of the instantiation it picked) and is held to the CPU oracle bit for
bit on count, max, zbuf and steps; zbuf after `+ 0.0f` on both sides for the depth cases only, which reach -0.0 (DESIGN.md
section 4). An oracle state is computed once and shared by the parameters that need it; the states of 1024 x 1024 pixels and more
are kept a few at a time (the parameter lists run the users of one state one after the other)."""
import math
from collections import OrderedDict

import numpy as np
import pytest

import depth_cases as DC
import split_phase_cases as SP
from strange_attractor_renderer_amd.sequence import frame_seed

pytestmark = pytest.mark.gpu

HINTS = (16, 32)
WINDOWS = (0, 2, 4, 8)
_REF, _KEEP = OrderedDict(), 6


def _ref(key, make):
    """The state under `key`, made once; the last _KEEP states are kept (16 bytes per pixel each)."""
    if key not in _REF:
        _REF[key] = make()
        while len(_REF) > _KEEP:
            _REF.popitem(last=False)
    _REF.move_to_end(key)
    return _REF[key]


def _frozen(ort):
    return ort.count.copy(), ort.max, ort.zbuf.copy(), ort.steps.copy()


def _oracle_state(oracle, cfg, starts, n):
    ort = oracle.Runtime(cfg.c.width, cfg.c.height)
    oracle.render_jobs(cfg.c, ort, starts, n)
    return _frozen(ort)


def _state(rt):
    return rt.count(), rt.max(), rt.zbuf(), rt.steps()


def _assert_same(got, want, what, fold_neg_zero=False):
    assert np.array_equal(got[0], want[0]), f"{what}: count differs on {int((got[0] != want[0]).sum())} pixels"
    assert got[1] == want[1], f"{what}: max {got[1]} vs {want[1]}"
    z_got, z_want = (got[2] + np.float32(0.0), want[2] + np.float32(0.0)) if fold_neg_zero else (got[2], want[2])
    assert np.array_equal(DC.bits(z_got), DC.bits(z_want)), f"{what}: zbuf differs on {int((DC.bits(z_got) != DC.bits(z_want)).sum())} pixels"
    assert np.array_equal(DC.bits(got[3]), DC.bits(want[3])), f"{what}: steps differs on {int((DC.bits(got[3]) != DC.bits(want[3])).sum())} pixels"


def _assert_described(d, name, hint_bits, park):
    for field in SP.description_fields(name, hint_bits, park):
        assert field in d, f"{name}: {field!r} is not in {d!r}"


def _runtime(sar, name, cfg, hint_bits=None, park=None, **tuning):
    """A fresh runtime on shape `name`: the geometry fixed by the test options, wave pairs asked for."""
    rt = sar.Runtime(cfg)
    rt.set_tuning(**{**SP.tuning(name), **tuning})
    if hint_bits is not None:
        rt.set_option("hint_bits", hint_bits)
    if park is not None:
        rt.set_option("depth_park", park)
    return rt


def _render(sar, name, cfg, starts, hint_bits=None, park=None, **tuning):
    """One render call on a fresh runtime; the runtime and its description, asserted against the table."""
    rt = _runtime(sar, name, cfg, hint_bits, park, **tuning)
    sar.render_jobs(cfg, rt, starts)
    d = rt.describe_last_launch()
    _assert_described(d, name, hint_bits or SP.auto_hint_bits(cfg.c.width, cfg.c.height, cfg.c.scale), SP.DEFAULT_PARK if park is None else park)
    return rt, d


def _saturne(sar, name, jobs=SP.JOBS, n=SP.N):
    w, h = SP.SHAPES[name]["size"]
    return sar.Config.poisson_saturne(iterations=jobs * n, width=w, height=h, jobs_total=jobs)


def _saturne_ref(sar, oracle, name, jobs=SP.JOBS):
    """The oracle's state of the first `jobs` jobs of the saturne frame on shape `name`."""
    cfg = _saturne(sar, name, jobs)
    return _ref(("saturne", name, jobs), lambda: _oracle_state(oracle, cfg, SP.saturne_starts(sar.start_points)[:jobs], SP.N))


# ---- a. every single-frame instantiation ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,hint_bits", [(s, b) for s in SP.PHASE1 + SP.PHASE2 for b in HINTS], ids=lambda v: str(v))
def test_every_park_window_of_every_instantiation(sar, oracle, gpu, name, hint_bits):
    """2 112 jobs x 1 201 iterations of poisson-saturne (an odd count: a job ends on half a pass of the depth pipeline; 512
    near-identical trajectories overflow staging buffers within one slot request), park windows 0 / 2 / 4 / 8: on r28_first and
    r60_mid these are the sixteen PH = 1 instantiations of k_iterate_split, on r28_last2 and r60_last2 — one bin and four bins
    fewer — the PH = 2 ones through the same code otherwise. All equal the oracle, the parked forms window 0 byte for byte."""
    cfg = _saturne(sar, name)
    st = SP.saturne_starts(sar.start_points)
    want = _saturne_ref(sar, oracle, name)
    assert int(want[0].sum(dtype=np.uint64)) > SP.JOBS * SP.N // 2, "most iterations were meant to land inside the image"
    got = {}
    for park in WINDOWS:
        rt, d = _render(sar, name, cfg, st, hint_bits, park)
        got[park] = _state(rt)
        _assert_same(got[park], want, f"{name} hint_bits {hint_bits} window {park} vs the oracle ({d})")
        rt.close()
    for park in WINDOWS[1:]:
        _assert_same(got[park], got[0], f"{name} hint_bits {hint_bits}: window {park} vs window 0")


# ---- b. the depth cases ---------------------------------------------------------------------------------------------------------------
DEPTH_SIZES = {SP.SHAPES[name]["size"]: name for name in SP.PHASE1}      # 1024 x 1024: R = 28, 1024 x 544: R = 60


def _depth_ref(oracle, case, size, n):
    """The oracle's state of the case at `size` with `n` iterations per job (None: the case's own, after its condition was checked
    on that very state)."""
    def make():
        if n is None:
            DC.check_condition(oracle, case, size)
            ref = DC.reference(oracle, case, size)
            state = ref.count, ref.max, ref.zbuf, ref.steps
            SP.forget_depth_references(DC, case, size)
            return state
        return _frozen(DC.oracle_runtime(oracle, case, size, n=n))
    return _ref(("depth", case, size, n), make)


def _depth_case(sar, oracle, case, size, n, hint_bits, park):
    want = _depth_ref(oracle, case, size, n)
    rt, d = _render(sar, DEPTH_SIZES[size], DC.config(sar, case, size, n=n), DC.starts(case), hint_bits, park)
    _assert_same(_state(rt), want, f"{case} {size} n={n} hint_bits {hint_bits} window {park} ({d})", fold_neg_zero=True)
    rt.close()


ALL_DEPTH = [(c, s, b) for c in DC.NAMES for s in DEPTH_SIZES for b in HINTS]


@pytest.mark.parametrize("case,size,hint_bits", ALL_DEPTH, ids=[f"{c}-{s[0]}x{s[1]}-hints{b}" for c, s, b in ALL_DEPTH])
def test_depth_cases(sar, oracle, gpu, case, size, hint_bits):
    """All eleven cases — every visit a winner, ties on every pixel, +-inf, the sentinel, subnormals, -0.0, NaN after the warm-up —
    at both sizes, both hint types, the product's park window."""
    _depth_case(sar, oracle, case, size, None, hint_bits, 8)


# One pixel wins again and again, or ties: a lane passes stage 1 while it still holds a parked visit and the wave flushes early;
# overflow_mid lands on pixel (0, 0) while visits are parked. n = 37 is odd and no multiple of the window, 5 = two trips and the
# tail, 2 = one trip and no tail, 1 = the tail alone: the drain finds parked visits and an unfinished window.
REPEATED = [(c, s, n, b) for c in ("rising", "rising_tied", "const_pos", "overflow_mid") for s in DEPTH_SIZES for n in (None, 37, 5, 2, 1)
            for b in HINTS]


@pytest.mark.parametrize("case,size,n,hint_bits", REPEATED, ids=[f"{c}-{s[0]}x{s[1]}-n-{n or 'own'}-hints{b}" for c, s, n, b in REPEATED])
def test_repeated_winners_in_a_short_window(sar, oracle, gpu, case, size, n, hint_bits):
    _depth_case(sar, oracle, case, size, n, hint_bits, 2)


# ---- c. the edges of both windows ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SP.NAMES)
def test_window_edges(sar, oracle, gpu, name):
    """Every row of the table, asked for as wave pairs with hints and park window left to the plan: it runs what the table says —
    the two rows one bin beyond the window say k_iterate_lean (phase=0, park=0) — and equals the oracle."""
    cfg = _saturne(sar, name)
    rt, d = _render(sar, name, cfg, SP.saturne_starts(sar.start_points))
    assert ("k_iterate_lean" in d) == name.endswith("_lean"), d
    _assert_same(_state(rt), _saturne_ref(sar, oracle, name), f"{name} ({d})")
    rt.close()


# ---- d. how a job is cut ----------------------------------------------------------------------------------------------------------------
SEGMENT_JOBS = 24        # "debug_max_ordinals" also caps a launch chunk at max_ordinals / segment length jobs: one job per launch here
CUTS = ("checkpoints", "launch-chunks", "two-calls", "segments")


@pytest.mark.parametrize("hint_bits", HINTS)
@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("name", SP.PHASE1)
def test_how_a_job_is_cut(sar, oracle, gpu, name, cut, hint_bits):
    """checkpoints: a stride of 100 iterations, thirteen checkpoints per job (a winner's steps are replayed from the last one);
    segments: "debug_max_ordinals" 401 — a job of 1 201 iterations runs as launches of 401, 401 and 399 that hand its state on, each
    with a tail of its own; launch-chunks: at most 512 jobs per launch, five chunks, the next chunk's warm-up run ahead; two-calls:
    jobs 0 .. 1 055, then the rest, into one un-reset runtime. Each equals the single call's state and the oracle."""
    jobs = SEGMENT_JOBS if cut == "segments" else SP.JOBS
    cfg = _saturne(sar, name, jobs)
    st = SP.saturne_starts(sar.start_points)[:jobs]
    want = _saturne_ref(sar, oracle, name, jobs)

    def single():
        rt, _ = _render(sar, name, cfg, st, hint_bits)
        state = _state(rt)
        rt.close()
        return state
    one = _ref(("single call", name, jobs, hint_bits), single)
    if cut == "checkpoints":
        rt, d = _render(sar, name, cfg, st, hint_bits, checkpoint_stride=100)
    elif cut == "segments":
        rt = _runtime(sar, name, cfg, hint_bits)
        rt.set_option("debug_max_ordinals", 401)
        sar.render_jobs(cfg, rt, st)
        d = rt.describe_last_launch()
        assert f"chunks={3 * jobs} " in d, d
    elif cut == "launch-chunks":
        rt, d = _render(sar, name, cfg, st, hint_bits, variant=3 | (512 << 8))
        assert "chunks=5 " in d, d
    else:
        half = jobs // 2
        rt = _runtime(sar, name, cfg, hint_bits)
        sar.render_job_range(cfg, rt, SP.N, st[:half])
        sar.render_job_range(cfg, rt, SP.N, st[half:])
        d = rt.describe_last_launch()
    _assert_described(d, name, hint_bits, SP.DEFAULT_PARK)
    got = _state(rt)
    _assert_same(got, one, f"{name} {cut} hint_bits {hint_bits} vs the single call ({d})")
    _assert_same(got, want, f"{name} {cut} hint_bits {hint_bits} vs the oracle ({d})")
    rt.close()


# ---- e. batches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hint_bits", HINTS)
@pytest.mark.parametrize("F", [2, 3])
@pytest.mark.parametrize("name", SP.PHASE1)
def test_batches(sar, oracle, gpu, name, F, hint_bits):
    """sar_render_jobs_batch with two (8 / F XCDs per frame) and three frames (eight runs of wave pairs) of solar-sail under F view
    angles, 1 024 jobs x 301 iterations, ~38 % of the jobs lost in the warm-up, every runtime of the group under the same options:
    the four PH = 1 instantiations of k_iterate_split_batch. Bins of 4096 pixels do share a batched launch (what the product plans
    for these bin counts, bins of 65536 pixels, does not: tests/test_gpu_batch.py has that fall-back). Every frame equals its own
    single-frame render — which parks, the batch does not — and the oracle."""
    jobs, n = 1024, 301
    w, h = SP.SHAPES[name]["size"]
    cfgs, starts = [], []
    for k in range(F):
        cfgs.append(sar.Config.solar_sail(iterations=jobs * n, width=w, height=h, jobs_total=jobs, render_kind=sar.SAR_RENDER_DEPTH, scale=1.0,
                                          angle=k * math.pi / 180.0 * 7.0, seed=11))
        starts.append(sar.start_points(frame_seed(11, k), 0, jobs))
    rts = sar.Runtime.group(cfgs[0], F)
    for rt in rts:
        rt.set_tuning(**SP.tuning(name))
        rt.set_option("hint_bits", hint_bits)
    sar.render_jobs_batch(cfgs, rts, starts)
    for rt in rts:
        d = rt.describe_last_launch()
        assert f"batch of {F} frames" in d, d
        _assert_described(d, name, hint_bits, 0)
    for i, (cfg, rt, st) in enumerate(zip(cfgs, rts, starts)):
        got = _state(rt)
        one, d1 = _render(sar, name, cfg, st, hint_bits)
        assert "batch" not in d1, d1
        _assert_same(got, _state(one), f"{name} hint_bits {hint_bits}: frame {i} of {F} vs its own render call")
        one.close()
        want = _ref(("batch frame", name, i), lambda: _oracle_state(oracle, cfg, st, n))
        assert i or want[0][0, 0] > 100 * n, "expected many divergent jobs in this sample"
        _assert_same(got, want, f"{name} hint_bits {hint_bits}: frame {i} of {F} vs the oracle")
    for rt in reversed(rts):
        rt.close()


# ---- f. as the product plans it -----------------------------------------------------------------------------------------------------------
PRODUCT_SCALE = 0.5      # (4096 * 0.5)^2 <= 11e6: the plan picks f32 hints by itself (at scale 1 it picks the 16-bit ones)


@pytest.mark.parametrize("hint_bits", [16, 32, None], ids=["hints16", "hints32", "hints-unset"])
def test_as_the_product_plans_it(sar, oracle, gpu, hint_bits):
    """4096 x 2049 with NO test option: 2 048 jobs x 301 iterations of poisson-saturne. The plan itself picks wave pairs, 28 records,
    256 interleaved bins of 65536 pixels, park window 8 — and so one iteration per phase — with the stable option "hint_bits" 16, 32
    and unset (f32 by the plan's own rule at this scale). The one large-image test of this file."""
    jobs, n = 2048, 301
    w, h = SP.PRODUCT["size"]
    assert SP.auto_hint_bits(w, h, PRODUCT_SCALE) == 32
    cfg = sar.Config.poisson_saturne(iterations=jobs * n, width=w, height=h, jobs_total=jobs, scale=PRODUCT_SCALE, seed=7)
    st = sar.start_points(7, 0, jobs)
    want = _ref("product", lambda: _oracle_state(oracle, cfg, st, n))
    assert int(want[0].sum(dtype=np.uint64)) > jobs * n // 2, "most iterations were meant to land inside the image"
    rt = sar.Runtime(cfg)
    if hint_bits is not None:
        rt.set_option("hint_bits", hint_bits)
    sar.render_jobs(cfg, rt, st)
    d = rt.describe_last_launch()
    for field in ("k_iterate_split ", " R=28 ", " bins=256x65536px ", " interleaved ", f" hints={'q16' if hint_bits == 16 else 'f32'}", " park=8 ",
                  " phase=1 ", "counters=u16-packed", "chunks=1 "):
        assert field in d, f"{field!r} is not in {d!r}"
    _assert_same(_state(rt), want, f"4096 x 2049, hint_bits {hint_bits} ({d})")
    rt.close()
