"""GPU: the depth test, its hints and the Depth colorize on the adversarial maps of tests/depth_cases.py — every visit a depth
candidate, depths beyond any range a warm-up measured, exact ties between jobs on every pixel, +-inf, the -1 sentinel, subnormals,
-0.0, frames whose depths are all negative or all equal — reached through render itself, so every state is one the reference
produces, and through every statement of the depth rule: the one-atomic-per-visit kernel, the binned path with both iterate kernels,
both hint types and both 16-bit hint layouts, the checkpoint replay, launch chunks and segments, an announced warm-up, the batched
kernels, the gallery's LDS copy, Runtime::merge and the multi-device exchange folds.

Every test compares with the CPU oracle on the same start points (tests/test_depth_cases_host.py pins that side). The bar: count,
max and steps bit for bit; zbuf bit for bit after `+ 0.0f` on both sides, and the device returns no -0.0 (a
depth that rounds to -0.0f is stored as +0.0f — the one deviation, asserted here rather than hidden); colorize bit for bit for
Depth and for Gas with transparent 0 and 1 (every count + 1 here is <= 2^20: ln comes from the host-libm table)."""
import re

import numpy as np
import pytest

import depth_cases as DC

pytestmark = pytest.mark.gpu

DEPTH, GAS = DC.oracle_lib.SAR_RENDER_DEPTH, DC.oracle_lib.SAR_RENDER_GAS
SIZE_IDS = dict(ids=lambda s: f"{s[0]}x{s[1]}")
ALL_SIZES = pytest.mark.parametrize("size", DC.SIZES, **SIZE_IDS)
ALL_CASES = pytest.mark.parametrize("case", DC.NAMES)
NEG_ZERO = 0x80000000


def _diff(got, want):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return f"{len(bad)} differ, first at {bad[:4].tolist()}: got {[got[tuple(i)].tolist() for i in bad[:4]]}, " \
           f"want {[want[tuple(i)].tolist() for i in bad[:4]]}"


def _assert_buffers(count, mx, zbuf, steps, ref, what):
    assert np.array_equal(count, ref.count), f"{what}: count: {_diff(count, ref.count)}"
    assert mx == ref.max, f"{what}: max {mx} vs {ref.max}"
    assert not (DC.bits(zbuf) == NEG_ZERO).any(), f"{what}: the device returned -0.0 on {int((DC.bits(zbuf) == NEG_ZERO).sum())} pixels"
    z_got, z_want = DC.bits(zbuf + np.float32(0.0)), DC.bits(ref.zbuf + np.float32(0.0))
    assert np.array_equal(z_got, z_want), f"{what}: zbuf: {_diff(z_got, z_want)}"
    assert np.array_equal(DC.bits(steps), DC.bits(ref.steps)), f"{what}: steps: {_diff(DC.bits(steps), DC.bits(ref.steps))}"


def _kinds(cfg):
    return (("Depth", cfg.replace(render_kind=DEPTH), DEPTH, 1), ("Gas opaque", cfg.replace(render_kind=GAS, transparent=0), GAS, 0),
            ("Gas transparent", cfg.replace(render_kind=GAS, transparent=1), GAS, 1))


def _assert_state(sar, cfg, rt, ref, what):
    _assert_buffers(rt.count(), rt.max(), rt.zbuf(), rt.steps(), ref, what)
    for name, c, kind, transparent in _kinds(cfg):
        img, want = sar.colorize(c, rt), ref.image(kind, transparent)
        assert np.array_equal(img, want), f"{what}: {name} image: {_diff(img, want)}"


def _render(sar, cfg, starts, **tuning):
    rt = sar.Runtime(cfg)
    if tuning:
        rt.set_tuning(**tuning)
    sar.render_jobs(cfg, rt, starts)
    return rt


# ---- every render path ------------------------------------------------------------------------------------------------------------
PATHS = {"atomic": dict(variant=1)}
for _waves in (1, 2):
    for _hints in (32, 16):
        PATHS[f"binned-waves{_waves}-hints{_hints}"] = dict(variant=3, split_waves=_waves, hint_bits=_hints)
TILE_PATHS = {f"binned-hints16-tile{t}": dict(variant=3, hint_bits=16, hint_tile=t) for t in (0, 1)}     # 256 x 64 only
PATH_PARAMS = [(s, p) for s in DC.SIZES for p in PATHS] + [(DC.SIZES[1], p) for p in TILE_PATHS]


@pytest.mark.parametrize("size,path", PATH_PARAMS, ids=[f"{s[0]}x{s[1]}-{p}" for s, p in PATH_PARAMS])
@ALL_CASES
def test_every_render_path(sar, oracle, gpu, case, size, path):
    tuning = {**PATHS, **TILE_PATHS}[path]
    DC.check_condition(oracle, case, size)
    cfg = DC.config(sar, case, size)
    rt = _render(sar, cfg, DC.starts(case), **tuning)
    d = rt.describe_last_launch()
    if tuning["variant"] == 1:
        assert "one global atomic per visit" in d, d
    else:
        assert "k_bin_accumulate" in d and ("q16" if tuning["hint_bits"] == 16 else "f32") in d, d
        if "split_waves" in tuning:
            assert ("k_iterate_lean" if tuning["split_waves"] == 1 else "k_iterate_split") in d, d
    _assert_state(sar, cfg, rt, DC.reference(oracle, case, size), f"{case} {path}: {d}")
    rt.close()


@pytest.mark.parametrize("stride", [7, 100000])
@ALL_SIZES
@pytest.mark.parametrize("case", ["rising", "rising_tied"])
def test_checkpoint_replay(sar, oracle, gpu, case, size, stride):
    """Every visit of `rising` wins its pixel for a while: a winner's steps are recomputed from a checkpoint up to `stride` back."""
    cfg = DC.config(sar, case, size)
    for variant in (1, 3):
        rt = _render(sar, cfg, DC.starts(case), variant=variant, checkpoint_stride=stride)
        _assert_state(sar, cfg, rt, DC.reference(oracle, case, size), f"{case} variant {variant} checkpoint_stride {stride}")
        rt.close()


@pytest.mark.parametrize("hint_bits", [32, 16])
@ALL_SIZES
@ALL_CASES
def test_two_calls_into_one_runtime(sar, oracle, gpu, case, size, hint_bits):
    """Jobs 0..159, then 160..319 without a reset: the first call's keys and hints filter the second. Equals the sequential render."""
    cfg, st, n = DC.config(sar, case, size), DC.starts(case), DC.CASES[case]["n"]
    rt = sar.Runtime(cfg)
    rt.set_tuning(variant=3, hint_bits=hint_bits)
    sar.render_job_range(cfg, rt, n, st[:160])
    _assert_buffers(rt.count(), rt.max(), rt.zbuf(), rt.steps(), DC.reference(oracle, case, size, 0, 160), f"{case}: the first call")
    sar.render_job_range(cfg, rt, n, st[160:])
    _assert_state(sar, cfg, rt, DC.reference(oracle, case, size), f"{case}: two calls, hint_bits {hint_bits}")
    rt.close()


@ALL_SIZES
@ALL_CASES
def test_launch_chunks(sar, oracle, gpu, case, size):
    """debug_chunk_jobs 64: five launch chunks, each finding the earlier chunks' keys final and their hints in place."""
    cfg = DC.config(sar, case, size)
    for tuning in (dict(variant=1 | (64 << 8)), dict(variant=3 | (64 << 8), hint_bits=32), dict(variant=3 | (64 << 8), hint_bits=16)):
        rt = _render(sar, cfg, DC.starts(case), **tuning)
        assert "chunks=5 " in rt.describe_last_launch(), rt.describe_last_launch()
        _assert_state(sar, cfg, rt, DC.reference(oracle, case, size), f"{case}: five chunks, {tuning}")
        rt.close()


@ALL_SIZES
@ALL_CASES
def test_segments(sar, oracle, gpu, case, size):
    """16 jobs under debug_max_ordinals 400: a job runs as several launches that hand its state on (previous_point included)."""
    jobs = 16
    cfg = DC.config(sar, case, size, jobs=jobs)
    for variant in (1, 3):
        rt = sar.Runtime(cfg)
        rt.set_tuning(variant=variant)
        rt.set_option("debug_max_ordinals", 400)
        sar.render_jobs(cfg, rt, DC.starts(case)[:jobs])
        d = rt.describe_last_launch()
        assert int(re.search(r"chunks=(\d+)", d).group(1)) >= -(-DC.CASES[case]["n"] // 400), d     # a launch per segment at least
        _assert_state(sar, cfg, rt, DC.reference(oracle, case, size, 0, jobs), f"{case}: segments, variant {variant}")
        rt.close()


@ALL_SIZES
@pytest.mark.parametrize("announced,rendered", [("rising_far", "rising_far"), ("alt_inf", "alt_inf"), ("alt_inf_warm", "alt_inf_warm"),
                                                ("rising", "rising_far")])
def test_announced_warm_up_with_narrow_hints(sar, oracle, gpu, announced, rendered, size):
    """prefetch_device, then render_job_range_device, hint_bits 16: the quantiser's range is what the announced warm-up saw, and the
    frame leaves it — upwards (rising_far), to +-inf (alt_inf), or the range itself has an infinite span (alt_inf_warm). Announced
    under `rising` and rendered as `rising_far` (the same map, another center_camera), every depth is 4 above the measured range."""
    import torch
    st, n = DC.starts(rendered), DC.CASES[rendered]["n"]
    dev = torch.from_numpy(st).cuda()
    torch.cuda.synchronize()
    cfg = DC.config(sar, rendered, size)
    rt = sar.Runtime(cfg)
    rt.set_tuning(variant=3, hint_bits=16)
    sar.prefetch_device(DC.config(sar, announced, size), rt, DC.JOBS, n, dev.data_ptr())
    sar.render_job_range_device(cfg, rt, DC.JOBS, n, dev.data_ptr())
    d = rt.describe_last_launch()
    assert "q16" in d and "warmup_ahead=1" in d, d
    _assert_state(sar, cfg, rt, DC.reference(oracle, rendered, size), f"{rendered} announced as {announced}")
    rt.close()


# ---- the batched kernels --------------------------------------------------------------------------------------------------------------
def _batch(sar, oracle, size, n, hint_bits):
    """The nat-start cases as the frames of one render_jobs_batch on a frame group, held to per-case oracle renders; then the
    group's images through colorize_device_batch."""
    import torch
    cases = DC.NAT
    cfgs = [DC.config(sar, c, size, n=n) for c in cases]           # n None: each case's own
    rts = sar.Runtime.group(cfgs[0], len(cases))
    if hint_bits:
        for rt in rts:
            rt.set_option("hint_bits", hint_bits)
    st = DC.start_set("nat")
    sar.render_jobs_batch(cfgs, rts, [st] * len(cases))
    refs = [DC.reference(oracle, c, size, n=n) for c in cases]
    for c, cfg, rt, ref in zip(cases, cfgs, rts, refs):
        _assert_state(sar, cfg, rt, ref, f"batch, frame {c}, n {n}, hint_bits {hint_bits}")
    w, h = size
    outs = [torch.zeros(w * h * 4, dtype=torch.int16, device="cuda") for _ in cases]
    torch.cuda.synchronize()
    for name, _, kind, transparent in _kinds(cfgs[0]):
        sar.colorize_device_batch([c.replace(render_kind=kind, transparent=transparent) for c in cfgs], rts, [o.data_ptr() for o in outs])
        rts[0].synchronize()
        for c, o, ref in zip(cases, outs, refs):
            img = o.cpu().numpy().view(np.uint16).reshape(h, w, 4)
            assert np.array_equal(img, ref.image(kind, transparent)), f"batched colorize, frame {c}, {name}: {_diff(img, ref.image(kind, transparent))}"
    d = rts[0].describe_last_launch()
    for rt in reversed(rts):
        rt.close()
    return d


@pytest.mark.parametrize("hint_bits", [0, 16])
@ALL_SIZES
def test_batch_of_the_cases_as_they_are(sar, oracle, gpu, size, hint_bits):
    """One call for the nine cases, each with its own iteration count (frames of different lengths do not share launches: the call
    renders them one after the other on the group's one stream)."""
    _batch(sar, oracle, size, None, hint_bits)


@pytest.mark.parametrize("hint_bits", [0, 16])
@ALL_SIZES
@pytest.mark.parametrize("n", sorted({DC.CASES[c]["n"] for c in DC.NAT}))
def test_batch_in_one_set_of_launches(sar, oracle, gpu, n, size, hint_bits):
    """The nine maps at ONE iteration count — each case's own in turn — so that the frames do share the batched kernels."""
    d = _batch(sar, oracle, size, n, hint_bits)
    assert f"batch of {len(DC.NAT)} frames" in d and (hint_bits != 16 or "q16" in d), d


# ---- the gallery's copy of the depth rule (in LDS) ----------------------------------------------------------------------------------------
GALLERY_RUNS = [("nat", 1500), ("tied", 1500), ("sentinel", 400), ("nat", 1200), ("nat", 900), ("nat", 600)]


@pytest.mark.parametrize("start_name,n", GALLERY_RUNS, ids=[f"{s}-{n}" for s, n in GALLERY_RUNS])
def test_gallery_tiles(sar, oracle, gpu, start_name, n):
    """All cases as 96 x 64 tiles of one atlas, under each start set (at its cases' iteration count) and under the plain stream at
    every other count a case has: each tile's count / max / zbuf / steps and its image under base.render_kind Gas and Depth."""
    size = DC.SIZES[0]
    st = DC.start_set(start_name)
    coeffs = np.stack([np.concatenate([DC.HENON_X, DC.HENON_Y, DC.coeff_z(c)]) for c in DC.NAMES])
    views = [((0.0, DC.CASES[c]["cy"], 0.0), DC.SCALE) for c in DC.NAMES]
    rt = sar.Runtime(DC.config(sar, "rising", size))
    for kind in (GAS, DEPTH):
        base = DC.config(sar, "rising", size, render_kind=kind)
        g = sar.gallery(rt, base, sar.gallery_items(coeffs, views, base=base), tile=size, cols=4, jobs=DC.JOBS, iterations=DC.JOBS * n,
                        starts=st, raw=True)
        for i, c in enumerate(DC.NAMES):
            ref = DC.reference(oracle, c, size, start_name=start_name, n=n)
            what = f"gallery tile {c}, starts {start_name}, n {n}, kind {kind}"
            _assert_buffers(g.count[i], int(g.stats["max"][i]), g.zbuf[i], g.steps[i], ref, what)
            assert np.array_equal(g.tile(i), ref.image(kind)), f"{what}: image: {_diff(g.tile(i), ref.image(kind))}"
    rt.close()


# ---- Runtime::merge and the multi-device exchange -----------------------------------------------------------------------------------------
def _part(sar, cfg, case, lo, hi):
    rt = sar.Runtime(cfg)
    sar.render_job_range(cfg, rt, DC.CASES[case]["n"], DC.starts(case)[lo:hi])
    return rt


def _merged_reference(oracle, case, size, cuts):
    parts = [DC.oracle_runtime(oracle, case, size, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for other in parts[1:]:
        assert oracle.merge(parts[0], other) == 0
    return DC.freeze(oracle, case, size, parts[0])


@pytest.mark.parametrize("cuts", [(0, 160, 320), (0, 107, 214, 320)], ids=["halves", "thirds"])
@ALL_SIZES
@ALL_CASES
def test_merge(sar, oracle, gpu, case, size, cuts):
    """Runtime.merge of part renders, folded in job order, against oracle.merge of the same parts."""
    cfg = DC.config(sar, case, size)
    ref = _merged_reference(oracle, case, size, cuts)
    whole = DC.reference(oracle, case, size)        # (contiguous slices folded in order are the sequential render: the oracle's own check)
    assert np.array_equal(DC.bits(ref.steps), DC.bits(whole.steps)) and np.array_equal(DC.bits(ref.zbuf), DC.bits(whole.zbuf))
    rts = [_part(sar, cfg, case, lo, hi) for lo, hi in zip(cuts[:-1], cuts[1:])]
    for other in rts[1:]:
        rts[0].merge(other)
    _assert_state(sar, cfg, rts[0], ref, f"{case}: merge of {len(rts)} parts")
    for rt in rts:
        rt.close()


@pytest.mark.parametrize("mode", [1, 2], ids=["dense", "sparse"])
@ALL_SIZES
@pytest.mark.parametrize("case", DC.NAT)
def test_multi_device_renderer(sar, oracle, gpu, case, size, mode):
    """Three shards on one device, 64 units x 5 jobs: the stream of seed 7, the exchange folds in rank order — dense and sparse."""
    ref = DC.reference(oracle, case, size)
    for name, cfg, kind, transparent in _kinds(DC.config(sar, case, size))[::2]:
        r = sar.ParallelRenderer(devices=[0, 0, 0], units=64, seed=DC.SEED)
        r.set_exchange(mode)
        img = sar.render_parallel(r, cfg, 5)
        assert np.array_equal(img, ref.image(kind, transparent)), f"{case} exchange {mode}: {name} image: {_diff(img, ref.image(kind, transparent))}"
        rm = r.runtime()
        _assert_buffers(rm.count(), rm.max(), rm.zbuf(), rm.steps(), ref, f"{case} exchange {mode}, after the {name} frame")
        r.shutdown()


def test_export_of_a_depth_image(sar, oracle, gpu):
    """colorize_format to RGB8 of falling_sentinel's Depth image: every depth negative, the range folded from the 0.0 seed."""
    case, size = "falling_sentinel", DC.SIZES[0]
    cfg = DC.config(sar, case, size, render_kind=DEPTH)
    rt = _render(sar, cfg, DC.starts(case))
    ref = DC.reference(oracle, case, size)
    fmt = sar.image_format(False, True)
    assert fmt == sar._abi.SAR_FMT_RGB8
    got = sar.colorize_format(cfg, rt, fmt)
    assert got.shape == (size[1], size[0], 3) and got.dtype == np.uint8 and 0 < got.max() < 255
    assert np.array_equal(got, oracle.convert(fmt, ref.depth))
    rt.close()
