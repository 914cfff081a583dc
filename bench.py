#!/usr/bin/env python3
"""bench.py — attractor iterations/second of the MI355X iterate/accumulate path.

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c4] [--full]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...
(`python bench.py --gpus N` alone spawns the N ranks itself through torch.distributed.run.)

A "step" is one whole frame on every GPU: reset the runtime (as every render_parallel frame does, reference
src/lib.rs:950-951), iterate/accumulate this rank's trajectories (start points resident in HBM), then — for N>1 —
the one exchange step (all-to-all of the image slices, merge in rank order, 4-scalar all-reduce) and the colorize
(sharded for N>1, RGBA16 gathered on rank 0) to an RGBA16 image in device memory.

  --config c2 (default)  BASELINE.json configs[1]: poisson-saturne, 1e9 iterations PER GPU, 2048x2048. WEAK scaling:
                         every GPU renders its own 1e9 iterations of an (N x 1e9)-iteration frame.
  --config c4            BASELINE.json configs[3]: poisson-saturne, 1e10 iterations, 4096x4096, jobs_total = 1 048 576
                         sharded over the ranks (shard_jobs). STRONG scaling: the frame is the same at every N; at
                         N=1 the one GPU runs all the jobs in launch chunks.

A plain run does what its headline figure needs and no more: set-up, the warm-up and timed steps, --dump-outputs, the line.
Everything reported NEXT to the headline runs only with --full; the timed steps are the same either way:

    --full               at N = 1 the PMC child passes behind roofline.traffic, the CPU baseline, the sustained and two-stream
                         loops; the frame checksums against tests/golden (`parity`, also under --native and --config c5); at N > 1
                         the merged-count `check` and, without --config, strong_c4 / strong_c2 / native (below); under --config c5
                         the sweep to RGBA16 in HBM and the cold sweeps

With --full, N > 1 and no --config the ONE command answers both scaling questions: `value` is the weak-scaling c2 line; then rank 0
alone renders the two strong-scaling frames whole (the N = 1 denominators, from THIS node), the same ranks render the c4 frame
(strong scaling: `strong_c4`, with `n1_same_node` / `speedup_same_node`) and the configs[1] frame cut over the ranks (`strong_c2`:
1e9 iterations IN TOTAL, the metric's literal reading), and rank 0 drives the same two
workloads through the C-ABI-only multi-device renderer (sar_renderer_new_multi: host threads + hipMemcpyPeerAsync, no
torch.distributed) — reported under `native`.

    python bench.py --native --gpus N [--config c2|c4]   only the C-ABI multi-device renderer, one process

    --dump-outputs DIR   after the timed steps, write what the last timed step computed as DIR/<name>.npy (see dump_outputs)

One JSON line on rank 0; see DESIGN.md "Measurement" for how each field is derived. This file holds the timed loops and the
line; what is reported NEXT to them (PMC child passes, CPU baseline, frame checksums against tests/golden, the sustained and
two-stream loops, the `sequence` sweep, the C-ABI-only renderer) lives in tools/bench_extras.py and is imported on demand.

With --full the line proves itself: `parity` holds the FNV-1a checksums of the frame's count / zbuf / steps / RGBA16 against
the committed golden of the same frame (tests/golden/fullsize_checksums.json: configs[1] at N = 1, configs[3] — the same frame
at every N — under `strong_c4`) and an N > 1 run checks merged count == sum of the ranks' counts. Every run's `run` records the
world size torch.distributed really saw, the backend and every rank's PCI device.
"""

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tools"))

WIDTH = HEIGHT = 2048
ITERS_PER_GPU = 1_000_000_000
DEFAULT_JOBS = 131072            # trajectories per GPU (2 waves per SIMD on 256 CUs); n = floor(1e9 / jobs)
# BASELINE configs[3]. SURVEY 8d sketched 524 288 jobs (65 536 per GPU at 8 GPUs) — but 65 536 trajectories are one per lane
# of the chip and no more, and the iterate kernel wants two per lane to hide its latencies (4096^2, 1.25e9 iterations: 14.2 ms
# with 65 536 jobs, 11.9 ms with 131 072). A strong-scaling frame must be the same frame at every N, so it is cut into 1 048 576 jobs (131 072 per GPU
# at 8): n = 9536 iterations per job. `--jobs 524288` reproduces SURVEY's split.
C4_SIZE, C4_ITERS, C4_JOBS = 4096, 10_000_000_000, 1048576
ALG_BYTES_PER_ITER = 12.0 + 12.0 * 0.0055   # count RMW 8 B + zbuf read 4 B + win-rate * 12 B
HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: 8.0 TB/s spec
FP64_OPS_PER_ITER = 88           # unfused fp64 ops per counted iteration; FMA is not allowed
FP64_PEAK_OPS = 78.6e12 / 2      # MI355X vector fp64 78.6 TFLOP/s counts an FMA as 2 -> 39.3e12 unfused op/s
DUMP_PIXELS, DUMP_SEED = 1 << 20, 20240928   # --dump-outputs: a fixed, seeded sample of the image's pixels (all of a smaller image)
K = {"WIDTH": WIDTH, "HEIGHT": HEIGHT, "ITERS_PER_GPU": ITERS_PER_GPU, "DEFAULT_JOBS": DEFAULT_JOBS, "C4_SIZE": C4_SIZE,
     "C4_ITERS": C4_ITERS, "C4_JOBS": C4_JOBS}


def dump_outputs(out_dir, np, rgba_dev, npix, rt=None):
    """--dump-outputs: the frame of the last timed step as float32 / float64 .npy files (44 MiB at most), so that two builds can
    be compared output for output. At DUMP_PIXELS pixels drawn with a fixed seed (pixel_index.npy, ascending): rgba16.npy, the
    RGBA16 image the caller receives ([pixels, 4], u16 samples); with `rt` (N = 1) also the runtime's count / zbuf / steps
    buffers there and max.npy, the frame's max count."""
    os.makedirs(out_dir, exist_ok=True)
    if npix <= DUMP_PIXELS:
        idx = np.arange(npix)
    else:
        idx = np.sort(np.random.default_rng(DUMP_SEED).choice(npix, DUMP_PIXELS, replace=False))
    arrays = {"pixel_index": idx.astype(np.float64),
              "rgba16": rgba_dev.cpu().numpy().view(np.uint16).reshape(npix, 4)[idx].astype(np.float32)}
    if rt is not None:
        arrays["count"] = rt.count().ravel()[idx].astype(np.float64)
        arrays["zbuf"] = rt.zbuf().ravel()[idx].astype(np.float32)
        arrays["steps"] = rt.steps().ravel()[idx].astype(np.float64)
        arrays["max"] = np.array([rt.max()], dtype=np.float64)
    for name, arr in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), arr)
    return sorted(arrays)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--jobs", type=int, default=None, help=f"trajectories per GPU (c2: {DEFAULT_JOBS}; c4: the frame's total, {C4_JOBS}; c5: per frame, 65536)")
    ap.add_argument("--iters", type=float, default=ITERS_PER_GPU, help="counted iterations per GPU per step")
    ap.add_argument("--cpu-seconds", type=float, default=20.0)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend for N>1 (nccl == RCCL; gloo only "
                    "to exercise the multi-rank path on a box with fewer GPUs than ranks)")
    ap.add_argument("--no-check", dest="check", action="store_false", help="--full, N>1: skip the (untimed) check that the merged count buffer "
                    "equals the sum of the per-rank buffers")
    ap.add_argument("--no-parity", dest="parity", action="store_false", help="--full: skip the (untimed) frame checksums against tests/golden")
    ap.add_argument("--host-starts", action="store_true", help="hand the start points over from host memory every step "
                    "(PCIe-inclusive rate; the default keeps them resident in HBM)")
    ap.add_argument("--lanes", type=int, default=0, help="--config c5: groups of runtimes (streams) per GPU the batches are rendered on in turn "
                    "(0: one for the read-back sweep, two for the sweep that leaves the frames in HBM)")
    ap.add_argument("--batch", type=int, default=0, help="--config c5: frames per set of launches (sar_render_jobs_batch); 0 = the "
                    "library's advice (a multiple of eight, at most --max-batch), 1 = a frame per launch")
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--rt-opt", action="append", default=[], help="--config c5: name=value runtime option (sar_runtime_set_option) of every runtime (A/B)")
    ap.add_argument("--cold-frames", type=int, default=360, help="--config c5 --full: frames of the COLD sweep (BASELINE configs[4] as stated: 360, "
                    "360 / N per GPU; wall time from the construction of the renderer to the last delivered frame); 0 = skip")
    ap.add_argument("--c5-only", default=None, choices=["readback", "hbm"], help="--config c5: only one of the two sweeps (profiling)")
    ap.add_argument("--config", default=None, choices=["c2", "c4", "c5"], help="c2: BASELINE configs[1], weak scaling (default); "
                    "c4: BASELINE configs[3] (1e10 iterations, 4096^2, 1048576 jobs sharded over the ranks), strong scaling. "
                    "c5: BASELINE configs[4], the solar-sail `sequence` sweep, 1e8 iterations per frame at 1800x2000, frame k on "
                    "rank k mod N, --steps frames per rank, no collective (replicas only). "
                    "With N > 1 and no --config: c2 as `value`, then c4 under `strong_c4` and both through the C ABI under `native`")
    ap.add_argument("--native", action="store_true", help="only the C-ABI multi-device renderer (sar_renderer_new_multi) over "
                    "--gpus devices in ONE process (device ordinals wrap around on a box with fewer GPUs)")
    ap.add_argument("--extras-seconds", type=float, default=240.0, help="--full, N > 1 without --config: time the strong_c4 + native "
                    "extras may take before the line is printed without them")
    ap.add_argument("--sustained-seconds", type=float, default=3.0, help="--full, N=1: length of the extra sustained-rate loop (0 = skip)")
    ap.add_argument("--exchange", default="sliced", choices=["sliced", "rooted"], help="N>1: all-to-all of image slices + "
                    "sharded colorize (default) or all-reduce MAX + reduce SUM onto rank 0")
    ap.add_argument("--no-prefetch", dest="prefetch", action="store_false", help="do not announce the next frame "
                    "(sar_runtime_prefetch_device): every frame runs its warm-up inside its own render call")
    ap.add_argument("--no-traffic", dest="traffic", action="store_false", help="--full: skip the two rocprofv3 --pmc child passes that measure "
                    "roofline.traffic (the child passes themselves run with it)")
    ap.add_argument("--no-pipeline", dest="pipeline", action="store_false", help="--full: skip the two-stream pipelined-throughput "
                    "measurement that is reported next to `value` at N=1")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the last one computed "
                    "(RGBA16 image; at N = 1 also count / zbuf / steps) at a fixed sample of pixels as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--full", action="store_true", help="also run what is reported next to the headline figure: PMC passes, CPU "
                    "baseline, sustained and two-stream loops, frame checksums, the N > 1 check and extras, the other c5 sweeps")
    ap.add_argument("--variant", type=lambda s: int(s, 0), default=0)
    ap.add_argument("--block", type=int, default=0)
    ap.add_argument("--stride", type=int, default=0)
    a = ap.parse_args()
    if a.dump_outputs and (a.native or a.config == "c5"):
        ap.error("--dump-outputs covers the c2 / c4 timed path, not --native or --config c5")
    jobs_given = a.jobs is not None
    a.jobs = a.jobs if jobs_given else DEFAULT_JOBS
    both_curves = a.config is None and not a.native and a.full  # N > 1 and nothing else said but --full
    a.config = a.config or "c2"
    if a.config == "c5" and a.c5_only is None and not a.full:
        a.c5_only = "readback"   # the sweep behind `value`; the one to RGBA16 in HBM and the cold sweeps are --full's

    if a.native:
        import torch
        import bench_extras as X
        import strange_attractor_renderer_amd as S
        ndev = max(S.device_count(), 1)
        res = X.native_measure(S, torch, [k % ndev for k in range(a.gpus)], a.config, a.steps, a.warmup, K, with_parity=a.full)
        res.update({"metric": "attractor iterations/sec through sar_render_parallel (C ABI, multi-device)", "n_gpus": a.gpus,
                    "physical_gpus": ndev, "higher_is_better": True, "dtype": "f64", "data": "synthetic", "vs_baseline": None,
                    "config": {"workload": f"BASELINE configs[{1 if a.config == 'c2' else 3}] through sar_renderer_new_multi"}})
        print(json.dumps(res), flush=True)
        return

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        # plain `python bench.py --gpus N`: become the launcher of N ranks (one process per GPU) and relay their output
        import socket
        import subprocess
        sock = socket.socket()
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
        sock.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
        raise SystemExit(subprocess.run(cmd).returncode)

    import numpy as np
    import torch
    import strange_attractor_renderer_amd as S
    from strange_attractor_renderer_amd.distributed import SlicedExchange, exchange_merge, shard_jobs

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    a.gpus = world
    if not torch.cuda.is_available() or S.device_count() <= 0:
        raise SystemExit("bench.py needs an MI355X: no HIP device visible and there is no CPU fallback")
    ndev = max(torch.cuda.device_count(), 1)
    if world > ndev and a.backend == "nccl":
        # more ranks than GPUs (a 1-GPU box exercising the N-rank path): RCCL refuses two ranks on one device
        a.backend = "gloo"
    local_rank %= ndev
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if a.backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(a.backend, rank=rank, world_size=world)

    # who really runs this: the world torch.distributed saw, the backend, every rank's physical device
    import ctypes as C
    pci = C.create_string_buffer(64)
    S.load_library().sar_device_pci_bus_id(local_rank, pci, 64)
    mine = {"rank": rank, "device": local_rank, "pci": pci.value.decode()}
    ranks = [mine]
    if world > 1:
        ranks = [None] * world
        dist.all_gather_object(ranks, mine)
    run_record = {"world_size_seen": dist.get_world_size() if world > 1 else 1, "world_size_env": world,
                  "backend": (a.backend + (" (RCCL)" if a.backend == "nccl" else "")) if world > 1 else None,
                  "devices": [r["pci"] for r in ranks], "distinct_devices": len({r["pci"] for r in ranks}),
                  "library_build_id": S.load_library().sar_build_id().decode()}

    if a.config == "c5":
        import bench_extras as X
        out = X.run_c5(a, S, torch, dist, world, rank, local_rank, jobs_given)
        if rank == 0:
            out["run"] = run_record
            print(json.dumps(out), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return

    def run_config(config, steps, warmup, extras):
        result = None
        if config == "c4":
            # STRONG scaling: the frame (1e10 iterations, 1 048 576 jobs, 4096^2) is the same at every N; rank r renders the
            # contiguous job slice shard_jobs gives it (src/lib.rs:1056-1062 split)
            width = height = C4_SIZE
            total_jobs = a.jobs if jobs_given else C4_JOBS
            n = int(a.iters if a.iters != ITERS_PER_GPU else C4_ITERS) // total_jobs
            first_job, jobs = shard_jobs(total_jobs, world, rank)
        elif config == "c2s":
            # the metric's LITERAL reading at N > 1: BASELINE configs[1] — 1e9 iterations in TOTAL, 2048^2, the 131 072 jobs of the
            # N = 1 frame — cut over the ranks. Strong scaling of a 5.8 ms frame: SURVEY 7-2 predicts it poor (16 384 jobs are one wave
            # pair per CU at 8 GPUs, the warm-up and the exchange do not shrink); reported because it is the number the metric names
            width = height = WIDTH
            total_jobs = DEFAULT_JOBS
            n = ITERS_PER_GPU // total_jobs
            first_job, jobs = shard_jobs(total_jobs, world, rank)
        else:
            # WEAK scaling: world*jobs trajectories of n iterations; this rank owns jobs [rank*jobs, (rank+1)*jobs)
            width = height = WIDTH
            jobs = a.jobs
            n = int(a.iters) // jobs
            total_jobs = jobs * world
            first_job = rank * jobs
        cfg = S.Config.poisson_saturne(iterations=n * total_jobs, width=width, height=height,
                                       jobs_total=total_jobs, transparent=0, seed=1)
        starts = S.start_points(1, first_job, jobs)
        tuning = dict(block_threads=a.block, checkpoint_stride=a.stride, variant=a.variant)
        check_note, parity = None, None

        stream = torch.cuda.Stream()
        with torch.cuda.stream(stream):
            rt = S.Runtime(cfg, device=local_rank)
            rt.set_stream(stream.cuda_stream)
            rt.enable_timing(True)
            rt.set_tuning(**tuning)
            npix = width * height
            rgba = torch.empty(npix * 4, dtype=torch.int16, device="cuda")
            ex = None
            if world > 1 and a.exchange == "sliced":
                ex = SlicedExchange(S, cfg, rt, rank, world, "cuda")
            elif world > 1:
                key = torch.empty(npix, dtype=torch.int64, device="cuda")
                sums = torch.empty(3 * npix, dtype=torch.int32, device="cuda")
                rooted = S.Exchange(rt, world, rank)
            # per timed step: start / render end / exchange end / colorize end (read after the closing fence, never inside the region)
            evs = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(max(steps, warmup, 1))] if world > 1 else []
            phase_ms = [0.0, 0.0, 0.0]
            step_no = [0]

            # the inputs of the path — the start points of this rank's trajectories — are resident in HBM before the
            # timed region starts (with host start points each frame uploads 3 MiB: +0.1 ms)
            starts_dev = torch.from_numpy(np.ascontiguousarray(starts)).cuda()

            def merge_ranks(rt_, ex_):
                if ex_ is not None:
                    # Runtime::merge folded in rank order, sliced: all-to-all of the image slices (16 B/px), the owner
                    # folds its slice, 4 scalars all-reduced (every rank then colorizes its slice, RGBA16 gathered on rank 0)
                    ex_.merge(dist)
                else:
                    # rooted: depth keys -> all-reduce MAX; counts + winner's steps -> reduce SUM; rank 0 colorizes
                    exchange_merge(rooted, dist, key, sums, dst=0)

            def step(more=True):
                if world > 1:
                    ev = evs[step_no[0] % len(evs)]
                    step_no[0] += 1
                    ev[3].record()
                rt.reset()
                if a.host_starts:
                    S.render_job_range(cfg, rt, n, starts)
                else:
                    S.render_job_range_device(cfg, rt, jobs, n, starts_dev.data_ptr())
                    # the frame loop knows its next frame (src/bin/main.rs:493-517): announce it, so that its 1000 uncounted
                    # warm-up iterations per job run under THIS frame's accumulate / fold / colorize. Every frame still does
                    # all of its work inside the timed region; the last one announces nothing.
                    if a.prefetch and more:
                        S.prefetch_device(cfg, rt, jobs, n, starts_dev.data_ptr())
                if world > 1:
                    ev[0].record()
                    merge_ranks(rt, ex)
                    ev[1].record()
                    if ex is not None:
                        ex.colorize(dist, dst=0)
                    elif rank == 0:
                        S.colorize_device(cfg, rt, rgba.data_ptr())
                    ev[2].record()
                else:
                    S.colorize_device(cfg, rt, rgba.data_ptr())

            def fence():
                if world > 1:
                    dist.barrier()
                torch.cuda.synchronize()

            for k in range(warmup):
                step(more=k + 1 < warmup)  # the last untimed frame announces nothing: no work of the timed region runs before it
            fence()
            if world > 1 and a.full and a.check:
                # each rank's own (un-merged) count summed over ranks must equal the merged count (untimed, --full)
                def reduce_sum(a_np):  # int64 SUM onto rank 0, through whatever the backend can move
                    t = torch.from_numpy(np.ascontiguousarray(a_np))
                    t = t.cuda() if a.backend == "nccl" else t
                    dist.reduce(t, dst=0, op=dist.ReduceOp.SUM)
                    return t.cpu().numpy()

                rt.reset()
                S.render_job_range(cfg, rt, n, starts)
                own = reduce_sum(rt.count().ravel().astype(np.int64))
                merge_ranks(rt, ex)
                torch.cuda.synchronize()
                if ex is not None:
                    mine_ = np.zeros(npix, np.int64)  # every rank holds the merged frame inside its own slice: assemble them
                    mine_[ex.first:ex.first + ex.count] = rt.count().ravel()[ex.first:ex.first + ex.count]
                    merged = reduce_sum(mine_)
                else:
                    merged = rt.count().ravel().astype(np.int64)
                if rank == 0:
                    ok = bool(np.array_equal(merged, own % (1 << 32))) and int(merged.sum()) == n * total_jobs
                    check_note = {"merged_count_equals_sum_of_rank_counts": ok, "iterations_in_the_merged_frame": int(merged.sum()),
                                  "expected": n * total_jobs}
                    print(f"[check] merged count over {world} ranks == sum of per-rank counts == {n * total_jobs}: {ok}", file=sys.stderr)
                fence()
            # HIP events around every launch of the timed region, recorded on the launch stream by the library and
            # summed until they are read after the closing fence (reading them synchronises, so not inside the region)
            rt.set_option("timing_accumulate", 1)
            t0 = time.perf_counter()
            step_no[0] = 0
            for k in range(steps):
                step(more=k + 1 < steps)
            fence()
            elapsed = time.perf_counter() - t0
            dumped = None
            if extras and a.dump_outputs and rank == 0:   # (before anything below renders into the runtime again)
                dumped = dump_outputs(a.dump_outputs, np, ex.rgba[:npix * 8].view(torch.int16) if ex is not None else rgba, npix,
                                      rt if world == 1 else None)
            for ev in evs[:steps]:
                phase_ms[0] += ev[3].elapsed_time(ev[0])
                phase_ms[1] += ev[0].elapsed_time(ev[1])
                phase_ms[2] += ev[1].elapsed_time(ev[2])
            tm = rt.last_timing()
            iter_ms, fold_ms, launches = tm.iterate_ms, tm.resolve_ms, tm.iterate_launches
            col_ms = tm.colorize_ms
            if world > 1:
                t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
                dist.all_reduce(t, op=dist.ReduceOp.MAX)
                elapsed = float(t.item())

            sustained = pipelined = None
            default_shape = int(a.iters) == ITERS_PER_GPU and not jobs_given
            if world == 1 and extras and a.full:
                import bench_extras as X
                if a.sustained_seconds > 0:
                    rt.enable_timing(False)  # no per-launch events in this loop: thousands of frames
                    sustained = X.sustained_loop(torch, stream, step, elapsed / steps, steps, a.sustained_seconds, n * total_jobs)
                if a.pipeline:
                    pipelined = X.pipelined_loop(S, torch, cfg, local_rank, jobs, n, starts_dev.data_ptr(), npix, steps, warmup, tuning)

            # The frame's checksums against the committed golden of the same frame (untimed): configs[1] as this bench runs it at
            # N = 1 (golden c2_131072), configs[3] — the same frame at every N — as tests/golden holds it (c4_full_1e10: seed 3,
            # the preset's transparent flag), rendered, merged and colorized once more by the same ranks.
            case = "c2_131072" if ((config == "c2" and world == 1) or config == "c2s") else ("c4_full_1e10" if config == "c4" else None)
            if a.full and a.parity and default_shape and case and not a.variant:
                import bench_extras as X
                try:
                    rt.enable_timing(False)
                    if config == "c4":
                        cfg_g = S.Config.poisson_saturne(iterations=n * total_jobs, width=width, height=height, jobs_total=total_jobs, seed=3)
                        starts_g = S.start_points(3, first_job, jobs)
                        ex_g = SlicedExchange(S, cfg_g, rt, rank, world, "cuda") if ex is not None else None
                    else:   # (c2s: the N = 1 frame itself, merged over the ranks' job slices)
                        cfg_g, starts_g, ex_g = cfg, starts, (ex if config == "c2s" else None)
                    rt.reset()
                    S.render_job_range(cfg_g, rt, n, starts_g)
                    if world > 1:
                        merge_ranks(rt, ex_g)
                    torch.cuda.synchronize()
                    frame = X.gather_merged_frame(S, torch, dist, np, rt, ex_g, cfg_g, rank, world, a.backend)
                    if rank == 0:
                        parity = X.frame_parity(S, case, *frame[:4], frame[4])
                        print(f"[parity] {case}: {parity['result']}", file=sys.stderr)
                    del ex_g
                except Exception as e:  # evidence next to the number: never lose the line over it
                    parity = {"result": "not checked", "error": repr(e)}
                if world > 1:
                    dist.barrier()

        counted = n * total_jobs * steps
        value = counted / elapsed
        if rank == 0:
            kern_s = iter_ms * 1e-3 / max(launches, 1)             # average duration of one launch of the iterate kernel
            launch_desc = rt.describe_last_launch()                # what the library really launched (not a guess made here)
            iterate_kernel = launch_desc.split(" ")[0]
            per_launch = n * jobs * steps / max(launches, 1)      # counted iterations one launch processes
            ach = ALG_BYTES_PER_ITER * per_launch / kern_s / 1e9
            out = {
                "metric": ("attractor iterations/sec at 1e9 iters, 2048x2048 buffer (poisson-saturne), per-GPU frame" if config == "c2"
                           else "attractor iterations/sec at 1e9 iters IN TOTAL, 2048x2048 buffer (poisson-saturne), whole frame" if config == "c2s"
                           else "attractor iterations/sec at 1e10 iters, 4096x4096 buffer (poisson-saturne), whole frame"),
                "value": value, "unit": "iterations/s", "n_gpus": world, "steps": steps, "warmup": warmup,
                "ms_per_step": elapsed / steps * 1e3, "higher_is_better": True,
                "scaling": "weak" if config == "c2" else "strong",
                "vs_baseline": None, "dtype": "f64", "data": "synthetic",
                "config": {"workload": ("BASELINE configs[1]: poisson-saturne, 1e9 iterations per GPU, 2048x2048, "
                                        "Gas colorize to RGBA16 in HBM") if config == "c2" else
                                       (f"BASELINE configs[1] as ONE frame: poisson-saturne, 1e9 iterations in total, 2048x2048, {total_jobs} jobs "
                                        "sharded over the GPUs, Gas colorize to RGBA16 in HBM") if config == "c2s" else
                                       (f"BASELINE configs[3]: poisson-saturne, 1e10 iterations, 4096x4096, {total_jobs} jobs "
                                        "sharded over the GPUs, Gas colorize to RGBA16 in HBM"),
                           "jobs_per_gpu": jobs, "jobs_total": total_jobs,
                           "iterations_per_job": n, "counted_iterations_per_step": n * total_jobs,
                           "warmup_iterations_per_job_uncounted": 1000,
                           "counted_over_executed_iterations": round(n / (n + 1000.0), 4),
                           "next_frame_announced": bool(a.prefetch and not a.host_starts),
                           "start_points": "uploaded from host memory every step" if a.host_starts else "resident in HBM",
                           "parallelism": f"trajectories sharded over {world} GPU(s)"
                                          + ((f"; all-to-all of image slices (16 B/px) + merge in rank order + sharded "
                                              f"colorize + RGBA16 gather (8 B/px)" if a.exchange == "sliced" else
                                              f"; all-reduce MAX (depth keys) + reduce SUM (count, steps)")
                                             + f" over {'RCCL/xGMI' if a.backend == 'nccl' else a.backend + ' (ranks share GPUs: staged through host)'}"
                                             if world > 1 else "")},
                "roofline": {"bound": "hbm", "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": ach / HBM_PEAK_GBS,
                             "traffic": None,
                             "traffic_source": None,
                             "kernel": iterate_kernel, "launch": launch_desc, "kernel_ms": kern_s * 1e3,
                             "alg_bytes_per_iteration": ALG_BYTES_PER_ITER,
                             "launches_timed": launches,
                             "valu_frac": FP64_OPS_PER_ITER * per_launch / kern_s / FP64_PEAK_OPS,
                             "note": "judged roofline per SURVEY 8(d) is HBM with 12.07 algorithmic B/iteration; the "
                                     "kernel's binding resource is fp64 VALU issue (88 unfused ops/iteration, no FMA "
                                     "allowed): valu_frac = 88*it/s / 39.3e12 op/s. traffic = HBM-side bytes per launch from the "
                                     "PMC counters (traffic_source), below the algorithmic bytes because the scatter state lives in LDS/L2"},
                "sustained": sustained,
                "kernel_ms_per_step": {"warmup_and_pack": tm.warmup_ms / steps, "iterate": iter_ms / steps,
                                       "accumulate_fold_resolve": fold_ms / steps,
                                       "colorize_last": col_ms},
                "parity": parity,
                "run": run_record,
            }
            if dumped:
                out["dumped_outputs"] = {"dir": a.dump_outputs, "arrays": dumped}
            if pipelined is not None:
                out["pipelined"] = pipelined
            if world > 1:
                out["phase_ms_per_step"] = {"render": phase_ms[0] / steps, "exchange": phase_ms[1] / steps,
                                            "colorize_and_gather": phase_ms[2] / steps, "form": a.exchange, "backend": a.backend,
                                            "note": "rank 0's stream: reset + warm-up + iterate + accumulate + fold | pack + all-to-all + merge + "
                                                    "scalars | sharded colorize + RGBA16 gather"}
                out["exchange_ms_per_step"] = {"merge": phase_ms[1] / steps, "colorize_and_gather": phase_ms[2] / steps,
                                               "form": a.exchange, "backend": a.backend}
                out["check"] = check_note
                if ex is not None:
                    out["exchange_ms_per_step"]["bytes_on_the_wire_per_rank"] = ex.bytes_on_the_wire()
            result = out
        if ex is not None:
            del ex
        rt.close()
        if rank == 0 and world == 1 and extras and a.full and config == "c2":
            import bench_extras as X
            # the measurement is done and the runtime released: the line goes to stderr before anything else can cost it
            print("[bench] line before the PMC passes / CPU baseline: " + json.dumps(result), file=sys.stderr, flush=True)
            if int(a.iters) == ITERS_PER_GPU and jobs == DEFAULT_JOBS and a.traffic:
                traffic, traffic_src = X.measure_traffic_live(iterate_kernel)
                if traffic is None:
                    why = traffic_src
                    traffic, traffic_src = X.pmc_traffic_bytes()
                    if traffic_src:
                        traffic_src = (f"{traffic_src}: PMC passes of this workload committed with the round ((2*FETCH_SIZE + WRITE_SIZE)*1024 per "
                                       f"launch), NOT measured by this run ({why})")
                result["roofline"]["traffic"], result["roofline"]["traffic_source"] = traffic, traffic_src
            if not a.no_cpu_baseline:
                result["cpu_baseline"] = X.cpu_baseline(a.cpu_seconds, WIDTH, HEIGHT, ITERS_PER_GPU)
                result["gpu_over_cpu"] = value / result["cpu_baseline"]["value"]
        return result

    out = run_config(a.config, a.steps, a.warmup, True)
    if world > 1 and both_curves:
        # The extras must never cost the line itself. They have never run on more than one physical GPU, so every rank arms
        # the same watchdog once the configs[1] measurement is done: if the extras are not through in time (a hang in a
        # collective, a dead peer), rank 0 prints the line it has — with what went wrong — and every rank leaves.
        import threading
        state = {"printed": False}
        lock = threading.Lock()

        def emit():
            with lock:
                if rank == 0 and not state["printed"]:
                    print(json.dumps(out), flush=True)
                state["printed"] = True

        def give_up():
            if rank == 0:
                out.setdefault("strong_c4", {"error": f"not finished within {a.extras_seconds:.0f} s: given up"})
                out.setdefault("strong_c2", {"error": f"not reached within {a.extras_seconds:.0f} s"})
                out.setdefault("native", {"error": f"not reached within {a.extras_seconds:.0f} s"})
            emit()
            sys.stdout.flush()
            os._exit(0)

        # ... and the line as it stands goes to stderr at once (flushed), so that even a kill from outside during the extras
        # leaves the configs[1] measurement on record; stdout keeps its ONE line, printed last.
        if rank == 0:
            print("[bench] weak-scaling line before the extras: " + json.dumps(out), file=sys.stderr, flush=True)
        dog = threading.Timer(a.extras_seconds, give_up)
        dog.daemon = True
        dist.barrier()
        dog.start()
        # The denominators first, from THIS node: rank 0 alone renders the two strong-scaling frames whole (N = 1) while the other
        # ranks wait — the pool's boxes differ by ~6 %, so a committed profile of another box cannot be what a speed-up divides by.
        n1 = {}
        try:
            if rank == 0:
                import bench_extras as X
                n1["c4"] = X.n1_same_node(S, torch, np, local_rank, C4_SIZE, C4_JOBS, C4_ITERS, 3, 1, seed=1)
                n1["c2s"] = X.n1_same_node(S, torch, np, local_rank, WIDTH, DEFAULT_JOBS, ITERS_PER_GPU, 10, 2, seed=1)
                print("[bench] N = 1 on this node: " + json.dumps(n1), file=sys.stderr, flush=True)
        except Exception as e:
            n1["error"] = repr(e)
        dist.barrier()
        try:
            # the strong-scaling frame on the same ranks: BASELINE configs[3], the same frame at every N
            c4 = run_config("c4", max(2, min(a.steps, 6)), 1, False)
            if rank == 0:
                ref, ref_file = None, None
                try:  # the committed N=1 line of the same workload (the newest round's)
                    import glob
                    ref_file = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench_c4_n1.json")))[-1]
                    ref = json.loads(open(ref_file).read().strip().splitlines()[-1])
                    ref_file = os.path.relpath(ref_file, ROOT)
                except Exception:
                    pass
                out["strong_c4"] = {"value": c4["value"], "unit": c4["unit"], "ms_per_step": c4["ms_per_step"], "steps": c4["steps"],
                                    "scaling": "strong", "workload": c4["config"]["workload"], "jobs_total": c4["config"]["jobs_total"],
                                    "parity": (c4["parity"] or {}).get("result", "not checked"), "parity_checksums": c4["parity"],
                                    "phase_ms_per_step": c4.get("phase_ms_per_step"), "check": c4.get("check"),
                                    "exchange_ms_per_step": c4.get("exchange_ms_per_step"), "kernel_ms_per_step": c4["kernel_ms_per_step"],
                                    "launch": c4["roofline"]["kernel"],
                                    "n1_same_node": n1.get("c4"),
                                    "speedup_same_node": (c4["value"] / n1["c4"]["value"]) if n1.get("c4") else None,
                                    "n1_profile": ({"file": ref_file, "value": ref["value"], "ms_per_step": ref["ms_per_step"]}
                                                   if ref else None),
                                    "speedup_vs_n1_profile": (c4["value"] / ref["value"]) if ref else None}
        except Exception as e:
            if rank == 0:
                out["strong_c4"] = {"error": repr(e)}
        try:
            # ... and the metric read literally: 1e9 iterations in TOTAL at 2048^2, the N = 1 frame's 131 072 jobs cut over the ranks
            c2s = run_config("c2s", max(4, min(a.steps, 20)), 2, False)
            if rank == 0:
                out["strong_c2"] = {"value": c2s["value"], "unit": c2s["unit"], "ms_per_step": c2s["ms_per_step"], "steps": c2s["steps"],
                                    "scaling": "strong", "workload": c2s["config"]["workload"], "jobs_total": c2s["config"]["jobs_total"],
                                    "jobs_per_gpu": c2s["config"]["jobs_per_gpu"],
                                    "parity": (c2s["parity"] or {}).get("result", "not checked"), "parity_checksums": c2s["parity"],
                                    "phase_ms_per_step": c2s.get("phase_ms_per_step"), "check": c2s.get("check"),
                                    "exchange_ms_per_step": c2s.get("exchange_ms_per_step"), "kernel_ms_per_step": c2s["kernel_ms_per_step"],
                                    "launch": c2s["roofline"]["kernel"],
                                    "n1_same_node": n1.get("c2s"),
                                    "speedup_same_node": (c2s["value"] / n1["c2s"]["value"]) if n1.get("c2s") else None,
                                    "note": "the metric's literal reading (1e9 iterations in total at every N); SURVEY 7-2 predicts this curve poor: a "
                                            "5.8 ms frame cut in N leaves each GPU 131072 / N trajectories (one wave pair per CU at 8), the 1000 "
                                            "warm-up iterations per job and the exchange do not shrink — the weak-scaling `value` and strong_c4 "
                                            "are the curves this path is built for"}
        except Exception as e:
            if rank == 0:
                out["strong_c2"] = {"error": repr(e)}
        try:
            # ... and both workloads through the C ABI alone (one process, rank 0, every GPU of the job; the other ranks wait)
            dist.barrier()
            if rank == 0:
                try:
                    import bench_extras as X
                    devs = list(range(min(world, max(torch.cuda.device_count(), 1))))
                    devs = [devs[k % len(devs)] for k in range(world)]
                    out["native"] = {"c2": X.native_measure(S, torch, devs, "c2", max(2, min(a.steps, 6)), 1, K),
                                     "c4": X.native_measure(S, torch, devs, "c4", max(2, min(a.steps, 4)), 1, K)}
                    out["run"]["peer_access_failures"] = max(out["native"]["c2"].get("peer_access_failures", 0),
                                                             out["native"]["c4"].get("peer_access_failures", 0))
                except Exception as e:  # an extra: never lose the line over it
                    out["native"] = {"error": repr(e)}
            dist.barrier()
        except Exception as e:
            if rank == 0:
                out.setdefault("native", {"error": repr(e)})
        dog.cancel()
        emit()
    elif rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
