"""Times volume rendering (include/sar.h: sar_runtime_volume*) on BASELINE configs[1]'s map and view (poisson-saturne) at 1024^2 with
1e8 iterations in 65 536 jobs, at D = 64 and 256 slabs: k_volume_accumulate (iterate_ms of a volume call, the sum over its launches)
next to the same build's Gas render of the same jobs (iterate_ms + resolve_ms of a render_job_range call), then k_volume_march and
k_volume_section alone (colorize_ms). Every figure is the best of three calls after a warm-up call, from the HIP events of the
runtime's timing. The accumulate is ATOMIC-BOUND: one scattered global atomic per stored visit.

    python tools/volume_time.py [--out profiles/volume_time.json] [--slabs 64,256] [--step-timeout 240]

Every D runs in a child process of its own under --step-timeout seconds; a child that fails or runs out of time ends the tool.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JOBS, WIDTH = 65536, 1024
ITERS = 100_000_000 // JOBS
REPEATS = 3


def step(slabs: int) -> dict:
    import strange_attractor_renderer_amd as S
    cfg = S.Config.poisson_saturne(iterations=ITERS * JOBS, width=WIDTH, height=WIDTH, scale=1.0, jobs_total=JOBS)
    rt = S.Runtime(cfg)
    try:
        starts = S.start_points(1, 0, JOBS)
        rt.enable_timing(True)
        render = []
        for _ in range(REPEATS + 1):
            rt.reset()
            S.render_job_range(cfg, rt, ITERS, starts)
            t = rt.last_timing()
            render.append(dict(iterate_ms=t.iterate_ms, resolve_ms=t.resolve_ms, warmup_ms=t.warmup_ms))
        v = S.volume(rt, cfg, jobs=JOBS, iterations=ITERS, slabs=slabs, starts=starts)     # warm-up call; learns the range
        z_range, accumulate = v.z_range, []
        for _ in range(REPEATS):
            v = S.volume(rt, cfg, jobs=JOBS, iterations=ITERS, slabs=slabs, z_range=z_range, starts=starts)
            t = rt.last_timing()
            accumulate.append(dict(iterate_ms=t.iterate_ms, launches=t.iterate_launches, warmup_ms=t.warmup_ms))
        march, section = [], []
        for _ in range(REPEATS + 1):
            v.march()
            march.append(rt.last_timing().colorize_ms)
            v.section()
            section.append(rt.last_timing().colorize_ms)
        _, march_stats = v.march(stats=True)
        best_render = min(r["iterate_ms"] + r["resolve_ms"] for r in render[1:])
        best_acc = min(a["iterate_ms"] for a in accumulate)
        return dict(slabs=slabs, z_range=z_range, stats=v.stats, march_stats=march_stats,
                    render_iterate_plus_resolve_ms=[round(r["iterate_ms"] + r["resolve_ms"], 4) for r in render[1:]],
                    k_volume_accumulate_ms=[round(a["iterate_ms"], 4) for a in accumulate], accumulate_launches=accumulate[0]["launches"],
                    k_volume_warm_ms=[round(a["warmup_ms"], 4) for a in accumulate],
                    k_volume_march_ms=[round(m, 4) for m in march[1:]], k_volume_section_ms=[round(m, 4) for m in section[1:]],
                    best=dict(render_ms=round(best_render, 4), accumulate_ms=round(best_acc, 4),
                              stored_visits_per_s=round(v.stats["stored"] / (best_acc * 1e-3), 1),
                              render_iterations_per_s=round(ITERS * JOBS / (best_render * 1e-3), 1),
                              accumulate_over_render=round(best_acc / best_render, 3),
                              march_ms=round(min(march[1:]), 4), section_ms=round(min(section[1:]), 4)))
    finally:
        rt.enable_timing(False)
        rt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--slabs", default="64,256")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", type=int, default=0, help="(internal) run one D in this process and print its row")
    a = ap.parse_args()
    if a.step:
        print(json.dumps(step(a.step)), flush=True)
        return 0
    rows = []
    for slabs in [int(s) for s in a.slabs.split(",") if s]:
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", str(slabs)], capture_output=True, text=True,
                                   timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"D = {slabs}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 1
        if child.returncode != 0:
            print(f"D = {slabs}: the step ended with status {child.returncode}; stopping\n{child.stderr[-2000:]}", file=sys.stderr)
            return 1
        rows.append(json.loads(child.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/volume_time.py", frame=f"poisson_saturne {WIDTH}x{WIDTH}, {JOBS} jobs x {ITERS} iterations",
                           note="best of three calls after a warm-up call, one run of the tool; k_volume_accumulate is atomic-bound "
                                "(one scattered global atomic per stored visit)", rows=rows), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
