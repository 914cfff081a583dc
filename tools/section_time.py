"""Times the Poincare sections of flows (include/sar.h: sar_runtime_section) on Lorenz at 1024^2 with 65 536 jobs of 64 samples, on
the plane z = 27 (upwards) and on the surface of the maxima of z, with plot off and on: k_flow_section (iterate_ms of a call, all its
launches), the useful steps and the recorded crossings per second, the longest single dispatch — the first launch of chunk_steps
steps, in which every lane still runs, timed by a call whose max_steps is one launch — and the share of the launched lane-steps
that lanes spent idle after their job had filled or escaped. Next to it the same build's k_flow_render with plot = 0 over the same
jobs and the same number of steps. Every figure is the best of three calls after a warm-up call, from the HIP events of the
runtime's timing. The start points are the stream's cube spread over the attractor's neighbourhood (|x|, |y| <= 10, 15 <= z <= 35):
from the cube itself every job follows one branch of the origin's unstable manifold for a long time, and all lanes would cross together.

    python tools/section_time.py [--out profiles/section_time.json] [--step-timeout 240]

Every (surface, plot) runs in a child process of its own under --step-timeout seconds; a child that fails or runs out of time ends
the tool.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JOBS, WIDTH, SAMPLES, MAX_STEPS, CHUNK_STEPS, TRANSIENT, DT = 65536, 1024, 64, 8192, 4096, 1000, 0.01
REPEATS = 3
ROWS = [(surface, plot) for surface in ("z27", "zmax") for plot in (0, 1)]


def step(surface: str, plot: int) -> dict:
    import numpy as np
    import strange_attractor_renderer_amd as S
    lorenz = S.flow_coefficients("lorenz")
    s, direction = (S.section_plane((0.0, 0.0, 1.0), 27.0), 1) if surface == "z27" else (S.section_extremum(lorenz, 2), -1)
    base = S.Config.from_coefficients(lorenz).replace(width=WIDTH, height=WIDTH)
    rt = S.Runtime(base)
    try:
        starts = S.start_points(1, 0, JOBS) * 100.0 + np.array([0.0, 0.0, 25.0])
        common = dict(dt=DT, transient=TRANSIENT, starts=starts)
        cfg = S.flow_section(base, rt, s, jobs=1024, samples=SAMPLES, direction=direction, max_steps=MAX_STEPS, **dict(common, starts=starts[:1024])).view(base)
        rt.enable_timing(True)

        def timed(max_steps):
            calls = []
            for _ in range(REPEATS + 1):
                rt.reset()
                fs = S.flow_section(cfg, rt, s, jobs=JOBS, samples=SAMPLES, direction=direction, max_steps=max_steps, plot=bool(plot), **common)
                t = rt.last_timing()
                calls.append(dict(section_ms=t.iterate_ms, launches=t.iterate_launches, transient_ms=t.warmup_ms, resolve_ms=t.colorize_ms))
            return fs, calls[1:]

        fs, calls = timed(MAX_STEPS)
        _, first = timed(CHUNK_STEPS)                               # one launch: the first, with every lane running
        flow = []
        for _ in range(REPEATS + 1):
            st = S.render_flow(cfg, rt, dt=DT, jobs=JOBS, steps=MAX_STEPS, transient=TRANSIENT, starts=starts, stats=True, plot=0)
            t = rt.last_timing()
            flow.append(dict(render_ms=t.iterate_ms, launches=t.iterate_launches))
        best, best_first, best_flow = min(c["section_ms"] for c in calls), min(c["section_ms"] for c in first), min(c["render_ms"] for c in flow[1:])
        launched = JOBS * MAX_STEPS
        stats = {k: (v.tolist() if hasattr(v, "tolist") else v) for k, v in fs.stats.items()}
        return dict(surface=surface, direction=direction, plot=plot, stats=stats,
                    k_flow_section_ms=[round(c["section_ms"], 4) for c in calls], section_launches=calls[0]["launches"],
                    first_launch_ms=[round(c["section_ms"], 4) for c in first],
                    k_flow_transient_ms=[round(c["transient_ms"], 4) for c in calls], k_flow_resolve_ms=[round(c["resolve_ms"], 4) for c in calls],
                    k_flow_render_plot0_ms=[round(c["render_ms"], 4) for c in flow[1:]], render_launches=flow[1]["launches"], flow_steps=st["steps"],
                    best=dict(section_ms=round(best, 4), steps_per_s=round(fs.stats["steps"] / (best * 1e-3), 1),
                              launched_lane_steps_per_s=round(launched / (best * 1e-3), 1),
                              crossings_per_s=round(fs.stats["crossings"] / (best * 1e-3), 1),
                              longest_dispatch_ms=round(best_first, 4),
                              idle_share=round(1.0 - fs.stats["steps"] / launched, 4),
                              steps_per_crossing=round(fs.stats["steps"] / max(fs.stats["crossings"] + fs.stats["clocked"], 1), 2),
                              flow_render_ms=round(best_flow, 4), flow_steps_per_s=round(st["steps"] / (best_flow * 1e-3), 1),
                              flow_longest_dispatch_ms=round(best_flow / flow[1]["launches"], 4)))
    finally:
        rt.enable_timing(False)
        rt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default="", help="(internal) run one row, surface,plot, in this process and print it")
    a = ap.parse_args()
    if a.step:
        surface, plot = a.step.split(",")
        print(json.dumps(step(surface, int(plot))), flush=True)
        return 0
    rows = []
    for surface, plot in ROWS:
        what = f"{surface},{plot}"
        try:
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", what], capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{what}: no result within {a.step_timeout} s; stopping", file=sys.stderr)
            return 1
        if child.returncode != 0:
            print(f"{what}: the step ended with status {child.returncode}; stopping\n{child.stderr[-2000:]}", file=sys.stderr)
            return 1
        rows.append(json.loads(child.stdout.strip().splitlines()[-1]))
        print(json.dumps(rows[-1]["best"] | dict(row=what)), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/section_time.py",
                           frame=f"{WIDTH}x{WIDTH}, Lorenz at dt {DT}, {JOBS} jobs x {SAMPLES} samples, at most {MAX_STEPS} steps in launches of "
                                 f"{CHUNK_STEPS}, the view framed on the section",
                           note="best of three calls after a warm-up call, one run of the tool, spread not measured; the longest dispatch is "
                                "the first launch, timed by a call of max_steps = one launch; idle_share is the share of jobs x max_steps "
                                "lane-steps that no job took (whole waves of finished jobs cost nothing, so it bounds the waste from above); "
                                "k_flow_render with plot = 0 runs the same jobs for max_steps steps", rows=rows), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
