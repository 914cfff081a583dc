"""Times flow rendering (include/sar.h: sar_runtime_render_flow) on Lorenz and Roessler at 1024^2 with 65 536 jobs of 4096 RK4 steps,
at dt = 0.01 and 0.001 and stride 1 and 8, each in a view framed by flow_view: k_flow_render (iterate_ms of a call: ONE launch at
these sizes, so it is also the longest dispatch of the counted steps), steps per second, the visits per count atomic that run merging
reaches, and next to it the same build's k_volume_accumulate at one slab on BASELINE configs[1]'s map with as many visits — the
un-merged rate of one scattered atomic per visit. Every figure is the best of three calls after a warm-up call, from the HIP events
of the runtime's timing.

    python tools/flow_time.py [--out profiles/flow_time.json] [--step-timeout 240]

Every (system, dt, stride) runs in a child process of its own under --step-timeout seconds; a child that fails or runs out of time
ends the tool.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
JOBS, WIDTH, STEPS = 65536, 1024, 4096
REPEATS = 3
ROWS = [(system, dt, stride) for system in ("lorenz", "rossler") for dt in (0.01, 0.001) for stride in (1, 8)]


def step(system: str, dt: float, stride: int) -> dict:
    import strange_attractor_renderer_amd as S
    transient = int(round(10.0 / dt))                          # ten time units: onto the attractor at either step
    base = S.Config.from_coefficients(S.flow_coefficients(system)).replace(width=WIDTH, height=WIDTH)
    rt = S.Runtime(base)
    try:
        starts = S.start_points(1, 0, JOBS)
        cfg = S.flow_view(base, rt, dt=dt, jobs=1024, steps=STEPS, transient=transient, starts=starts[:1024])
        rt.enable_timing(True)
        calls = []
        for _ in range(REPEATS + 1):
            rt.reset()
            st = S.render_flow(cfg, rt, dt=dt, jobs=JOBS, steps=STEPS, transient=transient, stride=stride, starts=starts, stats=True)
            t = rt.last_timing()
            calls.append(dict(render_ms=t.iterate_ms, launches=t.iterate_launches, transient_ms=t.warmup_ms, resolve_ms=t.colorize_ms))
        best = min(c["render_ms"] for c in calls[1:])
        # the same visits as one atomic each: k_volume_accumulate with a single slab that holds every depth
        mjobs = JOBS
        miters = max(int(round(st["visits"] / mjobs)), 1)
        mcfg = S.Config.poisson_saturne(iterations=miters * mjobs, width=WIDTH, height=WIDTH, scale=1.0, jobs_total=mjobs)
        v = S.volume(rt, mcfg, jobs=mjobs, iterations=miters, slabs=1, starts=starts)          # warm-up call; learns the range
        acc = []
        for _ in range(REPEATS):
            v = S.volume(rt, mcfg, jobs=mjobs, iterations=miters, slabs=1, z_range=v.z_range, starts=starts)
            acc.append(rt.last_timing().iterate_ms)
        return dict(system=system, dt=dt, stride=stride, transient=transient,
                    stats={k: (v_.tolist() if hasattr(v_, "tolist") else v_) for k, v_ in st.items()},
                    k_flow_render_ms=[round(c["render_ms"], 4) for c in calls[1:]], render_launches=calls[1]["launches"],
                    k_flow_transient_ms=[round(c["transient_ms"], 4) for c in calls[1:]],
                    k_flow_resolve_ms=[round(c["resolve_ms"], 4) for c in calls[1:]],
                    k_volume_accumulate_ms=[round(a, 4) for a in acc], volume_stored=v.stats["stored"],
                    best=dict(render_ms=round(best, 4), longest_dispatch_ms=round(best / calls[1]["launches"], 4) if calls[1]["launches"] == 1 else None,
                              steps_per_s=round(st["steps"] / (best * 1e-3), 1), visits_per_s=round(st["visits"] / (best * 1e-3), 1),
                              visits_per_count_atomic=round(st["visits"] / max(st["count_atomics"], 1), 3),
                              count_atomics_per_s=round(st["count_atomics"] / (best * 1e-3), 1),
                              volume_accumulate_ms=round(min(acc), 4), volume_stored_visits_per_s=round(v.stats["stored"] / (min(acc) * 1e-3), 1)))
    finally:
        rt.enable_timing(False)
        rt.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--step", default="", help="(internal) run one row, system,dt,stride, in this process and print it")
    a = ap.parse_args()
    if a.step:
        system, dt, stride = a.step.split(",")
        print(json.dumps(step(system, float(dt), int(stride))), flush=True)
        return 0
    rows = []
    for system, dt, stride in ROWS:
        what = f"{system},{dt},{stride}"
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
            json.dump(dict(tool="tools/flow_time.py", frame=f"{WIDTH}x{WIDTH}, {JOBS} jobs x {STEPS} RK4 steps, the view framed by flow_view",
                           note="best of three calls after a warm-up call, one run of the tool, spread not measured; k_volume_accumulate "
                                "with one slab is the same visits at one scattered atomic each", rows=rows), f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
