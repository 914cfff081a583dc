"""Throughput of the orbit diagrams (sar_runtime_orbit) on one GPU.

    python tools/orbit_time.py [--width 2048] [--height 1024] [--jobs 256] [--steps 4096] [--transient 1000] [--repeats 3]
                               [--out profiles/orbit_time.json]

Times a diagram on two lines — from poisson-saturne to solar-sail (x plotted) and the logistic family x' = r x - r x^2 for r in
[2.8, 4) — and, separately, two blocks of logistic columns: period 2 (r in [3.1, 3.4]) and chaotic (r in [3.9, 4)). In a periodic
window a whole wave adds to one or two LDS words, in a chaotic band its lanes spread over many: the contrast between the two blocks
is what merging equal bins within a wave before the atomic would have to win back. Each case reports the kernel time from the
runtime's HIP events (the best of --repeats, after one warm-up call), the wall time of the call, and map steps per second: nominal
(every job runs transient + steps) and live (what the statistics say really ran). Prints one JSON record and writes it to --out; the
record quotes the search's measured lane-steps per second and the frame path's iterations per second next
to its own.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SEARCH_LANE_STEPS_PER_S = 7.3e10      # k_search_lyapunov, DESIGN.md section 10
FRAME_ITERATIONS_PER_S = 1.6e11       # the frame path (DESIGN.md section 14 quotes it)


def logistic(lo, hi):
    import numpy as np
    a, b = np.zeros(30), np.zeros(30)
    a[1], a[2], b[1], b[2] = lo, -lo, hi, -hi
    return a, b


def measure(S, rt, name, a, b, args, v_range) -> dict:
    kw = dict(width=args.width, height=args.height, jobs=args.jobs, steps=args.steps, transient=args.transient, v_range=v_range)
    S.orbit_diagram(rt, a, b, **kw)   # warm-up call: code object, buffers
    best, wall = None, None
    for _ in range(args.repeats):
        rt.enable_timing(True)
        t0 = time.perf_counter()
        d = S.orbit_diagram(rt, a, b, **kw)
        w = time.perf_counter() - t0
        t = rt.last_timing()
        rt.enable_timing(False)
        if best is None or t.iterate_ms < best:
            best, wall, launches = t.iterate_ms, w, t.iterate_launches
    s = d.stats
    survivors = int(args.jobs * args.width - s["dead_transient"].sum())
    nominal = args.width * args.jobs * (args.transient + args.steps)
    live = int(s["hits"].sum() + s["misses"].sum()) + survivors * args.transient
    return {"case": name, "k_orbit_ms": best, "launches": launches, "wall_s": wall,
            "nominal_steps": nominal, "nominal_steps_per_s": nominal / (best * 1e-3) if best else None,
            "live_steps_at_least": live, "live_steps_per_s": live / (best * 1e-3) if best else None,
            "hits": int(s["hits"].sum()), "misses": int(s["misses"].sum()), "dead_transient": int(s["dead_transient"].sum()),
            "dead_late": int(s["dead_late"].sum()), "occupied_bins_mean": float(s["occupied"].mean()), "max": d.max}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--jobs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=4096)
    ap.add_argument("--transient", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orbit_time.json"))
    args = ap.parse_args()
    import strange_attractor_renderer_amd as S
    if S.device_count() <= 0:
        raise SystemExit("orbit_time needs a HIP device: a time from anywhere else says nothing")
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    cases = [measure(S, rt, "presets: poisson-saturne -> solar-sail", S.Config.poisson_saturne(), S.Config.solar_sail(), args, (-1.5, 1.5)),
             measure(S, rt, "logistic r in [2.8, 4)", *logistic(2.8, 3.9999), args, (0.0, 1.0)),
             measure(S, rt, "logistic block, period 2: r in [3.1, 3.4]", *logistic(3.1, 3.4), args, (0.0, 1.0)),
             measure(S, rt, "logistic block, chaotic: r in [3.9, 4)", *logistic(3.9, 3.9999), args, (0.0, 1.0))]
    rt.close()
    p2, ch = cases[2]["k_orbit_ms"], cases[3]["k_orbit_ms"]
    res = {"tool": "tools/orbit_time.py", "shape": {k: getattr(args, k) for k in ("width", "height", "jobs", "steps", "transient", "repeats")},
           "build_id": S.load_library().sar_build_id().decode(), "cases": cases,
           "period2_over_chaotic_time": p2 / ch if p2 and ch else None,
           "next_to": {"search_lane_steps_per_s": SEARCH_LANE_STEPS_PER_S, "frame_iterations_per_s": FRAME_ITERATIONS_PER_S}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
