"""Throughput of the basins of attraction (sar_runtime_basin) on one GPU.

    python tools/basin_time.py [--size 1024] [--transient 1000] [--steps 256] [--grid 32] [--repeats 3] [--out profiles/basin_time.json]

Times a size x size window of solar-sail's start box plane (z = 0.05, x and y in [-0.5, 0.5]) in a box learned by a grid = 1 first
pass, as basin_map(box=None) does. Reports the time of both kernels from the runtime's HIP events (the best of --repeats, after one
warm-up call: k_basin_screen is warmup_ms, k_basin_mark iterate_ms), the wall time of the call, and map steps per second: nominal for
the screen (every pixel runs transient + steps), live for the screen (what the escape steps say really ran) and for the mark kernel
(bounded pixels x steps). Prints one JSON record and writes it to --out; the record quotes the search's measured lane-steps per
second and the frame path's iterations per second next to its own.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--transient", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "basin_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    if S.device_count() <= 0:
        raise SystemExit("basin_time needs a HIP device: a time from anywhere else says nothing")
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    kw = dict(origin=(-0.5, -0.5, 0.05), du=(1.0, 0.0, 0.0), dv=(0.0, 1.0, 0.0), width=args.size, height=args.size,
              transient=args.transient, steps=args.steps, grid=args.grid)
    first = S.basin_map(rt, S.Config.solar_sail(), **kw)   # warm-up call: code object, buffers, and the box
    box = (tuple(first.params.box_lo), tuple(first.params.box_hi))
    best = None
    for _ in range(args.repeats):
        rt.enable_timing(True)
        t0 = time.perf_counter()
        b = S.basin_map(rt, S.Config.solar_sail(), box=box, **kw)
        wall = time.perf_counter() - t0
        t = rt.last_timing()
        rt.enable_timing(False)
        if best is None or t.warmup_ms + t.iterate_ms < best["k_basin_screen_ms"] + best["k_basin_mark_ms"]:
            best = {"k_basin_screen_ms": t.warmup_ms, "k_basin_mark_ms": t.iterate_ms, "launches": t.iterate_launches, "wall_s": wall}
    rt.close()
    st = b.stats
    total = args.transient + args.steps
    nominal = st["pixels"] * total
    live = int(st["bounded"]) * total + int(b.escape_step.astype(np.int64).sum())
    mark = int(st["bounded"]) * args.steps
    res = {"tool": "tools/basin_time.py", "map": "solar_sail", "window": {k: kw[k] for k in ("origin", "du", "dv")},
           "shape": {k: getattr(args, k) for k in ("size", "transient", "steps", "grid", "repeats")},
           "build_id": S.load_library().sar_build_id().decode(), **best,
           "stats": {k: int(v) for k, v in st.items() if k != "extent"}, "largest_basins": b.attractors["pixels"][:4].tolist(),
           "screen_nominal_steps": nominal, "screen_nominal_steps_per_s": nominal / (best["k_basin_screen_ms"] * 1e-3),
           "screen_live_steps_at_least": live, "screen_live_steps_per_s": live / (best["k_basin_screen_ms"] * 1e-3),
           "mark_steps": mark, "mark_steps_per_s": mark / (best["k_basin_mark_ms"] * 1e-3) if best["k_basin_mark_ms"] else None,
           "next_to": {"search_lane_steps_per_s": SEARCH_LANE_STEPS_PER_S, "frame_iterations_per_s": FRAME_ITERATIONS_PER_S}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
