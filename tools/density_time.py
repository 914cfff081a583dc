"""Times density estimation (include/sar.h: sar_runtime_density, k_density) on two frames a user renders — BASELINE configs[1]
(poisson-saturne, 2048^2, 1e9 iterations) and one frame of the configs[4] sweep (solar-sail, 1800x2000, 1e8 iterations, 65 536 jobs)
— for S = 16, 64 and 256: k_density's time from the HIP events of the runtime's timing (iterate_ms of a density call) after a warm-up
call, next to the same process's render time (wall, around a synchronise) and colorize time (HIP events) for that frame, the share of
tiles that took the copy-through path, and the call's statistics. Every S filters the SAME rendered state (read back once, loaded
again before each call). One run; the spread is not measured.

    python tools/density_time.py [--out profiles/density_time.json] [--samples 16,64,256]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _frames(S):
    jobs = 65536
    yield ("poisson_saturne 2048x2048 1e9 (configs[1])",
           S.Config.poisson_saturne(iterations=1_000_000_000, width=2048, height=2048, scale=1.0, transparent=0), None)
    yield ("solar_sail 1800x2000 1e8, 65536 jobs (a configs[4] sweep frame)",
           S.Config.solar_sail(iterations=(100_000_000 // jobs) * jobs, width=1800, height=2000, scale=1.0, transparent=0, jobs_total=jobs), jobs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--samples", default="16,64,256")
    a = ap.parse_args()
    import strange_attractor_renderer_amd as S
    rows = []
    for label, cfg, jobs in _frames(S):
        renderer = None
        if jobs is None:                                  # the flagship frame as bench.py renders it
            renderer = S.ParallelRenderer(device=0, seed=1)
            S.render_parallel(renderer, cfg, 12)          # warm
            t0 = time.perf_counter()
            S.render_parallel(renderer, cfg, 12)
            render_ms = (time.perf_counter() - t0) * 1e3  # (render_parallel ends with the colorize and its read-back)
            rt = renderer.runtime()
        else:
            rt = S.Runtime(cfg)
            starts = S.start_points(1, 0, jobs)
            S.render_jobs(cfg, rt, starts)                # warm
            rt.synchronize()
            rt.reset()
            rt.synchronize()
            t0 = time.perf_counter()
            S.render_jobs(cfg, rt, starts)
            rt.synchronize()
            render_ms = (time.perf_counter() - t0) * 1e3
        try:
            rt.enable_timing(True)
            S.colorize(cfg, rt)
            S.colorize(cfg, rt)
            colorize_ms = rt.last_timing().colorize_ms
            state = (rt.count(), rt.steps(), rt.zbuf(), rt.max())
            row = dict(frame=label, render_wall_ms=round(render_ms, 3), colorize_ms=round(colorize_ms, 4), filters=[])
            for samples in [int(s) for s in a.samples.split(",") if s]:
                rt.load(*state)
                rt.density_filter(stats=False, samples=samples)      # warm-up: the code object, the scratch, the plan
                rt.load(*state)
                stats = rt.density_filter(samples=samples)
                ms = rt.last_timing().iterate_ms
                tiles, copied = rt.density_tiles()
                row["filters"].append(dict(samples=samples, radius=S.density_radius(samples), k_density_ms=round(ms, 4),
                                           pct_of_render=round(100.0 * ms / render_ms, 2), tiles=tiles, tiles_copied=copied,
                                           copied_share=round(copied / tiles, 4), stats=stats))
            rows.append(row)
            print(json.dumps(row), flush=True)
        finally:
            rt.enable_timing(False)
            if renderer is not None:
                renderer.shutdown()
            else:
                rt.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/density_time.py", note="one run, spread not measured", rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
