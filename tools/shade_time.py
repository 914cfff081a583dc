"""Times shaded rendering (include/sar.h: sar_shade_device, k_shade) on two frames a user renders — BASELINE configs[1]
(poisson-saturne, 2048^2, 1e9 iterations) and one frame of the configs[4] sweep (solar-sail, 1800x2000, 1e8 iterations, 65 536 jobs)
— at R = 0, 6 and 8, with and without the smoothing: k_shade's time from the HIP events of the runtime's timing (colorize_ms of a
shade call) after a warm-up call, next to k_colorize_gas of the same state in the same process (colorize_ms of a colorize call) and
the render time (wall, around a synchronise), with the call's statistics. Every setting shades the SAME rendered state, which the call
only reads. One run; the spread is not measured.

    python tools/shade_time.py [--out profiles/shade_time.json] [--png PATH] [--radii 0,6,8]

--png writes the shaded configs[1] frame at the defaults (and PATH with _sweep before its suffix for the sweep frame), so that a
person can look at it.
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
           S.Config.poisson_saturne(iterations=1_000_000_000, width=2048, height=2048, scale=1.0, transparent=0), None, "")
    yield ("solar_sail 1800x2000 1e8, 65536 jobs (a configs[4] sweep frame)",
           S.Config.solar_sail(iterations=(100_000_000 // jobs) * jobs, width=1800, height=2000, scale=1.0, transparent=0, jobs_total=jobs), jobs,
           "_sweep")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--png", default="")
    ap.add_argument("--radii", default="0,6,8")
    a = ap.parse_args()
    import torch
    import strange_attractor_renderer_amd as S
    rows = []
    for label, cfg, jobs, tag in _frames(S):
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
            h, w = cfg.c.height, cfg.c.width
            dev = torch.zeros(w * h * 4, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            rt.enable_timing(True)
            S.colorize_device(cfg, rt, dev.data_ptr())
            S.colorize_device(cfg, rt, dev.data_ptr())
            rt.synchronize()
            colorize_ms = rt.last_timing().colorize_ms
            row = dict(frame=label, render_wall_ms=round(render_ms, 3), k_colorize_gas_ms=round(colorize_ms, 4), shades=[])
            for radius in [int(s) for s in a.radii.split(",") if s]:
                for smooth in (0, 1):
                    S.shade_device(cfg, rt, dev.data_ptr(), ao_radius=radius, smooth=smooth)   # warm-up: the code object, the block
                    S.shade_device(cfg, rt, dev.data_ptr(), ao_radius=radius, smooth=smooth)
                    rt.synchronize()
                    ms = rt.last_timing().colorize_ms
                    _, stats = rt.shade(cfg, stats=True, ao_radius=radius, smooth=smooth)
                    row["shades"].append(dict(ao_radius=radius, smooth=smooth, k_shade_ms=round(ms, 4),
                                              pct_of_render=round(100.0 * ms / render_ms, 2), stats=stats))
            rows.append(row)
            print(json.dumps(row), flush=True)
            if a.png:
                root, ext = os.path.splitext(a.png)
                S.write_image(rt.shade(cfg), root + tag + (ext or ".png"))
        finally:
            rt.enable_timing(False)
            if renderer is not None:
                renderer.shutdown()
            else:
                rt.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(dict(tool="tools/shade_time.py", note="one run, spread not measured", rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
