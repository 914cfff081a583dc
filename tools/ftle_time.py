"""Throughput of the FTLE family (sar_runtime_ftle) on one GPU, one run: kernel times of both passes — k_ftle_flow over its bands and
k_ftle_gram — from the runtime's HIP events after a warm-up call, for the Henon map (a = 1.4, b = 0.3; x' = 1 - a x^2 + y, y' = b x)
on the plane x in [-2.5, 2.5], y in [-3, 6] at 256^2, 1024^2 and 4096^2 pixels with N = 16 and 64.

    python tools/ftle_time.py [--out profiles/ftle_time.json]

Prints one JSON line per call and writes them all to --out: the two kernel times, the launches of the first pass, the wall time of the
whole call (the read-back of the records, the host finish and the upload of stretch2 included), pixel-steps per second over the
first pass's time — an upper figure: a wave stops once all its 64 pixels have escaped —, and the map's statistics. No threshold,
nothing compared with a peak.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ftle_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    a, b = 1.4, 0.3
    c = np.zeros(30)
    c[0], c[2], c[5], c[11] = 1.0, -a, 1.0, b
    geo = dict(origin=(-2.5, -3.0, 0.0), du=(5.0, 0.0, 0.0), dv=(0.0, 9.0, 0.0))
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    S.ftle_map(rt, c, width=64, height=64, steps=8, **geo)            # warm-up: the code object
    results = []
    for size in (256, 1024, 4096):
        for steps in (16, 64):
            rt.enable_timing(True)
            t0 = time.perf_counter()
            m = S.ftle_map(rt, c, width=size, height=size, steps=steps, **geo)
            wall = time.perf_counter() - t0
            t = rt.last_timing()
            rt.enable_timing(False)
            results.append({"size": size, "steps": steps, "flow_ms": t.iterate_ms, "flow_launches": t.iterate_launches, "gram_ms": t.resolve_ms,
                            "wall_s": wall, "pixel_steps_per_s": size * size * steps / (t.iterate_ms * 1e-3),
                            "gram_pixels_per_s": size * size / (t.resolve_ms * 1e-3), "stats": m.stats})
            print(json.dumps(results[-1]), flush=True)
            del m
    rt.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/ftle_time.py", "build_id": S.load_library().sar_build_id().decode(),
                   "note": "one run, spread not measured", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
