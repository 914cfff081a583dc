"""Throughput of the unstable-manifold family (sar_runtime_manifold) on one GPU, one run: kernel time of k_manifold from the runtime's
HIP events after a warm-up call, for the Henon map (a = 1.4, b = 0.3; x' = 1 - a x^2 + y, y' = b x), the branch of the saddle inside
the attractor (period 2, delta 1e-6), drawn into a `--size`^2 image of x, y in [-1.5, 1.5], at S = 2^12, 2^16 and 2^20 samples and at
32 and 64 steps.

    python tools/manifold_time.py [--size 1024] [--out profiles/manifold_time.json]

Prints one JSON line per call and writes them all to --out: the kernel time, the wall time of the whole call (clearing and reading
back both images included), segments and plots per second over the kernel's time, and the record's counts — the long and dead
segments say where the curve was under-resolved. No threshold, nothing compared with a peak.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "manifold_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    a, b = 1.4, 0.3
    row_x, row_y = np.zeros(10), np.zeros(10)
    row_x[0], row_x[2], row_x[5], row_y[1] = 1.0, -a, 1.0, b
    cfg = S.Config.solar_sail(width=args.size, height=args.size).replace(
        coeff_x=row_x, coeff_y=row_y, coeff_z=np.zeros(10), center_camera=(0.0, 0.0, 0.0), rotation_axis=(0.0, 0.0, 1.0), rotation_angle=0.0,
        scale=1.0 / 3.0, angle=0.0)
    xs = (-(1.0 - b) + math.sqrt((1.0 - b) ** 2 + 4.0 * a)) / (2.0 * a)
    lam = -a * xs - math.sqrt(a * a * xs * xs + b)
    norm = math.hypot(lam, b)
    branch = [((xs, b * xs, 0.0), (-lam / norm, -b / norm, 0.0), 1e-6, 2)]
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    S.manifolds(rt, cfg, branch, samples=4096, steps=8)            # warm-up: the code object, the image buffers
    results = []
    for samples in (1 << 12, 1 << 16, 1 << 20):
        for steps in (32, 64):
            rt.enable_timing(True)
            t0 = time.perf_counter()
            m = S.manifolds(rt, cfg, branch, samples=samples, steps=steps)
            wall = time.perf_counter() - t0
            t = rt.last_timing()
            rt.enable_timing(False)
            r = m.records[0]
            rec = {f: int(r[f]) for f in r.dtype.names if f not in ("_pad", "a", "b")}
            segments = (samples - 1) * (steps + 1)
            results.append({"samples": samples, "steps": steps, "size": args.size, "kernel_ms": t.iterate_ms, "wall_s": wall,
                            "segments": segments, "segments_per_s": segments / (t.iterate_ms * 1e-3),
                            "pixels": rec["pixels"], "plots_inside_per_s": rec["pixels"] / (t.iterate_ms * 1e-3),
                            "manifold_pixels": int((m.count > 0).sum()), "record": rec})
            print(json.dumps(results[-1]), flush=True)
    rt.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/manifold_time.py", "build_id": S.load_library().sar_build_id().decode(),
                   "note": "one run, spread not measured", "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
