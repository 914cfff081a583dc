"""Throughput of the period planes (sar_runtime_period) on one GPU: a size x size Hénon plane and a size x size plane around
solar-sail at the defaults (transient 2000, max_period 256, eps 1e-9), timed with the runtime's HIP events around every k_period
launch after a warm-up call, next to lyapunov_plane in "l1" mode on the same plane in the same process.

    python tools/period_time.py [--size 1024] [--d 0.1] [--out profiles/period_time.json]

Prints one JSON line per plane and writes them all to --out: kernel time, pixels/s and map steps/s of both calls (the steps every
pixel ran, from the records: transient_done + steps_done), the lanes' utilisation of the period call (the steps the lanes of an 8 x 8
tile did over 64 times its longest lane's, that lane rounded up to the 16-step check of the return loop; --size must be a multiple
of 8), the outcome counts and the wall time of the whole call (records read back included).
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
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--d", type=float, default=0.1, help="half-width of the solar-sail plane around the preset's coefficients")
    ap.add_argument("--axes", type=int, nargs=2, default=(5, 22), help="swept coefficients of the solar-sail plane")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "period_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    henon = np.zeros(30)
    henon[0], henon[5] = 1.0, 1.0                 # x' = 1 - a x^2 + y, y' = b x: coefficient 2 is -a, coefficient 11 is b
    cfg = S.Config.solar_sail()
    sail = np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    planes = [("henon", henon, (2, 11), (-1.45, 0.0), (0.0, 0.4)),
              ("solar_sail", sail, tuple(args.axes), *[(sail[a] - args.d, sail[a] + args.d) for a in args.axes])]
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    n, results = args.size // 8, []
    for name, base, axes, xr, yr in planes:
        S.period_plane(rt, base, axes, xr, yr, 64, 64)                         # warm-up: code objects
        S.lyapunov_plane(rt, base, axes, xr, yr, 64, 64, "l1", steps=200)
        rt.enable_timing(True)
        t0 = time.perf_counter()
        pl = S.period_plane(rt, base, axes, xr, yr, args.size, args.size)
        wall = time.perf_counter() - t0
        t = rt.last_timing()
        rec = pl.records
        steps = int(rec["transient_done"].sum(dtype=np.uint64)) + int(rec["steps_done"].sum(dtype=np.uint64))
        tile = rec["steps_done"].astype(np.int64).reshape(n, 8, n, 8).max(axis=(1, 3))
        longest = rec["transient_done"].astype(np.int64).reshape(n, 8, n, 8).max(axis=(1, 3)) + (tile + 15) // 16 * 16
        t0 = time.perf_counter()
        ly = S.lyapunov_plane(rt, base, axes, xr, yr, args.size, args.size, "l1")
        ly_wall = time.perf_counter() - t0
        lt = rt.last_timing()
        rt.enable_timing(False)
        ly_steps = int(ly.records["transient_done"].sum(dtype=np.uint64)) + int(ly.records["steps_done"].sum(dtype=np.uint64))
        s, ls, npix = t.iterate_ms * 1e-3, lt.iterate_ms * 1e-3, args.size * args.size
        results.append({"plane": name, "size": args.size, "axes": list(axes), "x_range": list(map(float, xr)), "y_range": list(map(float, yr)),
                        "period": {"kernel_ms": t.iterate_ms, "launches": t.iterate_launches, "wall_s": wall, "pixels_per_s": npix / s,
                                   "map_steps": steps, "map_steps_per_s": steps / s, "lane_utilisation": steps / (64.0 * longest.sum()),
                                   "stats": pl.stats},
                        "lyapunov_l1": {"kernel_ms": lt.iterate_ms, "launches": lt.iterate_launches, "wall_s": ly_wall,
                                        "pixels_per_s": npix / ls, "map_steps": ly_steps, "map_steps_per_s": ly_steps / ls,
                                        "stats": ly.stats},
                        "kernel_time_ratio_l1_over_period": lt.iterate_ms / t.iterate_ms,
                        "step_count_ratio_l1_over_period": ly_steps / steps})
        print(json.dumps(results[-1]), flush=True)
    rt.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/period_time.py", "build_id": S.load_library().sar_build_id().decode(), "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
