"""Throughput of the Lyapunov planes (sar_runtime_plane) on one GPU: a size x size plane in both modes, timed with the runtime's HIP
events around every k_plane launch, next to the search's phase-2 rate (7.3e10 lane-steps/s).

    python tools/plane_time.py [--size 1024] [--steps 20000] [--transient 1000] [--preset poisson_saturne] [--axes 0 13] [--d 0.3]

Prints one JSON line per mode: pixels/s, lane-steps/s (transient + tangent steps of every pixel that ran them, from the records:
transient_done + steps_done per pixel), the lanes' utilisation (the steps the lanes of an 8 x 8 tile did, over 64 times its
longest lane's: a wave runs until its last lane is done; --size must be a multiple of 8), the outcome counts and the wall time of
the whole call (records read back and finished on the host included).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEARCH_PHASE2_LANE_STEPS_PER_S = 7.3e10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--transient", type=int, default=1000)
    ap.add_argument("--preset", default="poisson_saturne")
    ap.add_argument("--axes", type=int, nargs=2, default=(0, 13))
    ap.add_argument("--d", type=float, default=0.3)
    ap.add_argument("--modes", nargs="+", default=["l1", "spectrum"])
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    cfg = getattr(S.Config, args.preset)()
    base = np.concatenate([cfg.coeff_x, cfg.coeff_y, cfg.coeff_z])
    xr, yr = [(base[a] - args.d, base[a] + args.d) for a in args.axes]
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    for mode in args.modes:
        S.lyapunov_plane(rt, base, args.axes, xr, yr, 64, 64, mode, transient=args.transient, steps=200)   # warm-up: code objects
        rt.enable_timing(True)
        t0 = time.perf_counter()
        pl = S.lyapunov_plane(rt, base, args.axes, xr, yr, args.size, args.size, mode, transient=args.transient, steps=args.steps)
        wall = time.perf_counter() - t0
        t = rt.last_timing()
        rt.enable_timing(False)
        npix = args.size * args.size
        lane_steps = int(pl.records["transient_done"].sum(dtype=np.uint64)) + int(pl.records["steps_done"].sum(dtype=np.uint64))
        tangent_steps = int(pl.records["steps_done"].sum(dtype=np.uint64))
        # lane utilisation: a wave (an 8 x 8 tile) runs as long as its longest lane; the steps its lanes did over 64 times that
        n = args.size // 8
        per = (pl.records["transient_done"].astype(np.int64) + pl.records["steps_done"]).reshape(n, 8, n, 8)
        util = per.sum() / (64.0 * per.max(axis=(1, 3)).sum())
        s = t.iterate_ms * 1e-3
        print(json.dumps({"mode": mode, "size": args.size, "transient": args.transient, "steps": args.steps, "preset": args.preset,
                          "axes": list(args.axes), "d": args.d, "kernel_ms": t.iterate_ms, "launches": t.iterate_launches,
                          "wall_s": wall, "pixels_per_s": npix / s, "lane_steps_per_s": lane_steps / s,
                          "tangent_lane_steps_per_s": tangent_steps / s,
                          "lane_utilisation": util, "active_lane_steps_per_s": lane_steps / s / util,
                          "vs_search_phase2": (lane_steps / s) / SEARCH_PHASE2_LANE_STEPS_PER_S, "stats": pl.stats}), flush=True)
    rt.close()


if __name__ == "__main__":
    main()
