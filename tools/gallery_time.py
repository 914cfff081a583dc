"""Tiles per second of the gallery (sar_runtime_gallery) on one GPU, next to the path that existed before it.

    python tools/gallery_time.py [--cases 1024x128 4096x64] [--search 65536] [--repeats 3] [--skip-frames]

The maps are what the search accepts among the first --search candidates of seed 1, cycled up to the tile count and framed
beforehand from their records' extents (frame_view_box), for both paths:

  (a) gallery      one sar_runtime_gallery call for all tiles at the defaults (1024 jobs, 2^20 iterations a tile). kernel_ms is
                   the runtime's HIP events around the k_gallery launches, wall_s the whole call (uploads, launches, the atlas
                   read back); the best of --repeats after one warm-up call.
  (b) frames       groups of 32 tile-sized runtimes (Runtime.group): reset_batch, render_jobs_batch, colorize_device_batch into
                   device memory, the group's stream waited for once per group; wall time of all groups, the best of --repeats
                   after one warm-up group. Tiles of different maps have different scales, so a group's frames do not share
                   launches (sar_render_jobs_batch then runs them one after the other): this is the path as a user gets it.

Prints one JSON line per case and path: tiles/s, iterations/s (counted iterations only; the warm-up's 1000 steps a job are
extra work both paths do) and the ratio.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FRAME_PATH_ITERATIONS_PER_S = 1.6e11   # README: the 2048^2 flagship frame


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["1024x128", "4096x64"], help="TILESxSIDE")
    ap.add_argument("--search", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--jobs", type=int, default=1024)
    ap.add_argument("--iterations", type=int, default=1 << 20)
    ap.add_argument("--skip-frames", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    import strange_attractor_renderer_amd as S

    base = S.Config.solar_sail()
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    recs, stats = S.search_attractors(rt, args.search, seed=1)
    coeffs = np.stack([S.search_candidate(1, int(c)).ravel() for c in recs["candidate"]])
    print(json.dumps({"maps": len(recs), "searched": args.search}), flush=True)
    for case in args.cases:
        n, side = (int(v) for v in case.split("x"))
        pick = np.arange(n) % len(recs)
        items = S.gallery_items(coeffs[pick], base=base, records=recs[pick], tile=(side, side))
        kw = dict(tile=(side, side), cols=32, jobs=args.jobs, iterations=args.iterations)
        counted = n * args.jobs * (args.iterations // args.jobs)
        S.gallery(rt, base, items[:64], **kw)                       # warm-up: code object, buffers
        best = None
        for _ in range(args.repeats):
            rt.enable_timing(True)
            t0 = time.perf_counter()
            g = S.gallery(rt, base, items, **kw)
            wall = time.perf_counter() - t0
            t = rt.last_timing()
            rt.enable_timing(False)
            if best is None or t.iterate_ms < best[0]:
                best = (t.iterate_ms, t.iterate_launches, wall)
        a = {"path": "gallery", "tiles": n, "side": side, "jobs": args.jobs, "iterations": args.iterations, "kernel_ms": best[0],
             "launches": best[1], "wall_s": best[2], "tiles_per_s_kernel": n / (best[0] * 1e-3), "tiles_per_s_wall": n / best[2],
             "iterations_per_s_kernel": counted / (best[0] * 1e-3), "vs_frame_path": counted / (best[0] * 1e-3) / FRAME_PATH_ITERATIONS_PER_S,
             "covered_mean": float(g.stats["covered"].mean()), "dead_jobs_mean": float(g.stats["dead_jobs"].mean())}
        print(json.dumps(a), flush=True)
        if args.skip_frames:
            continue
        F = 32
        cfgs = [g.config(i) for i in range(n)]
        starts = S.start_points(0, 0, args.jobs)
        rts = S.Runtime.group(cfgs[0], F, device=0)
        out = torch.empty((F, side, side, 4), dtype=torch.int16, device="cuda:0")
        ptrs = [out[i].data_ptr() for i in range(F)]

        def run(lo, hi):
            for first in range(lo, hi, F):
                m = min(F, hi - first)
                S.reset_batch(rts[:m])
                S.render_jobs_batch(cfgs[first:first + m], rts[:m], [starts] * m)
                S.colorize_device_batch(cfgs[first:first + m], rts[:m], ptrs[:m])
                rts[0].synchronize()

        run(0, min(F, n))                                            # warm-up group
        wall_b = None
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            run(0, n)
            w = time.perf_counter() - t0
            wall_b = w if wall_b is None else min(wall_b, w)
        for r in reversed(rts):
            r.close()
        print(json.dumps({"path": "frames", "tiles": n, "side": side, "group": F, "wall_s": wall_b, "tiles_per_s_wall": n / wall_b,
                          "iterations_per_s_wall": counted / wall_b, "gallery_speedup_wall": wall_b / best[2],
                          "gallery_speedup_kernel": wall_b / (best[0] * 1e-3)}), flush=True)
    rt.close()


if __name__ == "__main__":
    main()
