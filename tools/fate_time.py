"""Throughput of the basin probes (sar_runtime_basin_fates, sar_runtime_basin_uncertainty) on one GPU.

    python tools/fate_time.py [--repeats 3] [--size 512] [--out profiles/fate_time.json]

Times k_basin_ladder and k_basin_fate from the runtime's HIP events (the best of --repeats, after one warm-up call; the spread over
the repeats is recorded) on three maps, each with a basin picture of --size x --size pixels, 1000 + 64 steps, grid 32:

  henon        the Henon map a = 1.4, b = 0.3 (z' = 0.5 z) over [-2.5, 2.5]^2: a fractal boundary between the attractor and escape;
  pitchfork    x' = 1.5 x - x y, y' = x^2 over [-2, 2] x [-0.5, 2.5]: two mirror basins and escape;
  solar-sail   the preset over [-0.5, 0.5]^2 at z = 0.05.

k_basin_ladder runs 2^14, 2^16 and 2^18 base points x K = 24 (49 probes each), k_basin_fate 2^20 points. Next to them stands
k_basin_screen of the same call's picture — the same map, the same steps, one lane per pixel in 8 x 8 tiles: probes per second against
pixels per second. The ratio is reported, not asserted, and so is the alpha each case's default fit gives. Prints one JSON record and
writes it to --out.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LEVELS = 24


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fate_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    if S.device_count() <= 0:
        raise SystemExit("fate_time needs a HIP device: a time from anywhere else says nothing")
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)

    henon = np.zeros(30)
    henon[0], henon[2], henon[5], henon[11], henon[28] = 1.0, -1.4, 1.0, 0.3, 0.5
    pitchfork = np.zeros(30)
    pitchfork[1], pitchfork[3], pitchfork[12], pitchfork[28] = 1.5, -1.0, 1.0, 0.5
    sail = S.Config.solar_sail()
    maps = [("henon", henon, dict(origin=(-2.5, -2.5, 0.05), du=(5.0, 0.0, 0.0), dv=(0.0, 5.0, 0.0))),
            ("pitchfork", pitchfork, dict(origin=(-2.0, -0.5, 0.05), du=(4.0, 0.0, 0.0), dv=(0.0, 3.0, 0.0))),
            ("solar-sail", np.concatenate([sail.coeff_x, sail.coeff_y, sail.coeff_z]), dict(origin=(-0.5, -0.5, 0.05), du=(1.0, 0.0, 0.0), dv=(0.0, 1.0, 0.0)))]

    def timed(call):
        """(result, best kernel ms, slowest kernel ms, launches) of `call` over the repeats, after one warm-up call."""
        call()
        times, res, launches = [], None, 0
        for _ in range(args.repeats):
            rt.enable_timing(True)
            res = call()
            t = rt.last_timing()
            rt.enable_timing(False)
            times.append(t.iterate_ms)
            launches = t.iterate_launches
        return res, min(times), max(times), launches

    cases = []
    for name, coeffs, window in maps:
        kw = dict(width=args.size, height=args.size, transient=1000, steps=64, grid=32, **window)
        S.basin_map(rt, coeffs, **kw)   # warm-up call
        screen = []
        for _ in range(args.repeats):
            rt.enable_timing(True)
            b = S.basin_map(rt, coeffs, **kw)
            screen.append(rt.last_timing().warmup_ms)   # k_basin_screen of the picture itself (the call behind the grid = 1 pass)
            rt.enable_timing(False)
        npix = args.size * args.size
        case = {"case": name, "pixels": npix, "transient": 1000, "steps": 64, "grid": 32, "attractors": b.n_attractors,
                "bounded_share": b.stats["bounded"] / npix, "k_basin_screen_ms": min(screen), "k_basin_screen_ms_max": max(screen),
                "pixels_per_s": npix / (min(screen) * 1e-3), "levels": LEVELS, "ladders": []}
        for log2n in (14, 16, 18):
            n = 1 << log2n
            u, best, worst, launches = timed(lambda: b.uncertainty(n=n, levels=LEVELS, seed=1))
            probes = n * (1 + 2 * LEVELS)
            rec = {"base_points": n, "probes": probes, "k_basin_ladder_ms": best, "k_basin_ladder_ms_max": worst, "launches": launches,
                   "probes_per_s": probes / (best * 1e-3), "probes_over_pixels": probes / (best * 1e-3) / case["pixels_per_s"],
                   "uncertain": [int(v) for v in u.levels["uncertain"]], "unknown": [int(v) for v in u.levels["unknown"]],
                   "eps0": float(u.params.eps0)}
            try:
                fit = u.fit()
                rec.update(alpha=fit.alpha, alpha_err=fit.alpha_err, fit_levels=[int(k) for k in fit.levels], boundary_dimension=fit.boundary_dimension(2))
            except ValueError as e:
                rec.update(alpha=None, fit_levels=[], no_fit=str(e))
            case["ladders"].append(rec)
        pts = u.base[np.arange(1 << 20) % len(u.base)] + np.random.default_rng(2).random((1 << 20, 3)) * 1e-3
        f, best, worst, launches = timed(lambda: b.fates(pts))
        case["fates"] = {"points": len(pts), "k_basin_fate_ms": best, "k_basin_fate_ms_max": worst, "launches": launches,
                         "points_per_s": len(pts) / (best * 1e-3), "points_over_pixels": len(pts) / (best * 1e-3) / case["pixels_per_s"],
                         "diverged": int((f["status"] != 0).sum()), "unknown": int((f["label"] == S.BASIN_UNKNOWN).sum())}
        cases.append(case)
    rt.close()
    out = {"tool": "tools/fate_time.py", "build_id": S.load_library().sar_build_id().decode(), "repeats": args.repeats, "cases": cases}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
