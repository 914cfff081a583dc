"""Throughput of the recurrence analysis (sar_runtime_rqa) on one GPU.

    python tools/rqa_time.py [--repeats 3] [--columns 1024] [--label NAME] [--append] [--out profiles/rqa_time.json]

Times k_rqa_diag, k_rqa_vert and k_corr_orbit from the runtime's HIP events (the best of --repeats, after one warm-up call) on

  henon      the Henon map, 16 jobs of T = 1024, 4096 and 16384 points: chaos, most lines of length 1, all in one bin;
  period 2   the logistic map at r = 3.2, 16 jobs of 4096 points: half of all diagonals are one long line each;
  columns    --columns maps of the logistic line r = 2.8 .. 4.0, 4 jobs of 1024 points each: many short trajectories.

Next to k_rqa_diag stands k_corr_pairs (sar_runtime_pairs) on the same points, every trajectory a set of its own: it evaluates the
same distances, T^2 / 2 per trajectory where k_rqa_diag walks T^2 / 2 and k_rqa_vert T^2. The ratio is reported, not asserted. A
variant built with one copy of the LDS histogram (SAR_EXTRA_FLAGS=-DSAR_RQA_REPLICAS=1, python -m
strange_attractor_renderer_amd.build --variant onecopy, loaded through SAR_LIBRARY) run with --label onecopy --append adds its record
to the same file: what the copies are worth. Prints one JSON record and writes it to --out.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--columns", type=int, default=1024)
    ap.add_argument("--label", default="product")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rqa_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    if S.device_count() <= 0:
        raise SystemExit("rqa_time needs a HIP device: a time from anywhere else says nothing")
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)

    def logistic(r):
        c = np.zeros((np.size(r), 30))
        c[:, 1], c[:, 2] = r, -np.asarray(r)
        return c

    henon = np.zeros((1, 30))
    henon[0, 0], henon[0, 2], henon[0, 5], henon[0, 11], henon[0, 28] = 1.0, -1.4, 1.0, 0.3, 0.5

    def starts(jobs):
        s = np.zeros((jobs, 3))
        s[:, 0] = 0.1 + 0.8 * (np.arange(jobs) + 0.5) / jobs
        return s

    shapes = [("henon", henon, 16, 1024), ("henon", henon, 16, 4096), ("henon", henon, 16, 16384), ("period 2", logistic([3.2]), 16, 4096),
              ("columns", logistic(np.linspace(2.8, 4.0, args.columns)), 4, 1024)]
    cases = []
    for name, coeffs, jobs, samples in shapes:
        call = lambda: S.recurrence_analysis(rt, coeffs, starts=starts(jobs), jobs=jobs, samples=samples, theiler=1, points=True)
        call()   # warm-up call: code object, buffers
        best = None
        for _ in range(args.repeats):
            rt.enable_timing(True)
            t0 = time.perf_counter()
            res = call()
            wall = time.perf_counter() - t0
            t = rt.last_timing()
            rt.enable_timing(False)
            if best is None or t.iterate_ms < best["k_rqa_diag_ms"]:
                best = {"k_rqa_diag_ms": t.iterate_ms, "k_rqa_vert_ms": t.resolve_ms, "k_corr_orbit_ms": t.warmup_ms,
                        "diag_launches": t.iterate_launches, "wall_s": wall}
        # the yardstick: the pair histogram of the same points, a trajectory a set
        sets = res.points[res.status == 0].reshape(-1, samples, 3)
        pairs = lambda: S.pair_histogram(rt, sets, theiler=1)
        pairs()
        pairs_ms = None
        for _ in range(args.repeats):
            rt.enable_timing(True)
            pairs()
            t = rt.last_timing()
            rt.enable_timing(False)
            pairs_ms = t.iterate_ms if pairs_ms is None else min(pairs_ms, t.iterate_ms)
        counts = res.records["counts"]
        walked = int(counts["pairs"].sum())
        m = res.measures()
        best.update(case=name, maps=int(coeffs.shape[0]), bounded=int((res.status == 0).sum()), jobs=jobs, samples=samples, theiler=1,
                    line_bins=int(res.params.line_bins), diag_entries=walked, recurrences=int(counts["recurrences"].sum()),
                    diag_lines=int(counts["diag_lines"].sum()), lines_of_length_1=int(res.diag[:, 1].sum()),
                    diag_entries_per_s=walked / (best["k_rqa_diag_ms"] * 1e-3), vert_entries_per_s=2 * walked / (best["k_rqa_vert_ms"] * 1e-3),
                    k_corr_pairs_ms=pairs_ms, pairs_per_s=walked / (pairs_ms * 1e-3), diag_over_pairs=best["k_rqa_diag_ms"] / pairs_ms,
                    vert_over_pairs=best["k_rqa_vert_ms"] / pairs_ms, rr_median=float(np.nanmedian(m["rr"])),
                    det_median=float(np.nanmedian(m["det"])), lam_median=float(np.nanmedian(m["lam"])))
        cases.append(best)
    rt.close()
    run = {"label": args.label, "library": os.environ.get("SAR_LIBRARY", "product"), "build_id": S.load_library().sar_build_id().decode(),
           "repeats": args.repeats, "cases": cases}
    out = {"tool": "tools/rqa_time.py", "runs": []}
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            out["runs"] = json.load(f).get("runs", [])
    out["runs"].append(run)
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
