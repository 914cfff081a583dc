"""Throughput of the cycles family (sar_runtime_cycles) on one GPU, one run: kernel time of k_cycles_newton and k_cycles_merge from
the runtime's HIP events after a warm-up call, on two workloads — `--columns` columns of a Henon line (a from 1.0 to 1.4, b = 0.3) at
p = 1, 2, 4, 8 from the default 512 starts, and `--candidates` maps of the search stream at p = 1.

    python tools/cycles_time.py [--columns 1024] [--candidates 4096] [--out profiles/cycles_time.json]

Prints one JSON line per call and writes them all to --out: the two kernel times, the wall time of the whole call (read-back
included), the starts by outcome, the orbits found, Newton iterations per second from the records' totals over the Newton kernel's
time, and the share of the Newton passes that went into starts that ended NOT_CONVERGED (each of those ran max_newton + 1 passes).
No threshold, nothing compared with a peak.
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
    ap.add_argument("--columns", type=int, default=1024)
    ap.add_argument("--candidates", type=int, default=4096)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cycles_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    line = np.zeros((args.columns, 30))
    line[:, 0], line[:, 5], line[:, 11] = 1.0, 0.3, 1.0        # x' = 1 - a x^2 + 0.3 y, y' = x
    line[:, 2] = -np.linspace(1.0, 1.4, args.columns)
    stream = np.stack([S.search_candidate(args.seed, i).reshape(30) for i in range(args.candidates)])
    calls = [("henon_line", line, p) for p in (1, 2, 4, 8)] + [("search_candidates", stream, 1)]
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    S.cycles(rt, line[:8], period=2)                            # warm-up: code objects, the LDS attribute
    results = []
    for name, maps, p in calls:
        rt.enable_timing(True)
        t0 = time.perf_counter()
        c = S.cycles(rt, maps, period=p)
        wall = time.perf_counter() - t0
        t = rt.last_timing()
        rt.enable_timing(False)
        rec = c.records
        total = {f: int(rec[f].sum(dtype=np.uint64)) for f in rec.dtype.names if f != "_pad"}
        starts = len(maps) * len(c.starts)
        passes = total["newton_iterations"] + starts          # a start that ends at iteration n ran n + 1 passes
        lost = total["not_converged"] * (c.params.max_newton + 1)
        results.append({"workload": name, "maps": len(maps), "starts_per_map": len(c.starts), "period": p,
                        "newton_kernel_ms": t.iterate_ms, "merge_kernel_ms": t.resolve_ms, "launches": t.iterate_launches, "wall_s": wall,
                        "totals": total, "newton_iterations_per_s": total["newton_iterations"] / (t.iterate_ms * 1e-3),
                        "newton_passes": passes, "map_steps_per_s": passes * p / (t.iterate_ms * 1e-3),
                        "share_of_passes_on_not_converged": lost / passes})
        print(json.dumps(results[-1]), flush=True)
    rt.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/cycles_time.py", "build_id": S.load_library().sar_build_id().decode(), "note": "one run, spread not measured",
                   "results": results}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
