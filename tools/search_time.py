"""Throughput of the chaotic-map search (sar_runtime_search) on one GPU, with the numpy restatement's rate on the host next to it.

    python tools/search_time.py [--n 1048576] [--seed 1] [--steps 20000] [--transient 1000] [--host-n 4096] [--rocprof]

Prints one JSON line: candidates/s of the whole call (wall), the survivor fraction after the transient and the accepted fraction,
phase-1 (k_search_screen) and phase-2 (k_search_lyapunov) kernel times from the runtime's HIP events, and — with --rocprof — the
same two kernels' times from one `rocprofv3 --kernel-trace --stats` run of this script in a child process.
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def measure(args) -> dict:
    import strange_attractor_renderer_amd as S
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    kw = dict(seed=args.seed, steps=args.steps, transient=args.transient)
    S.search_attractors(rt, min(args.n, 65536), first=args.n, **kw)   # warm-up call: code objects, scratch
    rt.enable_timing(True)
    t0 = time.perf_counter()
    recs, stats = S.search_attractors(rt, args.n, **kw)
    wall = time.perf_counter() - t0
    t = rt.last_timing()
    rt.close()
    survivors = stats["tested"] - stats["diverged_transient"]
    return {"n": args.n, "seed": args.seed, "transient": args.transient, "steps": args.steps, "wall_s": wall,
            "candidates_per_s": args.n / wall, "survivor_fraction": survivors / args.n, "accepted_fraction": stats["accepted"] / args.n,
            "stats": stats, "events_ms": {"k_search_screen": t.warmup_ms, "k_search_lyapunov": t.iterate_ms,
                                         "lyapunov_launches": t.iterate_launches},
            "phase2_lane_steps_per_s": survivors * args.steps / (t.iterate_ms * 1e-3) if t.iterate_ms > 0 else None}


def rocprof(args) -> dict:
    """One child run under rocprofv3 --kernel-trace --stats: total / calls of the two search kernels."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "search", "-f", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--seed", str(args.seed), "--steps", str(args.steps),
               "--transient", str(args.transient), "--host-n", "0"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.rocprof_timeout)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exited {r.returncode}", "stderr_tail": r.stderr[-2000:]}
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv"}
        out = {}
        for row in csv.DictReader(open(files[0])):
            name = row.get("Name", "")
            for k in ("k_search_screen", "k_search_lyapunov"):
                if k in name:
                    out[k] = {"calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) * 1e-6,
                              "avg_ms": float(row["AverageNs"]) * 1e-6}
        return out


def host_rate(args) -> dict:
    import search_restatement as R
    t0 = time.perf_counter()
    R.search(args.seed, 0, args.host_n, transient=args.transient, steps=args.steps)
    dt = time.perf_counter() - t0
    return {"n": args.host_n, "seconds": dt, "candidates_per_s": args.host_n / dt}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20000)
    ap.add_argument("--transient", type=int, default=1000)
    ap.add_argument("--host-n", type=int, default=4096, help="candidates of the numpy restatement's timing on the host (0: none)")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--rocprof-timeout", type=float, default=600)
    args = ap.parse_args()
    res = measure(args)
    if args.host_n:
        res["host_restatement"] = host_rate(args)
    if args.rocprof:
        res["rocprofv3"] = rocprof(args)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
