"""Throughput of box counting (sar_runtime_boxes) on one GPU.

    python tools/boxdim_time.py [--repeats 3] [--out profiles/boxdim_time.json]

Times the box kernels (k_box_insert and the 16 launches of k_box_level) from the runtime's HIP events — the best of --repeats, after
one warm-up call — at 2^20 points and 16 levels on two sets: points of the Henon map (nearly every point in a cell of its own at the
finest level: the hash tables at their fullest) and a period-2 set (two cells: what the combining of equal keys within a wave is
for). Then it times the box kernels and k_corr_pairs on the same 32 768 Henon points: O(n levels) against O(n^2). Prints one JSON
record and writes it to --out. The figures are a record, not a gate.
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


def henon():
    import numpy as np
    c = np.zeros((3, 10))
    c[0, 0], c[0, 2], c[0, 5] = 1.0, -1.4, 1.0
    c[1, 1] = 0.3
    c[2, 8] = 0.5
    return c.reshape(30)


def best_of(rt, repeats, call):
    call()   # warm-up call: code object, buffers
    best = None
    for _ in range(repeats):
        rt.enable_timing(True)
        t0 = time.perf_counter()
        out = call()
        wall = time.perf_counter() - t0
        t = rt.last_timing()
        rt.enable_timing(False)
        if best is None or t.iterate_ms < best["kernels_ms"]:
            best = {"kernels_ms": t.iterate_ms, "launches": t.iterate_launches, "wall_s": wall}
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boxdim_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    if S.device_count() <= 0:
        raise SystemExit("boxdim_time needs a HIP device: a time from anywhere else says nothing")
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)

    n = 1 << 20
    res = S.box_dimension(rt, henon(), jobs=1024, samples=1024, stride=1, points=True)
    rec = res.records[0]
    two = np.empty((n, 3))
    two[0::2], two[1::2] = (0.25, 0.5, 0.75), (0.75, 0.25, 0.5)
    cases = []
    for name, pts, origin, size in (("henon, 2^20 points", res.points[0], rec["origin"], float(rec["size"])),
                                    ("period 2, 2^20 points", two, (0.0, 0.0, 0.0), 1.0)):
        best, rows = best_of(rt, args.repeats, lambda: S.box_counts(rt, pts, origin=origin, size=size, levels=16))
        best.update(case=name, points=n, levels=16, cells_finest=int(rows["cells"][16]), points_per_s=n / (best["kernels_ms"] * 1e-3))
        cases.append(best)
    cases[0].update(d0=float(res.d0[0]), d1=float(res.d1[0]), d2=float(res.d2[0]))

    small = S.box_dimension(rt, henon(), jobs=256, samples=128, stride=4, points=True)
    pts, srec = small.points[0], small.records[0]
    box, _ = best_of(rt, args.repeats, lambda: S.box_counts(rt, pts, origin=srec["origin"], size=float(srec["size"]), levels=16))
    pairs, hist = best_of(rt, args.repeats, lambda: S.pair_histogram(rt, pts))
    against = {"points": int(pts.shape[0]), "box_kernels_ms": box["kernels_ms"], "box_launches": box["launches"],
               "k_corr_pairs_ms": pairs["kernels_ms"], "pairs": int(hist.sum()), "pairs_over_boxes": pairs["kernels_ms"] / box["kernels_ms"]}
    rt.close()
    out = {"tool": "tools/boxdim_time.py", "repeats": args.repeats, "build_id": S.load_library().sar_build_id().decode(), "cases": cases,
           "against_k_corr_pairs": against}
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
