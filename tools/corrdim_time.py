"""Throughput of the correlation dimension (sar_runtime_corrdim, sar_runtime_pairs) on one GPU.

    python tools/corrdim_time.py [--repeats 3] [--out profiles/corrdim_time.json]

Times the two kernels from the runtime's HIP events (the best of --repeats, after one warm-up call) at two shapes — one map of 32 768
points (256 jobs x 128 samples: 5.4e8 pairs) and 1024 maps of 4096 points (64 x 64: 8.6e9 pairs), Henon maps with a between 1.36 and
1.4 — and reports pairs per second of k_corr_pairs next to the fp64 floor: a pair costs 8 fp64 instructions (three subtracts, three
multiplies, two adds; nothing fuses), and a CU issues 64 fp64 lanes per clock, so the floor is CUs x 64 x clock / 8 pairs per second.
With the hooks build it also times the pair kernel on a cloud of uniform random points and on a set whose points are all the same (every
pair in one bin) with 32 copies of the LDS histogram and with 1: what the copies are for. Prints one JSON record and writes it to --out.
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

CUS, FP64_LANES_PER_CU_CLOCK, CLOCK_HZ = 256, 64, 2.4e9     # MI355X: 256 CUs of 4 SIMDs x 16 fp64 lanes, 2.4 GHz peak engine clock
FP64_PER_PAIR = 8


def henon(a=1.4):
    import numpy as np
    c = np.zeros((3, 10))
    c[0, 0], c[0, 2], c[0, 5] = 1.0, -a, 1.0
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
        if best is None or t.iterate_ms < best["k_corr_pairs_ms"]:
            best = {"k_corr_pairs_ms": t.iterate_ms, "k_corr_orbit_ms": t.warmup_ms, "pair_launches": t.iterate_launches, "wall_s": wall}
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corrdim_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    from strange_attractor_renderer_amd import _abi
    hooks = os.path.exists(_abi.HOOKS_PATH)
    if hooks:
        _abi.use_hooks_build()
    if S.device_count() <= 0:
        raise SystemExit("corrdim_time needs a HIP device: a time from anywhere else says nothing")
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    floor = CUS * FP64_LANES_PER_CU_CLOCK * CLOCK_HZ / FP64_PER_PAIR
    cases = []
    for name, coeffs, kw in (("1 map x 32768 points", henon(), dict(jobs=256, samples=128, stride=4)),
                             ("1024 maps x 4096 points", np.stack([henon(1.36 + 0.04 * k / 1023) for k in range(1024)]),
                              dict(jobs=64, samples=64, stride=4))):
        best, res = best_of(rt, args.repeats, lambda: S.correlation_dimension(rt, coeffs, **kw))
        pairs = int(res.records["counted"].sum())
        steps = res.hist.shape[0] * kw["jobs"] * (1000 + kw["stride"] * kw["samples"])
        best.update(case=name, pairs=pairs, bounded=int((res.status == 0).sum()), maps=int(res.hist.shape[0]),
                    pairs_per_s=pairs / (best["k_corr_pairs_ms"] * 1e-3), map_steps_per_s=steps / (best["k_corr_orbit_ms"] * 1e-3),
                    d2_median=float(np.nanmedian(res.d2)))
        best["share_of_fp64_floor"] = best["pairs_per_s"] / floor
        cases.append(best)
    ab = []
    if hooks:
        lib = S.load_library()
        n = 32768
        rng = np.random.default_rng(1)
        for name, pts in (("uniform cloud", rng.random((n, 3))), ("one point 32768 times", np.full((n, 3), 0.25))):
            for copies in (0, 1):
                lib.sar_runtime_set_test_option(rt.handle, b"corr_replicas", copies)
                best, _ = best_of(rt, args.repeats, lambda: S.pair_histogram(rt, pts))
                ab.append({"case": name, "copies": 32 if copies == 0 else copies, "k_corr_pairs_ms": best["k_corr_pairs_ms"],
                           "pairs_per_s": n * (n - 1) / 2 / (best["k_corr_pairs_ms"] * 1e-3)})
        lib.sar_runtime_set_test_option(rt.handle, b"corr_replicas", 0)
    rt.close()
    res = {"tool": "tools/corrdim_time.py", "repeats": args.repeats, "build_id": S.load_library().sar_build_id().decode(), "cases": cases,
           "lds_copies_ab": ab,
           "fp64_floor": {"pairs_per_s": floor, "fp64_instructions_per_pair": FP64_PER_PAIR, "cus": CUS,
                          "fp64_lanes_per_cu_clock": FP64_LANES_PER_CU_CLOCK, "clock_hz": CLOCK_HZ}}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
