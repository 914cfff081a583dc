"""Throughput of the power spectra (sar_runtime_spectrum) on one GPU.

    python tools/spectrum_time.py [--repeats 3] [--columns 1024] [--label NAME] [--append] [--out profiles/spectrum_time.json]

Times k_spectrum, k_spectrum_fold and k_corr_orbit from the runtime's HIP events (the best of --repeats, after one warm-up call) on
--columns maps of the logistic line r = 2.8 .. 4.0 (past r = 4 a map leaves the bound box and has no spectrum), 16 jobs x 15 segments
each, at N = 256, 1024 and 4096 with hop N / 2, and reports k_spectrum next to k_corr_orbit of the same call and next to two floors
of its own work:

  fp64   a segment is N / 2 * log2(N) butterflies of 10 fp64 instructions (4 multiplies, 6 adds; nothing fuses) and about 13 N more
         (the plotted value 5, the two pairwise sums 3, the taper 2, the periodogram 3 per bin); a CU issues 64 fp64 lanes per clock.
  LDS    a butterfly reads and writes 4 doubles; the bit-reversed stores, the pairwise sums, the clearing of im[] and the periodogram
         move about 6 N doubles more in and 5 N out. ds_read_b64 moves 256 B per clock and CU, ds_write_b64 about 85.

Both floors assume every CU busy. A variant built without the LDS padding (SAR_EXTRA_FLAGS=-DSAR_SPECTRUM_PAD=0, python -m
strange_attractor_renderer_amd.build --variant nopad, loaded through SAR_LIBRARY) run with --label nopad --append adds its record to
the same file: what the padding is worth. Prints one JSON record and writes it to --out.
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

CUS, FP64_LANES_PER_CU_CLOCK, CLOCK_HZ = 256, 64, 2.4e9     # MI355X: 256 CUs of 4 SIMDs x 16 fp64 lanes, 2.4 GHz peak engine clock
LDS_READ_B_PER_CLOCK, LDS_WRITE_B_PER_CLOCK = 256.0, 85.0   # per CU: ds_read_b64, ds_write_b64
JOBS, SEGMENTS = 16, 15


def floors(n, segments_total):
    log2n = int(math.log2(n))
    fp64 = segments_total * (n // 2 * log2n * 10 + 13 * n)
    read = segments_total * 8 * (n // 2 * log2n * 4 + 6 * n)
    written = segments_total * 8 * (n // 2 * log2n * 4 + 5 * n)
    return {"fp64_instructions": fp64, "fp64_floor_ms": fp64 / (CUS * FP64_LANES_PER_CU_CLOCK * CLOCK_HZ) * 1e3,
            "lds_bytes_read": read, "lds_bytes_written": written,
            "lds_floor_ms": (read / LDS_READ_B_PER_CLOCK + written / LDS_WRITE_B_PER_CLOCK) / (CUS * CLOCK_HZ) * 1e3}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--columns", type=int, default=1024)
    ap.add_argument("--label", default="product")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spectrum_time.json"))
    args = ap.parse_args()
    import numpy as np
    import strange_attractor_renderer_amd as S
    if S.device_count() <= 0:
        raise SystemExit("spectrum_time needs a HIP device: a time from anywhere else says nothing")
    rt = S.Runtime(S.Config.solar_sail(width=64, height=64), device=0)
    coeffs = np.zeros((args.columns, 30))
    r = np.linspace(2.8, 4.0, args.columns)
    coeffs[:, 1], coeffs[:, 2] = r, -r
    starts = np.zeros((JOBS, 3))
    starts[:, 0] = 0.1 + 0.8 * (np.arange(JOBS) + 0.5) / JOBS
    cases = []
    for n in (256, 1024, 4096):
        call = lambda: S.power_spectrum(rt, coeffs, starts=starts, jobs=JOBS, segments=SEGMENTS, n=n, hop=n // 2)
        call()   # warm-up call: code object, buffers
        best = None
        for _ in range(args.repeats):
            rt.enable_timing(True)
            t0 = time.perf_counter()
            res = call()
            wall = time.perf_counter() - t0
            t = rt.last_timing()
            rt.enable_timing(False)
            if best is None or t.iterate_ms < best["k_spectrum_ms"]:
                best = {"k_spectrum_ms": t.iterate_ms, "k_spectrum_fold_ms": t.resolve_ms, "k_corr_orbit_ms": t.warmup_ms,
                        "spectrum_launches": t.iterate_launches, "wall_s": wall}
        bounded = int((res.status == 0).sum())
        segments_total = bounded * JOBS * SEGMENTS
        samples = (SEGMENTS - 1) * (n // 2) + n
        best.update(n=n, hop=n // 2, maps=args.columns, bounded=bounded, jobs=JOBS, segments=SEGMENTS, samples_per_job=samples,
                    segments_per_s=segments_total / (best["k_spectrum_ms"] * 1e-3),
                    map_steps_per_s=args.columns * JOBS * (1000 + samples) / (best["k_corr_orbit_ms"] * 1e-3),
                    flatness_median=float(np.median(res.flatness[res.status == 0])), **floors(n, segments_total))
        best["share_of_fp64_floor"] = best["fp64_floor_ms"] / best["k_spectrum_ms"]
        best["share_of_lds_floor"] = best["lds_floor_ms"] / best["k_spectrum_ms"]
        cases.append(best)
    rt.close()
    run = {"label": args.label, "library": os.environ.get("SAR_LIBRARY", "product"), "build_id": S.load_library().sar_build_id().decode(),
           "repeats": args.repeats, "cases": cases}
    res = {"tool": "tools/spectrum_time.py", "runs": [],
           "machine": {"cus": CUS, "fp64_lanes_per_cu_clock": FP64_LANES_PER_CU_CLOCK, "clock_hz": CLOCK_HZ,
                       "lds_read_bytes_per_cu_clock": LDS_READ_B_PER_CLOCK, "lds_write_bytes_per_cu_clock": LDS_WRITE_B_PER_CLOCK}}
    if args.append and os.path.exists(args.out):
        with open(args.out) as f:
            res["runs"] = json.load(f).get("runs", [])
    res["runs"].append(run)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
