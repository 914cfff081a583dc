"""Times the auto colour range (include/sar.h: sar_runtime_set_color_range) with HIP events on the runtime's stream: a whole-image
colorize with the mode off against the same colorize with it on (the difference is the select: five histogram passes and five
one-workgroup scans, plus what the window costs colorize itself), and auto exposure the same way for the same frame, at the
BASELINE shapes — 512^2 1e7 (configs[0]), 2048^2 1e9 (configs[1]), 1800x2000 1e9 (configs[2], Gas) and
4096^2 1e10 (configs[3]'s frame, here on one GPU) — and for a batch of 16 frames of
configs[4] (solar-sail, 1e8 iterations, 1800x2000, 65 536 jobs) in ONE sar_colorize_device_batch. Also prints the window the
default parameters give for each frame. --off-only times the colorize with both modes off and nothing else (the number to hold
against another build's).

    python tools/color_range_time.py [--reps 50] [--out color_range_time.json] [--off-only] [--shapes 0,1,2,3]
"""
import argparse
import json
import math
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _span(torch, stream, fn, reps):
    """median ms of fn() between two events on `stream` (fn only enqueues)."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(stream)
        fn()
        b.record(stream)
    stream.synchronize()
    ms = sorted(a.elapsed_time(b) for a, b in ev)
    return ms[len(ms) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default="")
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--shapes", default="0,1,2,3", help="which of the four single frames to time (the batch always is)")
    a = ap.parse_args()
    import torch
    import strange_attractor_renderer_amd as S
    from strange_attractor_renderer_amd.sequence import frame_seed
    rows = []
    frames = [("poisson_saturne", 512, 512, 10_000_000, "configs[0]"), ("poisson_saturne", 2048, 2048, 1_000_000_000, "configs[1]"),
              ("solar_sail", 1800, 2000, 1_000_000_000, "configs[2] (Gas)"), ("poisson_saturne", 4096, 4096, 10_000_000_000, "configs[3], one GPU")]
    for preset, w, h, iters, label in [frames[int(k)] for k in a.shapes.split(",") if k != ""]:
        cfg = getattr(S.Config, preset)(iterations=iters, width=w, height=h, scale=1.0, transparent=0)
        r = S.ParallelRenderer(device=0, seed=1)
        try:
            S.render_parallel(r, cfg, 12)           # warm
            t0 = time.perf_counter()
            S.render_parallel(r, cfg, 12)
            frame_ms = (time.perf_counter() - t0) * 1e3
            rt = r.runtime()
            dev = torch.empty(w * h * 4, dtype=torch.int16, device="cuda")
            torch.cuda.synchronize()
            st = torch.cuda.ExternalStream(rt.stream())
            off = _span(torch, st, lambda: S.colorize_device(cfg, rt, dev.data_ptr()), a.reps)
            row = dict(frame=f"{preset} {w}x{h} {iters:.0e} ({label})", frame_wall_ms=round(frame_ms, 3), colorize_ms=round(off, 4))
            if not a.off_only:
                c = S.color_range(cfg, rt)
                rt.set_color_range()
                on = _span(torch, st, lambda: S.colorize_device(cfg, rt, dev.data_ptr()), a.reps)
                rt.set_color_range(None)
                rt.set_exposure()
                expo = _span(torch, st, lambda: S.colorize_device(cfg, rt, dev.data_ptr()), a.reps)
                rt.set_exposure(None)
                row.update(colorize_ranged_ms=round(on, 4), color_range_ms=round(on - off, 4), exposure_ms=round(expo - off, 4),
                           color_range_pct_of_frame=round(100 * (on - off) / frame_ms, 2), lo=c.lo, hi=c.hi, covered=c.covered, applied=c.applied)
            rows.append(row)
        finally:
            r.shutdown()
        print(json.dumps(rows[-1]), flush=True)

    # a batch of 16 frames of configs[4]
    F, jobs, w, h = 16, 65536, 1800, 2000
    n = 100_000_000 // jobs
    cfgs = [S.Config.solar_sail(iterations=n * jobs, width=w, height=h, scale=1.0, transparent=0, jobs_total=jobs, angle=k * math.pi / 180.0)
            for k in range(F)]
    rts = S.Runtime.group(cfgs[0], F, device=0)
    try:
        starts = [S.start_points(frame_seed(4, k), 0, jobs) for k in range(F)]
        S.render_jobs_batch(cfgs, rts, starts)
        S.render_jobs_batch(cfgs, rts, starts)
        rts[0].synchronize()
        t0 = time.perf_counter()
        S.render_jobs_batch(cfgs, rts, starts)
        rts[0].synchronize()
        batch_ms = (time.perf_counter() - t0) * 1e3
        outs = [torch.empty(w * h * 4, dtype=torch.int16, device="cuda") for _ in range(F)]
        torch.cuda.synchronize()
        st = torch.cuda.ExternalStream(rts[0].stream())
        ptrs = [o.data_ptr() for o in outs]
        off = _span(torch, st, lambda: S.colorize_device_batch(cfgs, rts, ptrs), a.reps)
        row = dict(frame=f"configs[4] batch of {F}: solar_sail {w}x{h} 1e8, {jobs} jobs", batch_render_ms=round(batch_ms, 3),
                   colorize_batch_ms=round(off, 4), render_ms_per_frame=round(batch_ms / F, 4))
        if not a.off_only:
            for rt in rts:
                rt.set_color_range()
            on = _span(torch, st, lambda: S.colorize_device_batch(cfgs, rts, ptrs), a.reps)
            for rt in rts:
                rt.set_color_range(None)
                rt.set_exposure()
            expo = _span(torch, st, lambda: S.colorize_device_batch(cfgs, rts, ptrs), a.reps)
            recs = [S.color_range(c, rt) for c, rt in zip(cfgs, rts)]
            spread = {k: [min(getattr(e, k) for e in recs), max(getattr(e, k) for e in recs)] for k in ("lo", "hi", "covered")}
            row.update(colorize_batch_ranged_ms=round(on, 4), color_range_ms_per_frame=round((on - off) / F, 4),
                       exposure_ms_per_frame=round((expo - off) / F, 4), color_range_pct_of_frame=round(100 * (on - off) / batch_ms, 2),
                       first_frames=[dict(lo=e.lo, hi=e.hi, covered=e.covered, applied=e.applied) for e in recs[:3]],
                       range_over_the_batch=spread)
        rows.append(row)
        print(json.dumps(rows[-1]), flush=True)
    finally:
        for rt in rts:
            rt.close()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
