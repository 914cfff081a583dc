/* sar_color_range.c — the auto colour range of include/sar.h from a COMPILED C99 program, with no Python in the process:
 * measure, set the mode, colorize, hold, colorize, and the window as AdjustedVelocity constants. tests/test_gpu_color_range.py
 * builds it with gcc, runs it against the product library and compares the files it writes with the Python path's results.
 *
 *   sar_color_range <out_dir> <width> <height> <jobs> <iters_per_job> <seed>
 * exit code: 0 ok, 3 no HIP device (SAR_ERR_NO_DEVICE surfaced as a status, nothing crashed), 1 anything else. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sar.h"

static int fail(const char* what, int st) {
    fprintf(stderr, "%s: %s (%d): %s\n", what, sar_status_string(st), st, sar_last_error());
    return st == SAR_ERR_NO_DEVICE ? 3 : 1;
}
#define CHECK(call) do { int st_ = (call); if (st_ != SAR_OK) return fail(#call, st_); } while (0)
#define REFUSED(call) do { if ((call) != SAR_ERR_INVALID) { fprintf(stderr, "%s was not refused\n", #call); return 1; } } while (0)

static int dump(const char* dir, const char* name, const void* p, size_t bytes) {
    char path[1024];
    snprintf(path, sizeof path, "%s/%s", dir, name);
    FILE* f = fopen(path, "wb");
    if (!f) return 1;
    const size_t w = fwrite(p, 1, bytes, f);
    fclose(f);
    return w == bytes ? 0 : 1;
}

int main(int argc, char** argv) {
    if (argc != 7) { fprintf(stderr, "usage: %s out_dir width height jobs iters_per_job seed\n", argv[0]); return 1; }
    const char* dir = argv[1];
    const uint32_t W = (uint32_t)atoi(argv[2]), H = (uint32_t)atoi(argv[3]), jobs = (uint32_t)atoi(argv[4]);
    const uint64_t n = (uint64_t)atoll(argv[5]), seed = (uint64_t)atoll(argv[6]);
    if (sar_abi_version() != SAR_ABI_VERSION || SAR_ABI_VERSION < 10) { fprintf(stderr, "ABI mismatch\n"); return 1; }
    const size_t npix = (size_t)W * H;

    /* host only: the defaults, the refusals, the window as constants of the colour transform */
    sar_color_range_params p, bad;
    CHECK(sar_color_range_params_default(&p));
    if (p.q_lo != 0.01 || p.q_hi != 0.99 || p.pos_lo != 0. || p.pos_hi != 1.) { fprintf(stderr, "defaults\n"); return 1; }
    bad = p;
    bad.q_lo = 0.995;
    REFUSED(sar_runtime_set_color_range(NULL, &bad));
    REFUSED(sar_renderer_set_color_range(NULL, &bad));
    sar_config cfg, vel;
    CHECK(sar_config_solar_sail(&cfg));
    const sar_color_range by_hand = {-0.5, -0.25, 0., 1., 0u, 1};
    CHECK(sar_color_range_to_velocity(&cfg, &by_hand, &vel));
    if (vel.ct_offset != cfg.ct_offset - by_hand.lo / cfg.ct_factor || vel.ct_factor != cfg.ct_factor / (by_hand.hi - by_hand.lo)) {
        fprintf(stderr, "sar_color_range_to_velocity: other constants\n");
        return 1;
    }

    cfg.width = W; cfg.height = H; cfg.transparent = 0; cfg.seed = seed; cfg.scale = 1.0;
    cfg.jobs_total = jobs; cfg.iterations = (uint64_t)jobs * n;
    CHECK(sar_config_validate(&cfg));
    sar_runtime* rt = NULL;
    CHECK(sar_runtime_new(&cfg, 0, &rt));
    CHECK(sar_render_jobs(&cfg, rt, NULL));            /* start points from the runtime's stream (seed) */
    uint16_t* rgba = malloc(npix * 8);
    if (!rgba) return 1;

    /* measure (waits) */
    sar_color_range rec[2];
    CHECK(sar_runtime_color_range(&cfg, rt, NULL, &rec[0]));      /* NULL: the defaults */
    p.q_lo = 0.1; p.q_hi = 0.9; p.pos_lo = 1.0; p.pos_hi = 0.25;   /* a reversed part of the palette */
    CHECK(sar_runtime_color_range(&cfg, rt, &p, &rec[1]));
    if (dump(dir, "records.bin", rec, sizeof rec)) return 1;
    CHECK(sar_color_range_to_velocity(&cfg, &rec[0], &vel));
    const double constants[2] = {vel.ct_offset, vel.ct_factor};
    if (dump(dir, "velocity.bin", constants, sizeof constants)) return 1;
    REFUSED(sar_color_range_to_velocity(&cfg, &rec[1], &vel));    /* positions other than (0, 1) */

    /* no mode, no hold: the image as ever */
    CHECK(sar_colorize(&cfg, rt, rgba));
    if (dump(dir, "rgba_plain.bin", rgba, npix * 8)) return 1;
    /* the mode: the frame's own window, on the device */
    CHECK(sar_runtime_set_color_range(rt, &p));
    CHECK(sar_colorize(&cfg, rt, rgba));
    if (dump(dir, "rgba_mode.bin", rgba, npix * 8)) return 1;
    REFUSED(sar_colorize_range_device(&cfg, rt, 0, (uint32_t)(npix / 2), rgba));   /* refused before the pointer matters */
    /* the hold: one window, nothing measured; it ends the mode */
    CHECK(sar_runtime_hold_color_range(rt, &rec[0]));
    CHECK(sar_colorize(&cfg, rt, rgba));
    if (dump(dir, "rgba_hold.bin", rgba, npix * 8)) return 1;
    CHECK(sar_runtime_set_color_range(rt, NULL));       /* ends the mode only: the hold stays */
    CHECK(sar_colorize(&cfg, rt, rgba));
    if (dump(dir, "rgba_hold_again.bin", rgba, npix * 8)) return 1;
    CHECK(sar_runtime_hold_color_range(rt, NULL));
    CHECK(sar_colorize(&cfg, rt, rgba));
    if (dump(dir, "rgba_off.bin", rgba, npix * 8)) return 1;
    CHECK(sar_runtime_free(rt));

    /* the renderer's switch: render_parallel colorizes through the shard-0 runtime */
    sar_renderer* r = NULL;
    CHECK(sar_renderer_new(0, jobs, seed, &r));         /* units = jobs, 1 job per unit: the same jobs */
    CHECK(sar_renderer_set_color_range(r, &p));
    CHECK(sar_render_parallel(r, &cfg, 1, rgba));
    if (dump(dir, "rgba_parallel.bin", rgba, npix * 8)) return 1;
    CHECK(sar_renderer_shutdown(r));
    free(rgba);
    puts("ok");
    return 0;
}
