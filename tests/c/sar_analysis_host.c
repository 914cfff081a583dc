/* The host-only companions of the analysis families from C99, no device: sar_pairs_edges, sar_corrdim_fit and sar_boxdim_fit over
 * windows of 0, 2 and 3 usable bins / levels (a line needs 3), sar_plane_coeffs against sar_period_coeffs on the same sweep, and
 * -0.0 in the base. Prints "ok", or the line of the first check that failed. tests/test_analysis_refusals_host.py links it
 * against the product; linked against host objects compiled with -fsanitize=address,undefined it is the sanitizer run of this code. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "sar.h"

#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            fprintf(stderr, "line %d: %s (last error: %s)\n", __LINE__, #cond, sar_last_error());       \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

int main(void) {
    /* the edges of the default binning, and a histogram whose first bin already holds c_lo pairs */
    uint32_t bins = 0;
    CHECK(sar_pairs_edges(NULL, &bins, NULL) == SAR_OK && bins == 290);
    double* r = malloc(bins * sizeof(double));
    uint64_t* hist = calloc(bins, sizeof(uint64_t));
    CHECK(r && hist && sar_pairs_edges(NULL, &bins, r) == SAR_OK && isinf(r[bins - 1]));
    for (uint32_t b = 0; b + 1 < bins; ++b) {
        CHECK(r[b] > 0. && (b == 0 || r[b] > r[b - 1]));
        hist[b] = 100 + 3 * b * b;
    }
    /* r_hi = r[k]: bins 1 .. k are usable */
    const uint32_t usable[] = {0, 2, 3, 288};
    for (int i = 0; i < 4; ++i) {
        sar_corrdim_line line;
        memset(&line, 0xAB, sizeof(line));
        CHECK(sar_corrdim_fit(hist, NULL, 10., r[usable[i]], &line) == SAR_OK);
        if (usable[i] < 3) {
            CHECK(line.status == SAR_CORRDIM_NO_WINDOW && line.used == 0 && isnan(line.slope) && isnan(line.intercept) && isnan(line.rms));
        } else {
            CHECK(line.status == SAR_CORRDIM_FIT_OK && line.used == usable[i] && line.first_bin == 1 && line.last_bin == usable[i]);
            CHECK(isfinite(line.slope) && line.slope > 0. && isfinite(line.intercept) && line.rms >= 0.);
        }
    }
    sar_corrdim_line line;
    CHECK(sar_corrdim_fit(hist, NULL, 1e30, r[100], &line) == SAR_OK && line.status == SAR_CORRDIM_NO_WINDOW);  /* c_lo never reached */
    sar_pairs_params coarse;
    CHECK(sar_pairs_params_default(&coarse) == SAR_OK);
    coarse.sub_bits = 0;
    coarse.e_min = -2;
    coarse.e_max = 2;  /* 6 bins: 4 usable at the most */
    CHECK(sar_pairs_edges(&coarse, &bins, r) == SAR_OK && bins == 6 && r[0] == 0.5 && r[4] == 2. && isinf(r[5]));
    CHECK(sar_corrdim_fit(hist, &coarse, 10., 100., &line) == SAR_OK && line.status == SAR_CORRDIM_FIT_OK && line.used == 4);
    free(r);
    free(hist);

    /* levels 0 .. 8 of 1000 points, 2^l cells at level l: with min_occupancy 4 the levels up to 7 are usable */
    sar_box_level levels[9];
    for (uint32_t l = 0; l <= 8; ++l) {
        levels[l].cells = 1u << l;
        levels[l].singles = 0;
        levels[l].sum_sq = 1000000u >> l;
        CHECK(sar_box_log2_q32(1000u >> l, &levels[l].n_log_n) == SAR_OK);
        levels[l].n_log_n *= 1000;
    }
    const uint32_t l_min[] = {8, 6, 5, 1};  /* 0, 2, 3 and 7 usable levels */
    for (int i = 0; i < 4; ++i) {
        sar_boxdim_lines lines;
        memset(&lines, 0xAB, sizeof(lines));
        CHECK(sar_boxdim_fit(levels, 8, 1000, l_min[i], 4., &lines) == SAR_OK);
        if (i < 2) {
            CHECK(lines.status == SAR_BOXDIM_NO_WINDOW && lines.used == 0 && isnan(lines.d0.slope) && isnan(lines.d1.rms) && isnan(lines.d2.intercept));
        } else {
            CHECK(lines.status == SAR_BOXDIM_FIT_OK && lines.used == 8 - l_min[i] && lines.first_level == l_min[i] && lines.last_level == 7);
            CHECK(fabs(lines.d0.slope - 1.) < 1e-12 && fabs(lines.d2.slope - 1.) < 1e-2 && isfinite(lines.d1.slope) && lines.d0.rms < 1e-12);
        }
    }

    /* one sweep through both families: the same 30 doubles, bit for bit, at every pixel; -0.0 in the base comes out as +0.0 */
    sar_plane_params pl;
    sar_period_params pe;
    CHECK(sar_plane_params_default(&pl) == SAR_OK && sar_period_params_default(&pe) == SAR_OK);
    for (int j = 0; j < 30; ++j) pl.base[j] = pe.base[j] = j == 5 ? -0. : 0.01 * j - 0.1;
    pl.axis[0] = pe.axis[0] = 7;
    pl.axis[1] = pe.axis[1] = 22;
    pl.lo[0] = pe.lo[0] = -0.3;
    pl.hi[0] = pe.hi[0] = 0.7;
    pl.lo[1] = pe.lo[1] = 1.;
    pl.hi[1] = pe.hi[1] = -1.;
    pl.width = pe.width = 5;
    pl.height = pe.height = 3;
    for (uint32_t y = 0; y < 3; ++y)
        for (uint32_t x = 0; x < 5; ++x) {
            double a[30], b[30];
            CHECK(sar_plane_coeffs(&pl, x, y, a) == SAR_OK && sar_period_coeffs(&pe, x, y, b) == SAR_OK);
            CHECK(memcmp(a, b, sizeof(a)) == 0 && a[5] == 0. && !signbit(a[5]) && a[3] == pl.base[3]);
            CHECK((x != 0 || a[7] == -0.3) && (x != 4 || a[7] == 0.7) && (y != 0 || a[22] == -1.) && (y != 2 || a[22] == 1.));
        }
    pl.width = pe.width = 1;  /* a single column sits at lo */
    double one[30];
    CHECK(sar_plane_coeffs(&pl, 0, 1, one) == SAR_OK && one[7] == -0.3 && sar_period_coeffs(&pe, 0, 1, one) == SAR_OK && one[7] == -0.3);
    CHECK(sar_plane_coeffs(&pl, 1, 0, one) == SAR_ERR_INVALID && sar_period_coeffs(&pe, 0, 3, one) == SAR_ERR_INVALID);
    printf("ok\n");
    return 0;
}
