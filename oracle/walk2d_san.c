/*
 * walk2d_san.c -- stand-alone check of the oracle's 2D walk under the sanitizers (`make -C oracle
 * walk2d-san` builds and runs it).  TEST INFRASTRUCTURE ONLY, not a pytest: it links
 * eikonal_oracle.c with -fsanitize=undefined,float-cast-overflow,address and runs the walks whose
 * coordinates leave the range of the index type -- walks that leave through each side of the
 * raster, points in (-1, 0), starts at NaN, +-inf, -1, 2^31, 2^32 - 0.5 and 2^32 + 5.5 on either
 * axis, a step to -inf, the NaN fallback's wrapped node read -- and checks status and row count.
 * Any sanitizer report aborts.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int orc_gdm2d_events(const double *T, int64_t H, int64_t W, double ix, double iy, double ex, double ey, double tau,
                     double *out, int64_t max_out, int64_t *n_out, int *status, int exact, int64_t max_steps,
                     int64_t *ev);

enum { H = 12, W = 14, CAP = 30004 };
static double T[H * W], out[2 * CAP];
static int failed;

static void fill(double cx, double cy) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) T[y * W + x] = cx * x + cy * y;
}

static void walk(const char *name, double sx, double sy, double ex, double ey, int want_st, int64_t want_n) {
    for (int exact = 0; exact < 2; ++exact) {
        int64_t n = -1, ev[12];
        int st = -1;
        int rc = orc_gdm2d_events(T, H, W, sx, sy, ex, ey, 0.5, out, CAP, &n, &st, exact, 0, ev);
        const int ok = st == want_st && n == want_n;
        printf("%-18s exact %d rc %d status %d n %lld (want %d, %lld) steps %lld exit %lld  %s\n", name, exact, rc, st,
               (long long)n, want_st, (long long)want_n, (long long)ev[0], (long long)ev[9], ok ? "ok" : "FAILED");
        if (!ok) failed = 1;
    }
}

int main(void) {
    const double bad[] = {NAN, INFINITY, -INFINITY, -1.0, 2147483648.0, 4294967295.5, 4294967301.5, -1e300, 1e300};
    char name[32];
    fill(1.0, 0.0); /* T = x: the walk that read 32 GB past the field through the unchecked cast */
    walk("leave_x0", 3.2, 5.5, 12, 10, 2, 10);
    walk("neg_cell_x", 2.2, 5.5, -2.2, 5.5, 0, 8);
    walk("start_m1eps_x", -1.0 + 0x1p-52, 5.5, 1, 5.5, 2, 2);
    for (unsigned q = 0; q < sizeof bad / sizeof *bad; ++q) {
        snprintf(name, sizeof name, "start_x_%.11g", bad[q]);
        walk(name, bad[q], 5.5, 1, 5.5, 2, 1);
    }
    walk("start_last_col", 13.0, 5.5, 8, 5.5, 2, 1);
    fill(-1.0, 0.0);
    walk("leave_xhi", 10.2, 5.5, 2, 2, 2, 7);
    fill(0.0, 1.0);
    walk("leave_y0", 5.5, 3.2, 12, 10, 2, 10);
    walk("neg_cell_y", 5.5, 2.2, 5.5, -2.2, 0, 8);
    for (unsigned q = 0; q < sizeof bad / sizeof *bad; ++q) {
        snprintf(name, sizeof name, "start_y_%.11g", bad[q]);
        walk(name, 5.5, bad[q], 5.5, 1, 2, 1);
    }
    walk("start_last_row", 5.5, 11.0, 5.5, 6, 2, 1);
    fill(0.0, -1.0);
    walk("leave_yhi", 5.5, 8.2, 2, 2, 2, 7);
    /* a step to (-inf, NaN): row 0 holds 2^-950 x, row 1 is 2^-10, the rows below fall from -2^-10 */
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x) T[y * W + x] = y == 0 ? 0x1p-950 * x : y == 1 ? 0x1p-10 : -0x1p-10 * (y - 1);
    walk("step_to_minus_inf", 5.5, 0.5, 1, 0.5, 2, 2);
    /* the NaN fallback at a low edge: rint = -1 wraps to the last column (finite, then +inf) */
    fill(1.0, 0.0);
    T[5 * W + 0] = INFINITY;
    walk("wrap_low_x", -0.7, 5.3, 5, 5, 1, 1);
    T[5 * W + W - 1] = INFINITY;
    walk("wrap_low_x_inf", -0.7, 5.3, 5, 5, 1, 0);
    printf(failed ? "FAILED\n" : "walk2d_san: all walks as expected, no sanitizer report\n");
    return failed;
}
