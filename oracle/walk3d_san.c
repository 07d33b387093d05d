/*
 * walk3d_san.c -- stand-alone check of the oracle's 3D walk under the sanitizers (`make -C oracle
 * walk3d-san` builds and runs it).  TEST INFRASTRUCTURE ONLY, not a pytest: it links
 * eikonal_oracle.c with -fsanitize=undefined,float-cast-overflow,address and runs the walks whose
 * coordinates leave the range of the index type -- a walk that leaves through a low face, NaN
 * starts, a step to +inf / -inf -- and checks status and point count.  Any sanitizer report aborts.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

int orc_gdm3d_events(const double *T, int64_t H, int64_t W, int64_t L, const double *init, const double *end,
                     double tau, double *out, int64_t max_out, int64_t *n_out, int *status, int64_t *ev);
double orc_interp3(double px, double py, double pz, const double *M_, int64_t m, int64_t n, int64_t o, int *err);

enum { H = 10, W = 12, L = 9, CAP = 30004 };
static double T[H * W * L], out[3 * CAP];
static int failed;

static void fill(double cx, double cy, double cz) {
    for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
            for (int z = 0; z < L; ++z) T[(y * W + x) * L + z] = cx * x + cy * y + cz * z;
}

static void walk(const char *name, double sx, double sy, double sz, double ex, double ey, double ez, int want_st,
                 int64_t want_n) {
    const double init[3] = {sx, sy, sz}, end[3] = {ex, ey, ez};
    int64_t n = -1, ev[6];
    int st = -1;
    int rc = orc_gdm3d_events(T, H, W, L, init, end, 0.5, out, CAP, &n, &st, ev);
    const int ok = st == want_st && n == want_n;
    printf("%-16s rc %d status %d n %lld (want %d, %lld) steps %lld normalised %lld  %s\n", name, rc, st, (long long)n,
           want_st, (long long)want_n, (long long)ev[5], (long long)ev[4], ok ? "ok" : "FAILED");
    if (!ok) failed = 1;
}

int main(void) {
    fill(1e-3, 2e-3, 0.0); /* the flat field: 20 normalised steps, then y = -1.444 */
    walk("leave_flat", 9.5, 7.5, 4.5, 2, 2, 4, 2, 21);
    fill(3.0, 0.0, 0.0); /* 2.2 -> 0.7 -> -0.8 -> -2.3 */
    walk("leave_low", 2.2, 5, 4, 6, 2, 4, 2, 4);
    fill(-3.0, 0.0, 0.0);
    walk("leave_high", 8.2, 5, 4, 6, 2, 4, 2, 3);
    fill(-3e300, 0.0, 0.0); /* one step to 1.5e300, far past every integer type */
    walk("leave_far", 8.2, 5, 4, 6, 2, 4, 2, 2);
    fill(1.0, 0.05, 0.03);
    walk("nan_start", NAN, 5, 4, 1, 5, 4, 2, 1);
    walk("nan_start_all", NAN, NAN, NAN, 1, 5, 4, 2, 1);
    walk("inf_start", INFINITY, 5, 4, 1, 5, 4, 2, 1);
    walk("neg_inf_start", 3, -INFINITY, 4, 1, 5, 4, 2, 1);
    T[(5 * W + 4) * L + 5] = INFINITY; /* one +inf cell: a gradient of -inf, a step to x = +inf */
    walk("inf_cell", 9, 5, 5, 1, 5, 5, 2, 14);
    fill(1.0, 0.05, 0.03);
    T[(5 * W + (W - 1 - 4)) * L + 5] = INFINITY;
    for (int y = 0; y < H; ++y) /* the mirror image: x -> W - 1 - x */
        for (int x = 0; x < W; ++x)
            for (int z = 0; z < L; ++z)
                if (isfinite(T[(y * W + x) * L + z])) T[(y * W + x) * L + z] = (W - 1 - x) + 0.05 * y + 0.03 * z;
    walk("inf_cell_mirror", 2, 5, 5, 10, 5, 5, 2, 15);
    int err = 0;
    const double probe[] = {-1.0, -1.3, -1e300, 1e300, 4294967298.5, NAN, INFINITY, -INFINITY, -0.5};
    for (unsigned q = 0; q < sizeof probe / sizeof *probe; ++q) {
        double v = orc_interp3(probe[q], 5, 4, T, H, W, L, &err);
        printf("interp3 x = %-12g err %d value %g\n", probe[q], err, v);
    }
    printf(failed ? "FAILED\n" : "walk3d_san: all walks as expected, no sanitizer report\n");
    return failed;
}
