/* examples/monte_carlo_closed_loop.c -- a Monte-Carlo study of a closed loop under process noise, without the host in the loop.
 *
 * 4 096 planar double integrators (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) start from ONE
 * state and are driven to the origin: 60 MPC steps fused into one kernel launch, the plant stepped on the GPU.  Every instance has its
 * own disturbance sequence (tiny_batch_set_disturbance): at every plant step a gust kicks its velocities, w[k][i] ~ N(0, sigma^2).
 * The same episode is run again without the sequence; the program prints the spread of the final states of both.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/monte_carlo_closed_loop.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o monte_carlo_closed_loop && ./monte_carlo_closed_loop
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "tinympc_amd.h"

#define NX 4
#define NU 2
#define NH 10
#define BATCH 4096
#define STEPS 60

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ < 0) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, tiny_batch_last_error(h)); return 1; } \
    } while (0)

/* a standard normal number (Box-Muller on rand()) */
static double gauss(void) {
    const double u1 = (rand() + 1.0) / (RAND_MAX + 2.0), u2 = (rand() + 1.0) / (RAND_MAX + 2.0);
    return sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
}

/* mean and standard deviation of the final positions' distance from the origin */
static void spread(const double* x, double* mean, double* sd, double* worst) {
    double s = 0.0, s2 = 0.0;
    *worst = 0.0;
    for (int b = 0; b < BATCH; ++b) {
        const double d = hypot(x[b * NX + 0], x[b * NX + 1]);
        s += d;
        if (d > *worst) *worst = d;
    }
    *mean = s / BATCH;
    for (int b = 0; b < BATCH; ++b) {                  /* (two passes: identical instances give exactly 0) */
        const double d = hypot(x[b * NX + 0], x[b * NX + 1]) - *mean;
        s2 += d * d;
    }
    *sd = sqrt(s2 / BATCH);
}

int main(void) {
    const double dt = 0.1, sigma = 0.05;                /* velocity kick per step: 0.05 m/s */
    /* column-major A (nx x nx), B (nx x nu): states (px, py, vx, vy) */
    double A[NX * NX] = {0}, B[NX * NU] = {0}, Q[NX] = {10, 10, 1, 1}, R[NU] = {0.5, 0.5};
    for (int i = 0; i < NX; ++i) A[i + NX * i] = 1.0;
    A[0 + NX * 2] = dt; A[1 + NX * 3] = dt;
    B[0 + NX * 0] = 0.5 * dt * dt; B[2 + NX * 0] = dt;
    B[1 + NX * 1] = 0.5 * dt * dt; B[3 + NX * 1] = dt;

    TinyBatch* h = NULL;
    int rc = tiny_batch_setup(&h, A, B, NULL, Q, R, 1.0, NX, NU, NH, BATCH, 0, 0);
    if (rc) { fprintf(stderr, "tiny_batch_setup failed (%d): no MI355X?\n", rc); return 1; }

    /* box constraints, replicated over the horizon: |v| <= 2 m/s, |a| <= 1 m/s^2 */
    double xmin[NX * NH], xmax[NX * NH], umin[NU * (NH - 1)], umax[NU * (NH - 1)];
    for (int k = 0; k < NH; ++k)
        for (int i = 0; i < NX; ++i) { xmax[i + NX * k] = i < 2 ? 1e17 : 2.0; xmin[i + NX * k] = -xmax[i + NX * k]; }
    for (int e = 0; e < NU * (NH - 1); ++e) { umax[e] = 1.0; umin[e] = -1.0; }
    CHECK(tiny_batch_set_bound_constraints(h, xmin, xmax, umin, umax));
    CHECK(tiny_batch_update_settings(h, 1e-3, 1e-3, 100, 1, 1, 1, 0, 0, 0, 0, 0, 0));
    CHECK(tiny_batch_set_option(h, "steps_per_launch", STEPS));  /* the whole episode in one kernel launch */

    /* every instance its own gusts: w [STEPS][BATCH][NX], step-major; positions are not kicked */
    double* w = (double*)calloc((size_t)STEPS * BATCH * NX, sizeof(double));
    double* x = (double*)malloc(sizeof(double) * BATCH * NX);
    if (!w || !x) return 1;
    srand(7);
    for (size_t e = 0; e < (size_t)STEPS * BATCH; ++e) { w[e * NX + 2] = sigma * gauss(); w[e * NX + 3] = sigma * gauss(); }
    const double start[NX] = {1.5, -1.0, 0.0, 0.0};

    double mean[2], sd[2], worst[2];
    for (int run = 0; run < 2; ++run) {                          /* 0: under the gusts, 1: the perfect model following itself */
        CHECK(tiny_batch_set_disturbance(h, run == 0 ? w : NULL, run == 0 ? STEPS : 0, TINY_HOST));
        CHECK(tiny_batch_reset(h));
        CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
        CHECK(tiny_batch_solve(h));
        CHECK(tiny_batch_get(h, TINY_F_X0, x, TINY_HOST));       /* the plant state after the episode */
        spread(x, &mean[run], &sd[run], &worst[run]);
        printf("%s: %d instances x %d MPC steps in one launch, kernel path %d, disturbance applied %ld, rows used %ld\n",
               run == 0 ? "gusts   " : "no gusts", BATCH, STEPS, tiny_batch_kernel_path(h), tiny_batch_get_option(h, "last_disturbance"),
               tiny_batch_get_option(h, "disturbance_step"));
        printf("          distance from the origin after %.0f s: mean %.5f m, standard deviation %.3e m, largest %.5f m\n", STEPS * dt, mean[run],
               sd[run], worst[run]);
    }
    free(w);
    free(x);
    tiny_batch_destroy(h);
    /* the undisturbed batch ends in one point; the gusts spread it, and the controller holds the spread small */
    return (sd[1] < 1e-12 && sd[0] > 1e-4 && worst[0] < 0.5 && worst[1] < 0.2) ? 0 : 2;
}
