/* examples/sensor_noise_closed_loop.c -- a closed loop under sensor noise, without the host in the loop.
 *
 * 4 096 planar double integrators (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) start from ONE
 * state and are driven to the origin: 60 MPC steps fused into one kernel launch.  The plant is the model itself, but the controller
 * never sees its state: at every step it solves from a reading that is off by a few centimetres and centimetres per second, every
 * instance its own sequence (tiny_batch_set_measurement_noise), while the state is handed on from the TRUE one.  The state log (option
 * "state_log") holds those true states; the program prints the spread of the end states with the noise installed and, the episode run
 * again, without it -- where all instances end in one point.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/sensor_noise_closed_loop.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o sensor_noise_closed_loop && ./sensor_noise_closed_loop
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

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

/* mean, standard deviation and largest value of the positions' distance from the origin in one row [BATCH][NX] of the state log */
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
    const double dt = 0.1;
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
    CHECK(tiny_batch_set_option(h, "state_log", 1));             /* ... and every true state of it kept */

    /* every instance its own readings: v [STEPS][BATCH][NX], positions off by up to 3 cm, velocities by up to 5 cm/s */
    double* v = (double*)malloc(sizeof(double) * (size_t)STEPS * BATCH * NX);
    double* log = (double*)malloc(sizeof(double) * (size_t)STEPS * BATCH * NX);
    if (!v || !log) return 1;
    srand(17);
    for (size_t e = 0; e < (size_t)STEPS * BATCH * NX; ++e) v[e] = (e % NX) < 2 ? uniform(-0.03, 0.03) : uniform(-0.05, 0.05);
    const double start[NX] = {1.5, -1.0, 0.0, 0.0};

    double mean[2], sd[2], worst[2];
    for (int run = 0; run < 2; ++run) {                          /* 0: noisy readings, 1: the exact state */
        if (run == 0) CHECK(tiny_batch_set_measurement_noise(h, v, STEPS, TINY_HOST));
        else CHECK(tiny_batch_set_measurement_noise(h, NULL, 0, TINY_HOST));
        CHECK(tiny_batch_reset(h));
        CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
        CHECK(tiny_batch_solve(h));
        CHECK(tiny_batch_get_state_log(h, log, STEPS));          /* [STEPS][BATCH][NX]: the last row is the end state */
        spread(log + (size_t)(STEPS - 1) * BATCH * NX, &mean[run], &sd[run], &worst[run]);
        printf("%s: %d instances x %d MPC steps in one launch, kernel path %d, sequence of %ld steps, applied %ld\n", run == 0 ? "noisy" : "exact", BATCH,
               STEPS, tiny_batch_kernel_path(h), tiny_batch_get_option(h, "measurement_noise"), tiny_batch_get_option(h, "last_measurement_noise"));
        printf("       distance from the origin after %.0f s: mean %.5f m, standard deviation %.3e m, largest %.5f m\n", STEPS * dt, mean[run], sd[run],
               worst[run]);
    }
    free(v);
    free(log);
    tiny_batch_destroy(h);
    /* with the exact state the batch ends in one point; the noise spreads it, and the controller still keeps every instance near home */
    return (sd[1] < 1e-12 && sd[0] > 1e-6 && worst[0] < 0.5 && worst[1] < 0.2) ? 0 : 2;
}
