/* examples/closed_loop_score.c -- a closed-loop study that comes back with its outcome: four numbers per instance, no log.
 *
 * 4 096 planar point-mass vehicles (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) hold a hover
 * point at the origin for 60 MPC steps, fused into one kernel launch.  Every instance flies in its own gusts (an additive disturbance
 * on the velocities, tiny_batch_set_disturbance), reads its position through a sensor of its own quality
 * (tiny_batch_set_measurement_noise) and solves from the estimate of its own steady-state Kalman filter (tiny_batch_set_estimator).
 * What the study asks is what the realised flight cost and whether the vehicle left its corridor: tiny_batch_set_score installs the
 * stage weights [Q | R], the hover point as the target and every instance's own corridor -- |position| within 5 .. 20 cm, |velocity|
 * within 0.5 m/s, |acceleration| within 0.95 m/s^2 --, and the launch accumulates cost, worst violation, violated steps and first
 * violation on the device.  Neither the state log nor the step log is switched on.  The program prints the share of instances that ever
 * left their corridor, the largest violation and the minimum, median and maximum of the cost.
 *
 * With a file name as its argument the program flies the same episode once more WITHOUT the score and with both logs on, and writes
 * the setup and the logs there (ints STEPS, BATCH, NX, NU; doubles weight | target | lo | hi [BATCH][NX+NU] each, states
 * [STEPS][BATCH][NX], u0 [STEPS][BATCH][NU]): what a caller had to pull to the host before, and what tests/test_gpu_score.py scores
 * with the Python reference.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/closed_loop_score.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o closed_loop_score && ./closed_loop_score
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "tinympc_amd.h"

#define NX 4
#define NU 2
#define NZ (NX + NU)
#define NH 10
#define BATCH 4096
#define STEPS 60

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ < 0) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, tiny_batch_last_error(h)); return 1; } \
    } while (0)

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }
static int by_value(const void* a, const void* b) { return (*(const double*)a > *(const double*)b) - (*(const double*)a < *(const double*)b); }

/* the steady-state Kalman gain of ONE axis (examples/output_feedback_closed_loop.c): L [2] */
static void kalman_gain(double dt, double r, double w_p, double w_v, double L[2]) {
    double p00 = 1.0, p01 = 0.0, p11 = 1.0;
    for (int it = 0; it < 500; ++it) {
        const double s = p00 + r;
        L[0] = p00 / s; L[1] = p01 / s;
        const double q00 = p00 - L[0] * p00, q01 = p01 - L[0] * p01, q11 = p11 - L[1] * p01;
        p00 = q00 + 2.0 * dt * q01 + dt * dt * q11 + w_p;
        p01 = q01 + dt * q11;
        p11 = q11 + w_v;
    }
}

int main(int argc, char** argv) {
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

    /* the controller's own box, replicated over the horizon: |v| <= 2 m/s, |a| <= 1 m/s^2 */
    double xmin[NX * NH], xmax[NX * NH], umin[NU * (NH - 1)], umax[NU * (NH - 1)];
    for (int k = 0; k < NH; ++k)
        for (int i = 0; i < NX; ++i) { xmax[i + NX * k] = i < 2 ? 1e17 : 2.0; xmin[i + NX * k] = -xmax[i + NX * k]; }
    for (int e = 0; e < NU * (NH - 1); ++e) { umax[e] = 1.0; umin[e] = -1.0; }
    CHECK(tiny_batch_set_bound_constraints(h, xmin, xmax, umin, umax));
    CHECK(tiny_batch_update_settings(h, 1e-3, 1e-3, 100, 1, 1, 1, 0, 0, 0, 0, 0, 0));
    CHECK(tiny_batch_set_option(h, "steps_per_launch", STEPS));  /* the whole episode in one kernel launch */

    const size_t rows = (size_t)STEPS * BATCH;
    double* w = (double*)malloc(sizeof(double) * rows * NX);
    double* v = (double*)malloc(sizeof(double) * rows * NX);
    double* M = (double*)calloc((size_t)BATCH * NX * NX, sizeof(double));
    double* setup = (double*)malloc(sizeof(double) * 4 * BATCH * NZ);
    double* cost = (double*)malloc(sizeof(double) * BATCH);
    double* worst = (double*)malloc(sizeof(double) * BATCH);
    int* steps = (int*)malloc(sizeof(int) * BATCH);
    int* first = (int*)malloc(sizeof(int) * BATCH);
    if (!w || !v || !M || !setup || !cost || !worst || !steps || !first) return 1;
    double *weight = setup, *target = setup + (size_t)BATCH * NZ, *lo = setup + 2 * (size_t)BATCH * NZ, *hi = setup + 3 * (size_t)BATCH * NZ;
    srand(29);
    const double start[NX] = {0.0, 0.0, 0.0, 0.0};
    for (int b = 0; b < BATCH; ++b) {
        const double gust = uniform(0.02, 0.12), amp = uniform(0.005, 0.02), corridor = uniform(0.05, 0.2);
        double L[2];
        kalman_gain(dt, amp * amp / 3.0, 1e-6, gust * gust / 3.0, L);
        double* Mb = M + (size_t)b * NX * NX;
        Mb[0 + NX * 0] = L[0]; Mb[2 + NX * 0] = L[1];
        Mb[1 + NX * 1] = L[0]; Mb[3 + NX * 1] = L[1];
        for (int k = 0; k < STEPS; ++k) {
            double *wr = w + ((size_t)k * BATCH + b) * NX, *vr = v + ((size_t)k * BATCH + b) * NX;
            wr[0] = 0.0; wr[1] = 0.0; wr[2] = uniform(-gust, gust); wr[3] = uniform(-gust, gust);        /* gusts push the velocities */
            vr[0] = uniform(-amp, amp); vr[1] = uniform(-amp, amp); vr[2] = 0.0; vr[3] = 0.0;            /* the position is measured */
        }
        for (int c = 0; c < NZ; ++c) {
            const size_t at = (size_t)b * NZ + c;
            weight[at] = c < NX ? Q[c] : R[c - NX];
            target[at] = 0.0;
            hi[at] = c < 2 ? corridor : c < NX ? 0.5 : 0.95;
            lo[at] = -hi[at];
        }
    }
    CHECK(tiny_batch_set_disturbance(h, w, STEPS, TINY_HOST));
    CHECK(tiny_batch_set_measurement_noise(h, v, STEPS, TINY_HOST));
    CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
    CHECK(tiny_batch_set_estimator(h, M, TINY_HOST));            /* (the estimate starts at x0) */
    CHECK(tiny_batch_set_score(h, weight, target, lo, hi, TINY_HOST));
    CHECK(tiny_batch_solve(h));
    CHECK(tiny_batch_get_score(h, cost, worst, steps, first));
    printf("score: %d instances x %d MPC steps in one launch, kernel path %d, score %ld (applied %ld, counter %ld), state_log %ld\n", BATCH, STEPS,
           tiny_batch_kernel_path(h), tiny_batch_get_option(h, "score"), tiny_batch_get_option(h, "last_score"), tiny_batch_get_option(h, "score_step"),
           tiny_batch_get_option(h, "state_log"));
    int violated = 0, earliest = STEPS;
    long violated_steps = 0;
    double largest = 0.0;
    for (int b = 0; b < BATCH; ++b) {
        if (steps[b] > 0) { ++violated; violated_steps += steps[b]; if (first[b] < earliest) earliest = first[b]; }
        if (worst[b] > largest) largest = worst[b];
    }
    qsort(cost, BATCH, sizeof(double), by_value);
    printf("score: %d of %d instances ever left their corridor (%.1f %%), %ld violated steps, the earliest at step %d\n", violated, BATCH, 100.0 * violated / BATCH,
           violated_steps, earliest);
    printf("score: largest violation %.17g\n", largest);
    printf("score: cost minimum %.17g median %.17g maximum %.17g\n", cost[0], cost[BATCH / 2], cost[BATCH - 1]);

    if (argc > 1) {                                              /* what it took before: both logs, pulled to the host */
        double* states = (double*)malloc(sizeof(double) * rows * NX);
        double* u0 = (double*)malloc(sizeof(double) * rows * NU);
        int* iters = (int*)malloc(sizeof(int) * rows);
        if (!states || !u0 || !iters) return 1;
        CHECK(tiny_batch_reset(h));
        CHECK(tiny_batch_set_score(h, NULL, NULL, NULL, NULL, TINY_HOST));
        CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
        CHECK(tiny_batch_set_estimator(h, NULL, TINY_HOST));
        CHECK(tiny_batch_set_estimator(h, M, TINY_HOST));        /* (installed afresh: the estimate starts at x0 again) */
        CHECK(tiny_batch_set_option(h, "disturbance_step", 0));
        CHECK(tiny_batch_set_option(h, "measurement_step", 0));
        CHECK(tiny_batch_set_option(h, "state_log", 1));
        CHECK(tiny_batch_set_option(h, "step_log", 1));
        CHECK(tiny_batch_solve(h));
        CHECK(tiny_batch_get_state_log(h, states, STEPS));
        CHECK(tiny_batch_get_step_log(h, iters, u0, STEPS));
        printf("logs: kernel path %d, score %ld (applied %ld)\n", tiny_batch_kernel_path(h), tiny_batch_get_option(h, "score"), tiny_batch_get_option(h, "last_score"));
        FILE* f = fopen(argv[1], "wb");
        const int dims[4] = {STEPS, BATCH, NX, NU};
        if (!f || fwrite(dims, sizeof(int), 4, f) != 4 || fwrite(setup, sizeof(double), 4 * (size_t)BATCH * NZ, f) != 4 * (size_t)BATCH * NZ ||
            fwrite(states, sizeof(double), rows * NX, f) != rows * NX || fwrite(u0, sizeof(double), rows * NU, f) != rows * NU || fclose(f) != 0) {
            fprintf(stderr, "cannot write %s\n", argv[1]);
            return 1;
        }
        free(states); free(u0); free(iters);
    }
    free(w); free(v); free(M); free(setup); free(cost); free(worst); free(steps); free(first);
    tiny_batch_destroy(h);
    /* a study worth its name: some vehicles leave their corridor, some never do */
    return (violated > 0 && violated < BATCH && largest > 0.0) ? 0 : 2;
}
