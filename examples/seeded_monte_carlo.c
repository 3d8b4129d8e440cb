/* examples/seeded_monte_carlo.c -- a Monte-Carlo closed-loop study that takes a seed up and brings four numbers per instance down.
 *
 * 4 096 planar point-mass vehicles (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) hold a hover
 * point at the origin for 60 MPC steps, fused into one kernel launch.  The gusts on the velocities (a diagonal process noise) and the
 * sensor noise on the positions are GENERATED on the device from one seed (tiny_batch_generate_disturbance,
 * tiny_batch_generate_measurement_noise): no [steps][batch][nx] array is drawn on the host or copied.  Every vehicle solves from the
 * estimate of a steady-state Kalman filter (tiny_batch_set_estimator) and is scored on the device (tiny_batch_set_score).  The program
 * prints the batch mean cost and the number of vehicles that ever left their corridor.
 *
 * A deviate is a pure function of (seed, stream, instance id, step, entry): the program then flies the WORST vehicle once more, alone,
 * as a batch of one with id_base = its index, and prints that its cost matches the study's to the last bit.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/seeded_monte_carlo.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o seeded_monte_carlo && ./seeded_monte_carlo
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tinympc_amd.h"

#define NX 4
#define NU 2
#define NZ (NX + NU)
#define NH 10
#define BATCH 4096
#define STEPS 60
#define SEED 20261021ULL

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ < 0) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, tiny_batch_last_error(h)); return 1; } \
    } while (0)

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

/* one study: `batch` vehicles whose ids start at id_base, the whole episode in one launch -> cost, violated_steps [batch] */
static int fly(int batch, long long id_base, double* cost, int* violated_steps, int* path) {
    const double dt = 0.1, gust = 0.05, sensor = 0.01;
    /* column-major A (nx x nx), B (nx x nu): states (px, py, vx, vy) */
    double A[NX * NX] = {0}, B[NX * NU] = {0}, Q[NX] = {10, 10, 1, 1}, R[NU] = {0.5, 0.5};
    for (int i = 0; i < NX; ++i) A[i + NX * i] = 1.0;
    A[0 + NX * 2] = dt; A[1 + NX * 3] = dt;
    B[0 + NX * 0] = 0.5 * dt * dt; B[2 + NX * 0] = dt;
    B[1 + NX * 1] = 0.5 * dt * dt; B[3 + NX * 1] = dt;

    TinyBatch* h = NULL;
    int rc = tiny_batch_setup(&h, A, B, NULL, Q, R, 1.0, NX, NU, NH, batch, 0, 0);
    if (rc) { fprintf(stderr, "tiny_batch_setup failed (%d): no MI355X?\n", rc); return 1; }

    /* the controller's own box, replicated over the horizon: |v| <= 2 m/s, |a| <= 1 m/s^2 */
    double xmin[NX * NH], xmax[NX * NH], umin[NU * (NH - 1)], umax[NU * (NH - 1)];
    for (int k = 0; k < NH; ++k)
        for (int i = 0; i < NX; ++i) { xmax[i + NX * k] = i < 2 ? 1e17 : 2.0; xmin[i + NX * k] = -xmax[i + NX * k]; }
    for (int e = 0; e < NU * (NH - 1); ++e) { umax[e] = 1.0; umin[e] = -1.0; }
    CHECK(tiny_batch_set_bound_constraints(h, xmin, xmax, umin, umax));
    CHECK(tiny_batch_update_settings(h, 1e-3, 1e-3, 100, 1, 1, 1, 0, 0, 0, 0, 0, 0));
    CHECK(tiny_batch_set_option(h, "steps_per_launch", STEPS));  /* the whole episode in one kernel launch */

    /* what goes up: a seed, the ids and two scale vectors -- gusts push the velocities, the positions are measured */
    const double w_scale[NX] = {0.0, 0.0, gust, gust}, v_scale[NX] = {sensor, sensor, 0.0, 0.0};
    TinyNoiseSpec spec;
    memset(&spec, 0, sizeof(spec));
    spec.seed = SEED; spec.id_base = id_base; spec.id_stride = 1; spec.n_steps = STEPS; spec.flags = TINY_HOST | TINY_BROADCAST;
    spec.scale = w_scale;
    CHECK(tiny_batch_generate_disturbance(h, &spec));
    spec.scale = v_scale;
    CHECK(tiny_batch_generate_measurement_noise(h, &spec));

    double M[NX * NX] = {0}, L[2];
    kalman_gain(dt, sensor * sensor, 1e-6, gust * gust, L);
    M[0 + NX * 0] = L[0]; M[2 + NX * 0] = L[1];
    M[1 + NX * 1] = L[0]; M[3 + NX * 1] = L[1];
    const double start[NX] = {0.0, 0.0, 0.0, 0.0};
    CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
    CHECK(tiny_batch_set_estimator(h, M, TINY_HOST | TINY_BROADCAST));      /* (the estimate starts at x0) */
    /* the score: the stage weights, the hover point, a corridor of 15 cm around it; |velocity| within 0.5 m/s, |acceleration| within 0.95 */
    const double weight[NZ] = {10, 10, 1, 1, 0.5, 0.5}, hi[NZ] = {0.15, 0.15, 0.5, 0.5, 0.95, 0.95}, lo[NZ] = {-0.15, -0.15, -0.5, -0.5, -0.95, -0.95};
    CHECK(tiny_batch_set_score(h, weight, NULL, lo, hi, TINY_HOST | TINY_BROADCAST));
    CHECK(tiny_batch_solve(h));
    CHECK(tiny_batch_get_score(h, cost, NULL, violated_steps, NULL));
    if (tiny_batch_get_option(h, "disturbance_generated") != 1 || tiny_batch_get_option(h, "measurement_noise_generated") != 1 ||
        tiny_batch_get_option(h, "last_disturbance") != 1 || tiny_batch_get_option(h, "last_measurement_noise") != 1) {
        fprintf(stderr, "the generated sequences were not applied\n");
        return 1;
    }
    *path = tiny_batch_kernel_path(h);
    tiny_batch_destroy(h);
    return 0;
}

int main(void) {
    double* cost = (double*)malloc(sizeof(double) * BATCH);
    int* steps = (int*)malloc(sizeof(int) * BATCH);
    if (!cost || !steps) return 1;
    int path = -1;
    if (fly(BATCH, 0, cost, steps, &path)) return 1;
    double sum = 0.0;
    int violated = 0, worst = 0;
    for (int b = 0; b < BATCH; ++b) {
        sum += cost[b];
        if (steps[b] > 0) ++violated;
        if (cost[b] > cost[worst]) worst = b;
    }
    printf("study: seed %llu, %d instances x %d MPC steps in one launch, kernel path %d\n", SEED, BATCH, STEPS, path);
    printf("study: batch mean cost %.17g, %d of %d instances ever left their corridor\n", sum / BATCH, violated, BATCH);
    printf("study: the worst instance is %d with cost %.17g (%d violated steps)\n", worst, cost[worst], steps[worst]);

    /* the worst vehicle again, alone: a batch of one whose id is its index in the study */
    double again = 0.0;
    int again_steps = 0;
    if (fly(1, worst, &again, &again_steps, &path)) return 1;
    const int same = memcmp(&again, &cost[worst], sizeof(double)) == 0 && again_steps == steps[worst];
    printf("re-run: instance %d alone (batch of 1, id_base %d), kernel path %d: cost %.17g, %d violated steps -- %s\n", worst, worst, path, again, again_steps,
           same ? "matches the study to the last bit" : "DIFFERS from the study");
    free(cost); free(steps);
    /* a study worth its name: some vehicles leave their corridor, some never do; and the re-run reproduces */
    return (same && violated > 0 && violated < BATCH) ? 0 : 2;
}
