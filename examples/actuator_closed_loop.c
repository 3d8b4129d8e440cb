/* examples/actuator_closed_loop.c -- a robustness study of the one link a controller cannot see: its own motors.
 *
 * 4 096 planar point-mass vehicles (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) fly from
 * (1.5, -1.0) m to a hover point at the origin and hold it, 60 MPC steps fused into one kernel launch.  The controller believes its
 * box: |a| <= 1 m/s^2.  The vehicles do not behave that way (tiny_batch_set_actuator): every instance follows its command with a lag
 * of its own (alpha 0.4 .. 0.9), delivers 70 .. 100 % of it, carries a trim error of up to 0.02 m/s^2, and its thrust is noisy --
 * seeded on the device (tiny_batch_generate_actuation_noise, 0.02 m/s^2).  The odd instances, in addition, saturate early: their motors
 * give 0.3 .. 0.6 m/s^2 at the most; the even ones have limits of 2 m/s^2, which the loop never reaches.  tiny_batch_set_score installs
 * the stage weights [Q | R] with the hover point as the target, and the launch accumulates every instance's realised cost on the device
 * -- over the state the plant really reached and the control the motors really applied.  The program prints the mean cost of the two
 * halves and, from the step log, how often a command lay outside its motor's limits.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/actuator_closed_loop.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o actuator_closed_loop && ./actuator_closed_loop
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

    /* the controller's own box, replicated over the horizon: |v| <= 2 m/s, |a| <= 1 m/s^2 */
    double xmin[NX * NH], xmax[NX * NH], umin[NU * (NH - 1)], umax[NU * (NH - 1)];
    for (int k = 0; k < NH; ++k)
        for (int i = 0; i < NX; ++i) { xmax[i + NX * k] = i < 2 ? 1e17 : 2.0; xmin[i + NX * k] = -xmax[i + NX * k]; }
    for (int e = 0; e < NU * (NH - 1); ++e) { umax[e] = 1.0; umin[e] = -1.0; }
    CHECK(tiny_batch_set_bound_constraints(h, xmin, xmax, umin, umax));
    CHECK(tiny_batch_update_settings(h, 1e-3, 1e-3, 100, 1, 1, 1, 0, 0, 0, 0, 0, 0));
    CHECK(tiny_batch_set_option(h, "steps_per_launch", STEPS));  /* the whole episode in one kernel launch */
    CHECK(tiny_batch_set_option(h, "step_log", 1));              /* (the commands, to count the saturated ones below) */

    const size_t rows = (size_t)STEPS * BATCH, cells = (size_t)BATCH * NU;
    double* act = (double*)malloc(sizeof(double) * 5 * cells);
    double* weight = (double*)malloc(sizeof(double) * 2 * BATCH * NZ);
    double* cost = (double*)malloc(sizeof(double) * BATCH);
    double* u0 = (double*)malloc(sizeof(double) * rows * NU);
    int* iters = (int*)malloc(sizeof(int) * rows);
    if (!act || !weight || !cost || !u0 || !iters) return 1;
    double *lo = act, *hi = act + cells, *alpha = act + 2 * cells, *gain = act + 3 * cells, *offset = act + 4 * cells, *target = weight + (size_t)BATCH * NZ;
    srand(31);
    for (int b = 0; b < BATCH; ++b) {
        for (int c = 0; c < NU; ++c) {
            const size_t at = (size_t)b * NU + c;
            hi[at] = (b & 1) ? uniform(0.3, 0.6) : 2.0;          /* the odd instances saturate before the controller's box does */
            lo[at] = -hi[at];
            alpha[at] = uniform(0.4, 0.9);
            gain[at] = uniform(0.7, 1.0);
            offset[at] = uniform(-0.02, 0.02);
        }
        for (int c = 0; c < NZ; ++c) { weight[(size_t)b * NZ + c] = c < NX ? Q[c] : R[c - NX]; target[(size_t)b * NZ + c] = 0.0; }
    }
    const double start[NX] = {1.5, -1.0, 0.0, 0.0}, thrust_noise[NU] = {0.02, 0.02};
    TinyNoiseSpec spec;
    spec.seed = 2026; spec.id_base = 0; spec.id_stride = 1; spec.n_steps = STEPS; spec.flags = TINY_HOST | TINY_BROADCAST;
    spec.scale = thrust_noise; spec.mean = NULL;
    CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
    CHECK(tiny_batch_set_actuator(h, lo, hi, alpha, gain, offset, TINY_HOST));
    CHECK(tiny_batch_generate_actuation_noise(h, &spec));
    CHECK(tiny_batch_set_score(h, weight, target, NULL, NULL, TINY_HOST));
    CHECK(tiny_batch_solve(h));
    CHECK(tiny_batch_get_score(h, cost, NULL, NULL, NULL));
    CHECK(tiny_batch_get_step_log(h, iters, u0, STEPS));
    printf("actuator: %d instances x %d MPC steps in one launch, kernel path %d, actuator %ld (lag %ld, applied %ld, counter %ld), score %ld (applied %ld)\n", BATCH, STEPS,
           tiny_batch_kernel_path(h), tiny_batch_get_option(h, "actuator"), tiny_batch_get_option(h, "actuator_lag"), tiny_batch_get_option(h, "last_actuator"),
           tiny_batch_get_option(h, "actuation_step"), tiny_batch_get_option(h, "score"), tiny_batch_get_option(h, "last_score"));
    double sum[2] = {0.0, 0.0};
    long saturated[2] = {0, 0};
    for (int b = 0; b < BATCH; ++b) {
        sum[b & 1] += cost[b];
        for (int k = 0; k < STEPS; ++k)
            for (int c = 0; c < NU; ++c) {
                const double u = u0[((size_t)k * BATCH + b) * NU + c];
                if (u < lo[(size_t)b * NU + c] || u > hi[(size_t)b * NU + c]) ++saturated[b & 1];
            }
    }
    const double mean_free = sum[0] / (BATCH / 2), mean_sat = sum[1] / (BATCH / 2);
    printf("saturated steps: %ld in the limited half, in the other half %ld\n", saturated[1], saturated[0]);
    printf("cost: saturated mean %.17g\n", mean_sat);
    printf("cost: unsaturated mean %.17g\n", mean_free);
    free(act); free(weight); free(cost); free(u0); free(iters);
    tiny_batch_destroy(h);
    /* a study worth its name: the motors that saturate cost the fleet something */
    return (saturated[1] > 0 && saturated[0] == 0 && mean_sat > mean_free) ? 0 : 2;
}
