/* examples/delayed_closed_loop.c -- how much latency does a controller tolerate, and how much does a predictor buy back?
 *
 * 4 096 planar point-mass vehicles (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) fly from
 * (1.5, -1.0) m to a hover point at the origin and hold it, 60 MPC steps fused into one kernel launch.  The controller is a stiff one
 * -- position weight 100, input weight 0.1, |a| <= 3 m/s^2 --, the kind that tolerates little latency.  The command computed for
 * period k reaches the motors d periods later (tiny_batch_set_actuator_delay): instance i has d = i % 4, so a quarter of the fleet
 * has no latency, the others 0.1, 0.2 and 0.3 s.  tiny_batch_set_score installs the stage weights [Q | R] with the hover point as the
 * target, and the launch accumulates every instance's realised cost on the device -- over the state the plant really reached and the
 * control the motors really applied.  The same fleet flies twice: once as it is, once with option "delay_compensation", under which
 * every MPC step solves from the state the model predicts for the moment its command arrives.  The program prints the mean cost per
 * delay of both flights.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/delayed_closed_loop.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o delayed_closed_loop && ./delayed_closed_loop
 */
#include <stdio.h>
#include <stdlib.h>

#include "tinympc_amd.h"

#define NX 4
#define NU 2
#define NZ (NX + NU)
#define NH 10
#define BATCH 4096
#define STEPS 60
#define D_MAX 3

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ < 0) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, tiny_batch_last_error(h)); return 1; } \
    } while (0)

int main(void) {
    const double dt = 0.1;
    /* column-major A (nx x nx), B (nx x nu): states (px, py, vx, vy) */
    double A[NX * NX] = {0}, B[NX * NU] = {0}, Q[NX] = {100, 100, 1, 1}, R[NU] = {0.1, 0.1};
    for (int i = 0; i < NX; ++i) A[i + NX * i] = 1.0;
    A[0 + NX * 2] = dt; A[1 + NX * 3] = dt;
    B[0 + NX * 0] = 0.5 * dt * dt; B[2 + NX * 0] = dt;
    B[1 + NX * 1] = 0.5 * dt * dt; B[3 + NX * 1] = dt;

    TinyBatch* h = NULL;
    int rc = tiny_batch_setup(&h, A, B, NULL, Q, R, 0.1, NX, NU, NH, BATCH, 0, 0);
    if (rc) { fprintf(stderr, "tiny_batch_setup failed (%d): no MI355X?\n", rc); return 1; }

    /* the controller's box, replicated over the horizon: |v| <= 2 m/s, |a| <= 3 m/s^2 */
    double xmin[NX * NH], xmax[NX * NH], umin[NU * (NH - 1)], umax[NU * (NH - 1)];
    for (int k = 0; k < NH; ++k)
        for (int i = 0; i < NX; ++i) { xmax[i + NX * k] = i < 2 ? 1e17 : 2.0; xmin[i + NX * k] = -xmax[i + NX * k]; }
    for (int e = 0; e < NU * (NH - 1); ++e) { umax[e] = 3.0; umin[e] = -3.0; }
    CHECK(tiny_batch_set_bound_constraints(h, xmin, xmax, umin, umax));
    CHECK(tiny_batch_update_settings(h, 1e-3, 1e-3, 100, 1, 1, 1, 0, 0, 0, 0, 0, 0));
    CHECK(tiny_batch_set_option(h, "steps_per_launch", STEPS));  /* the whole episode in one kernel launch */

    int* d = (int*)malloc(sizeof(int) * BATCH);
    double* weight = (double*)malloc(sizeof(double) * 2 * BATCH * NZ);
    double* cost = (double*)malloc(sizeof(double) * 2 * BATCH);
    if (!d || !weight || !cost) return 1;
    double* target = weight + (size_t)BATCH * NZ;
    for (int b = 0; b < BATCH; ++b) {
        d[b] = b % (D_MAX + 1);
        for (int c = 0; c < NZ; ++c) { weight[(size_t)b * NZ + c] = c < NX ? Q[c] : R[c - NX]; target[(size_t)b * NZ + c] = 0.0; }
    }
    const double start[NX] = {1.5, -1.0, 0.0, 0.0};
    for (int flight = 0; flight < 2; ++flight) {                 /* 0: the delay as it is, 1: with the predictor */
        CHECK(tiny_batch_reset(h));
        CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
        CHECK(tiny_batch_set_actuator_delay(h, d, D_MAX, TINY_HOST));      /* (installing it empties every queue) */
        CHECK(tiny_batch_set_option(h, "delay_compensation", flight));
        CHECK(tiny_batch_set_score(h, weight, target, NULL, NULL, TINY_HOST));
        CHECK(tiny_batch_solve(h));
        CHECK(tiny_batch_get_score(h, cost + (size_t)flight * BATCH, NULL, NULL, NULL));
        printf("flight %d: %d instances x %d MPC steps in one launch, kernel path %d, delay %ld, compensation %ld, applied %ld\n", flight, BATCH, STEPS, tiny_batch_kernel_path(h),
               tiny_batch_get_option(h, "actuator_delay"), tiny_batch_get_option(h, "delay_compensation"), tiny_batch_get_option(h, "last_actuator"));
    }
    double sum[2][D_MAX + 1] = {{0}};
    int worse = 0, undelayed_differ = 0;
    for (int b = 0; b < BATCH; ++b) {
        sum[0][d[b]] += cost[b];
        sum[1][d[b]] += cost[BATCH + b];
        if (d[b] > 0 && cost[BATCH + b] > cost[b]) ++worse;
        if (d[b] == 0 && cost[BATCH + b] != cost[b]) ++undelayed_differ;
    }
    for (int k = 0; k <= D_MAX; ++k)
        printf("cost: delay %d uncompensated mean %.17g compensated mean %.17g\n", k, sum[0][k] / (BATCH / (D_MAX + 1)), sum[1][k] / (BATCH / (D_MAX + 1)));
    printf("delayed instances that score worse with the predictor: %d; undelayed instances it moves: %d\n", worse, undelayed_differ);
    free(d); free(weight); free(cost);
    tiny_batch_destroy(h);
    /* a study worth its name: the predictor costs no delayed instance anything and leaves the others alone */
    return (worse == 0 && undelayed_differ == 0) ? 0 : 2;
}
