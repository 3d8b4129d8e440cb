/* examples/model_mismatch_closed_loop.c -- a robustness study of a closed loop under model mismatch, without the host in the loop.
 *
 * 4 096 planar double integrators (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) start from ONE
 * state and are driven to the origin: 60 MPC steps fused into one kernel launch.  The controller predicts with the nominal model; the
 * state is handed on by every instance's OWN plant (tiny_batch_set_plant): its actuator gain is off by up to +-20 % and its mass by up
 * to +-15 % (both scale B_p), and a little drag the model does not know slows it down (A_p).  The state log (option "state_log") gives
 * the realised trajectory of every instance; the program prints the spread of the realised end states, and runs the episode again with
 * the nominal model installed as the one plant for all.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/model_mismatch_closed_loop.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o model_mismatch_closed_loop && ./model_mismatch_closed_loop
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
    CHECK(tiny_batch_set_option(h, "state_log", 1));             /* ... and every realised state of it kept */

    /* every instance its own truth: A_p [BATCH][NX*NX], B_p [BATCH][NX*NU], column-major like A and B */
    double* Ap = (double*)calloc((size_t)BATCH * NX * NX, sizeof(double));
    double* Bp = (double*)calloc((size_t)BATCH * NX * NU, sizeof(double));
    double* log = (double*)malloc(sizeof(double) * (size_t)STEPS * BATCH * NX);
    if (!Ap || !Bp || !log) return 1;
    srand(11);
    for (int b = 0; b < BATCH; ++b) {
        const double gain = uniform(0.8, 1.2), mass = uniform(0.85, 1.15), drag = uniform(0.0, 0.3);      /* drag: 1/s */
        double* a = Ap + (size_t)b * NX * NX;
        double* bb = Bp + (size_t)b * NX * NU;
        for (int e = 0; e < NX * NX; ++e) a[e] = A[e];
        a[2 + NX * 2] = 1.0 - drag * dt; a[3 + NX * 3] = 1.0 - drag * dt;
        for (int e = 0; e < NX * NU; ++e) bb[e] = B[e] * gain / mass;
    }
    const double start[NX] = {1.5, -1.0, 0.0, 0.0};

    double mean[2], sd[2], worst[2];
    for (int run = 0; run < 2; ++run) {                          /* 0: every instance its own plant, 1: the model as the one plant */
        if (run == 0) CHECK(tiny_batch_set_plant(h, Ap, Bp, NULL, TINY_HOST));
        else CHECK(tiny_batch_set_plant(h, A, B, NULL, TINY_HOST | TINY_BROADCAST));
        CHECK(tiny_batch_reset(h));
        CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
        CHECK(tiny_batch_solve(h));
        CHECK(tiny_batch_get_state_log(h, log, STEPS));          /* [STEPS][BATCH][NX]: the last row is the end state */
        spread(log + (size_t)(STEPS - 1) * BATCH * NX, &mean[run], &sd[run], &worst[run]);
        double mid_mean, mid_sd, mid_worst;
        spread(log + (size_t)(STEPS / 4) * BATCH * NX, &mid_mean, &mid_sd, &mid_worst);
        printf("%s: %d instances x %d MPC steps in one launch, kernel path %d, plant %ld, applied %ld\n", run == 0 ? "mismatch" : "nominal ", BATCH, STEPS,
               tiny_batch_kernel_path(h), tiny_batch_get_option(h, "plant"), tiny_batch_get_option(h, "last_plant"));
        printf("          distance from the origin after %.1f s: mean %.5f m, standard deviation %.3e m; after %.0f s: mean %.5f m, standard "
               "deviation %.3e m, largest %.5f m\n", (STEPS / 4 + 1) * dt, mid_mean, mid_sd, STEPS * dt, mean[run], sd[run], worst[run]);
    }
    free(Ap);
    free(Bp);
    free(log);
    tiny_batch_destroy(h);
    /* under the nominal plant the batch ends in one point; the mismatch spreads it, and the controller still brings every instance home */
    return (sd[1] < 1e-12 && sd[0] > 1e-6 && worst[0] < 0.5 && worst[1] < 0.2) ? 0 : 2;
}
