/* examples/output_feedback_closed_loop.c -- output-feedback MPC: sensor, observer and controller in one kernel launch.
 *
 * 4 096 planar double integrators (nx = 4: position / velocity in x and y, nu = 2: accelerations, N = 10, dt = 0.1 s) start from ONE
 * state and are driven to the origin: 60 MPC steps fused into one kernel launch.  Only the POSITION is measured, every instance by a
 * sensor of its own quality (readings off by up to 1 .. 5 cm, every instance its own sequence: tiny_batch_set_measurement_noise).
 * Between the sensor and the controller sits a steady-state Kalman filter (tiny_batch_set_estimator): every instance its own gain
 * M = L C, C = [I 0] the position read-out, L from a short fixed-point iteration of the filter Riccati equation written below.  The
 * velocity columns of M are zero: whatever the noise sequence holds there is multiplied by zero.  The filter starts 2 cm and
 * 2 cm/s off the truth.  The program prints the RMS estimation error and the RMS tracking error with the estimator and -- the episode
 * run again without it, the controller handed the raw readings of the full state, velocities off by up to 5 cm/s -- without.
 *
 *   gcc -std=c99 -O2 -Iinclude examples/output_feedback_closed_loop.c -Ltinympc_amd -ltinympc_amd \
 *       -Wl,-rpath,$PWD/tinympc_amd -lm -o output_feedback_closed_loop && ./output_feedback_closed_loop
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
#define TAIL 20                                          /* the tracking error is taken over the last TAIL steps */

#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ < 0) { fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, tiny_batch_last_error(h)); return 1; } \
    } while (0)

static double uniform(double lo, double hi) { return lo + (hi - lo) * (rand() / (double)RAND_MAX); }

/* the steady-state Kalman gain of ONE axis (position p, velocity v; p measured with variance r; process noise w_p, w_v): the
 * a-priori covariance P is iterated to its fixed point, P <- A (P - L [1 0] P) A' + W with L = P [1 0]' / (P_pp + r); L [2] */
static void kalman_gain(double dt, double r, double w_p, double w_v, double L[2]) {
    double p00 = 1.0, p01 = 0.0, p11 = 1.0;
    for (int it = 0; it < 500; ++it) {
        const double s = p00 + r;
        L[0] = p00 / s; L[1] = p01 / s;
        const double q00 = p00 - L[0] * p00, q01 = p01 - L[0] * p01, q11 = p11 - L[1] * p01;   /* a-posteriori covariance */
        p00 = q00 + 2.0 * dt * q01 + dt * dt * q11 + w_p;                                      /* A = [1 dt; 0 1] */
        p01 = q01 + dt * q11;
        p11 = q11 + w_v;
    }
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
    CHECK(tiny_batch_set_option(h, "state_log", 1));             /* ... every true state of it kept */
    CHECK(tiny_batch_set_option(h, "estimate_log", 1));          /* ... and every estimate the controller solved from */

    const size_t all = (size_t)STEPS * BATCH * NX;
    double* v = (double*)malloc(sizeof(double) * all);
    double* states = (double*)malloc(sizeof(double) * all);
    double* xhat = (double*)malloc(sizeof(double) * all);
    double* M = (double*)calloc((size_t)BATCH * NX * NX, sizeof(double));
    double* xp = (double*)malloc(sizeof(double) * (size_t)BATCH * NX);
    if (!v || !states || !xhat || !M || !xp) return 1;
    srand(23);
    const double start[NX] = {1.5, -1.0, 0.0, 0.0};
    /* every instance its own sensor: position readings off by up to amp[b] (uniform: variance amp^2 / 3), and with it its own gain
     * M = L C, column-major: the position columns hold L, the velocity columns stay zero */
    for (int b = 0; b < BATCH; ++b) {
        const double amp = uniform(0.01, 0.05);
        double L[2];
        kalman_gain(dt, amp * amp / 3.0, 1e-6, 1e-5, L);
        double* Mb = M + (size_t)b * NX * NX;
        Mb[0 + NX * 0] = L[0]; Mb[2 + NX * 0] = L[1];            /* x axis: rows px, vx of column px */
        Mb[1 + NX * 1] = L[0]; Mb[3 + NX * 1] = L[1];            /* y axis: rows py, vy of column py */
        for (int k = 0; k < STEPS; ++k) {
            double* row = v + ((size_t)k * BATCH + b) * NX;
            row[0] = uniform(-amp, amp); row[1] = uniform(-amp, amp);
            row[2] = uniform(-0.05, 0.05); row[3] = uniform(-0.05, 0.05);   /* (no velocity sensor: only the raw run reads these) */
        }
        for (int i = 0; i < NX; ++i) xp[b * NX + i] = start[i] + (rand() & 1 ? 0.02 : -0.02);
    }
    CHECK(tiny_batch_set_measurement_noise(h, v, STEPS, TINY_HOST));

    double est_err[2], track_err[2];
    for (int run = 0; run < 2; ++run) {                          /* 0: the estimator between sensor and controller, 1: the raw readings */
        CHECK(tiny_batch_reset(h));
        CHECK(tiny_batch_set(h, TINY_F_X0, start, TINY_HOST | TINY_BROADCAST));
        if (run == 0) {
            CHECK(tiny_batch_set_estimator(h, M, TINY_HOST));
            CHECK(tiny_batch_set_estimate(h, xp, TINY_HOST));
        } else CHECK(tiny_batch_set_estimator(h, NULL, TINY_HOST));
        CHECK(tiny_batch_set_option(h, "measurement_step", 0));
        CHECK(tiny_batch_solve(h));
        CHECK(tiny_batch_get_state_log(h, states, STEPS));       /* [STEPS][BATCH][NX]: row k is the true state AFTER step k */
        if (run == 0) CHECK(tiny_batch_get_estimate_log(h, xhat, STEPS));
        /* what the controller solved from at step k, against the true state it stood in: the start, then row k - 1 of the state log */
        double e2 = 0.0, t2 = 0.0;
        for (int k = 0; k < STEPS; ++k)
            for (int b = 0; b < BATCH; ++b)
                for (int i = 0; i < NX; ++i) {
                    const size_t at = ((size_t)k * BATCH + b) * NX + i;
                    const double truth = k == 0 ? start[i] : states[at - (size_t)BATCH * NX];
                    const double seen = run == 0 ? xhat[at] : truth + v[at];
                    e2 += (seen - truth) * (seen - truth);
                    if (k >= STEPS - TAIL && i < 2) t2 += states[at] * states[at];
                }
        est_err[run] = sqrt(e2 / (double)all);
        track_err[run] = sqrt(t2 / ((double)TAIL * BATCH));
        printf("%s: %d instances x %d MPC steps in one launch, kernel path %d, estimator %ld (applied %ld)\n", run == 0 ? "estimator" : "raw", BATCH, STEPS,
               tiny_batch_kernel_path(h), tiny_batch_get_option(h, "estimator"), tiny_batch_get_option(h, "last_estimator"));
        printf("%s: RMS estimation error %.6f, RMS tracking error %.6f m over the last %.0f s\n", run == 0 ? "estimator" : "raw", est_err[run], track_err[run],
               TAIL * dt);
    }
    free(v); free(states); free(xhat); free(M); free(xp);
    tiny_batch_destroy(h);
    /* the filter knows the model: what it hands the controller is closer to the truth than the readings are */
    return (est_err[0] < est_err[1] && track_err[0] < 0.5 && track_err[1] < 0.5) ? 0 : 2;
}
