/*
 * tinympc_amd.h -- C ABI of the MI355X-native batched TinyMPC ADMM solver (libtinympc_amd.so).
 *
 * Two surfaces, both plain C (pointers and sizes only, no C++/Eigen/torch types):
 *
 *  (A) the BATCHED, device-resident surface (tiny_batch_*): what the throughput metric is measured
 *      on.  It mirrors the reference's operator interface for the hot path one-for-one --
 *      tiny_setup / tiny_set_bound_constraints / tiny_set_cone_constraints / tiny_update_settings /
 *      tiny_set_x0 / tiny_set_x_ref / tiny_set_u_ref / tiny_solve  (src/tinympc/tiny_api.hpp:10-54)
 *      -- but every per-instance quantity carries a leading batch axis and lives in HBM.
 *
 *  (B) the reference's own entry points (tiny_setup, tiny_solve, ... same names, same argument
 *      meaning, same return codes) over plain-data mirrors of the reference structs, so existing
 *      callers compiled against the reference's headers link against this library unchanged
 *      (INTEGRATION.md).  tiny_solve(TinySolver*) is a batch of one on the GPU.
 *
 * There is NO CPU fallback: every solve runs the HIP kernels; without a GPU the calls fail with
 * TINY_ERR_NO_DEVICE.
 *
 * Matrix conventions: column-major (Eigen default).  Per-instance matrices of a batch are stored
 * back to back: Xref is [batch][N][nx] doubles (instance-major, then knot point, then row).
 */
#ifndef TINYMPC_AMD_H
#define TINYMPC_AMD_H

#include <stdint.h>
#include <stdbool.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------------------------ */
/* return codes: 0 / 1 keep the reference's meaning (tiny_solve: 0 = all converged, 1 = some
 * instance hit max_iter, admm.cpp:441,454; setters: 0 = ok, 1 = dimension error).              */
#define TINY_OK                 0
#define TINY_ERR_DIM            1
#define TINY_ERR_NULL          (-1)
#define TINY_ERR_NO_DEVICE     (-2)   /* no MI355X / HIP runtime failure: there is no CPU path   */
#define TINY_ERR_UNSUPPORTED   (-3)   /* (nx,nu,N) not instantiated, or an out-of-scope feature   */
#define TINY_ERR_HIP           (-4)
#define TINY_ERR_ARG           (-5)

/* work->status values (admm.cpp:336,431) */
#define TINY_STATUS_SOLVED      1
#define TINY_STATUS_UNSOLVED   11

typedef struct TinyBatch TinyBatch;   /* opaque, owns its HBM buffers */

/* Per-instance fields (reference names, src/tinympc/types.hpp:88-208). State-sized = nx x N,
 * input-sized = nu x (N-1). */
typedef enum {
    TINY_F_X0 = 0,      /* nx            tiny_set_x0  (x[:,0])                */
    TINY_F_XREF,        /* nx x N        tiny_set_x_ref                        */
    TINY_F_UREF,        /* nu x (N-1)    tiny_set_u_ref                        */
    TINY_F_X,           /* work->x      (primal; col 0 is x0)                 */
    TINY_F_U,           /* work->u                                             */
    TINY_F_VNEW,        /* work->vnew   (== solution->x after a solve)         */
    TINY_F_ZNEW,        /* work->znew   (== solution->u)                       */
    TINY_F_G,           /* work->g                                             */
    TINY_F_Y,           /* work->y                                             */
    TINY_F_V,           /* work->v                                             */
    TINY_F_Z,           /* work->z                                             */
    TINY_F_VCNEW,       /* work->vcnew  (cone slack, only with a cone enabled) */
    TINY_F_ZCNEW,
    TINY_F_GC,
    TINY_F_YC,
    TINY_F_Q,           /* work->q / r / p / d of the last iteration: kept by  */
    TINY_F_R,           /* a solve after tiny_batch_set_option("debug", 1);    */
    TINY_F_P,           /* settable as inputs of tiny_batch_phase              */
    TINY_F_D,
    TINY_F_VLNEW,       /* work->vlnew / zlnew / gl / yl: static linear-constraint slack + dual   */
    TINY_F_ZLNEW,
    TINY_F_GL,
    TINY_F_YL,
    TINY_F_VLNEW_TV,    /* work->vlnew_tv / zlnew_tv / gl_tv / yl_tv: time-varying linear          */
    TINY_F_ZLNEW_TV,
    TINY_F_GL_TV,
    TINY_F_YL_TV,
    TINY_F_COUNT
} TinyField;

/* flags for tiny_batch_set / tiny_batch_get */
#define TINY_HOST        0   /* pointer is host memory, [batch] matrices back to back          */
#define TINY_DEVICE      1   /* pointer is device (HBM) memory on the batch's GPU               */
#define TINY_BROADCAST   2   /* (set only) ONE matrix, replicated to every instance              */
#define TINY_NOISE_FACTOR 4  /* (TinyNoiseSpec only) scale is an nx x nx factor, not a diagonal   */

/* ---- problem family ---------------------------------------------------------------------- */
int tiny_batch_device_count(void);

/* == tiny_setup (tiny_api.hpp:10-12, tiny_api.cpp:21-147) for `batch` instances sharing one
 * (A, B, f, Q, R, rho).  Qdiag/Rdiag are the USER diagonals (the reference's callers pass
 * Q.asDiagonal()); rho is added the way the reference does (twice on the cache path).
 * Runs the infinite-horizon Riccati recursion on the host (tiny_api.cpp:307-381), allocates the
 * HBM records (zero-initialised, like tiny_setup) on GPU `device`.                                */
int tiny_batch_setup(TinyBatch** out, const double* Adyn, const double* Bdyn, const double* fdyn,
                     const double* Qdiag, const double* Rdiag, double rho,
                     int nx, int nu, int N, int batch, int device, int verbose);
/* Heterogeneous batch: instance i has its OWN (A_i, B_i, f_i, Q_i, R_i, rho_i) -- arrays with a leading batch
 * axis ([batch][nx*nx] column-major, [batch][nx*nu], [batch][nx] (may be NULL), [batch][nx], [batch][nu], [batch]).
 * tiny_precompute_and_set_cache (tiny_api.cpp:307-381) runs on the GPU for all instances at once; the solve kernel
 * then streams each instance's own cache.  Cones and settings stay shared; the box is shared unless tiny_batch_set_instance_bounds gives every
 * instance its own.  Any nx + nu <= 32, nu <= 16 (round 5): shapes the
 * one-row kernel holds run its HET variant, wide and long shapes the tile kernel's per-instance form on the shape's fastest box form
 * (run-time instantiated: needs hipRTC or the prebuilt store); TINY_ERR_UNSUPPORTED when neither kernel holds the shape.  Round 6: cones
 * that share rows, more half-spaces per knot than the register variants hold, or a variant hipRTC cannot make send a heterogeneous
 * batch to the coverage kernel, which reads the same per-instance tables.  Adaptive rho combines with per-instance data on the shapes
 * the one-row kernel holds (nx + nu <= 16): every instance then moves its own cache by its own sensitivity tables
 * (tiny_batch_compute_sensitivity), or by the one set tiny_batch_set_sensitivity installs for all of them. */
int tiny_batch_setup_hetero(TinyBatch** out, const double* Adyn, const double* Bdyn, const double* fdyn,
                            const double* Qdiag, const double* Rdiag, const double* rho,
                            int nx, int nu, int N, int batch, int device, int verbose);
/* one instance's cache member (names as tiny_batch_get_cache, plus "riccati_iters") */
int tiny_batch_get_cache_instance(TinyBatch* b, int instance, const char* name, double* out, int capacity);
int tiny_batch_destroy(TinyBatch* b);

/* == tiny_set_bound_constraints (tiny_api.hpp:13-15): nx x N, nx x N, nu x (N-1), nu x (N-1),
 * column-major, shared by every instance. */
int tiny_batch_set_bound_constraints(TinyBatch* b, const double* x_min, const double* x_max,
                                     const double* u_min, const double* u_max);
/* every instance its own box: x_min / x_max are [batch][N][nx] (per instance nx x N column-major, like Xref),
 * u_min / u_max [batch][N-1][nu].  flags: TINY_HOST or TINY_DEVICE (copied; the caller may free); TINY_BROADCAST is TINY_ERR_ARG (one box
 * for all: the shared setter above).  The latest setter wins: this one replaces a shared box, a later tiny_batch_set_bound_constraints
 * replaces this one; en_state_bound / en_input_bound act as on the shared box (a disabled family is (-inf, +inf)); tiny_batch_reset leaves
 * the box alone.  Works on tiny_batch_setup and tiny_batch_setup_hetero batches.  Synchronous.  Read-backs (tiny_batch_get_option):
 * "instance_bounds" 1 while such a box is installed, "last_instance_bounds" 1 when the last solve's kernel read one;
 * "last_uniform_bounds" keeps its meaning -- a UB form ran, which here means EVERY instance's box is knot-invariant for the enabled families.
 * Where it runs: the one-row kernel's PB forms (run-time instantiated, full rows, no prefetch: "last_half_rows" and "last_prefetch" read
 * 0) for the plain box variants of the shapes that kernel holds, with every launch form of those; the coverage kernel -- correct, not
 * fast, tiny_batch_kernel_path says so -- for tile-kernel shapes (nx + nu > 16 or a horizon beyond the one-row kernel), an enabled cone
 * or half-space family, "debug", "force_general", "no_jit" or a missing hipRTC.  Adaptive rho with a per-instance box fails the solve
 * with TINY_ERR_UNSUPPORTED.  Out of scope: the tile kernel, the cone and half-space register variants, tiny_codegen and
 * tiny_solve_batch (which goes on taking solvers[0]'s bounds for all solvers). */
int tiny_batch_set_instance_bounds(TinyBatch* b, const double* x_min, const double* x_max,
                                   const double* u_min, const double* u_max, int flags);
/* what instance `instance` is bound by, as set (whatever the enable switches say); on a shared box: the shared one ((-inf, +inf) when
 * none was ever set).  any pointer may be NULL */
int tiny_batch_get_instance_bounds(TinyBatch* b, int instance, double* x_min, double* x_max, double* u_min, double* u_max);
/* == tiny_set_cone_constraints (tiny_api.cpp:176-208): STATE triple first (the definition's
 * positional order).  Cones have dimension 3 (admm.cpp:53).  Cones of one family may share rows: the reference projects them
 * one after the other (admm.cpp:111-135) and so does this library -- on the coverage kernel (single-step launches, shared
 * problem data); disjoint cones run on the register-resident kernels. */
int tiny_batch_set_cone_constraints(TinyBatch* b, int n_state_cones, const int* Acx, const int* qcx,
                                    const double* cx, int n_input_cones, const int* Acu,
                                    const int* qcu, const double* cu);
/* == tiny_set_linear_constraints (tiny_api.hpp:19-21, tiny_api.cpp:210-251): half-spaces a_k' z <= b_k,
 * Alin_x is n_state x nx column-major (one ROW per constraint), blin_x n_state; same for the inputs. */
int tiny_batch_set_linear_constraints(TinyBatch* b, int n_state, const double* Alin_x, const double* blin_x,
                                      int n_input, const double* Alin_u, const double* blin_u);
/* == tiny_set_tv_linear_constraints (tiny_api.hpp:22-24, tiny_api.cpp:253-304): counts are PER KNOT POINT;
 * tv_Alin_x is (n_state*N) x nx column-major (row n_state*i + k = constraint k at knot i), tv_blin_x
 * n_state x N; tv_Alin_u (n_input*(N-1)) x nu, tv_blin_u n_input x (N-1). */
int tiny_batch_set_tv_linear_constraints(TinyBatch* b, int n_state, const double* tv_Alin_x, const double* tv_blin_x,
                                         int n_input, const double* tv_Alin_u, const double* tv_blin_u);
/* every instance its own half-spaces: every array is the shared setter's array with a leading batch axis -- instance i's block has
 * exactly the shape and column-major layout documented above (static: Alin_x [batch][n_state x nx], blin_x [batch][n_state]; time-varying:
 * tv_Alin_x [batch][(n_state*N) x nx], tv_blin_x [batch][n_state x N], the inputs likewise over N-1 knots).  The counts (per knot for the
 * time-varying set) are the same for all instances: an instance that needs fewer half-spaces pads with a row of zeros and b = +inf, which
 * is inert (cv = 0 > +inf is false).  flags: TINY_HOST or TINY_DEVICE (copied; the caller may free); TINY_BROADCAST is TINY_ERR_ARG (one
 * set for all: the shared setters above).  The latest setter wins, per set: the static and the time-varying set are independent, one may be
 * per instance while the other is shared; a later shared setter of the same set replaces the per-instance one and frees its arrays.  A
 * failed call leaves what was installed.  The en_*_linear switches act as on shared sets; tiny_batch_reset leaves the constraints alone.
 * Works on tiny_batch_setup and tiny_batch_setup_hetero batches.
 * Offsets-only update (the closed-loop pattern: only b moves from step to step): with a per-instance set of the same counts installed, a
 * NULL coefficient array keeps that family's coefficients and rewrites only its offsets -- when every family with a positive count passes
 * NULL, nothing is uploaded or squared again but the offsets; NULL with nothing installed, or with other counts, is TINY_ERR_ARG.
 * Read-backs (tiny_batch_get_option): "instance_linear" is a bit mask, 1 static, 2 time-varying, of the sets installed per instance;
 * "last_instance_linear" the same mask for what the last solve's kernel read.
 * Where it runs: the one-row kernel's PL forms (run-time instantiated, at KMAX = the smallest power of two that holds the enabled counts,
 * 1 and 2 included; tiny_batch_kernel_path 3) for the shapes that kernel holds, with a disjoint cone, per-instance problem data and every
 * launch form of those, where the slack planes and the four rows' tables fit a wave's LDS; the coverage kernel -- correct, not fast,
 * tiny_batch_kernel_path says so -- for tile-kernel shapes (nx + nu > 16 or a horizon beyond the one-row kernel), planes that do not fit
 * (long horizons with a time-varying set), cones that share rows, a per-instance box at the same time, "debug", "force_general", "no_jit"
 * or a missing hipRTC.  Adaptive rho fails the solve with TINY_ERR_UNSUPPORTED, as it does with shared half-spaces.  Out of scope: the tile
 * kernel, tiny_codegen, tiny_solve_batch and the drop-in structs (which go on taking one set for all solvers). */
int tiny_batch_set_instance_linear_constraints(TinyBatch* b, int n_state, const double* Alin_x, const double* blin_x,
                                               int n_input, const double* Alin_u, const double* blin_u, int flags);
int tiny_batch_set_instance_tv_linear_constraints(TinyBatch* b, int n_state, const double* tv_Alin_x, const double* tv_blin_x,
                                                  int n_input, const double* tv_Alin_u, const double* tv_blin_u, int flags);
/* what instance `instance` is held to by the static (tv = 0) or the time-varying (tv = 1) set, as set (whatever the enable switches say),
 * in the shared setter's layout; on a shared set: the shared one.  any pointer may be NULL */
int tiny_batch_get_instance_linear_constraints(TinyBatch* b, int instance, int tv, double* A_x, double* b_x, double* A_u, double* b_u);
/* every instance its own cone coefficients on the cones the last tiny_batch_set_cone_constraints installed: cx [batch][n_state_cones],
 * cu [batch][n_input_cones], instance i's coefficients in the order of Acx / Acu.  Where the cones sit, how many there are and whether
 * they share rows stays a property of the batch; with no cone set installed the call is TINY_ERR_ARG.  A NULL array for a family that has
 * cones keeps that family's shared coefficients for every instance; both NULL is TINY_ERR_ARG.  flags: TINY_HOST or TINY_DEVICE (copied;
 * the caller may free); TINY_BROADCAST is TINY_ERR_ARG (one coefficient for all: tiny_batch_set_cone_constraints).  The values are stored
 * as given and truncated to float where admm.cpp:39 does so; nothing is validated that the shared setter does not validate.  The latest
 * setter wins: a later call replaces both families (one passed as NULL is back on the shared coefficients), a later
 * tiny_batch_set_cone_constraints drops the per-instance coefficients and frees their arrays.  A failed call leaves what was installed.
 * The en_state_soc / en_input_soc switches act as on a shared set; tiny_batch_reset leaves the coefficients alone.  Works on
 * tiny_batch_setup and tiny_batch_setup_hetero batches.
 * Read-backs (tiny_batch_get_option): "instance_cones" is 1 while per-instance coefficients are installed; "last_instance_cones" is 1 when
 * the last solve's kernel read them: installed and a cone family on.
 * Where it runs: the one-row kernel's PC forms (run-time instantiated; tiny_batch_kernel_path 3) for the shapes that kernel holds, with
 * per-instance problem data and every launch form of the shared cone variant; the coverage kernel -- correct, not fast,
 * tiny_batch_kernel_path says so -- for tile-kernel shapes, cones that share rows (projected one after the other, each with the
 * instance's own coefficient), half-spaces (shared or per instance) or a per-instance box at the same time, "debug", "force_general",
 * "no_jit" or a missing hipRTC.  Adaptive rho fails the solve with TINY_ERR_UNSUPPORTED.  Out of scope: per-instance cone positions or
 * counts, the tile kernel, per-instance half-spaces together with these on the one-row kernel, adaptive rho, tiny_codegen,
 * tiny_solve_batch and the drop-in structs (which go on taking one coefficient set for all solvers). */
int tiny_batch_set_instance_cone_coefficients(TinyBatch* b, const double* cx, const double* cu, int flags);
/* what instance `instance` is held to, as set (whatever the enable switches say): cx [n_state_cones], cu [n_input_cones]; on a shared
 * set, and for a family that kept the shared coefficients: the shared values.  either pointer may be NULL */
int tiny_batch_get_instance_cone_coefficients(TinyBatch* b, int instance, double* cx, double* cu);
/* every instance its own additive disturbance sequence, applied on the device at the plant step of a closed loop (advance_x0,
 * steps_per_launch > 1): a batch of closed loops under process noise, gusts or unmodelled forces without the host in the loop.
 * w is [n_steps][batch][nx], step-major (a launch reads one contiguous [batch][nx] block per MPC step).  flags: TINY_HOST or TINY_DEVICE
 * (copied; the caller may free); with TINY_BROADCAST w is ONE sequence [n_steps][nx] for every instance (expanded on the device).
 * w == NULL or n_steps <= 0 removes the sequence and frees it.  A failed call leaves what was installed.  Synchronous; works on
 * tiny_batch_setup and tiny_batch_setup_hetero batches.
 * Meaning: while a sequence is installed, the plant step of MPC step k stores fl(x1 + w[k][i]) as instance i's next x0, x1 being what
 * the undisturbed plant step stores (work->x[:,1] of that solve): one IEEE double addition, nothing fused into it.  k is the batch's
 * disturbance step counter: the setter puts it to 0, every MPC step of a launch that takes a plant step advances it by one (inside
 * fused launches and their stretches, too), tiny_batch_set_option("disturbance_step", k) moves it, tiny_batch_reset leaves sequence
 * and counter alone.  Steps with k >= n_steps or k < 0 take the undisturbed plant step bit for bit (no addition, not one of zero);
 * where no plant step happens (max_iter = 0) nothing is added and the counter still advances.  A launch without a plant step reads
 * nothing, leaves the counter alone and runs the kernel form it runs without a sequence.  Only x0 moves: work->x and solution->x keep
 * the solver's prediction.
 * Read-backs (tiny_batch_get_option): "disturbance" is n_steps as installed (0: none), "disturbance_step" the counter,
 * "last_disturbance" 1 when the last solve's launches applied the sequence (installed and a plant step taken).
 * Where it runs: the one-row kernel's PD forms (run-time instantiated; tiny_batch_kernel_path 3) of the box, cone, half-space,
 * per-instance-data and per-instance box / half-space / cone-coefficient forms, on full rows ("last_half_rows" and "last_prefetch"
 * read 0); the coverage kernel -- correct, not fast -- for tile-kernel shapes, overlapping cones, "debug", "force_general", "no_jit",
 * a missing hipRTC and whatever runs there without a sequence.  Adaptive rho on a launch with a plant step fails the solve with
 * TINY_ERR_UNSUPPORTED ("adaptive rho does not combine with a per-instance disturbance").
 * Out of scope: the tile kernel (its shapes run on the coverage kernel while a disturbance applies), the half-row and PREFETCH forms,
 * tiny_codegen, tiny_solve_batch and the drop-in structs.  (A plant of its own and a log of the realised x0: tiny_batch_set_plant.) */
int tiny_batch_set_disturbance(TinyBatch* b, const double* w, int n_steps, int flags);
/* row `step` of instance `instance` as installed: w_out [nx]; TINY_ERR_ARG with none installed or an index outside it */
int tiny_batch_get_disturbance(TinyBatch* b, int step, int instance, double* w_out);
/* a plant model of its own at the plant step of a closed loop (advance_x0, steps_per_launch > 1): the controller keeps predicting with
 * its A, B, f while the state is handed on by A_p, B_p, f_p -- model mismatch (mass, inertia, actuator gain, drag per vehicle; a finer
 * discretisation as "truth") without the host in the loop.
 * flags TINY_HOST or TINY_DEVICE: every instance its own plant, A_p [batch][nx*nx] column-major, B_p [batch][nx*nu], f_p [batch][nx] or
 * NULL for zero (the layout of tiny_batch_setup_hetero); copied, the caller may free.  With TINY_BROADCAST: ONE plant for all, [nx*nx],
 * [nx*nu], [nx], stored once.  A_p == NULL removes the plant and frees it; B_p == NULL with A_p != NULL is TINY_ERR_ARG.  A failed call
 * leaves what was installed; tiny_batch_reset leaves the plant alone.  Synchronous; works on tiny_batch_setup and
 * tiny_batch_setup_hetero batches.
 * Meaning: while a plant is installed, wherever a launch takes a plant step (the next fused step's x0, the x0_next store of
 * advance_x0), state row j of instance i becomes
 *     acc = f_p[j];  for k < nx: acc = fma(x0[k], A_p[j][k], acc);  for k < nu: acc = fma(u0[k], B_p[j][k], acc);  x0_next[j] = acc
 * (then fl(acc + w[k][i]) where a disturbance row applies): x0 the state this MPC step started from, u0 the control it applied (what
 * the step log records); ONE chain, one rounding per term, in this order, whatever "dpp_mode" says and on every kernel path.  It is the
 * order of the one-row kernel's forward pass under the default "dpp_mode": a plant equal to the model reproduces the run without a
 * plant bit for bit.  A step that ran no iteration (max_iter = 0) takes no plant step.  Only x0 moves: work->x, solution->x and the x
 * record keep the solver's prediction.  A launch without a plant step reads nothing of the plant and runs the kernel form it runs
 * without one.
 * Read-backs (tiny_batch_get_option): "plant" 0 none, 1 one for all, 2 every instance its own; "last_plant" 1 when the last solve's
 * launches took their plant step through it.
 * Where it runs: the one-row kernel's PP forms (run-time instantiated; tiny_batch_kernel_path 3) of every form the PD forms exist for,
 * with or without a disturbance, on full rows; everywhere else (tile-kernel shapes, overlapping cones, "debug", "force_general",
 * "no_jit", a missing hipRTC) a helper kernel behind each single-step launch of the coverage kernel, same bits.  Adaptive rho on a
 * launch with a plant step fails the solve with TINY_ERR_UNSUPPORTED ("adaptive rho does not combine with a plant of its own ...").
 * Out of scope: the tile kernel, the half-row and PREFETCH forms, tiny_codegen, tiny_solve_batch and the drop-in structs. */
int tiny_batch_set_plant(TinyBatch* b, const double* A_p, const double* B_p, const double* f_p, int flags);
/* the plant instance `instance` is stepped by, as installed: A_p [nx*nx], B_p [nx*nu], f_p [nx] (zeros where none was given); any pointer
 * may be NULL.  TINY_ERR_ARG with none installed or an instance outside the batch */
int tiny_batch_get_plant(TinyBatch* b, int instance, double* A_p, double* B_p, double* f_p);
/* option "state_log" = 1: every launch that takes a plant step (fused steps -- cut into stretches or not --, single steps with
 * advance_x0) records, per MPC step of the solve call and per instance, the state the plant step handed on: the x0 the next step
 * started from, plant and disturbance included; a step that took no plant step logs the x0 it left in place.  x0_next is
 * [steps][batch][nx], steps at most what the last solve call ran (a single step: one row).  With neither a plant nor a disturbance
 * installed the launch takes a PD form with an empty sequence (same bits as the plain form; tiny_batch_kernel_path 3: run-time
 * instantiated even for a compiled-in shape) and a tile-kernel shape runs on the coverage kernel.  Unlike "step_log", the log does not
 * combine with adaptive rho: a launch that takes a plant step with the log on is refused (TINY_ERR_UNSUPPORTED, "adaptive rho does not
 * combine with the state log") */
int tiny_batch_get_state_log(TinyBatch* b, double* x0_next, int steps);
/* measurement noise in a closed loop (advance_x0, steps_per_launch > 1): the controller solves from a noisy reading of the state while
 * the plant evolves from the true one -- sensor noise without the host in the loop.  v [n_steps][batch][nx], step-major; flags TINY_HOST
 * or TINY_DEVICE, with TINY_BROADCAST one [n_steps][nx] for all (as tiny_batch_set_disturbance); copied, the caller may free.  v == NULL or
 * n_steps <= 0 removes the sequence.  A failed call leaves what was installed; tiny_batch_reset leaves the sequence and its counter alone.
 * Meaning: while a sequence is installed, the x0 record is the plant's TRUE state.
 *   Measurement: MPC step k of a launch that takes a plant step hands the solver xm = fl(x0 + v[k][i]) -- ONE IEEE double addition,
 *     nothing fused into it; work->x[:,0] of that solve is xm and the whole solve runs from xm.
 *   Plant step: it then starts from the true x0 and the applied u0, through the one fma chain tiny_batch_set_plant documents: by the
 *     installed plant, or with none by the batch's own model A, B, f (instance i's own on a tiny_batch_setup_hetero batch; the library
 *     forms the block itself, "plant" keeps reading 0); then fl(. + w[k][i]) where a disturbance row applies.  The result is the next
 *     true x0, and what the state log records.
 *   Step counter: k is a counter of its own with the disturbance counter's rules -- the setter rewinds it, every MPC step of a launch
 *     with a plant step advances it (inside stretches too), option "measurement_step" moves it; steps with k outside [0, n_steps) hand
 *     on x0 itself: no addition, not one of zero.
 *   A step that ran no iteration (max_iter = 0) still sees its measurement in x[:,0]; it takes no plant step.
 *   A launch without a plant step reads nothing, leaves the counter alone and runs the form it runs without a sequence.
 * Read-backs (tiny_batch_get_option): "measurement_noise" n_steps as installed (0: none), "measurement_step" the counter,
 * "last_measurement_noise" 1 when the last solve's launches applied the sequence.
 * Where it runs: the one-row kernel's PM forms (run-time instantiated; always on a plant block: every form the PP forms exist for);
 * everywhere else (tile-kernel shapes, overlapping cones, "debug", "force_general", "no_jit", a missing hipRTC) a helper kernel in front
 * of each single-step launch of the coverage kernel forms the measurements and the one behind it takes the plant step, same bits.
 * Adaptive rho on such a launch fails the solve with TINY_ERR_UNSUPPORTED ("adaptive rho does not combine with measurement noise
 * (tiny_batch_set_measurement_noise)").
 * Out of scope: any estimator or filter (the solver is handed the reading as it is); the tile kernel (its shapes go to the coverage
 * kernel, as with a plant); the half-row and PREFETCH forms; tiny_codegen; tiny_solve_batch and the drop-in structs. */
int tiny_batch_set_measurement_noise(TinyBatch* b, const double* v, int n_steps, int flags);
/* row `step` of instance `instance` as installed: v_out [nx]; TINY_ERR_ARG with none installed or an index outside it */
int tiny_batch_get_measurement_noise(TinyBatch* b, int step, int instance, double* v_out);
/* the same two sequences GENERATED on the device from a seed: a Monte-Carlo episode takes a seed and a few scale vectors up instead of
 * [n_steps][batch][nx] doubles drawn on the host.  Every entry is a pure function of (seed, stream, instance id, row, entry): the noise
 * of an instance does not depend on how a study is batched or sharded, and one instance can be run again alone (a batch of one with
 * id_base = its id).  The whole definition (csrc/noise_gen.hpp holds it as code, for host and device from one text):
 *   Ids: instance i of the batch has the 64-bit id = id_base + i * id_stride (wrapping).  stream is 0 for the disturbance, 1 for the
 *     measurement noise; k is the sequence row -- the value the step counters index; p = 0 .. ceil(nx/2) - 1 the pair index.
 *   Bits: (r0, r1, r2, r3) = Philox4x32-10 of counter (id low 32, id high 32, k, (stream << 16) | p) under key (seed low 32, seed
 *     high 32): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten rounds, one round being
 *     c' = (hi(M1*c2) ^ c1 ^ k0, lo(M1*c2), hi(M0*c0) ^ c3 ^ k1, lo(M0*c0)) on 32 x 32 -> 64 bit products, then key += increments.
 *   Uniforms (exact): n1 = (r0 << 20) | (r1 >> 12), u1 = (2 n1 + 1) * 2^-53;  n2 = (r2 << 20) | (r3 >> 12), octant q = n2 >> 49,
 *     m = n2 & (2^49 - 1), t = (2 m + 1) * 2^-50;  the angle is theta = (q + t) * pi/4.
 *   Box-Muller: R = sqrt(-2 ln u1), g[2p] = R cos(theta), g[2p+1] = R sin(theta); |g| < 8.6.  ln, sin and cos are fma Horner chains of
 *     the library's own in a fixed order, on integer operations, + - * /, sqrt and fma alone (no libm): with K = 2 n1 + 1, P its top
 *     bit, e = P - 53, F = (K << (52 - P)) & (2^52 - 1): if F > 0x6A09E667F3BCD then mr = (1 + F 2^-52) / 2, e += 1, else
 *     mr = 1 + F 2^-52;  f = mr - 1, d = 2 + f, s = f / d, z = s * s;  w = 1/23, then w = fma(w, z, 1/(2j+1)) for j = 10 .. 1;
 *     zw = z * w, h = fma(s, zw, s), ln u1 = fma((double)e, LN2, h + h), LN2 = 0x3FE62E42FEFA39EF.  With a = t for even q and 1 - t for
 *     odd q: x = a * PIO4 (0x3FE921FB54442D18), y = x * x;  ws = -1/19!, then ws = fma(ws, y, c) for c = +1/17!, -1/15!, ..., -1/3!,
 *     yw = y * ws, sn = fma(x, yw, x);  wc = 1/20!, then wc = fma(wc, y, c) for c = -1/18!, +1/16!, ..., -1/2!, cs = fma(y, wc, 1);
 *     cos(theta) = (q in {1, 2, 5, 6} ? sn : cs), negated for q in {2, 3, 4, 5}; sin(theta) = (q in {1, 2, 5, 6} ? cs : sn), negated
 *     for q >= 4.  Every constant 1/n is the rounded division of the two doubles.  Host and device give the same bits.
 *   Row k of instance i: with a diagonal scale  row[j] = fma(g[j], scale[j], mean[j]);  with TINY_NOISE_FACTOR scale is an nx x nx
 *     column-major matrix S (a Cholesky factor: correlated noise; the upper triangle is read like any other entry) and
 *     acc = mean[j]; for c = 0 .. nx-1 ascending: acc = fma(g[c], S[j + nx*c], acc); row[j] = acc.  mean == NULL means zeros.  For odd
 *     nx the last pair's second deviate is dropped.
 * TinyNoiseSpec: flags is TINY_HOST or TINY_DEVICE for scale and mean (copied; the caller may free), [batch][nx] each ([batch][nx*nx]
 * for a factor), or with TINY_BROADCAST one of each for all; TINY_NOISE_FACTOR as above.
 * Installing: the call fills a fresh [n_steps][batch][nx] device buffer (one fill kernel on the batch's stream; synchronous) and
 * installs it exactly as tiny_batch_set_disturbance / tiny_batch_set_measurement_noise install a caller's sequence: the step counter
 * is rewound, a failed call leaves what was installed, tiny_batch_reset leaves it alone, and removal stays
 * tiny_batch_set_disturbance(b, NULL, 0, 0).  Everything downstream sees an ordinary sequence: the kernel forms, the getters, the options
 * "disturbance", "disturbance_step", "last_disturbance" and their measurement twins.
 * Read-backs: "disturbance_generated" / "measurement_noise_generated" read 1 while the installed sequence came from these calls, 0 once
 * a setter replaced or removed it.
 * TINY_ERR_ARG: a NULL spec or scale, n_steps <= 0, id_stride < 1, id_base < 0, unknown flag bits (a row of more than 65 536 pairs
 * cannot occur: nx <= 32).
 * Out of scope: generating inside the solve kernels instead of filling the buffer they read; distributions other than the normal;
 * tiny_codegen, tiny_solve_batch and the drop-in structs. */
typedef struct { unsigned long long seed; long long id_base, id_stride; int n_steps; int flags;
                 const double* scale; const double* mean; } TinyNoiseSpec;
int tiny_batch_generate_disturbance(TinyBatch* b, const TinyNoiseSpec* spec);
int tiny_batch_generate_measurement_noise(TinyBatch* b, const TinyNoiseSpec* spec);
/* host only, no GPU touched: rows [n_steps][batch][nx] exactly as the device fills them; stream 0 / 1; scale / mean host arrays
 * (TINY_DEVICE, a NULL out, batch <= 0, nx <= 0, nx > 131 072 or another stream: TINY_ERR_ARG) */
int tiny_noise_generate(const TinyNoiseSpec* spec, int stream, int batch, int nx, double* out);
/* a state estimator in a closed loop (advance_x0, steps_per_launch > 1): between the sensor and the MPC sits a fixed-gain observer --
 * output-feedback MPC without the host in the loop.  One nx x nx innovation gain M per instance, or with TINY_BROADCAST one for all:
 * M = L*C covers a Luenberger observer or a steady-state Kalman filter with any output matrix C.  Unmeasured states are zero columns
 * of M (the noise entries on those columns are multiplied by zero); output-space noise v_y is installed as any v with C v = v_y
 * (tiny_batch_set_measurement_noise takes state-space rows).
 * Meaning: while an estimator is installed, the x0 record is the plant's TRUE state, as under measurement noise, and the batch carries
 * an estimate record xp [batch][nx], the predicted estimate.  MPC step k of a launch that takes a plant step does, for instance i:
 *   Measurement: xm = fl(x0 + v[k][i]) where a row of an installed measurement-noise sequence applies, by that feature's rules and
 *     counter; else xm = x0, no addition: an estimator without noise is a perfect sensor behind a filter.
 *   Correction: e[c] = fl(xm[c] - xp[c]), one IEEE subtraction per state; state row j: acc = xp[j]; acc = fma(e[c], M[j][c], acc),
 *     c = 0 .. nx-1; xhat[j] = acc -- ONE chain, ascending c, one rounding per term, whatever dpp_mode says and on every kernel path.
 *   Solve: from xhat -- work->x[:,0] of that solve is xhat, the slot-0 cone and half-space slack see it.
 *   Prediction: by the controller's own model: acc = f[j]; acc = fma(xhat[c], A[j][c], acc), c < nx; acc = fma(u0[c], B[j][c], acc),
 *     c < nu; xp[j] = acc -- the chain of tiny_batch_set_plant over the batch's model (instance i's own on a tiny_batch_setup_hetero batch).
 *   Plant step: exactly as under measurement noise -- from the TRUE x0 and the applied u0, by the installed plant or with none by the
 *     model, plus the disturbance row where one applies; the state log records the true states.
 *   A step that ran no iteration (max_iter = 0) shows xhat in x[:,0]; it takes no plant step and no prediction, the estimate record keeps xp.
 *   A launch without a plant step reads nothing, leaves the estimate record alone and runs the form it runs without an estimator.
 * Two consequences: M = 0 with xp = x0 (no plant of its own, no disturbance) is bit-identical to a handle with nothing installed,
 * whatever noise is installed; and with xp = x0, no noise and no plant of its own, e = 0 at every step and the same holds for any finite M.
 * M [batch][nx*nx] column-major, or with TINY_BROADCAST one [nx*nx]; TINY_HOST | TINY_DEVICE; copied.  M == NULL removes the
 * estimator (the estimate record is freed).  Installing one where none is installed sets xp = the x0 record as it stands;
 * replacing the gain keeps xp.  A failed call leaves what was installed; tiny_batch_reset leaves gain and estimate alone.
 * Read-backs (tiny_batch_get_option): "estimator" 0 none, 1 one gain for all, 2 per instance; "last_estimator" 1 when the last solve's
 * launches went through it; "estimate_log".
 * Where it runs: the one-row kernel's PE forms (run-time instantiated; every form the PM forms exist for); everywhere else (tile-kernel
 * shapes, overlapping cones, "debug", "force_general", "no_jit", a missing hipRTC) helper kernels around each single-step launch of
 * the coverage kernel correct and predict, same bits.  Adaptive rho on such a launch fails the solve with TINY_ERR_UNSUPPORTED
 * ("adaptive rho does not combine with a state estimator (tiny_batch_set_estimator)").
 * Out of scope: time-varying or covariance-propagating filters; an output vector of its own dimension; gains computed on the device;
 * the tile kernel; the half-row and PREFETCH forms; tiny_codegen; tiny_solve_batch and the drop-in structs. */
int tiny_batch_set_estimator(TinyBatch* b, const double* M, int flags);
int tiny_batch_get_estimator(TinyBatch* b, int instance, double* M_out);           /* as installed; TINY_ERR_ARG with none */
int tiny_batch_set_estimate(TinyBatch* b, const double* xp, int flags);            /* [batch][nx]; HOST | DEVICE | BROADCAST ([nx]); TINY_ERR_ARG with no estimator */
int tiny_batch_get_estimate(TinyBatch* b, double* xp_out);                         /* [batch][nx], host */
int tiny_batch_get_estimate_log(TinyBatch* b, double* xhat, int steps);            /* option "estimate_log" = 1: [steps][batch][nx], the xhat every MPC step solved from */
/* a per-instance score of a closed loop (advance_x0, steps_per_launch > 1): what the realised trajectory cost and whether the true
 * state and the applied control left their limits, accumulated on the device -- a study reads four numbers per instance instead of
 * pulling the state log and the step log to the host.
 * All four arrays run over z = [x | u], nx + nu entries, states first: weight, target, lo, hi.  Each [batch][nx+nu], or with
 * TINY_BROADCAST one [nx+nu] for all; TINY_HOST | TINY_DEVICE; copied, the caller may free.  target == NULL means zeros, lo == NULL /
 * hi == NULL mean -inf / +inf.  weight == NULL removes the score and frees it.  A failed call leaves what was installed.
 * Meaning: while a score is installed, once per MPC step of a launch that takes a plant step, for instance i: xn is the state the
 * plant step handed on -- exactly what the state log records: by the plant installed or the model, plus the disturbance row, the TRUE
 * state under measurement noise or a state estimator --, u0 the applied control, what the step log records, z = [xn | u0].
 *   Cost: for c = 0 .. nx+nu-1 ascending: d = fl(z[c] - target[c]); s = fl(fl(weight[c] * d) * d); cost = fl(cost + s) -- three separate
 *     IEEE roundings per term, nothing fused; ONE running sum in this order on every kernel path, whatever dpp_mode says.
 *   Violation: e[c] = max(fl(z[c] - hi[c]), fl(lo[c] - z[c]), 0); m = max over c of e[c]; worst = max(worst, m); where m > 0:
 *     violated_steps += 1 and, if first_violation < 0, first_violation = k.
 *   Counter: k is a score step counter with the disturbance counter's rules: the setter and tiny_batch_reset_score rewind it, every MPC
 *     step of a launch with a plant step advances it (inside the stretches of "step_regroup" too), option "score_step" moves it.
 *   A zeroed record is cost = 0, worst = 0, violated_steps = 0, first_violation = -1.  Installing or replacing a score zeroes the
 *     record and rewinds the counter; tiny_batch_reset_score does the same and keeps the setup; tiny_batch_reset leaves setup, record
 *     and counter alone, as it does for the disturbance.
 *   The record is indexed by instance and accumulates over launches: 2 + 3 steps equal 5, bit for bit, whatever the launch form.
 *   A step that ran no iteration (max_iter = 0) takes no plant step and is not scored; the counter still advances.
 *   A launch without a plant step reads nothing, leaves record and counter alone and runs the form it runs without a score.
 *   Only the record moves: every other output of the solve keeps the bits it has without a score.
 *   Non-finite z: the record's values are unspecified.
 * Read-backs (tiny_batch_get_option): "score" 0 none, 1 one setup for all, 2 per instance; "score_step" the counter; "last_score" 1 when
 * the last solve's launches scored.
 * Where it runs: the one-row kernel's PS forms (run-time instantiated; every form the PD / PP / PM / PE forms exist for; with nothing
 * else installed the PD form with an empty sequence); everywhere else (tile-kernel shapes, overlapping cones, "debug", "force_general",
 * "no_jit", a missing hipRTC) one helper kernel behind the plant step of each single-step launch of the coverage kernel, same bits.
 * Adaptive rho on such a launch fails the solve with TINY_ERR_UNSUPPORTED ("adaptive rho does not combine with a closed-loop score
 * (tiny_batch_set_score)").
 * Out of scope: a moving target (the reference window); cone and half-space violations; sums over the batch on the device; the tile
 * kernel; the half-row and PREFETCH forms; tiny_codegen; tiny_solve_batch and the drop-in structs. */
int tiny_batch_set_score(TinyBatch* b, const double* weight, const double* target, const double* lo, const double* hi, int flags);
/* the setup instance `instance` is scored by: [nx+nu] each, any may be NULL; TINY_ERR_ARG with none installed */
int tiny_batch_get_score_setup(TinyBatch* b, int instance, double* weight, double* target, double* lo, double* hi);
/* the record: [batch] each, host, any may be NULL; TINY_ERR_ARG with none installed */
int tiny_batch_get_score(TinyBatch* b, double* cost, double* worst, int* violated_steps, int* first_violation);
int tiny_batch_reset_score(TinyBatch* b);                                          /* zeroes the record, rewinds the counter, keeps the setup */
/* an actuator model between the command and the plant step of a closed loop (advance_x0, steps_per_launch > 1): motors that saturate
 * earlier than the controller's box says, follow a command with a lag, lose effectiveness or carry a trim error, and whose thrust is
 * noisy -- the plant receives the APPLIED control ua, no longer the u0 the solver computed.
 * Setup: lo, hi, alpha, gain, offset, each [batch][nu], or with TINY_BROADCAST one [nu] for all; TINY_HOST | TINY_DEVICE; copied, the
 * caller may free.  Any may be NULL (its stage is absent); all five NULL removes the actuator.  lo[c] > hi[c] anywhere is TINY_ERR_ARG.
 * A failed call leaves what was installed.
 * Meaning: while an actuator or an actuation-noise sequence is installed, every MPC step of a launch that takes a plant step (fused
 * steps, advance_x0, the stretches of "step_regroup") turns the commanded control into the applied one.  For instance i, input
 * c = 0 .. nu-1 and actuation step counter k, uc = u0[c] is the command -- what the step log, the u record and the estimator's
 * prediction keep on seeing:
 *   1. Limits: s = uc < lo[c] ? lo[c] : (uc > hi[c] ? hi[c] : uc) -- two comparisons and two selects, no fmin / fmax: inside the limits
 *      s has uc's own bits, the sign of a zero included.  NULL lo / hi mean -inf / +inf.
 *   2. Lag (only if alpha is installed): d = fl(s - a[c]); m = fma(alpha[c], d, a[c]); a[c] <- m, where a [batch][nu] is the actuator
 *      state record.  Without alpha m = s: no arithmetic happens and no record exists.
 *   3. Gain and offset: g = fma(m, gain[c], offset[c]).  NULL gain means 1.0 and NULL offset means -0.0, so the neutral stage returns
 *      m's bits for every m.
 *   4. Noise: ua[c] = fl(g + n[k][i][c]) where row k of an installed sequence applies; otherwise ua[c] = g: no addition, not one of zero.
 * ua replaces u0 in exactly two places: the plant step -- the fma chain tiny_batch_set_plant documents, over the installed plant or,
 * with none, over the batch's own model block, as under measurement noise -- and the u entries of the score's z.  The estimator's
 * prediction uses uc: a controller does not know what its actuator did.
 *   The state log records the state handed on under ua.  Option "actuation_log" = 1 keeps ua per step: tiny_batch_get_actuation_log
 *     returns [steps][batch][nu] of the last solve call.
 *   A step that ran no iteration (max_iter = 0) takes no plant step: no stage runs, a stays, and the counter still advances.
 *   A launch without a plant step reads nothing and runs the form it runs without an actuator.
 *   Counter: k has the disturbance counter's rules: tiny_batch_set_actuation_noise and tiny_batch_generate_actuation_noise rewind it,
 *     every MPC step of a launch with a plant step advances it (inside the stretches of "step_regroup" too), option "actuation_step"
 *     moves it, rows outside [0, n_steps) add nothing.
 *   Installing a lag where none was installed zeroes a; replacing the setup keeps a.  tiny_batch_reset leaves the setup, the record,
 *     the sequence and the counter alone.
 *   An actuator with gain = ones and nothing else, on a handle whose plant equals its model, reproduces the run with nothing
 *     installed, bit for bit.
 * Read-backs (tiny_batch_get_option): "actuator" 0 none, 1 one setup for all, 2 per instance; "actuator_lag" 1 while a lag is
 * installed; "actuation_noise" n_steps as installed; "actuation_noise_generated" 1 while the installed sequence came from the
 * generator; "actuation_step" the counter; "last_actuator" 1 when the last solve's launches went through the actuator;
 * "actuation_log" the log switch.
 * Where it runs: the one-row kernel's PA forms (run-time instantiated; always on a PP form, with the PD / PM / PE / PS bits as
 * installed); everywhere else (tile-kernel shapes, overlapping cones, "debug", "force_general", "no_jit", a missing hipRTC) one helper
 * kernel behind each single-step launch of the coverage kernel, same bits.  Adaptive rho on such a launch fails the solve with
 * TINY_ERR_UNSUPPORTED ("adaptive rho does not combine with an actuator model (tiny_batch_set_actuator)").
 * Out of scope: pure transport delays; rate limits; an estimator that is told ua; the tile kernel; the half-row and PREFETCH forms;
 * tiny_codegen; tiny_solve_batch and the drop-in structs.  (Of these the transport delay has since become a stage of its own in front of
 * the limits, with an estimator that is told what left the queue: tiny_batch_set_actuator_delay below.) */
int tiny_batch_set_actuator(TinyBatch* b, const double* lo, const double* hi, const double* alpha, const double* gain, const double* offset, int flags);
/* the setup instance `instance` is actuated by, as installed, defaults filled in (alpha reads 1.0 with no lag): [nu] each, any may be
 * NULL; TINY_ERR_ARG with none installed */
int tiny_batch_get_actuator(TinyBatch* b, int instance, double* lo, double* hi, double* alpha, double* gain, double* offset);
int tiny_batch_set_actuator_state(TinyBatch* b, const double* a, int flags);       /* [batch][nu]; HOST | DEVICE | BROADCAST ([nu]); TINY_ERR_ARG with no lag */
int tiny_batch_get_actuator_state(TinyBatch* b, double* a_out);                    /* [batch][nu], host; TINY_ERR_ARG with no lag */
/* the noise of stage 4: n [n_steps][batch][nu] step-major, or with TINY_BROADCAST [n_steps][nu]; tiny_batch_set_disturbance's rules
 * (NULL / n_steps <= 0 removes; the setter rewinds the counter).  Noise alone, with no actuator, is allowed: only stage 4 runs */
int tiny_batch_set_actuation_noise(TinyBatch* b, const double* n, int n_steps, int flags);
int tiny_batch_get_actuation_noise(TinyBatch* b, int step, int instance, double* n_out);    /* [nu] */
/* ... generated on the device (tiny_batch_generate_disturbance's rules): stream 2, rows of nu entries -- scale and mean [batch][nu]
 * ([nu] with TINY_BROADCAST; TINY_NOISE_FACTOR: scale [..][nu*nu]) */
int tiny_batch_generate_actuation_noise(TinyBatch* b, const TinyNoiseSpec* spec);
/* ... and the same rows on the host, no GPU touched: out [n_steps][batch][nu] (tiny_noise_generate keeps to streams 0 and 1) */
int tiny_actuation_noise_generate(const TinyNoiseSpec* spec, int batch, int nu, double* out);
int tiny_batch_get_actuation_log(TinyBatch* b, double* ua, int steps);             /* option "actuation_log" = 1: [steps][batch][nu], the control every plant step of the last solve call received */
/* stage 0 of the actuator, a transport delay: the command computed for period k reaches the motors d periods later (the solve and the
 * link take time) -- dead time, which the lag of stage 2, a first-order filter, cannot stand in for.
 * d [batch] ints, or with TINY_BROADCAST one for all; TINY_HOST | TINY_DEVICE; 0 <= d[i] <= d_max <= TINY_MAX_DELAY, otherwise
 * TINY_ERR_ARG.  d == NULL or d_max <= 0 removes the delay.  A failed call leaves what was installed.
 * Meaning: the queue is a FIFO of instance i's last d[i] commands, state of the batch like the lag's record a.  Installing (or
 * replacing) a delay fills it with +0.0.  At every MPC step that takes a plant step, with command uc (what the step log and the u record
 * keep): d[i] == 0: s0 = uc, its own bits, nothing is read or written; d[i] > 0: s0 is the oldest entry, which leaves, and uc enters as
 * the newest.  s0 is what the limits of stage 1 see: delay -> limits -> lag -> gain -> noise.  A step that ran no iteration takes no plant
 * step: no stage runs and the queue stays.  The actuation log keeps the applied control of the delayed command.  A delay alone, with no
 * actuator and no noise, is allowed.  d == 0 everywhere reproduces the run without a delay, bit for bit.  tiny_batch_set_actuator
 * (installing, replacing, removing) and tiny_batch_reset leave the delay and its queue alone.
 * The queue: q [batch][d_max][nu], oldest first (TINY_BROADCAST: [d_max][nu]); only the first d[i] rows of an instance's slice mean
 * anything, the getter returns them oldest first and +0.0 behind them.  Setter and getter answer TINY_ERR_ARG with no delay installed.
 * The predictor (tiny_batch_set_option "delay_compensation" = 1, default 0; inert with no delay installed): MPC step k of instance i
 * does not solve from xin -- the x0 record, the reading xm under measurement noise, or xhat under an estimator -- but from
 *     xs = xin;  for t = 0 .. d[i]-1 (oldest first):  xs = f + A xs + B q[t]
 * with A, B, f the batch's OWN model (never the installed plant), every step the fma chain tiny_batch_set_plant documents (the
 * accumulator starts at f), q the queue as it stands BEFORE this step's push; d[i] == 0 leaves xin's bits alone.  As under measurement
 * noise the x0 record is the TRUE state while compensation applies: the plant step starts from it (through the installed plant or, with
 * none, the model), and the state log records true states.  With an estimator the estimate log keeps xhat, not xs, and the model's
 * prediction of the next xp starts from xhat and uses s0 -- the command the controller knows is reaching the actuator now; with
 * compensation off it keeps using uc.
 * Read-backs: "actuator_delay" d_max as installed, 0 when none; "delay_compensation" the switch; "last_actuator" covers the delay.
 * Where it runs: the one-row kernel's PQ forms (the queue; on a PA form) and PX forms (the predictor; on a PQ and a PM form), run-time
 * instantiated; everywhere else helper kernels around each single-step launch of the coverage kernel, same bits.  Adaptive rho is
 * refused as with an actuator model, in its text.
 * Out of scope: per-input delays; fractional delays; a delay on the measurement side. */
#define TINY_MAX_DELAY 8
int tiny_batch_set_actuator_delay(TinyBatch* b, const int* d, int d_max, int flags);
int tiny_batch_get_actuator_delay(TinyBatch* b, int instance, int* d_out);
int tiny_batch_set_actuator_queue(TinyBatch* b, const double* q, int flags);
int tiny_batch_get_actuator_queue(TinyBatch* b, double* q_out);                    /* [batch][d_max][nu], host, oldest first */
/* == tiny_update_settings (tiny_api.hpp:36-42).  With a linear / time-varying-linear switch on (or a shape
 * without a register-resident instantiation) the solve runs the coverage kernel (general_kernel.hip.h). */
int tiny_batch_update_settings(TinyBatch* b, double abs_pri_tol, double abs_dua_tol, int max_iter,
                               int check_termination, int en_state_bound, int en_input_bound,
                               int en_state_soc, int en_input_soc, int en_state_linear,
                               int en_input_linear, int en_tv_state_linear, int en_tv_input_linear);
/* == settings->adaptive_rho, adaptive_rho_min, adaptive_rho_max, adaptive_rho_enable_clipping (types.hpp:75-79).  With it on,
 * every 5th ADMM iteration re-estimates rho from the residuals of an OSQP-style restatement of the problem and moves Kinf,
 * Pinf (and the dead copies C1, C2) by a first-order Taylor step, as admm.cpp:397-423 / rho_benchmark.cpp:14-249 do -- NOT
 * Quu_inv, AmBKt, APf, BPf, Q, R, which the reference keeps as they were.  The cache then is per-instance STATE that persists
 * from solve to solve (tiny_batch_reset puts tiny_setup's cache back).  The reference's RhoAdapter flag is read uninitialised
 * upstream; the behaviour reproduced is the one with that flag false ("matrices sized by the first adaptation of every
 * solve"), which is also the only one that does not crash (profiles/r02_adaptive_rho_probe.txt).  One-row kernel only, shared
 * family or per-instance batch (tiny_batch_setup_hetero); not with half-spaces, overlapping cones, one_shot or repack_after.  Without
 * sensitivity tables (the two entry points below) the solve fails with TINY_ERR_DIM. */
int tiny_batch_set_adaptive_rho(TinyBatch* b, int enable, double rho_min, double rho_max, int enable_clipping);
/* == cache->dKinf_drho (nu x nx), dPinf_drho (nx x nx), dC1_drho (nu x nu), dC2_drho (nx x nx): column-major, shared by every
 * instance; dC1 / dC2 may be NULL (zero).  tiny_initialize_sensitivity_matrices (tiny_api.cpp:479-540) is the quadrotor's set.  On a
 * per-instance batch: the same tables for every instance. */
int tiny_batch_set_sensitivity(TinyBatch* b, const double* dKinf_drho, const double* dPinf_drho, const double* dC1_drho,
                               const double* dC2_drho);
/* The same four tables COMPUTED on the GPU (csrc/sensitivity_kernel.hip.h) for this batch's own system: the derivative with respect
 * to rho of the cache tiny_setup computes -- rho enters Q and R twice there -- evaluated at the cache as it stands (after
 * tiny_batch_set_cache too).  With K = Kinf, C1 = Quu_inv, Acl = A - B K:  dPinf solves dP = Acl' dP Acl + 2 (I + K' K),
 * dKinf = C1 (B' dP Acl - 2 K), dC1 = -C1 (2 I + B' dP B) C1, dC2 = -(B dKinf)'.  The reference declares such a function
 * (tiny_api.hpp:29-31) and defines none; its quadrotor literals are a DIFFERENT set (not this derivative) and stay what
 * tiny_initialize_sensitivity_matrices installs.  Shared family: installed exactly as tiny_batch_set_sensitivity would.
 * Per-instance batch: every instance's own tables, kept on the device.  Any nx + nu <= 32, nu <= 16; TINY_ERR_ARG when
 * A - B Kinf is not a contraction (no derivative exists) -- nothing is installed then.  On a per-instance batch the message
 * names the first such instance, NO instance's tables are usable and an adaptive solve fails with TINY_ERR_DIM until a later call
 * succeeds or tiny_batch_set_sensitivity installs one set; tiny_batch_get_sensitivity_instance still reads what was computed. */
int tiny_batch_compute_sensitivity(TinyBatch* b);
/* What is installed, computed or set: name = "dKinf_drho" | "dPinf_drho" | "dC1_drho" | "dC2_drho"; returns the element count. */
int tiny_batch_get_sensitivity(TinyBatch* b, const char* name, double* out, int capacity);
/* ... of one instance of a per-instance batch; the same names, or "steps": the squarings the Lyapunov solve took (1 .. 64;
 * -1: it did not converge for this instance, 0: the tables were set by the caller). */
int tiny_batch_get_sensitivity_instance(TinyBatch* b, int instance, const char* name, double* out, int capacity);
/* per-instance cache state of an adaptive batch, host arrays with a leading batch axis, column-major matrices: which =
 * "rho" [batch], "Kinf" [batch][nu*nx], "Pinf" [batch][nx*nx], "C1" [batch][nu*nu], "C2" [batch][nx*nx] */
int tiny_batch_set_cache_state(TinyBatch* b, const char* which, const double* src);
int tiny_batch_get_cache_state(TinyBatch* b, const char* which, double* dst);
/* Read back one cache matrix (TinyCache, types.hpp:43-59) by name: "Kinf" (nu x nx), "Pinf",
 * "Quu_inv", "AmBKt", "APf", "BPf", or "Q"/"R" (work->Q/R = user + rho).  Returns element count. */
int tiny_batch_get_cache(TinyBatch* b, const char* name, double* out, int capacity);
/* Overwrite one of them (same names and sizes, plus "rho": one double): a caller's own cache instead of the Riccati recursion of
 * tiny_batch_setup -- what the code generated by tiny_codegen uses to restore a frozen TinyCache. */
int tiny_batch_set_cache(TinyBatch* b, const char* name, const double* src);

/* ---- per-instance data ------------------------------------------------------------------- */
/* tiny_set_x0 / tiny_set_x_ref / tiny_set_u_ref and direct workspace pokes of the examples
 * (work->Xref = ..., work->y = 0, examples/quadrotor_tracking.cpp:89-93). */
int tiny_batch_set(TinyBatch* b, TinyField field, const double* src, int flags);
int tiny_batch_get(TinyBatch* b, TinyField field, double* dst, int flags);
/* zero every warm-start record (x,u,vnew,znew,v,z,g,y,vcnew,zcnew,gc,yc) = state after tiny_setup */
int tiny_batch_reset(TinyBatch* b);

/* ---- the hot path ------------------------------------------------------------------------ */
/* == tiny_solve (tiny_api.hpp:34): one ADMM solve of every instance from its warm state.
 * Synchronous; returns 0 when every instance converged, 1 otherwise (admm.cpp:441,454). */
int tiny_batch_solve(TinyBatch* b);
/* Same launch, asynchronous on the batch's stream; returns TINY_OK after enqueueing. */
int tiny_batch_solve_async(TinyBatch* b);
int tiny_batch_synchronize(TinyBatch* b);
/* ONE phase of the ADMM iteration over the whole batch, on the device records as they are (asynchronous): the
 * batched form of the phase functions the reference exports (src/tinympc/admm.hpp:12-17).  Reads / writes exactly
 * the workspace fields the reference function does (x|u, q|r, p|d, the slack and dual families). */
enum {
    TINY_PHASE_LINEAR_COST = 1,   /* update_linear_cost     admm.cpp:262-304 */
    TINY_PHASE_BACKWARD = 2,      /* backward_pass_grad     admm.cpp:13-20   */
    TINY_PHASE_FORWARD = 3,       /* forward_pass           admm.cpp:25-32   */
    TINY_PHASE_SLACK = 4,         /* update_slack           admm.cpp:81-211  */
    TINY_PHASE_DUAL = 5,          /* update_dual            admm.cpp:219-256 */
    TINY_PHASE_TERMINATION = 6    /* termination_condition  admm.cpp:310-328: the four residuals (always evaluated);
                                     tiny_batch_get_status' `solved` array then holds the returned bool */
};
int tiny_batch_phase(TinyBatch* b, int phase);
/* solution->iter, solution->solved, work->status, and the four residuals
 * {primal_state, primal_input, dual_state, dual_input} ([batch][4]); any pointer may be NULL. */
int tiny_batch_get_status(TinyBatch* b, int* iter, int* solved, int* status, double* residuals);
/* Device-side reduction over the batch: out[0..9] = {sum iter, sum solved, batch,
 * max primal_state, max primal_input, max dual_state, max dual_input,
 * iterations accumulated since the last tiny_batch_reset, converged solves accumulated, 0}.
 * host_out and/or device_out (a device pointer to 10 doubles, e.g. the buffer handed to an
 * RCCL collective) may be NULL. */
int tiny_batch_reduce_stats(TinyBatch* b, double* host_out, void* device_out);

/* ---- plumbing ---------------------------------------------------------------------------- */
/* Options: "advance_x0" (1: each solve also writes x0 <- A x0 + B u[:,0] + f, the plant step of
 * the examples' closed loop, examples/quadrotor_hovering.cpp:92), "debug" (1: keep q,r,p,d),
 * "grid_waves_per_cu" (persistent-grid size, 0 = one wave per tile), "dpp_mode" (2 [default] fused
 * v_fmac_f64_dpp on one accumulator chain, 0 the same on two chains, 1 v_mov_dpp + v_fma), "timing" (n: record HIP events for the next n solves),
 * "prefer_tile" / "no_tile" (experiments: take / avoid the tile kernel where a choice exists),
 * "force_general" (1: use the coverage kernel even when a
 * register-resident instantiation exists), "steps_per_launch" (T >= 1: every solve call runs T closed-loop MPC steps -- solve, plant step
 * x0 <- A x0 + B u[:,0] + f, solve, ... -- inside ONE launch with the ADMM state held in registers;
 * references stay fixed during the launch), "step_log" (1: keep per-step iteration counts / u0),
 * "reset_duals" (1: g = 0, y = 0 before every solve, examples/quadrotor_tracking.cpp:92-93), "traj_step",
 * "one_shot" (one-shot / cold solves: the warm-start state is taken as zero -- the state after tiny_setup or
 * tiny_batch_reset -- WITHOUT being read, and only the results are written: 1 = x|u and vnew|znew (solution->x|u),
 * 2 = x|u only, the bytes_cold = 8(nx+2S)+44 traffic of a solve that is not going to be warm-started; the other
 * warm-start records are left as they were.  Round 5: every shape -- wide and long ones on the tile kernel's EXT forms, as are
 * reference windows, "reset_duals" and per-instance problem data; the coverage kernel (overlapping cones, no hipRTC) runs these launch
 * forms and fused steps too, as a loop of single-step launches, and then writes every record back),
 * "repack_tail" (default -1 = 0; 1: the open instances of a split solve's capped first stage run to max_iter in ONE launch of the tile
 * kernel's dynamic slot form instead of the follow-up stages; bit-identical; measured slower than the staged lists under the default
 * dispatch -- profiles/r06_negative_results.md -- and therefore off; read-back "last_tail_tile"),
 * "one_shot_fast" (default 1, round 6: a one-shot launch of a wide / long shape rides on the shape's fast box form -- LDS-offload set,
 * dynamic slots; a form that streams v|z streams into a scratch array of the record's shape, allocated on first use, so that the
 * record stays untouched -- 1.2-1.9x the rate of the all-in-registers form, which 0 brings back; profiles/r06_one_shot_tile_forms.md),
 * "plan" (default 1: a fresh handle whose shape, settings and batch bucket match an entry of tinympc_amd/data/plans.txt -- or of the
 * file TINYMPC_AMD_PLANS names; "0": none -- takes that entry's launch form on its FIRST solve instead of probing; read-back
 * "plan_shipped"; tools/make_plans.py writes the file),
 * "het_ub" (default 1: per-instance problem data with a knot-invariant box takes the variant that keeps the box in two registers),
 * "repack_after" (-1, the default: automatic -- K is derived from the iteration histogram of the batch's previous solve by a
 * cost model, 0 (a plain launch) when the counts are uniform enough that splitting would not pay 5 %; 0: never split;
 * K > 0: split solve for batches whose iteration counts diverge -- the launch stops at iteration K, the
 * instances still open are listed by the kernel itself and carried on to 2K, 4K, ... max_iter by follow-up launches, four
 * open instances per wave at every stage, so that a slow instance no longer holds a wave by itself.  Results are
 * bit-identical to the unsplit solve; K is rounded down to a multiple of check_termination.  Worth it for cold solves
 * with a tail of slow instances (config 3: -16 %), not for warm MPC steps (every stage is a launch).  One-row kernel,
 * single-step launches without "advance_x0" / "one_shot"; ignored elsewhere.  "repack_growth" (default 2) and
 * "repack_waves_per_cu" (default 8) tune the stage schedule and the grid of the follow-up launches),
 * "store_primal" (default 1; 0: launches do not write work->x|u back -- between closed-loop steps with "advance_x0" it has
 * no consumer, the plant step and solution->x|u = vnew|znew are still written; tiny_batch_get(TINY_F_X / TINY_F_U) then
 * returns stale data; 2: only the first knot is written -- x[:,0], x[:,1] and u[:,0], the control a closed-loop caller applies.
 * Ignored while a cone / half-space family is enabled, whose slack the next solve initialises from x|u).
 * "share_ref" (default 1: when Xref and Uref were set with TINY_BROADCAST -- or never -- every instance reads ONE reference
 * record instead of its own copy; 0 switches that off).
 * "launch_order" (default 1: successive plain launches of the register kernel walk the batch in ALTERNATING directions, so that a
 * warm launch begins with the records its predecessor touched last -- the ones the 256 MiB Infinity Cache in front of HBM still
 * holds; 0: always ascending; 2: always descending.  Instances are independent: no result depends on it.  With the same aim the box
 * variants store work->x|u -- written once per launch, never read back by a kernel -- with nontemporal stores).
 * "half_rows" (default -1 / 1: shapes with nx + nu <= 8 run TWO instances per 16-lane row, eight per wavefront, where that form is
 * compiled in -- bit-identical to the one-instance-per-row form; 0: off; read-back "last_half_rows").
 * "prefetch" (round 6; default -1: a plain single-step launch of the register kernel's box variant over a batch that gives every
 * resident wavefront at least three tiles -- and the first stage of a split solve -- runs as PERSISTENT waves that draw their tiles
 * from a ticket counter and receive the NEXT tile's warm-start / reference records by LDS-DMA while the current tile iterates: at
 * two waves per SIMD a wave's load phase otherwise hides behind one neighbour only; 0: never; 1: wherever the form exists, any
 * batch size.  Same instructions per iteration, instances independent: bit-identical.  "prefetch_static" (default -1 = by rule, 75 for warm launches and 50 for cold ones: percent of
 * a wave's tiles it takes by grid stride before it draws tickets), "prefetch_waves" (default 0 = what is resident; > 0: cap on the
 * persistent grid); read-back "last_prefetch").
 * "step_regroup" (fused launches, "steps_per_launch" > 1, of the register kernel.  The four rows of a wavefront run in lock step: a
 * wave costs what its slowest row costs.  -1, the default: when the iteration totals of the batch's previous fused launch say that
 * this costs >= 5 %, the launch runs as STRETCHES of K = steps / 4 (at least 8) MPC steps, each over the instances ordered by the
 * iteration count of their last solve -- a counting sort on the device between the stretches; K > 0: stretches of K steps; 0: never.
 * Every stretch is the launch steps_per_launch = K would have made: bit-identical results, step logs included.  Rocket landing with
 * the thrust cone, 65 536 instances x 90 steps: 30.2 -> 27.0 ms; a batch of identical instances is never cut.
 * "step_regroup_streams" (default 2: the two halves of the batch on two streams, half a stretch out of step, joined back into the
 * batch's stream inside the solve call; 1: one stream).  Read-backs "step_regroup_stretches", "step_regroup_verdict",
 * "lockstep_permille"),
 * "repack_sort" (split solves: -1, the default: a follow-up stage predicted to run >= 60 us takes its list of open instances ordered
 * by residual / tolerance, largest first -- instances that are equally far from converging share a wave; 1: every stage; 0: never.
 * Bit-identical; (12,2,30) x 131 072: 12.6 -> 10.9 ms.  Read-back "repack_sorted_stages").
 * A solve that converges at its first termination check never stores v|z: the reference returns before v = vnew. */
int tiny_batch_set_option(TinyBatch* b, const char* name, long value);
/* derived state: "auto_split_k" (the K the automatic split solve derived from the last iteration histogram; 0 = plain launch),
 * "auto_split_permille" (its predicted time, in 1/1000 of the plain launch's), "repack_after" */
long tiny_batch_get_option(TinyBatch* b, const char* name);
/* The settled launch form of a batch as plain data.  The library decides by the clock how a batch is launched (plain or split solve
 * and its K / stage schedule, the tile kernel's dynamic form for a one-row shape, stretches of MPC steps for a fused launch); the first
 * solves of a batch are probes.  tiny_batch_get_plan exports what they found, tiny_batch_set_plan imports it into another handle of
 * the same (nx, nu, N) -- in this process or another one: the plan is a POD without pointers, write it to a file as it is -- which
 * then takes the settled form on its FIRST solve.  A plan is advice about launch forms only: results are bit-identical whatever it
 * says.  It applies to solves with the max_iter it was learnt for (auto_cap_max_iter).  open_questions > 0: the exporter had not
 * finished probing (the importer carries on where it stopped). */
#define TINY_PLAN_MAGIC   0x4e4c5054   /* "TPLN" */
#define TINY_PLAN_VERSION 1
typedef struct TinyBatchPlan {
    int magic, version, bytes;
    int nx, nu, N, batch, max_iter, check_termination;
    int open_questions;
    int auto_verdict, auto_cap, auto_cap_max_iter, auto_growth, growth_verdict, auto_probes;   /* split solve: 1 kept / -1 rejected, K, its max_iter, stage growth 2 | 4 */
    int tile_verdict, regroup_verdict, hist_valid;                                             /* tile alternative / stretches of MPC steps: 1 on, -1 off, 0 open */
    double auto_plain_rate, auto_split_rate, auto_gain, tile_rate, lockstep_ratio;             /* the clock readings behind the verdicts (ms per instance-iteration) */
    unsigned hist[1024];                                                                       /* iteration histogram the schedule came from */
} TinyBatchPlan;
int tiny_batch_get_plan(TinyBatch* b, TinyBatchPlan* out);
int tiny_batch_set_plan(TinyBatch* b, const TinyBatchPlan* in);
/* the cost model behind "repack_after" = -1 by itself (host arithmetic, no GPU): hist[1024], hist[i] = instances whose solve takes
 * i iterations; returns the proposed K (0 = plain launch), *ratio = predicted time of the best split / of the plain launch */
int tiny_predict_split(const unsigned* hist, int nx, int nu, int N, int max_iter, int check_termination, int num_cus, double* ratio);
/* the schedule behind "step_regroup" by itself (host arithmetic, no GPU): the stretches a fused launch of `steps` MPC steps is cut into
 * -- k > 0: stretches of k steps, k <= 0: the automatic length (steps / 4, at least 8); known = 0: nothing is known about the instances
 * yet, ONE step of all of them goes first; half = 1: the second half of the batch under "step_regroup_streams" = 2, half a stretch out
 * of step with the first.  Writes the lengths to out[0 .. capacity), returns their number (their sum is `steps`). */
int tiny_step_regroup_plan(int steps, int k, int known, int half, int* out, int capacity);
int tiny_batch_set_stream(TinyBatch* b, void* hip_stream);      /* run on a caller-owned stream */
/* Closed-loop tracking (examples/quadrotor_tracking.cpp:65,89): a reference trajectory of n_points state
 * vectors ([n_points][nx] doubles), shared by every instance.  While it is set, the state reference of a solve
 * is the N-knot window starting at (MPC step counter + offsets[instance]); the counter starts at 0, advances by
 * one per MPC step (also inside fused launches) and can be moved with set_option("traj_step", k).  offsets may be
 * NULL; xref_points == NULL switches back to the per-instance Xref records.
 * What is left in the records DIFFERS by kernel path (tiny_batch_kernel_path tells which one runs):
 *   - register-resident kernels (one-row, tile): the window lives in registers; the Xref records keep what the caller set, and
 *     "one_shot" writes only the records its store mask names (g|y, v|z stay as they were);
 *   - coverage kernel (overlapping cones, no hipRTC): every windowed launch WRITES the window of its last MPC step into the Xref
 *     records (they are per-instance from then on: after set_reference_trajectory(NULL) they hold that window, not the caller's
 *     earlier reference -- set Xref again), and a "one_shot" launch rewrites EVERY warm-start record (prim, slack, dual,
 *     slack_prev, cone and half-space slacks) with the state the solve ended in.
 * A caller that leaves one_shot / windowed mode and must not depend on the path resets the batch (tiny_batch_reset) or sets Xref
 * and the warm-start fields it relies on. */
int tiny_batch_set_reference_trajectory(TinyBatch* b, const double* xref_points, int n_points, const int* offsets, int flags);
/* After a launch with "steps_per_launch" = T > 1 and "step_log" = 1: per fused MPC step and instance,
 * iters[T][batch] (negative = that solve hit max_iter) and the applied control u0[T][batch][nu]. */
int tiny_batch_get_step_log(TinyBatch* b, int* iters, double* u0, int steps);
/* kernel durations (ms) of the solves recorded since "timing" was set; returns the count */
int tiny_batch_get_timing(TinyBatch* b, float* ms, int capacity);
const char* tiny_batch_last_error(TinyBatch* b);
/* (nx,nu,N) kernel instantiations compiled into the library: writes up to capacity triples, returns the count */
int tiny_batch_supported_dims(int* triples, int capacity);
/* which kernel the next solve runs: 0 one-row register-resident kernel (admm_kernel.hip.h), 1 tile kernel
 * (tile_kernel.hip.h: wide / long shapes, W x R DPP rows per instance), 2 coverage kernel (general_kernel.hip.h),
 * 3 / 4 the one-row / tile kernel instantiated at run time with hipRTC for a shape outside kernel_dims.txt / tile_dims.txt
 * (first use costs about a second; option "no_jit" = 1 keeps such shapes on the coverage kernel) */
int tiny_batch_kernel_path(TinyBatch* b);
/* Run-time instantiated kernels and the disk cache.  With the environment variable TINYMPC_AMD_JIT_CACHE=<directory> the
 * compiled code objects are kept in that directory (one file per instantiation, keyed by the kernel sources, the compile
 * options and the hipRTC version; written atomically, so the ranks of a job may share it) and later processes load them
 * instead of compiling.  tiny_jit_compile() compiles one instantiation by its C++ name, e.g.
 * "tinympc_amd::admm_solve_kernel<5, 3, 7, false, false, 0, 0, false, 4>", without loading it: it needs no GPU, so an image
 * build can fill the directory.  tiny_jit_used() lists the names this process instantiated so far (newline separated) --
 * what to feed tiny_jit_compile() elsewhere.  Returns the code-object size in bytes (> 0; *from_disk = 1 if it was found in
 * the directory), or TINY_ERR_HIP with the reason in msg. */
long tiny_jit_compile(const char* instantiation, int* from_disk, char* msg, int msg_len);
/* The PREBUILT store (round 6): <directory of the library>/jit_prebuilt/ (TINYMPC_AMD_JIT_PREBUILT=<dir> overrides, "0": off) holds
 * code objects compiled at BUILD time -- tinympc_amd.build() calls tiny_jit_prebuild() for every name of csrc/jit_prebuilt.txt (the
 * run-time instantiated forms the BASELINE-shaped workloads of bench.py take).  They are keyed by the kernel sources, the name and the
 * options, NOT by the hipRTC version of the running process: a process that has loaded another ROCm's compiler (PyTorch wheels bring
 * their own libhiprtc / libamd_comgr) runs the build's code, and the first launch of a listed form reads a file instead of compiling.
 * Looked up after TINYMPC_AMD_JIT_CACHE, before compiling.  Returns the code-object size, 0 if the file was already there, or
 * TINY_ERR_HIP with the reason in msg.  dir NULL: the library's own store. */
long tiny_jit_prebuild(const char* instantiation, const char* dir, char* msg, int msg_len);
int tiny_jit_used(char* out, int out_len);                   /* returns the number of names; out may be NULL */
/* bytes of HBM traffic one warm solve must move per instance: 8*(nx + 8*S) + 44, S = nx*N + nu*(N-1)
 * (SURVEY.md section 8(d)); cold = 8*(nx + 2*S) + 44 */
long tiny_batch_algorithmic_bytes(TinyBatch* b, int cold);   /* cold: 0 bytes_warm, 1 bytes_cold (one_shot = 2), 2 one_shot = 1 */

/* ------------------------------------------------------------------------------------------ */
/* (C) Multi-GPU.  The path shards embarrassingly: instances are independent QPs, so a batch is
 * split over the GPUs with NO data-path collective; the only exchange is one 64-byte statistics message per shard --
 * {sum iter, sum solved, accumulated iterations, accumulated solves, the four residual maxima} -- moved by ONE RCCL
 * all-gather over xGMI and reduced (SUM / MAX) on the host.
 *
 * TinyGroup: ONE host process (the reference's callers are single-process C++ programs, examples/quadrotor_hovering.cpp)
 * drives several GPUs.  Each shard is an ordinary TinyBatch on its own device and stream (tiny_group_shard): a group
 * solve enqueues every shard without waiting.  interleaved = 0: contiguous blocks of instances per shard; 1: instance i
 * lives on shard i % n_shards (round-robin: balances batches whose iteration counts diverge).  devices == NULL: shard k
 * on GPU k % device_count; n_shards <= 0: one shard per GPU.  Shards that share a GPU (more shards than GPUs) exchange
 * through host memory -- RCCL refuses two ranks on one device -- with the identical reduction. */
typedef struct TinyGroup TinyGroup;
int tiny_group_setup(TinyGroup** out, const double* Adyn, const double* Bdyn, const double* fdyn, const double* Qdiag,
                     const double* Rdiag, double rho, int nx, int nu, int N, int batch, const int* devices, int n_shards,
                     int interleaved, int verbose);
int tiny_group_destroy(TinyGroup* g);
int tiny_group_shards(TinyGroup* g);                          /* number of shards */
TinyBatch* tiny_group_shard(TinyGroup* g, int k);             /* shard k: every tiny_batch_* call works on it */
int tiny_group_shard_indices(TinyGroup* g, int k, int* idx, int capacity);   /* caller-order instance ids of shard k; returns its size */
int tiny_group_uses_rccl(TinyGroup* g);                       /* 1: the exchange is an RCCL all-gather, 0: host memory (shared devices) */
const char* tiny_group_last_error(TinyGroup* g);
/* problem-family setters and options: forwarded to every shard (same meaning as the tiny_batch_* functions) */
int tiny_group_set_bound_constraints(TinyGroup* g, const double* x_min, const double* x_max, const double* u_min, const double* u_max);
int tiny_group_set_instance_bounds(TinyGroup* g, const double* x_min, const double* x_max,
                                   const double* u_min, const double* u_max);   /* host, full batch axis, caller order */
int tiny_group_set_cone_constraints(TinyGroup* g, int n_state_cones, const int* Acx, const int* qcx, const double* cx,
                                    int n_input_cones, const int* Acu, const int* qcu, const double* cu);
int tiny_group_set_linear_constraints(TinyGroup* g, int n_state, const double* Alin_x, const double* blin_x,
                                      int n_input, const double* Alin_u, const double* blin_u);
int tiny_group_set_tv_linear_constraints(TinyGroup* g, int n_state, const double* tv_Alin_x, const double* tv_blin_x,
                                         int n_input, const double* tv_Alin_u, const double* tv_blin_u);
/* every instance its own half-spaces (tiny_batch_set_instance_linear_constraints / ..._tv_...): host, full batch axis, caller order */
int tiny_group_set_instance_linear_constraints(TinyGroup* g, int n_state, const double* Alin_x, const double* blin_x,
                                               int n_input, const double* Alin_u, const double* blin_u);
int tiny_group_set_instance_tv_linear_constraints(TinyGroup* g, int n_state, const double* tv_Alin_x, const double* tv_blin_x,
                                                  int n_input, const double* tv_Alin_u, const double* tv_blin_u);
/* every instance its own cone coefficients (tiny_batch_set_instance_cone_coefficients): host, full batch axis, caller order; flags: TINY_HOST */
int tiny_group_set_instance_cone_coefficients(TinyGroup* g, const double* cx, const double* cu, int flags);
/* every instance its own disturbance sequence (tiny_batch_set_disturbance): host, [n_steps][batch][nx] over the full batch axis in the
 * caller's order, or with TINY_BROADCAST one [n_steps][nx]; NULL removes.  tiny_group_set_option forwards "disturbance_step" */
int tiny_group_set_disturbance(TinyGroup* g, const double* w, int n_steps, int flags);
/* a plant of its own (tiny_batch_set_plant): host arrays over the full batch axis in the caller's order, or with TINY_BROADCAST one
 * plant; A_p == NULL removes.  tiny_group_set_option forwards "state_log"; the log is read shard by shard (tiny_group_shard) */
int tiny_group_set_plant(TinyGroup* g, const double* A_p, const double* B_p, const double* f_p, int flags);
/* measurement noise (tiny_batch_set_measurement_noise): host, [n_steps][batch][nx] over the full batch axis in the caller's order, or
 * with TINY_BROADCAST one [n_steps][nx]; NULL removes.  tiny_group_set_option forwards "measurement_step" */
int tiny_group_set_measurement_noise(TinyGroup* g, const double* v, int n_steps, int flags);
/* the two sequences generated on the shards' devices (tiny_batch_generate_disturbance / ..._measurement_noise): id_base / id_stride name
 * the CALLER-order instance; scale / mean host arrays over the full batch axis in the caller's order, or with TINY_BROADCAST one.
 * Every shard fills its own instances' rows: the noise of caller-order instance i does not depend on the sharding */
int tiny_group_generate_disturbance(TinyGroup* g, const TinyNoiseSpec* spec);
int tiny_group_generate_measurement_noise(TinyGroup* g, const TinyNoiseSpec* spec);
/* a state estimator (tiny_batch_set_estimator, tiny_batch_set_estimate): host, M [batch][nx*nx] / xp [batch][nx] over the full batch
 * axis in the caller's order, or with TINY_BROADCAST one; M == NULL removes.  tiny_group_set_option forwards "estimate_log"; the log
 * and the estimate are read shard by shard (tiny_group_shard) */
int tiny_group_set_estimator(TinyGroup* g, const double* M, int flags);
int tiny_group_set_estimate(TinyGroup* g, const double* xp, int flags);
/* a closed-loop score (tiny_batch_set_score): host, [batch][nx+nu] each over the full batch axis in the caller's order, or with
 * TINY_BROADCAST one; weight == NULL removes.  tiny_group_set_option forwards "score_step"; the record is read shard by shard
 * (tiny_group_shard) */
int tiny_group_set_score(TinyGroup* g, const double* weight, const double* target, const double* lo, const double* hi, int flags);
/* an actuator model (tiny_batch_set_actuator and its neighbours): host, [batch][nu] each over the full batch axis in the caller's order,
 * or with TINY_BROADCAST one; the noise [n_steps][batch][nu]; generated noise does not depend on the sharding.  tiny_group_set_option
 * forwards "actuation_step" and "actuation_log"; the record and the log are read shard by shard (tiny_group_shard) */
int tiny_group_set_actuator(TinyGroup* g, const double* lo, const double* hi, const double* alpha, const double* gain, const double* offset, int flags);
int tiny_group_set_actuator_state(TinyGroup* g, const double* a, int flags);
int tiny_group_set_actuation_noise(TinyGroup* g, const double* n, int n_steps, int flags);
int tiny_group_generate_actuation_noise(TinyGroup* g, const TinyNoiseSpec* spec);
/* the transport delay (tiny_batch_set_actuator_delay, tiny_batch_set_actuator_queue): host, d [batch] / q [batch][d_max][nu] over the
 * full batch axis in the caller's order, or with TINY_BROADCAST one; tiny_group_set_option forwards "delay_compensation"; the queue is
 * read shard by shard (tiny_group_shard) */
int tiny_group_set_actuator_delay(TinyGroup* g, const int* d, int d_max, int flags);
int tiny_group_set_actuator_queue(TinyGroup* g, const double* q, int flags);
int tiny_group_update_settings(TinyGroup* g, double abs_pri_tol, double abs_dua_tol, int max_iter, int check_termination,
                               int en_state_bound, int en_input_bound, int en_state_soc, int en_input_soc,
                               int en_state_linear, int en_input_linear, int en_tv_state_linear, int en_tv_input_linear);
int tiny_group_set_option(TinyGroup* g, const char* name, long value);
/* per-instance data with the FULL batch axis, host memory, the caller's instance order (flags: TINY_HOST or TINY_BROADCAST) */
int tiny_group_set(TinyGroup* g, TinyField field, const double* src, int flags);
int tiny_group_get(TinyGroup* g, TinyField field, double* dst);
int tiny_group_reset(TinyGroup* g);
/* == tiny_solve on every shard; tiny_group_solve returns 0 when every instance on every GPU converged, else 1 */
int tiny_group_solve(TinyGroup* g);
int tiny_group_solve_async(TinyGroup* g);
int tiny_group_synchronize(TinyGroup* g);
int tiny_group_get_status(TinyGroup* g, int* iter, int* solved, int* status, double* residuals);   /* caller order */
/* the one exchange: out10 = job-wide statistics in the tiny_batch_reduce_stats layout (waits for every shard) */
int tiny_group_allreduce_stats(TinyGroup* g, double* out10);
/* One process per GPU (MPI / torchrun-style hosts): the same 64-byte exchange on a communicator the CALLER created with
 * ncclCommInitRank; rccl_comm = its ncclComm_t.  Enqueued on the batch's stream behind the solve, returns when the
 * stream has drained, the same job-wide vector on every rank.  total_batch = the unsharded batch size. */
int tiny_batch_allreduce_stats(TinyBatch* b, void* rccl_comm, int n_ranks, int rank, long total_batch, double* out10);
/* Communicator plumbing for hosts that have no RCCL binding of their own: rank 0 draws the 128-byte ncclUniqueId, the host
 * hands it to every rank (MPI_Bcast, a file, torch.distributed ...), each rank joins on its device.  *comm is an ncclComm_t. */
int tiny_rccl_unique_id(void* id128);
int tiny_rccl_comm_init_rank(void** comm, int n_ranks, const void* id128, int rank, int device);
int tiny_rccl_comm_destroy(void* comm);
int tiny_rccl_comm_count(void* comm);    /* ranks of the communicator (ncclCommCount), or TINY_ERR_NULL / TINY_ERR_HIP (< 0) */
int tiny_rccl_available(void);          /* 1: librccl could be loaded next to this library's HIP runtime (no communicator is created) */
/* Only the message: the 8 doubles {sum iter, sum solved, accumulated iterations, accumulated solves, max primal_state,
 * primal_input, dual_state, dual_input} of this batch, written to device memory on the batch's stream behind the solve,
 * for hosts that run the collective themselves (bench.py hands it to torch.distributed = RCCL). */
int tiny_batch_stats_message(TinyBatch* b, void* device_out);
/* ... and the host reduction of the gathered n_shards x 8 table -> the 10-entry statistics vector (SUM over the counts, MAX over
 * the residuals; a NaN residual survives), as the two allreduce entry points run it.  Host code only: works without a GPU. */
int tiny_reduce_stats_messages(const double* table, int n_shards, long total_batch, double* out10);

/* ------------------------------------------------------------------------------------------ */
/* (B) Reference entry points over plain-data mirrors of the reference structs.
 *
 * Layout contract (x86-64, Eigen 3.4.90, measured with offsetof against the reference's own
 * src/tinympc/types.hpp, see SURVEY.md section 8(b) and tests/test_abi_layout.py):
 *   tinyMatrix  = {double* data; int64 rows; int64 cols}   (DenseStorage.h:453-457)
 *   tinyVector  = {double* data; int64 rows}                (DenseStorage.h:613-616)
 *   VectorXi    = {int* data;    int64 rows}
 * Eigen objects passed BY VALUE through C linkage arrive, under the Itanium C++ ABI, as a
 * pointer to a caller-owned temporary -- hence the `const Tiny*POD*` parameters below.          */
typedef struct { double* data; int64_t rows; int64_t cols; } TinyMatrixPOD;
typedef struct { double* data; int64_t rows; } TinyVectorPOD;
typedef struct { int* data; int64_t rows; } TinyVectorXiPOD;

typedef struct {                 /* types.hpp:32-37, 56 bytes */
    int iter;
    int solved;
    TinyMatrixPOD x;
    TinyMatrixPOD u;
} TinySolution;

typedef struct {                 /* types.hpp:43-59, 280 bytes */
    double rho;
    TinyMatrixPOD Kinf, Pinf, Quu_inv, AmBKt;
    TinyVectorPOD APf, BPf;
    TinyMatrixPOD C1, C2;
    TinyMatrixPOD dKinf_drho, dPinf_drho, dC1_drho, dC2_drho;
} TinyCache;

typedef struct {                 /* types.hpp:63-82, 88 bytes */
    double abs_pri_tol;
    double abs_dua_tol;
    int max_iter;
    int check_termination;
    int en_state_bound;
    int en_input_bound;
    int en_state_soc;
    int en_input_soc;
    int en_state_linear;
    int en_input_linear;
    int en_tv_state_linear;
    int en_tv_input_linear;
    int adaptive_rho;
    double adaptive_rho_min;
    double adaptive_rho_max;
    int adaptive_rho_enable_clipping;
} TinySettings;

typedef struct {                 /* types.hpp:88-208, 1328 bytes */
    int nx, nu, N;
    TinyMatrixPOD x, u, q, r, p, d, v, vnew, z, znew, g, y;
    TinyMatrixPOD x_min, x_max, u_min, u_max;
    int numStateCones, numInputCones;
    TinyVectorPOD cx, cu;
    TinyVectorXiPOD Acx, Acu, qcx, qcu;
    TinyMatrixPOD vc, vcnew, zc, zcnew, gc, yc;
    int numStateLinear, numInputLinear;
    TinyMatrixPOD Alin_x;
    TinyVectorPOD blin_x;
    TinyMatrixPOD Alin_u;
    TinyVectorPOD blin_u;
    TinyMatrixPOD vl, vlnew, zl, zlnew, gl, yl;
    int numtvStateLinear, numtvInputLinear;
    TinyMatrixPOD tv_Alin_x, tv_blin_x, tv_Alin_u, tv_blin_u;
    TinyMatrixPOD vl_tv, vlnew_tv, zl_tv, zlnew_tv, gl_tv, yl_tv;
    TinyVectorPOD Q, R;
    TinyMatrixPOD Adyn, Bdyn;
    TinyVectorPOD fdyn;
    TinyMatrixPOD Xref, Uref;
    TinyVectorPOD Qu;
    double primal_residual_state, primal_residual_input, dual_residual_state, dual_residual_input;
    int status;
    int iter;
} TinyWorkspace;

typedef struct {                 /* types.hpp:213-218, 32 bytes */
    TinySolution* solution;
    TinySettings* settings;
    TinyCache* cache;
    TinyWorkspace* work;
} TinySolver;

/* tiny_api.hpp:10-12 */
int tiny_setup(TinySolver** solverp, const TinyMatrixPOD* Adyn, const TinyMatrixPOD* Bdyn,
               const TinyMatrixPOD* fdyn, const TinyMatrixPOD* Q, const TinyMatrixPOD* R,
               double rho, int nx, int nu, int N, int verbose);
/* tiny_api.hpp:13-15 */
int tiny_set_bound_constraints(TinySolver* solver, const TinyMatrixPOD* x_min, const TinyMatrixPOD* x_max,
                               const TinyMatrixPOD* u_min, const TinyMatrixPOD* u_max);
/* tiny_api.hpp:16-18; positional binding of the DEFINITION (tiny_api.cpp:176-178): state first */
int tiny_set_cone_constraints(TinySolver* solver, const TinyVectorXiPOD* Acx, const TinyVectorXiPOD* qcx,
                              const TinyVectorPOD* cx, const TinyVectorXiPOD* Acu,
                              const TinyVectorXiPOD* qcu, const TinyVectorPOD* cu);
/* tiny_api.hpp:19-24 */
int tiny_set_linear_constraints(TinySolver* solver, const TinyMatrixPOD* Alin_x, const TinyVectorPOD* blin_x,
                                const TinyMatrixPOD* Alin_u, const TinyVectorPOD* blin_u);
int tiny_set_tv_linear_constraints(TinySolver* solver, const TinyMatrixPOD* tv_Alin_x, const TinyMatrixPOD* tv_blin_x,
                                   const TinyMatrixPOD* tv_Alin_u, const TinyMatrixPOD* tv_blin_u);
/* tiny_api.hpp:25-27 */
int tiny_precompute_and_set_cache(TinyCache* cache, const TinyMatrixPOD* Adyn, const TinyMatrixPOD* Bdyn,
                                  const TinyMatrixPOD* fdyn, const TinyMatrixPOD* Q, const TinyMatrixPOD* R,
                                  int nx, int nu, double rho, int verbose);
/* tiny_api.hpp:34, admm.hpp:9 */
int tiny_solve(TinySolver* solver);
int solve(TinySolver* solver);
/* tiny_api.hpp:36-43 */
int tiny_update_settings(TinySettings* settings, double abs_pri_tol, double abs_dua_tol, int max_iter,
                         int check_termination, int en_state_bound, int en_input_bound,
                         int en_state_soc, int en_input_soc, int en_state_linear, int en_input_linear,
                         int en_tv_state_linear, int en_tv_input_linear);
int tiny_set_default_settings(TinySettings* settings);
/* tiny_api.hpp:45-47 */
int tiny_set_x0(TinySolver* solver, const TinyVectorPOD* x0);
int tiny_set_x_ref(TinySolver* solver, const TinyMatrixPOD* x_ref);
int tiny_set_u_ref(TinySolver* solver, const TinyMatrixPOD* u_ref);
/* tiny_api.hpp:54: fills cache->dKinf_drho (4 x 12), dPinf_drho (12 x 12), dC1_drho (4 x 4), dC2_drho (12 x 12) with the
 * reference's quadrotor tables (tiny_api.cpp:479-540).  With settings->adaptive_rho = 1 tiny_solve then re-estimates rho
 * every 5th iteration (admm.cpp:397-423) and writes the moved cache (rho, Kinf, Pinf, C1, C2) back into the TinyCache. */
void tiny_initialize_sensitivity_matrices(TinySolver* solver);
/* The same four cache members computed for the solver's OWN system, any nx + nu <= 32, nu <= 16 (tiny_batch_compute_sensitivity:
 * the derivative of tiny_setup's cache, on the GPU).  0, or a TINY_ERR_* code.  Not the reference's declared-and-never-defined
 * function of a similar name: that one stays unexported. */
int tiny_compute_sensitivity(TinySolver* solver);
/* codegen.hpp:9-18.  The reference freezes one TinySolver into Eigen-initialised C++ for microcontrollers; these freeze the
 * solver's PROBLEM FAMILY (dimensions, settings, the cache as it stands, dynamics, costs, bounds, cones, half-spaces,
 * references; with adaptive_rho on also the sensitivity tables) into a plain-C project for this library:
 * <dir>/tinympc/tiny_data.h, <dir>/src/tiny_data.c (round-trip literals + tiny_generated_batch / tiny_generated_group, which
 * rebuild the device-resident batch -- or the multi-GPU group -- of any size from the data), <dir>/src/tiny_main.c, <dir>/Makefile. */
int tiny_codegen(TinySolver* solver, const char* output_dir, int verbose);
int tiny_codegen_with_sensitivity(TinySolver* solver, const char* output_dir, TinyMatrixPOD* dK, TinyMatrixPOD* dP,
                                  TinyMatrixPOD* dC1, TinyMatrixPOD* dC2, int verbose);
int codegen_create_directories(const char* output_dir, int verbose);
int codegen_data_header(const char* output_dir, int verbose);
int codegen_data_source(TinySolver* solver, const char* output_dir, int verbose);
int codegen_example(const char* output_dir, int verbose);
/* admm.hpp:12-17: the individual phases of one ADMM iteration on a solver's workspace.  Each uploads the workspace,
 * runs the phase on the GPU (tiny_batch_phase with a batch of one) and writes the fields the reference function
 * writes back into the workspace. */
void update_linear_cost(TinySolver* solver);
void backward_pass_grad(TinySolver* solver);
void forward_pass(TinySolver* solver);
void update_slack(TinySolver* solver);
void update_dual(TinySolver* solver);
bool termination_condition(TinySolver* solver);
/* admm.hpp:25, :34 -- `tinyVector project_soc(tinyVector s, float mu)` and
 * `tinyVector project_hyperplane(const tinyVector& z, const tinyVector& a, tinytype b)`: under the Itanium ABI the
 * Eigen return value is constructed by the callee in caller-provided storage (hidden first argument, returned in
 * rax) and the by-value Eigen argument arrives as a pointer; the result buffer is malloc'd (Eigen frees it). */
TinyVectorPOD* project_soc(TinyVectorPOD* result, const TinyVectorPOD* s, float mu);
TinyVectorPOD* project_hyperplane(TinyVectorPOD* result, const TinyVectorPOD* z, const TinyVectorPOD* a, double b);
/* rho_benchmark.hpp:5-94 -- the adaptive-rho module's own helpers.  Upstream they are C++ functions (no extern "C"), so the
 * library exports them under their Itanium names and a C header cannot declare them; for C++ callers the reference's
 * rho_benchmark.hpp IS the declaration.  The structs they take, as plain data (layout checked against the real header):
 *   void     initialize_format_matrices(RhoAdapter*, int nx, int nu, int N)                    rho_benchmark.cpp:14-43
 *   void     format_matrices(RhoAdapter*, x, u, v, z, g, y (const tinyMatrix&), TinyCache*, TinyWorkspace*, int N)   :45-145
 *   void     compute_residuals(RhoAdapter*, tinytype* pri_res, dual_res, pri_norm, dual_norm)  :147-178   (on the GPU)
 *   tinytype predict_rho(RhoAdapter*, pri_res, dual_res, pri_norm, dual_norm, current_rho)     :180-201
 *   void     update_matrices_with_derivatives(TinyCache*, tinytype new_rho)                    :203-217
 *   void     benchmark_rho_adaptation(RhoAdapter*, x, u, v, z, g, y, TinyCache*, TinyWorkspace*, int N, RhoBenchmarkResult*)   :219-253
 *   uint32_t micros()                                                                          :9-11 */
typedef struct {
    double rho_min, rho_max;
    bool clip, matrices_initialized;
    TinyMatrixPOD A_matrix, z_vector, y_vector, x_decision, P_matrix, q_vector;
    TinyMatrixPOD Ax_vector, r_prim_vector, r_dual_vector, Px_vector, ATy_vector;
    int format_nx, format_nu, format_N;
} TinyRhoAdapterPOD;
typedef struct {
    uint32_t time_us;
    double initial_rho, final_rho, pri_res, dual_res, pri_norm, dual_norm;
} TinyRhoBenchmarkResultPOD;
/* NEW: n solvers that share one cache / settings / bounds, solved in ONE launch (gather from and
 * scatter to ordinary TinySolver workspaces).  Returns 0 when all converged, else 1. */
int tiny_solve_batch(TinySolver** solvers, int n);
/* NEW: the reference has no destroy (tiny_api.cpp:25-29 leaks); this frees host + device state. */
int tiny_destroy(TinySolver* solver);

#ifdef __cplusplus
}
#endif
#endif /* TINYMPC_AMD_H */
