// admm_kernel.hip.h -- the MI355X (gfx950 / CDNA4) ADMM solve kernel.
//
// What it computes: one tiny_solve() (reference src/tinympc/admm.cpp:331-455) for each of
// `batch` independent MPC QPs that share one TinyCache (Kinf, Pinf, Quu_inv, AmBKt, APf, BPf)
// and one set of bounds / cones / settings.  Per ADMM iteration, in the reference's order:
//   update_linear_cost (admm.cpp:262-297) -> backward_pass_grad (:13-20) -> forward_pass (:25-32)
//   -> update_slack (:81-135, box + second-order cone) -> update_dual (:219-235)
//   -> termination_condition (:310-328) -> v = vnew, z = znew (:445-446).
//
// Mapping (designed for CDNA4, not translated from anything):
//   * A 16-lane DPP row of a wave64 owns ONE problem instance; a wavefront carries 4.
//     Lane j of the row owns ROW j of the stacked knot vector [x_i ; u_i] (j < nx: state row j,
//     nx <= j < nx+nu: input row j-nx) for EVERY knot point i.  All per-element ADMM state
//     (x/u, vnew/znew, v/z, g/y, the reference-cost term) therefore lives in that lane's
//     registers as N-long arrays, and every element-wise phase (linear cost, slack projection,
//     dual update, residuals) is lane-local: no LDS, no shuffles.
//   * The Riccati sweeps need y = M * w with M a shared <=16x16 matrix and w spread one entry
//     per lane.  Lane j keeps row j of M in registers and the row-broadcast of w_k comes for free
//     from the DPP `row_newbcast:k` modifier folded into the FMA:
//         v_fmac_f64_dpp acc, w, M[j][k] row_newbcast:k       (gfx90a+ "DP-ALU DPP")
//     i.e. one FP64 FMA issue slot per matrix column, no LDS traffic, no cross-lane reduction.
//     (A broadcast-through-LDS formulation is LDS-bandwidth bound at 2x the FMA time on CDNA4:
//     8 B of LDS read per FMA vs 256 B/clk/CU LDS and 64 FP64 FMA/clk/CU.)
//   * No MFMA: FP64 MFMA on MI355X runs at the vector FP64 rate and the path is bounded by HBM
//     (few-iteration warm solves) or FP64 VALU issue (cold solves), never by matrix throughput.
//   * HBM layout = "knot-point interleaved" records, [instance][knot i][row j] with row stride
//     nx+nu, so a DPP row reads/writes one contiguous (nx+nu)*8-byte segment per knot point
//     (128 B for the quadrotor) and consecutive instances are contiguous: every byte of every
//     touched cache line is used.
//   * One workgroup = one wavefront (no __syncthreads anywhere) = by default one tile of 4 instances, so that the hardware
//     dispatcher balances tiles with different iteration counts (with a capped grid the waves walk the tiles with a grid
//     stride instead).  Rows that converge early are masked off by EXEC (per-row exit), the wave leaves the iteration loop
//     when its last row has converged.
//   * Template variants: SOC (second-order-cone slacks), DBG (keep q, r, p, d), MODE (how the row broadcast is issued),
//     LIN / KMAX (static / time-varying half-spaces), HET (per-instance problem data), ADAPT, UB, HALF, PF, PB (per-instance box), PL (per-instance half-spaces), PC (per-instance cone coefficients), PD (per-instance disturbance at the plant step), PP (a plant model of its own there), PM (the solve from a measured state; see
//     the kernel).  kernel_dims.txt lists the shapes
//     compiled into the library; every other shape / variant is instantiated at run time from this very header (jit.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tinympc_amd {

// ---- table layout shared with the host (batch_tables.hip builds it) -----------------------
// All lane tables are [column k][lane j], doubles: four matrices of `cols` columns x `lw` lanes, the VEC_* lane vectors, the bounds
// [lo | hi][N][lw], then the half-space blocks (below).  The one statement of the layout: every writer and reader of a table -- the
// host builders, the Riccati epilogue, the coverage kernel's per-instance load, both register kernels -- takes its offsets from here.
enum : int {
    VEC_CB = 0,          // backward constant: APf (state lanes), Quu_inv*BPf (input lanes)
    VEC_CF = 1,          // forward constant: fdyn (state lanes)
    VEC_QR = 2,          // work->Q / work->R (user diagonal + rho)
    VEC_SMASK = 3,       // 1.0 on state lanes else 0
    VEC_NIM = 4,         // -1.0 on input lanes else 0
    VEC_SOCFLAG = 5,     // 1.0 when this lane's cone slack is enabled (admm.cpp:102-109)
    VEC_CONE_BASE = 6,   // first lane of the cone this lane belongs to, or -1
    VEC_CONE_MU = 7,     // cone coefficient (double; truncated to float as admm.cpp:39 does)
    VEC_RHO = 8,         // per-instance tables only (HET; written by riccati_kernel.hip.h): the instance's rho on every lane
    VEC_LINFLAG = 9,     // 1.0 when this lane has a static linear-constraint slack (admm.cpp:138-145)
    VEC_TLINFLAG = 10,   // same for the time-varying family (admm.cpp:176-183)
    VEC_COUNT = 16,
};
struct LaneTab {
    int cols, lw;
    constexpr int MB() const { return 0; }                    // backward:  cols k<nx multiply p_{i+1}[k], cols nx.. multiply r_i[k-nx]
    constexpr int MF1() const { return cols * lw; }           // forward 1: cols k<nx multiply x_i[k]   (state lanes: A, input lanes: -Kinf)
    constexpr int MF2() const { return 2 * cols * lw; }       // forward 2: cols nx.. multiply u_i[k-nx] (state lanes: B)
    constexpr int PT() const { return 3 * cols * lw; }        // terminal:  cols k<nx multiply Xref[k, N-1] (state lanes: Pinf[k][j])
    constexpr int VEC() const { return 4 * cols * lw; }       // lw-entry lane vectors, see VEC_* above
    constexpr int BOUNDS() const { return VEC() + VEC_COUNT * lw; }
    constexpr int het_doubles() const { return BOUNDS(); }    // a per-instance table: the matrix + vector part (cones / masks stay shared; a per-instance box is an array of its own: SolveArgs::inst_bounds)
    // half-space tables of the LIN variants behind the bounds: static [3][kmax][lw], then per slot [N][3][kmax][lw]
    constexpr int lin_offset(int N) const { return BOUNDS() + 2 * N * lw; }
    constexpr int tlin_offset(int N, int kmax) const { return lin_offset(N) + 3 * kmax * lw; }
    constexpr int doubles(int N, int kmax) const { return tlin_offset(N, kmax) + 3 * N * kmax * lw; }
};
constexpr LaneTab ROW_TAB{16, 16};                            // the one-row kernel's tables (the tile kernel's: tile_kernel.hip.h TileTab<W>)
enum : int {
    TAB_MB = ROW_TAB.MB(), TAB_MF1 = ROW_TAB.MF1(), TAB_MF2 = ROW_TAB.MF2(), TAB_PT = ROW_TAB.PT(), TAB_VEC = ROW_TAB.VEC(),
    TAB_BOUNDS = ROW_TAB.BOUNDS(),
};
// Half-space tables of the register-resident linear-constraint variant, appended after the bounds.  Each entry is
// [constraint k < LIN_KMAX][16 lanes]: the coefficient of this lane's row (state lanes: Alin_x[k][j], input lanes:
// Alin_u[k][j-nx]), the offset b_k and ||a_k||^2 of this lane's family (b = +inf where there is no constraint k).
// The time-varying tables carry one such block per slot (input lanes shifted by one knot, like the bounds).
enum : int { LIN_KMAX = 4, LIN_KMAX_BIG = 32 };      // half-spaces per knot and family: compiled-in variants / largest run-time instantiated one
// Lane tables of the adaptive-rho variant (ADAPT; SolveArgs::atab), [column k][16 lanes] each:
enum : int {
    ATAB_AT = 0,         // cols k<nx multiply g_{i+1}[k]: state lanes A[k][j] (A' g), input lanes B[k][j-nx] (B' g)
    ATAB_DK = 256,       // dKinf_drho: state lanes cols k<nu dK[k][j] (their -Kinf' entries), input lanes cols k<nx dK[j-nx][k]
    ATAB_DP = 512,       // dPinf_drho: state lanes cols k<nx dP[k][j] (column j, the one lane j keeps up to date)
    ATAB_DC1 = 768,      // dC1_drho:   lanes j<nu cols k<nu dC1[k][j]
    ATAB_DC2 = 1024,     // dC2_drho:   state lanes cols k<nx dC2[k][j]
    ATAB_DOUBLES = 1280,
};
static inline int tab_lin_offset(int N) { return ROW_TAB.lin_offset(N); }
static inline int tab_tlin_offset(int N, int kmax = LIN_KMAX) { return ROW_TAB.tlin_offset(N, kmax); }
static inline int tab_doubles(int N, int kmax = LIN_KMAX) { return ROW_TAB.doubles(N, kmax); }

// what a closed-loop score (tiny_batch_set_score) keeps per instance: the running cost, the largest violation, the MPC steps that
// violated a limit and the first of them (-1: none)
struct ScoreRecord {
    double cost, worst;
    int violated_steps, first_violation;
};
static_assert(sizeof(ScoreRecord) == 24, "ScoreRecord: two doubles and two ints");

// what the PA forms read of an actuator model (tiny_batch_set_actuator, tiny_batch_set_actuation_noise): ONE device-resident record per
// solve call, written on the batch's stream in front of its first launch -- SolveArgs has room for one pointer to it and one int.
// tab: [instances][lo | hi | alpha | gain | offset][16 lanes] (actuator_entry of lane_tables.hpp), bit 0 of the pointer: one block for
// all, as at `plant`, bit 1: a lag is installed; the rest null: no actuator, the noise alone.  state [batch][NU]: the lag's record a.
// noise [noise_steps][batch][NU], step-major like dist, or null.  log: null, or [rows][batch][NU], the applied control of every MPC step
// of the solve call; the step whose actuation counter is k writes row k - log_step0.  All indexed by INSTANCE
struct ActuatorLaunch {
    const double* tab;
    double* state;
    const double* noise;
    double* log;
    int noise_steps, log_step0;
};
static_assert(sizeof(ActuatorLaunch) == 40, "ActuatorLaunch: four pointers and two ints");
// ... and what the PQ / PX forms read of a transport delay (tiny_batch_set_actuator_delay) and its predictor (option
// "delay_compensation"): the record grows BEHIND the 40 bytes the PA forms know -- what SolveArgs::act names is an ActuatorRecord, the
// two structs one behind the other in one device allocation, so that SolveArgs needs no further field (delay_launch_of).  delay [batch] the
// instance's d, queue [batch][d_max][NU] a ring per instance over its first d rows, head [batch] the row of the OLDEST entry (the next
// to leave; the newest enters in its place).  The predictor: model the MODEL's plant block (the layout and the bit 0 of `plant`), xhat
// [batch][NX] where a PE form keeps the corrected estimate while slot 0 of the state lanes holds the predicted state
struct DelayLaunch {
    const int* delay;
    double* queue;
    int* head;
    const double* model;
    double* xhat;
    int d_max, pad_;
};
static_assert(sizeof(DelayLaunch) == 48 && sizeof(ActuatorLaunch) % alignof(DelayLaunch) == 0, "DelayLaunch: five pointers and two ints, right behind an ActuatorLaunch");
struct ActuatorRecord {                // what Actuator::desc holds and SolveArgs::act points at: the PA forms read `a`, the PQ / PX forms `d` as well
    ActuatorLaunch a;
    DelayLaunch d;
};
static_assert(sizeof(ActuatorRecord) == 88 && __builtin_offsetof(ActuatorRecord, a) == 0 && __builtin_offsetof(ActuatorRecord, d) == sizeof(ActuatorLaunch), "ActuatorRecord: the two structs, packed");
__host__ __device__ inline const DelayLaunch* delay_launch_of(const ActuatorLaunch* act) { return &reinterpret_cast<const ActuatorRecord*>(act)->d; }

struct SolveArgs {
    const double* tab;        // tab_doubles(N) doubles
    const double* x0;         // [batch][nx]
    const double* ref;        // KPI: Xref/Uref
    double* prim;             // KPI: x/u        (out; also in when a cone is enabled, admm.cpp:352-357)
    double* slack;            // KPI: vnew/znew  (in/out)
    double* dual;             // KPI: g/y        (in/out)
    double* slack_prev;       // KPI: v/z        (in/out)
    double* cslack;           // KPI: vcnew/zcnew (out, SOC only)
    double* cdual;            // KPI: gc/yc      (in/out, SOC only)
    int4* status;             // [batch] {iter, solved, status (1 | 11), checked}
    double* resid;            // [batch][4] {pri_state, pri_input, dua_state, dua_input}
    double* x0_next;          // optional [batch][nx]: plant step x1 = A x0 + B u0 + f (may alias x0)
    double* dbg_qr;           // optional KPI: q/r of the last iteration (work->q, work->r)
    double* dbg_pd;           // optional KPI: p/d of the last iteration (work->p, work->d)
    uint2* accum;             // optional [batch] {iterations, solves converged} accumulated over successive solves
    int* iter_log;            // optional [steps][batch]: per-MPC-step iteration count (negative: not converged), steps > 1
    double* u0_log;           // optional [steps][batch][nu]: the applied control u[:,0] of every fused MPC step
    double rho, tol_pri, tol_dua;
    int batch, max_iter, check_termination;   // max_iter: where THIS launch stops (a stage of a split solve: its cap) -- the last termination test
                                              // before it is always a full one, so the residuals a launch leaves are those of its last check
    int steps;                // closed-loop MPC steps fused into this launch (>= 1; > 1 implies the plant step)
    // Reference-trajectory window (examples/quadrotor_tracking.cpp:65,89): when traj != nullptr the state
    // reference of MPC step k is traj[k + offset_b + 0 .. N-1][nx] (shared by all instances) instead of the
    // Xref part of the ref record; the window advances one knot per fused step.
    const double* traj;       // [traj_points][nx] or nullptr
    const int* traj_offsets;  // optional [batch] per-instance start offsets
    int traj_points, traj_step0;
    int reset_duals;          // 1: g = 0, y = 0 before every solve (examples/quadrotor_tracking.cpp:92-93)
    // Heterogeneous problem families (riccati_kernel.hip.h): per-instance matrix/vector tables
    // ([batch][TAB_BOUNDS] doubles, same layout as `tab`); cones and masks stay shared, and so do the bounds unless the launch is a
    // PB form (inst_bounds below), which composes with this one.
    const double* het_tabs;
    // register-resident linear constraints (LIN variants): KPI records of vlnew|zlnew, gl|yl, vlnew_tv|zlnew_tv,
    // gl_tv|yl_tv and the number of half-spaces applied per knot (max over the state / input families)
    double *lslack, *ldual, *tlslack, *tldual;
    int n_lin, n_tlin;
    // One-shot solves (SURVEY.md 8(d) bytes_cold): 1 = the warm-start state is taken as zero (the state after
    // tiny_setup / a reset) without being read.  store_mask: which records the launch writes back -- bit 0 x|u,
    // bit 1 vnew|znew (= solution->x|u), bit 2 g|y, bit 3 v|z, bit 4 the cone / linear slack and dual records, bit 5 (without bit 0) only the first
    // knot of x|u.
    int cold, store_mask;
    // Resumed solves (batch_dispatch.hip "repack_after"): an earlier launch capped at iter_base iterations has stored the ADMM
    // state of the instances that did not converge; index[0 .. *count) lists them and this launch carries on from
    // iteration iter_base with four of them per wave again.  The cone / half-space slacks are then read from their own records
    // instead of being initialised from x (admm.cpp:352-374 runs once per solve).  index == nullptr: a plain launch.
    // next_index != nullptr: this launch is itself capped below the solver's max_iter, and lists the instances it leaves
    // open for the next stage (one atomic per wave that has any; the order in the list is irrelevant to the results).
    const int* index;
    const int* count;
    int iter_base;
    int* next_index;
    int* next_count;
    // Adaptive rho (ADAPT variants; admm.cpp:397-423 + rho_benchmark.cpp): the cache is per-instance STATE -- rho, Kinf, Pinf
    // (and the dead copies C1, C2) move every 5th iteration and persist from solve to solve.  arho [batch]; aK [batch][nu*nx],
    // aP [batch][nx*nx], aC1 [batch][nu*nu], aC2 [batch][nx*nx] column-major (aC1 / aC2 may be null); atab: ATAB_* lane tables --
    // one set for the family, or (HET && ADAPT) [batch][ATAB_DOUBLES], every instance's own (sensitivity_kernel.hip.h).
    // PE forms: a fixed-gain state estimator between the measurement and the solve -- est_gain [instances][NX columns][16 lanes]
    // (gain_entry of lane_tables.hpp; bit 0 of the pointer: one block for all, as at `plant`), est_xp [batch][NX] the predicted
    // estimate, read at the top of a launch and stored behind its last step, est_log optional [steps][batch][NX], the xhat every MPC step
    // solved from, est_model the MODEL's plant block (the layout and the bit 0 of `plant`), which predicts.  All indexed by INSTANCE.
    // Only ADAPT forms read the adaptive-rho pointers, and no PE form is one: the four lie over the first four of them
    union {
        struct { double *arho, *aK, *aP, *aC1; };
        struct {
            const double* est_gain;
            double* est_xp;
            double* est_log;
            const double* est_model;
        };
    };
    // PS forms: a closed-loop score at the plant step -- score_tab [instances][weight | target | lo | hi][16 lanes] (score_entry of
    // lane_tables.hpp; bit 0 of the pointer: one block for all, as at `plant`), score_rec [batch] the record (ScoreRecord), read and
    // written once per scored MPC step by lane 0 of the row, score_step0 the score step counter at the launch's first MPC step.  Indexed
    // by INSTANCE.  Only ADAPT forms read aC2, atab, arho_min and arho_max, and no PS form is one: the three lie over them
    union {
        struct {
            double* aC2;
            const double* atab;
            double arho_min, arho_max;
        };
        struct {
            const double* score_tab;
            ScoreRecord* score_rec;
            int score_step0;
            // PA forms: an actuator model between the command and the plant step -- act_step0 the actuation step counter at the launch's
            // first MPC step, in the padding behind score_step0; act the solve call's record, over arho_max.  No PA form is an ADAPT form
            int act_step0;
            const ActuatorLaunch* act;
        };
    };
    int aclip;
    // 1: every instance has the same Xref | Uref record (set with TINY_BROADCAST, or never set): all rows read instance 0's
    // record -- one L2-resident line set instead of 8S bytes of HBM per instance
    int ref_shared;
    // tile kernel, dynamic form (tile_kernel.hip.h DYN): ONE device-wide counter of the instances handed out so far, zeroed by
    // the host before the launch; a slot of a persistent wave takes the next instance off it the moment it is free.
    // one-row kernel: the counter of 4-instance tiles handed out BEYOND the grid's first ones (null: fixed grid stride)
    int* work_counter;
    // one-row kernel, plain launches: 1 = the grid walks the tiles from the LAST one down.  Successive warm launches over one batch
    // alternate the direction, so that a launch begins with the records its predecessor touched last -- the ones the 256 MiB
    // Infinity Cache in front of HBM still holds (a batch whose records exceed it would otherwise stream through it without a hit).
    // Instances are independent: the order changes nothing in the results.
    int reverse;
    // one-row kernel, plain launches: slot s of the grid solves instance perm[s] (null: instance s).  A fused closed-loop launch that
    // is cut into stretches of MPC steps (batch_dispatch.hip "step_regroup") hands every stretch the instances ordered by the iteration
    // count of their last solve: the four rows of a wave run in lock step, so a wave costs what its slowest row costs, and rows
    // that took alike counts at the last step take alike counts at the next ones.  Same reason as above: nothing in the results.
    const int* perm;
    int perm_count;           // slots of `perm` (a launch may take a part of the batch: batch_dispatch.hip runs two halves on two streams)
    // tile kernel, forms that stream v|z out of the register file (TILE_LM_VPG): where the stream goes.  null: the instance's v|z record
    // (what a warm-started solve must leave there anyway); a ONE-SHOT launch promises not to touch that record, and hands a scratch
    // array of the same shape here instead (round 6: one_shot rides on the shape's fast box form, not on the all-in-registers one)
    double* vz_stream;
    // one-row kernel, PREFETCH form (template PF; round 6): persistent waves whose NEXT tile's records are on their way into the wave's
    // LDS buffer (LDS-DMA, global_load_lds_dwordx4: no register holds them) while the current tile iterates -- at two waves per SIMD
    // (247 VGPRs) a wave's load phase otherwise hides behind ONE neighbour only (tools/ubench/ubench_stream_forms.hip: the record traffic
    // of a warm solve beyond the Infinity Cache 4.3 -> 5.4 TB/s).  pf_mask: which record arrays travel that way (bit 0 vnew|znew, 1 g|y,
    // 2 v|z, 3 Xref|Uref; the others are read as in the plain form); the buffer is the launch's dynamic LDS, [x0 piece][arrays in bit
    // order] in 1-KiB pieces.  Which tiles a wave takes: its first pf_static ones by grid stride (block index + i * grid: no
    // communication, and no value in flight that the wave would have to wait for at a tile's top -- the stores of the tile before stay
    // in flight), the rest by TICKET, so that the waves drain together whatever their tiles cost.  pf_counter: ticket counters, one per
    // SHARD (pf_shards = 8 or 1; 64 bytes apart): ticket k of shard x is tile pf_static * grid + k * pf_shards + x, a wave belongs to
    // shard blockIdx % pf_shards (one counter for the whole device saturates at ~90 returning atomics per microsecond: 65 536 tiles
    // would take 0.7 ms).  The counters are never reset: a shard's waves draw exactly (its ticketed tiles) + (its waves) tickets per
    // launch, pf_base[x] is where this launch's begin (the host keeps the sums)
    // PM forms: the solve of MPC step `step` runs from the MEASURED state fl(x0 + v[meas_step0 + step][instance]) -- meas
    // [meas_steps][batch][NX], step-major, indexed by INSTANCE like dist -- while the plant step starts from the true x0.  Only the PREFETCH
    // form reads pf_mask, pf_shards and pf_static, and no PM form is one: the pointer and its two ints lie over them and the padding behind
    union {
        struct { int pf_mask, pf_shards, pf_static; };
        struct {
            const double* meas;
            int meas_steps, meas_step0;
        };
    };
    // one-row kernel, PB forms: every instance its own box -- [batch][lo | hi][N slots][16 lanes], the slot convention of the shared table's
    // bounds block (lane_tables.hpp box_entry; built by batch_instance.hip from the caller's arrays).  PB and PF exclude each other, so the
    // pointer takes the place of the PREFETCH form's ticket counters: the argument block of every other form keeps its size and offsets
    // PL forms: every instance its own half-spaces -- [batch][the blocks of the form's LIN sets: static [3][KMAX][16], then [N][3][KMAX][16]]
    // (lane_tables.hpp halfspace_entry; built by batch_instance.hip).  PL excludes PF and PB alike, so it shares their place
    // PC forms: every instance its own cone coefficients -- [batch][16 lanes], lane j the coefficient of the cone whose rows include lane j
    // (lane_tables.hpp cone_entry; built by batch_instance.hip).  PF and PB are box forms, PL + PC is not built: the same place again
    union {
        unsigned* pf_counter;
        const double* inst_bounds;
        const double* inst_lin;
        const double* inst_cones;
    };
    // PD forms: every instance its own additive disturbance at the plant step -- dist [dist_steps][batch][NX], step-major; MPC step
    // `step` of this launch adds row dist_step0 + step of its INSTANCE (not its grid slot) to the x1 it hands on, where that row
    // exists.  No PD form is a PREFETCH form, the only reader of pf_base: the pointer and its two ints lie over it, the place of the
    // PB / PL / PC pointer stays free and PD composes with each of them
    union {
        unsigned pf_base[8];
        struct {
            const double* dist;
            int dist_steps, dist_step0;
            // PP forms: a plant model of its own at the plant step -- plant [instances][(NX+NU) columns + the f_p vector][16 lanes]
            // (plant_entry of lane_tables.hpp).  A shared plant is ONE block: bit 0 of the pointer (the blocks are 8-byte aligned)
            // says so, which spares a field here and a template bit.  Null in a form without PP
            const double* plant;
            // PD and PP forms: optional [steps][batch][NX], the x0 every MPC step of this launch handed on (option "state_log")
            double* state_log;
        };
    };
};
// (the PB / PL / PC pointers share the ticket counters' place: the argument block every compiled-in form was built against stays what it was)
static_assert(sizeof(SolveArgs) == 472 && __builtin_offsetof(SolveArgs, het_tabs) == 208 && __builtin_offsetof(SolveArgs, pf_mask) == 416 &&
              __builtin_offsetof(SolveArgs, pf_counter) == 432 && __builtin_offsetof(SolveArgs, pf_base) == 440, "SolveArgs: size and offsets are fixed");
// (the PE pointers lie over arho, aK, aP and aC1, which stay where they were, and so does everything behind them)
static_assert(__builtin_offsetof(SolveArgs, arho) == 304 && __builtin_offsetof(SolveArgs, est_gain) == 304 && __builtin_offsetof(SolveArgs, est_xp) == 312 &&
              __builtin_offsetof(SolveArgs, est_log) == 320 && __builtin_offsetof(SolveArgs, est_model) == 328 && __builtin_offsetof(SolveArgs, aC1) == 328 &&
              __builtin_offsetof(SolveArgs, aC2) == 336 && __builtin_offsetof(SolveArgs, atab) == 344, "SolveArgs: the estimator's pointers share the adaptive-rho ones' place");

// (the PS fields lie over aC2, atab and arho_min, which stay where they were, and so does everything behind them)
static_assert(__builtin_offsetof(SolveArgs, aC2) == 336 && __builtin_offsetof(SolveArgs, score_tab) == 336 && __builtin_offsetof(SolveArgs, atab) == 344 &&
              __builtin_offsetof(SolveArgs, score_rec) == 344 && __builtin_offsetof(SolveArgs, arho_min) == 352 && __builtin_offsetof(SolveArgs, score_step0) == 352 &&
              __builtin_offsetof(SolveArgs, arho_max) == 360 && __builtin_offsetof(SolveArgs, aclip) == 368, "SolveArgs: the score's fields share the adaptive-rho tables' place");

// (the PA fields: the padding behind score_step0 and the place of arho_max; aclip and everything behind stay where they were)
static_assert(__builtin_offsetof(SolveArgs, act_step0) == 356 && __builtin_offsetof(SolveArgs, act) == 360 && __builtin_offsetof(SolveArgs, arho_max) == 360 &&
              __builtin_offsetof(SolveArgs, aclip) == 368 && __builtin_offsetof(SolveArgs, ref_shared) == 372, "SolveArgs: the actuator's fields share arho_max's place");

// ---- DPP row-broadcast FMA blocks ------------------------------------------------------------
// One asm statement per block so that the two wait states a DPP read needs after a VALU write of
// its source (CDNA ISA "VALU writes VGPR -> DPP reads that VGPR") are paid once (the leading
// s_nop 1), and no compiler-inserted copy can land between the FMAs.  The accumulators are
// EARLY-CLOBBER ("&"): they are written while src / m[] are still being read, so they must never
// share a register with an input (without it hipcc happily aliases an accumulator with src).
//
// Every block is ONE column instruction repeated by ONE ladder:
//   DPP_FMA(acc, src, m, lane, bank)  acc += bcast(src, lane) * m on the lanes of `bank`.  The arguments are strings: operand NAMES of the
//                                     enclosing asm statement, `lane` any text the assembler folds to a number ("%[c0]+3")
//   DPP_REP(K, S)                     S(0, 0) S(1, 1) S(2, 0) ... S(K-1, (K-1) & 1): column index and its parity; K = 1 .. 16, a number or a macro
//                                     that expands to one.  S: a DPP_FMA with its chain's names filled in, or an operand-list entry (with its comma)
#define DPP_FMA(acc, src, m, lane, bank) "v_fmac_f64_dpp %[" acc "], %[" src "], %[" m "] row_newbcast:" lane " row_mask:0xf bank_mask:" bank "\n\t"
#define DPP_REP1(S) S(0, 0)
#define DPP_REP2(S) DPP_REP1(S) S(1, 1)
#define DPP_REP3(S) DPP_REP2(S) S(2, 0)
#define DPP_REP4(S) DPP_REP3(S) S(3, 1)
#define DPP_REP5(S) DPP_REP4(S) S(4, 0)
#define DPP_REP6(S) DPP_REP5(S) S(5, 1)
#define DPP_REP7(S) DPP_REP6(S) S(6, 0)
#define DPP_REP8(S) DPP_REP7(S) S(7, 1)
#define DPP_REP9(S) DPP_REP8(S) S(8, 0)
#define DPP_REP10(S) DPP_REP9(S) S(9, 1)
#define DPP_REP11(S) DPP_REP10(S) S(10, 0)
#define DPP_REP12(S) DPP_REP11(S) S(11, 1)
#define DPP_REP13(S) DPP_REP12(S) S(12, 0)
#define DPP_REP14(S) DPP_REP13(S) S(13, 1)
#define DPP_REP15(S) DPP_REP14(S) S(14, 0)
#define DPP_REP16(S) DPP_REP15(S) S(15, 1)
#define DPP_REP_(K, S) DPP_REP##K(S)
#define DPP_REP(K, S) DPP_REP_(K, S)
// operand lists: the matrix row m[] of a ring block as [m0] .. [mK-1]; ma[] / mb_[] of a fused sweep step as [a0] .. and [b0] ..
#define DPP_ROW_M(k, p) , [m##k] "v"(m[k])
#define DPP_ROW_A(k, p) , [a##k] "v"(ma[k])
#define DPP_ROW_B(k, p) , [b##k] "v"(mb_[k])
// ring blocks.  Two accumulators: even columns on a0, odd ones on a1, every column an fmac (both accumulators carry a value in); or one
#define RING2_COL(k, p) DPP_FMA("a" #p, "src", "m" #k, "%[c0]+" #k, "0xf")
#define RING1_COL(k, p) DPP_FMA("a0", "src", "m" #k, "%[c0]+" #k, "0xf")
#define RING_CASE(K)                                                                                                                     \
    if constexpr (NCOL == K)                                                                                                             \
        asm("s_nop 1\n\t" DPP_REP(K, RING2_COL) : [a0] "+&v"(a0), [a1] "+&v"(a1) : [src] "v"(src), [c0] "i"(COL0) DPP_REP(K, DPP_ROW_M));
#define RING1_CASE(K)                                                                                                                    \
    if constexpr (NCOL == K)                                                                                                             \
        asm("s_nop 1\n\t" DPP_REP(K, RING1_COL) : [a0] "+&v"(a0) : [src] "v"(src), [c0] "i"(COL0) DPP_REP(K, DPP_ROW_M));

template <int C>
__device__ __forceinline__ double row_bcast(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x150 + C, 0xf, 0xf, false);   // DPP_ROW_NEWBCAST0 + C
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x150 + C, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int COL0, int NCOL, int K>
struct RingB {
    static __device__ __forceinline__ void run(double& a0, double& a1, double src, const double* m) {
        if constexpr (K < NCOL) {
            if constexpr ((K & 1) == 0) a0 = fma(row_bcast<COL0 + K>(src), m[K], a0);
            else a1 = fma(row_bcast<COL0 + K>(src), m[K], a1);
            RingB<COL0, NCOL, K + 1>::run(a0, a1, src, m);
        }
    }
};

// a{0,1} += sum_{k<NCOL} bcast(src, lane COL0+k) * m[k]   (even k -> a0, odd k -> a1)
// MODE 0: fused v_fmac_f64_dpp (1 issue slot / column); MODE 1: v_mov_b32_dpp x2 + v_fma_f64.
template <int MODE, int COL0, int NCOL>
__device__ __forceinline__ void ring(double& a0, double& a1, double src, const double* m) {
    static_assert(NCOL >= 1 && NCOL <= 16 && COL0 + NCOL <= 16, "one DPP row");
    if constexpr (MODE == 0) {
        RING_CASE(1) RING_CASE(2) RING_CASE(3) RING_CASE(4) RING_CASE(5) RING_CASE(6) RING_CASE(7) RING_CASE(8)
        RING_CASE(9) RING_CASE(10) RING_CASE(11) RING_CASE(12) RING_CASE(13) RING_CASE(14) RING_CASE(15) RING_CASE(16)
    } else {
        RingB<COL0, NCOL, 0>::run(a0, a1, src, m);
    }
}
// single accumulator chain: a0 += sum_k bcast(src, COL0+k) * m[k]
template <int COL0, int NCOL>
__device__ __forceinline__ void ring1(double& a0, double src, const double* m) {
    static_assert(NCOL >= 1 && NCOL <= 16 && COL0 + NCOL <= 16, "one DPP row");
    RING1_CASE(1) RING1_CASE(2) RING1_CASE(3) RING1_CASE(4) RING1_CASE(5) RING1_CASE(6) RING1_CASE(7) RING1_CASE(8)
    RING1_CASE(9) RING1_CASE(10) RING1_CASE(11) RING1_CASE(12) RING1_CASE(13) RING1_CASE(14) RING1_CASE(15) RING1_CASE(16)
}
// init + sum_{k<NA} bcast(srcA, k) mA[k] + sum_{k<NB} bcast(srcB, NA+k) mB[k]
//   MODE 0: two accumulator chains (fused DPP FMA);  MODE 2: one chain;  MODE 1: compiler-scheduled mov_dpp + fma
template <int MODE, int NA, int NB>
__device__ __forceinline__ double ring_sum2(double init, double srcA, const double* mA, double srcB, const double* mB) {
    if constexpr (MODE == 2) {
        double a0 = init;
        ring1<0, NA>(a0, srcA, mA);
        ring1<NA, NB>(a0, srcB, mB);
        return a0;
    } else {
        double a0 = init, a1 = 0.0;
        ring<MODE, 0, NA>(a0, a1, srcA, mA);
        ring<MODE, NA, NB>(a0, a1, srcB, mB);
        return a0 + a1;
    }
}
template <int MODE, int COL0, int NCOL>
__device__ __forceinline__ double ring_sum(double init, double src, const double* m) {
    if constexpr (MODE == 2) {
        double a0 = init;
        ring1<COL0, NCOL>(a0, src, m);
        return a0;
    } else {
        double a0 = init, a1 = 0.0;
        ring<MODE, COL0, NCOL>(a0, a1, src, m);
        return a0 + a1;
    }
}
// short blocks (the forward pass' B u_i): always one chain when fused
template <int MODE, int COL0, int NCOL>
__device__ __forceinline__ double ring_short(double init, double src, const double* m) {
    if constexpr (MODE == 1) return ring_sum<1, COL0, NCOL>(init, src, m);
    else { double a0 = init; ring1<COL0, NCOL>(a0, src, m); return a0; }
}


// HALF rows: lanes 0-7 and 8-15 of a DPP row carry two different instances.  `row_newbcast:k` broadcasts ONE lane to the whole row, so
// a column of the mat-vec takes two instructions, each writing one half only (bank_mask: write-enable per bank of 4 lanes; honoured by
// the DP-ALU DPP form at no cost, tools/ubench/ubench_dpp_bankmask.hip): lanes 0-7 get lane k, lanes 8-15 get lane 8+k.  Per instance
// that is the same number of FMA issue slots as a full row gives -- the gain is everywhere else: every lane-local instruction (the
// slot update is 13 of the 25 instructions per slot at (4,2)) now serves twice the instances, and so does every register.
// HARDWARE NOTE (measured, tools/ubench/ubench_dpp_bankmask2.hip; not in the LLVM hazard tables): a bank-masked DPP instruction
// writes its DISABLED lanes back with the value of vdst it read at operand fetch ("old"), and that read is NOT interlocked against a
// VALU write of vdst in the instruction before -- `fmac bank_mask:0x3` directly followed by `fmac bank_mask:0xc` on the same
// accumulator loses the first one's result (the second writes the stale lanes 0-7 back).  One wait state in between is enough.
// So a chain runs all its low-half FMAs (their enabled lanes accumulate through the interlocked src2 path; the disabled lanes keep
// being re-written with a value that does not change), then `s_nop 0`, then all its high-half FMAs.
#define RINGH_LO(k, p) DPP_FMA("a0", "src", "m" #k, "%[c0]+" #k, "0x3")
#define RINGH_HI(k, p) DPP_FMA("a0", "src", "m" #k, "8+%[c0]+" #k, "0xc")
#define RINGH_CASE(K)                                                                                                                    \
    if constexpr (NCOL == K)                                                                                                             \
        asm("s_nop 1\n\t" DPP_REP(K, RINGH_LO) "s_nop 0\n\t" DPP_REP(K, RINGH_HI) : [a0] "+&v"(a0) : [src] "v"(src), [c0] "i"(COL0) DPP_REP(K, DPP_ROW_M));
// a0 += sum_k bcast_half(src, COL0+k) * m[k]   (each half of the row reads its OWN lanes COL0+k)
template <int COL0, int NCOL>
__device__ __forceinline__ void ring1_half(double& a0, double src, const double* m) {
    static_assert(NCOL >= 1 && COL0 + NCOL <= 8, "one half row");
    RINGH_CASE(1) RINGH_CASE(2) RINGH_CASE(3) RINGH_CASE(4) RINGH_CASE(5) RINGH_CASE(6) RINGH_CASE(7) RINGH_CASE(8)
}


// ---- fused sweep steps (single-chain mode, box-only variants) --------------------------------------------------------------
// The leading `s_nop 1` of a DPP block only waits out the two wait states a DPP read needs after a VALU write of its source.
// Here the lane-local instructions a sweep step needs anyway stand in front of the DPP chain INSIDE the same asm statement --
// the linear-cost terms of the backward step, the first half of the slot update of the forward step -- so the wait states are
// filled with work (38 s_nop per (12,4,10) iteration gone, +2.7 % measured as an upper bound with the nops simply deleted)
// and no compiler-inserted copy can land between the producer of a source and its first DPP read.  Same instructions, same
// operand order as the unfused code: bit-identical results.
// One (nx, nu) pair per translation unit: the Makefile (compiled-in shapes) and jit.hip (run-time instantiated ones) define
// TINYMPC_FUSED_NX / _NU as plain numbers in front of this header (DPP_REP takes its column count from the preprocessor), so that
// exactly one pair of asm statements is spelled out.  For every other pair, and without the defines, the step functions are empty;
// fused_shape() is what the kernels ask before they call one.
#if defined(TINYMPC_FUSED_NX) && defined(TINYMPC_FUSED_NU)
#define TINYMPC_FUSED 1
constexpr bool fused_shape(int na, int nb) { return na == TINYMPC_FUSED_NX && nb == TINYMPC_FUSED_NU; }
// the tail of every step's input operands: where the second chain's lanes begin, and the two matrix rows
#define FUSED_ROW_OPERANDS [c0] "i"(TINYMPC_FUSED_NX) DPP_REP(TINYMPC_FUSED_NX, DPP_ROW_A) DPP_REP(TINYMPC_FUSED_NU, DPP_ROW_B)
#else
constexpr bool fused_shape(int, int) { return false; }
#endif
// the chains' columns.  A: lanes 0 .. nx-1 of the first source times ma[]; B: lanes nx .. nx+nu-1 of the second source times mb_[]
#define BWD_COL_A(k, p) DPP_FMA("acc", "sa", "a" #k, #k, "0xf")
#define BWD_COL_B(k, p) DPP_FMA("acc", "sb", "b" #k, "%[c0]+" #k, "0xf")
#define FWD_COL_A(k, p) DPP_FMA("t", "xi", "a" #k, #k, "0xf")
#define FWD_COL_B(k, p) DPP_FMA("xn", "t", "b" #k, "%[c0]+" #k, "0xf")
#define FWD_COL_B_INPLACE(k, p) DPP_FMA("t", "t", "b" #k, "%[c0]+" #k, "%[bm]")
// backward step: qlo = fma(-rho, vn - g, qx); acc = fma(qlo, smask, cb) + sum_k bcast(sa, k) ma[k] + sum_k bcast(sb, NA + k) mb_[k]
template <int NA, int NB>
__device__ __forceinline__ void fused_backward_step(double& qlo, double& acc, double vn, double g, double qx, double rho, double smask, double cb,
                                                    double sa, double sb, const double* ma, const double* mb_) {
#ifdef TINYMPC_FUSED
    if constexpr (fused_shape(NA, NB)) {
        double tmp;
        asm("v_add_f64 %[tmp], %[vn], -%[g]\n\t"
            "v_fma_f64 %[qlo], -%[rho], %[tmp], %[qx]\n\t"
            "v_fma_f64 %[acc], %[qlo], %[smask], %[cb]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, BWD_COL_A) DPP_REP(TINYMPC_FUSED_NU, BWD_COL_B)
            : [qlo] "=&v"(qlo), [acc] "=&v"(acc), [tmp] "=&v"(tmp)
            : [vn] "v"(vn), [g] "v"(g), [qx] "v"(qx), [rho] "v"(rho), [smask] "v"(smask), [cb] "v"(cb), [sa] "v"(sa), [sb] "v"(sb), FUSED_ROW_OPERANDS);
    }
#endif
}
// the same with the cone slack's linear-cost term (admm.cpp:269 | :282 | :295): qlo = fma(-rho, w, fma(-rho, vn - g, qx)), w = vcnew - gc
// (formed once, by the cone step: the W plane of the cone slack cells)
template <int NA, int NB>
__device__ __forceinline__ void fused_backward_step_soc(double& qlo, double& acc, double vn, double g, double qx, double w, double rho,
                                                        double smask, double cb, double sa, double sb, const double* ma, const double* mb_) {
#ifdef TINYMPC_FUSED
    if constexpr (fused_shape(NA, NB)) {
        double tmp;
        asm("v_add_f64 %[tmp], %[vn], -%[g]\n\t"
            "v_fma_f64 %[qlo], -%[rho], %[tmp], %[qx]\n\t"
            "v_fma_f64 %[qlo], -%[rho], %[w], %[qlo]\n\t"
            "v_fma_f64 %[acc], %[qlo], %[smask], %[cb]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, BWD_COL_A) DPP_REP(TINYMPC_FUSED_NU, BWD_COL_B)
            : [qlo] "=&v"(qlo), [acc] "=&v"(acc), [tmp] "=&v"(tmp)
            : [vn] "v"(vn), [g] "v"(g), [qx] "v"(qx), [rho] "v"(rho), [smask] "v"(smask), [cb] "v"(cb), [sa] "v"(sa), [sb] "v"(sb),
              [w] "v"(w), FUSED_ROW_OPERANDS);
    }
#endif
}
// forward step: tt = xi + g; vn = min(hi, max(lo, tt)); t += sum_k bcast(xi, k) ma[k]; xn = t + sum_k bcast(t, NA + k) mb_[k]
// (INPLACE: the in-place B u chain where NA is a multiple of 4 -- t and xn are then one register; the one-row kernel's short box loop only)
template <int NA, int NB, bool INPLACE = false>
__device__ __forceinline__ void fused_forward_step(double& tt, double& vn, double& t, double& xn, double xi, double g, double lo, double hi,
                                                   const double* ma, const double* mb_) {
#ifdef TINYMPC_FUSED
    if constexpr (fused_shape(NA, NB) && !(INPLACE && TINYMPC_FUSED_NX % 4 == 0)) {
        double vm;
        asm("v_add_f64 %[tt], %[xi], %[g]\n\t"
            "v_max_f64 %[vm], %[lo], %[tt]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, FWD_COL_A)
            "v_min_f64 %[vn], %[hi], %[vm]\n\t"
            "v_mov_b64 %[xn], %[t]\n\t"
            DPP_REP(TINYMPC_FUSED_NU, FWD_COL_B)
            : [tt] "=&v"(tt), [vm] "=&v"(vm), [vn] "=&v"(vn), [xn] "=&v"(xn), [t] "+&v"(t)
            : [xi] "v"(xi), [g] "v"(g), [lo] "v"(lo), [hi] "v"(hi), FUSED_ROW_OPERANDS);
    }
    // B u_i accumulated IN PLACE (nx a multiple of 4): bank_mask keeps the lanes from nx on -- u_i on the input lanes, the broadcast
    // sources of the chain -- out of every FMA, so t needs no copy into a second accumulator.  A disabled lane is re-written with the
    // value it held (the same u_k whether the read was early or late), which is why the chain may read t right behind writing it.  State
    // lanes: the same FMAs in the same order on the same values as with the copy.  Input lanes keep u_i itself where the copy form added
    // u_k * 0 to it (the two differ only in the sign of an exact zero, or when some u_k is not finite).
    if constexpr (fused_shape(NA, NB) && INPLACE && TINYMPC_FUSED_NX % 4 == 0) {
        asm("v_add_f64 %[tt], %[xi], %[g]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, FWD_COL_A)
            "v_max_f64 %[vn], %[lo], %[tt]\n\t"
            "v_min_f64 %[vn], %[hi], %[vn]\n\t"
            DPP_REP(TINYMPC_FUSED_NU, FWD_COL_B_INPLACE)
            : [tt] "=&v"(tt), [vn] "=&v"(vn), [t] "+&v"(t)
            : [xi] "v"(xi), [g] "v"(g), [lo] "v"(lo), [hi] "v"(hi), [bm] "i"((1 << (TINYMPC_FUSED_NX / 4)) - 1), FUSED_ROW_OPERANDS);
        xn = t;
    }
#endif
}
// ---- the same fused steps for HALF rows (nx+nu <= 8: two instances per DPP row, see ring1_half): every column is a pair of
// bank-masked FMAs -- all low halves, ONE wait state (a bank-masked DPP op re-writes its disabled lanes with the vdst it read
// without interlock), all high halves.  In the forward step the wait state between the two halves of the first chain is the
// step's own v_min.
#if defined(TINYMPC_FUSED) && TINYMPC_FUSED_NX + TINYMPC_FUSED_NU <= 8
#define TINYMPC_FUSED_HALF 1
#endif
#define HBWD_COL_A_LO(k, p) DPP_FMA("acc", "sa", "a" #k, #k, "0x3")
#define HBWD_COL_A_HI(k, p) DPP_FMA("acc", "sa", "a" #k, "8+" #k, "0xc")
#define HBWD_COL_B_LO(k, p) DPP_FMA("acc", "sb", "b" #k, "%[c0]+" #k, "0x3")
#define HBWD_COL_B_HI(k, p) DPP_FMA("acc", "sb", "b" #k, "8+%[c0]+" #k, "0xc")
#define HFWD_COL_A_LO(k, p) DPP_FMA("t", "xi", "a" #k, #k, "0x3")
#define HFWD_COL_A_HI(k, p) DPP_FMA("t", "xi", "a" #k, "8+" #k, "0xc")
#define HFWD_COL_B_LO(k, p) DPP_FMA("xn", "t", "b" #k, "%[c0]+" #k, "0x3")
#define HFWD_COL_B_HI(k, p) DPP_FMA("xn", "t", "b" #k, "8+%[c0]+" #k, "0xc")
// Every wait state such a chain needs is a lane-local instruction the iteration needs anyway (no s_nop): behind the write of the
// accumulator stands the forward constant of the step BEFORE (Dn = fma(p | d, nim, cf) of the source the chain is about to broadcast),
// between the two halves the `vn - g` of the NEXT step; in the forward step `g <- (x + g) - vnew` (the residual terms are NOT pulled in:
// they are only formed when the termination test can pass).  Same instructions, same operands as the one-instance-per-row form: bit-identical results.
// backward: qlo = fma(-rho, tmp, qx) with tmp = vn - g handed in (formed by the step before); dnp = fma(sa, nim, cf); tmpn = vnn - gn for
// the next step.  forward: additionally gnew = tt - vn
template <int NA, int NB>
__device__ __forceinline__ void fused_backward_step_half(double& qlo, double& acc, double& dnp, double& tmpn, double tmp, double vnn, double gn, double qx,
                                                         double rho, double smask, double cb, double nim, double cf, double sa, double sb,
                                                         const double* ma, const double* mb_) {
#ifdef TINYMPC_FUSED_HALF
    if constexpr (fused_shape(NA, NB)) {
        asm("v_fma_f64 %[qlo], -%[rho], %[tmp], %[qx]\n\t"
            "v_fma_f64 %[acc], %[qlo], %[smask], %[cb]\n\t"
            "v_fma_f64 %[dnp], %[sa], %[nim], %[cf]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, HBWD_COL_A_LO) DPP_REP(TINYMPC_FUSED_NU, HBWD_COL_B_LO)
            "v_add_f64 %[tmpn], %[vnn], -%[gn]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, HBWD_COL_A_HI) DPP_REP(TINYMPC_FUSED_NU, HBWD_COL_B_HI)
            : [qlo] "=&v"(qlo), [acc] "=&v"(acc), [dnp] "=&v"(dnp), [tmpn] "=&v"(tmpn)
            : [tmp] "v"(tmp), [vnn] "v"(vnn), [gn] "v"(gn), [qx] "v"(qx), [rho] "v"(rho), [smask] "v"(smask), [cb] "v"(cb),
              [nim] "v"(nim), [cf] "v"(cf), [sa] "v"(sa), [sb] "v"(sb), FUSED_ROW_OPERANDS);
    }
#endif
}
template <int NA, int NB>
__device__ __forceinline__ void fused_forward_step_half(double& tt, double& vn, double& t, double& xn, double& gnew, double xi, double g,
                                                        double lo, double hi, const double* ma, const double* mb_) {
#ifdef TINYMPC_FUSED_HALF
    if constexpr (fused_shape(NA, NB)) {
        double vm;
        asm("v_add_f64 %[tt], %[xi], %[g]\n\t"
            "v_max_f64 %[vm], %[lo], %[tt]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, HFWD_COL_A_LO)
            "v_min_f64 %[vn], %[hi], %[vm]\n\t"
            DPP_REP(TINYMPC_FUSED_NX, HFWD_COL_A_HI)
            "v_mov_b64 %[xn], %[t]\n\t"
            "v_add_f64 %[gnew], %[tt], -%[vn]\n\t"
            DPP_REP(TINYMPC_FUSED_NU, HFWD_COL_B_LO)
            "s_nop 0\n\t"
            DPP_REP(TINYMPC_FUSED_NU, HFWD_COL_B_HI)
            : [tt] "=&v"(tt), [vm] "=&v"(vm), [vn] "=&v"(vn), [xn] "=&v"(xn), [t] "+&v"(t), [gnew] "=&v"(gnew)
            : [xi] "v"(xi), [g] "v"(g), [lo] "v"(lo), [hi] "v"(hi), FUSED_ROW_OPERANDS);
    }
#endif
}

// v_max_f64 / v_min_f64 without the canonicalising `v_max x, x` hipcc puts in front of fmax/fmin
// operands that come from memory (the box bounds): the hardware quiets NaNs by itself.
__device__ __forceinline__ double vmax64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double vmin64(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// a - b where it is written: the empty volatile statement behind it keeps hipcc from sinking the subtraction to the loop latch.  (The
// subtraction itself stays a compiler instruction: hipcc's hazard bookkeeping counts an asm statement as no wait state at all.)
__device__ __forceinline__ double pinned_sub64(double a, double b) {
    double r = a - b;
    asm volatile("" : "+v"(r));
    return r;
}
// min(hi, max(lo, t)) as ONE asm statement: the two of vmin64(hi, vmax64(lo, t)) are back to back, and hipcc pads such a pair with an s_nop
__device__ __forceinline__ double vclamp64(double lo, double hi, double t) {
    double r;
    asm("v_max_f64 %0, %1, %2\n\tv_min_f64 %0, %3, %0" : "=&v"(r) : "v"(lo), "v"(t), "v"(hi));
    return r;
}

// max(a, |b|) as ONE opaque instruction (long horizons only, N > 12): spelled with fmax / fabs the N residual updates of a sweep
// form a reduction that the compiler re-associates into a tree BEHIND the sweep, so every slot's x, vnew and x + g stay live to the
// end of the sweep -- at N = 30 that is accumulation-register traffic on every access.  v_max_f64 returns the other operand when
// one is a NaN, as fmax does.
__device__ __forceinline__ double vmax_abs64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, |%2|" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
template <bool OPAQUE>
__device__ __forceinline__ double resid_max(double a, double b) {
    if constexpr (OPAQUE) return vmax_abs64(a, b);
    else return fmax(a, fabs(b));
}

// The x|u trajectory is written once per launch and never read back by a kernel: it need not displace the warm-start records
// (vnew|znew, g|y, v|z: 240 MiB at 65 536 quadrotor instances) from the 256 MiB Infinity Cache in front of HBM.
// TINYMPC_PRIM_STORE: 0 plain, 1 nontemporal, 2 sc1, 3 sc0 sc1 (experiment builds, tools/build_variants.py)
#ifndef TINYMPC_PRIM_STORE
#define TINYMPC_PRIM_STORE 1
#endif
#ifndef TINYMPC_REF_LOAD
#define TINYMPC_REF_LOAD 1
#endif
// record stores as whole knot segments (see the write-back of admm_solve_kernel): 0 never, 1 the PREFETCH form, 2 every box variant
#ifndef TINYMPC_FULL_LINE_STORES
#define TINYMPC_FULL_LINE_STORES 2
#endif
// per-instance Xref|Uref records are read once per launch and never written by a kernel: the same argument (1 = nontemporal load)
__device__ __forceinline__ double load_ref(const double* p) {
#if TINYMPC_REF_LOAD == 1
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
__device__ __forceinline__ void store_primal(double* p, double v) {
#if TINYMPC_PRIM_STORE == 1
    __builtin_nontemporal_store(v, p);
#elif TINYMPC_PRIM_STORE == 2
    asm volatile("global_store_dwordx2 %0, %1, off sc1" : : "v"(p), "v"(v) : "memory");
#elif TINYMPC_PRIM_STORE == 3
    asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1" : : "v"(p), "v"(v) : "memory");
#elif TINYMPC_PRIM_STORE == 4
    asm volatile("global_store_dwordx2 %0, %1, off sc0 sc1 nt" : : "v"(p), "v"(v) : "memory");
#else
    *p = v;
#endif
}

__device__ __forceinline__ double grp_max16(double v) {
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, 16));
    return v;
}
template <int W>
__device__ __forceinline__ double grp_maxw(double v) {                 // max over the W (8 | 16) lanes of an instance
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) v = fmax(v, __shfl_xor(v, off, W));
    return v;
}

// project_soc (admm.cpp:39-60) for a whole 3-cone held by ONE lane (s0, s1, s2) -> (r0, r1, r2): the transposed form of the cone step
// (one lane per (cone, knot) pair) pays the square root and the two divisions once per iteration instead of once per knot.  mu and the
// norm are float, a/mu is a float division.  The reference is built without FMA contraction, and `a` is truncated to float before the
// branch tests, so the sum of squares must not be fused.  The two divisions of the "outside" branch are skipped when no lane of the
// wave is outside its cone.
// soc_all_inside: EVERY cone of the wave is inside with a margin that the float rounding of the norm cannot bridge -- sqrt(q) <= u0
// (1 - 2^-21) => (float)sqrt(q) <= u0 (a float rounding moves the norm by at most 2^-24 of it); u0 above 1e-30 and q below 1e70 keep
// the float normal and finite; NaNs fail the test and take the exact path:
// every projection of the pass is then the identity (:49) -- the common case of a constraint that is not active -- and the cone step
// neither takes a square root nor rewrites what the forward sweep left.  `&` on purpose: three compares and two s_and, no EXEC regions.
__device__ __forceinline__ bool soc_all_inside(double s0, double s1, double s2, float mu) {
#pragma clang fp contract(off)
    const double u0 = s2 * (double)mu;                                  // :40
    const double q0 = s0 * s0, q1 = s1 * s1;
    const double q = q0 + q1;
    // (u0 < 1e300: a non-finite last component takes the exact path, where gc = (x + gc) - vcnew becomes the NaN the reference gets)
    const bool sure_inside = (u0 > 1e-30) & (u0 < 1e300) & (q <= (u0 * u0) * (1.0 - 0x1p-20)) & (q < 1e70);
    return __builtin_amdgcn_ballot_w64(!sure_inside) == 0ull;
}
// rmu_exact: every mu of the wave is a power of two and rmu = 1 / mu exactly (wave-uniform) -- then a * rmu IS a / mu, rounded once
// like the division (2^k scalings are exact, overflow and gradual underflow included), without the ten instructions of one.
__device__ __forceinline__ void soc_project3(double s0, double s1, double s2, float mu, float rmu, bool rmu_exact, double& r0, double& r1, double& r2) {
#pragma clang fp contract(off)
    const double u0 = s2 * (double)mu;                                  // :40
    const double q0 = s0 * s0, q1 = s1 * s1;
    const double q = q0 + q1;
    const float a = (float)sqrt(q);                                     // :42
    const double ad = (double)a;
    const bool below = ad <= -u0, inside = ad <= u0;                    // :46 | :49
    const bool outside = !below && !inside && (ad >= fabs(u0));         // :52 (else :58 -> 0)
    const bool zero = below || !inside;
    r0 = zero ? 0.0 : s0; r1 = zero ? 0.0 : s1; r2 = zero ? 0.0 : s2;
    if (__builtin_amdgcn_ballot_w64(outside) != 0ull) {
        const double scale = 0.5 * (1.0 + u0 / ad);                     // :55
        const double last = (double)(rmu_exact ? a * rmu : a / mu);      // :54
        r0 = outside ? scale * s0 : r0;
        r1 = outside ? scale * s1 : r1;
        r2 = outside ? scale * last : r2;
    }
}
// (cone, knot) items of a row whose cones start at the lanes of `heads`
__device__ __forceinline__ int soc_items_of(unsigned heads, int nx, int n) {
    int c = 0;
    for (unsigned m = heads; m; m &= m - 1) c += (__builtin_ctz(m) < nx) ? n : n - 1;
    return c;
}
// passes of 16 (cone, knot) items a row needs when every lane triple of the state / input rows carries a cone
constexpr int soc_item_passes(int nx, int nu, int n) { return ((nx / 3) * n + (nu / 3) * (n - 1) + 15) / 16; }

// a + d * b with the product rounded before the sum, as the reference's x86-64 build (no FMA contraction) evaluates
// `Kinf + delta_rho * dKinf_drho` (rho_benchmark.cpp:201-204)
// C1 and C2 are state the iteration never reads (backward_pass_grad works with Quu_inv / AmBKt, admm.cpp:63-77): their Taylor
// steps are logged and applied ADAPT_LOG at a time, in the reference's order (same roundings), instead of one read-modify-write
// of 2 x (nx^2 + nu^2) doubles of HBM per adaptation.
constexpr int ADAPT_LOG = 32;
__device__ __forceinline__ double taylor_step(double a, double d, double b) {
#pragma clang fp contract(off)
    const double t = d * b;
    return a + t;
}

// ---- the kernel -------------------------------------------------------------------------------
// Slot convention: lane j keeps N-long register arrays indexed by "slot" s.  State lanes (j < NX):
// slot s = knot s.  Input lanes: slot s = knot s-1 (slot 0 is a neutral dummy), because the forward
// step i produces x_{i+1} on the state lanes and u_i on the input lanes in the SAME instruction
// stream -- storing both at slot i+1 needs no per-lane select.
// Register budget: 6 N-long FP64 arrays per lane (+2 with a cone) + the matrix rows.  N <= 12 fits the
// 256-VGPR budget of two waves per SIMD; longer horizons take the whole 512-entry file (one wave per SIMD).
// Half-space variants (LIN) take one wave; the adaptive-rho variant keeps two up to N = 10 (its adaptation block, every 5th
// iteration, works out of LDS and spills only on the rare flush_c path).
constexpr int solve_kernel_waves_per_simd(int nz, int n, bool soc, bool lin = false, bool adapt = false) {
    if (lin) return 1;
    if (adapt) return n <= 10 ? 2 : 1;
    return (n <= 10 || 2 * ((soc ? 8 : 6) * n + 2 * nz + 8) + 40 <= 256) ? 2 : 1;
}

// Half-space variants: the slacks live in LDS planes (see the kernel), so a lane holds the box kernel's arrays and the variant takes
// the box kernel's two waves per SIMD -- when eight waves' planes and tables fit the CU's LDS
#ifndef TINYMPC_LIN_WAVES
#define TINYMPC_LIN_WAVES 0                        // (experiments: 1 / 2 instead of the rule)
#endif
// static LDS of a half-space variant with its slack planes: the tables, two planes per set, the cone slack's three, Pinf', the bounds
// (pl: the tables are per-ROW quantities -- every instance its own half-spaces --, one copy for each of the wave's four rows)
constexpr long solve_kernel_lin_lds(int nx, int nu, int n, bool soc, int lin, int kmax, bool ub, bool pl = false) {
    const int nz = nx + nu, csl = (nz + 1) | 1, cs = (nz + 1) | 1, tabs = pl ? 4 : 1;
    return 8L * (nx * 16 + (ub ? 2 : 2 * n * 16) + ((lin & 1) ? tabs * 3 * kmax * 16 + 2 * 4 * n * csl : 0) +
                 ((lin & 2) ? tabs * 3 * n * kmax * 16 + 2 * 4 * n * csl : 0) + (soc ? (4 * n + 1) * 3 * cs : 0));
}
// ... which must fit a wave's 64 KiB of static LDS; a variant whose planes do not (long horizons with time-varying tables) keeps its
// slacks in register arrays and projects per knot, as every half-space variant did before round 4 (one wave per SIMD)
constexpr bool solve_kernel_lin_planes(int nx, int nu, int n, bool soc, int lin, int kmax, bool ub, bool pl = false) {
    return lin != 0 && solve_kernel_lin_lds(nx, nu, n, soc, lin, kmax, ub, pl) <= 64 * 1024 - 512;
}
constexpr int solve_kernel_lin_waves(int nx, int nu, int n, bool soc, int lin, int kmax, bool ub, bool pl = false) {
    if (!solve_kernel_lin_planes(nx, nu, n, soc, lin, kmax, ub, pl)) return 1;
    if (TINYMPC_LIN_WAVES > 0) return TINYMPC_LIN_WAVES;
    return (solve_kernel_waves_per_simd(nx + nu, n, soc) == 2 && 8 * solve_kernel_lin_lds(nx, nu, n, soc, lin, kmax, ub, pl) <= 158 * 1024) ? 2 : 1;
}
// One lane projects whole (knot, family) columns of a half-space slack: column c of instance `inst`, rows [R0, R0 + NF) -- the cells
// pv[(inst * n + c) * csl + R0 ...] hold x + gl; the family's half-spaces are applied one after the other, only when violated
// (admm.cpp:148-173, 186-211; project_hyperplane :70-73; a'z as the ORACLE forms it: products rounded, summed in row order -- the
// reference's Eigen reductions pair the terms differently once a row has more than 3 entries, at most 2.5e-16 relative on the rocket
// problem's slacks, none on a 3-row family; tests/test_halfspace_ref_cpu.py bounds that difference by the summation bound), vlnew
// goes back to pv and gl = (x + gl) - vlnew (:239-254) to pg.  Lane t of the LPI lanes of an instance takes columns S0 + t, S0 + t +
// LPI, ...; tab: [3][KMAX][LW] coefficient | offset | squared norm, + c * tab_stride for the time-varying family.
template <int NF, int KMAX_, int LW_, int LPI_>
__device__ __forceinline__ void project_halfspace_columns(const int t, const int inst, const int n, const int csl, const int R0, const int S0,
                                                          double* pv, double* pg, const double* tab, const int tab_stride, const int nk) {
#pragma clang fp contract(off)
    for (int c = S0 + t; c < n; c += LPI_) {
        const int at = (inst * n + c) * csl + R0;
        const double* tk = tab + c * tab_stride;
        double z[NF], t0[NF];
#pragma unroll
        for (int r = 0; r < NF; ++r) { z[r] = pv[at + r]; t0[r] = z[r]; }
        for (int k = 0; k < nk; ++k) {
            double cv = 0.0;
#pragma unroll
            for (int r = 0; r < NF; ++r) { const double pr = tk[k * LW_ + R0 + r] * z[r]; cv = cv + pr; }
            const double bk = tk[KMAX_ * LW_ + k * LW_ + R0];
            if (cv > bk) {
                const double dist = (cv - bk) / tk[2 * KMAX_ * LW_ + k * LW_ + R0];
#pragma unroll
                for (int r = 0; r < NF; ++r) { const double pr = dist * tk[k * LW_ + R0 + r]; z[r] = z[r] - pr; }
            }
        }
#pragma unroll
        for (int r = 0; r < NF; ++r) { pv[at + r] = z[r]; pg[at + r] = t0[r] - z[r]; }
    }
}

// the disturbed plant step of the PD forms: ONE IEEE double addition.  x1 passes through an empty asm, so that no multiply that
// produced it can be contracted with this addition into an FMA (the undisturbed forms hand on x1 as it is)
__device__ __forceinline__ double plant_add(double x1, const double w) {
    asm volatile("" : "+v"(x1));
    return x1 + w;
}
// the innovation of the PE forms: ONE IEEE double subtraction, kept apart from what produced its operands in the same way
__device__ __forceinline__ double plant_sub(double xm, double xp) {
    asm volatile("" : "+v"(xm), "+v"(xp));
    return xm - xp;
}
// the plant step of the PP forms, columns COL0 .. COL0 + NCOL - 1 of ONE chain: acc = fma(bcast(src, lane c), m[c], acc), column after
// column on the one accumulator.  Cut into blocks of at most four columns, each loading its own operands (m: this lane's entry of column
// COL0, the columns 16 doubles apart): the same instructions in the same order as one ring1 over all columns, hence the same bits, at
// 8 transient registers instead of 2 * NCOL
// a pointer field of the argument block, read from the kernel-argument segment WHERE IT IS USED (the offset passes through an empty asm,
// so the load stays behind it).  The PE forms read their four pointers this way: read as P.field they are loaded at the kernel's entry
// and held in scalar registers through the tile, step and iteration loops -- on forms whose scalar registers already spill into
// vector lanes, that cost vector registers and put rematerialised instructions into the iteration loop.  SolveArgs is the kernel's one
// parameter: a field's offset in the segment is its offset in the struct
template <class T>
__device__ __forceinline__ T* late_arg(unsigned offset) {
    asm volatile("" : "+s"(offset));
    const char __attribute__((address_space(4)))* seg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
    return *(T* const __attribute__((address_space(4)))*)(seg + offset);
}
// (... and a plain field of it, read the same way: the PS forms' step counter)
template <class T>
__device__ __forceinline__ T late_value(unsigned offset) {
    asm volatile("" : "+s"(offset));
    const char __attribute__((address_space(4)))* seg = (const char __attribute__((address_space(4)))*)__builtin_amdgcn_kernarg_segment_ptr();
    return *(const T __attribute__((address_space(4)))*)(seg + offset);
}
template <int COL0, int NCOL>
__device__ __forceinline__ void plant_chain(double& acc, const double src, const double* m) {
    if constexpr (NCOL > 0) {
        constexpr int K = NCOL < 4 ? NCOL : 4;
        double r[K];
#pragma unroll
        for (int k = 0; k < K; ++k) r[k] = m[k * 16];
        ring1<COL0, K>(acc, src, r);
        plant_chain<COL0 + K, NCOL - K>(acc, src, m + K * 16);
    }
}
// the score of the PS forms, the lane-local part: the cost term s = fl(fl(w * d) * d), d = fl(z - target), and the violation
// e = max(fl(z - hi), fl(lo - z), 0) of this lane's entry of z -- every operation ONE IEEE rounding, nothing contracted
struct ScoreTerm { double s, e; };
__device__ __forceinline__ ScoreTerm score_term(double z, const double w, const double target, const double lo, const double hi) {
#pragma clang fp contract(off)
    asm volatile("" : "+v"(z));
    const double d = z - target;
    const double wd = w * d;
    ScoreTerm t;
    t.s = wd * d;
    t.e = fmax(fmax(z - hi, lo - z), 0.0);
    return t;
}
// ... the row maximum of the violations, on every lane of the row: four rotations within the DPP row (row_ror 8, 4, 2, 1), no lane index
// and no LDS crossbar -- the maximum is order-free
template <int R>
__device__ __forceinline__ double row_rotated(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x120 + R, 0xf, 0xf, false);   // DPP_ROW_RR0 + R
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x120 + R, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double score_row_max(double v) {
    v = fmax(v, row_rotated<8>(v));
    v = fmax(v, row_rotated<4>(v));
    v = fmax(v, row_rotated<2>(v));
    return fmax(v, row_rotated<1>(v));
}
// ... and the running sum: cost = fl(cost + bcast(s, lane c)), c = COL0 .. COL0 + NCOL - 1, ONE chain in ascending order -- the DPP fmac
// chain against ones (fma(s, 1, cost) is exactly fl(cost + s)), in blocks of four columns as plant_chain, whatever MODE says
template <int COL0, int NCOL>
__device__ __forceinline__ void score_chain(double& cost, const double s) {
    if constexpr (NCOL > 0) {
        constexpr int K = NCOL < 4 ? NCOL : 4;
        const double one[4] = {1.0, 1.0, 1.0, 1.0};
        ring1<COL0, K>(cost, s, one);
        score_chain<COL0 + K, NCOL - K>(cost, s);
    }
}
// the actuator of the PA forms, the lane-local arithmetic of one input: limits by two comparisons and two selects (inside them the
// command keeps its bits, the sign of a zero included; no fmin / fmax), the lag d = fl(s - a), m = fma(alpha, d, a), gain and offset
// g = fma(m, gain, offset) -- every operation ONE IEEE rounding, nothing contracted
__device__ __forceinline__ double actuator_limits(const double uc, const double lo, const double hi) { return uc < lo ? lo : (uc > hi ? hi : uc); }
__device__ __forceinline__ double actuator_lag(const double s, const double a, const double alpha) {
#pragma clang fp contract(off)
    const double d = s - a;
    return __builtin_fma(alpha, d, a);
}
__device__ __forceinline__ double actuator_gain(const double m, const double gain, const double offset) { return __builtin_fma(m, gain, offset); }

// LIN: bit 0 = static half-spaces (admm.cpp:137-173), bit 1 = time-varying ones (:176-211); 0 = neither
// HET: per-instance problem data (riccati_kernel.hip.h): the matrix rows are re-loaded for every instance
// ADAPT: adaptive rho (admm.cpp:397-423): per-instance rho / Kinf / Pinf, re-estimated every 5th iteration
// UB: the box is the same at every knot (the usual case: constant state / input limits): the two bounds of a lane live in
// registers instead of being read from LDS slot by slot -- 18 LDS reads and as many waits less per iteration at N = 10
// HALF: nx+nu <= 8 -- TWO instances per DPP row (lanes 0-7 | 8-15), eight per wave: every lane-local instruction and every register
// serves twice the instances; a mat-vec column is a pair of bank-masked FMAs (fused_*_step_half).  Plain box variants only.
// PF: the PREFETCH form (SolveArgs::pf_mask): plain box variants, plain launches (no index / perm / trajectory window)
// PB: every instance its own box (SolveArgs::inst_bounds) -- the bounds are per-ROW quantities, reloaded for each tile: with UB (every
// instance's box is knot-invariant) four doubles per lane next to the HET table loads, no LDS and the UB form's register count; without
// it the row's block of sLo / sHi [IPW][N * 16], filled at the top of the tile by the row's own lanes.  The iteration loop is the one of
// the shared-box form: the bounds were operands of its step blocks already.  Box variants on full rows, not the PREFETCH form; with
// HET and every MODE.  Instantiated at run time only (jit.hip).  The flag travels as bit 2 of the sixth template argument (MODE_PB =
// MODE | 4): a template parameter of its own, even one with a default, would lengthen the mangled name of EVERY instantiation, and those
// names are what the registry, the register-budget tests and tools/isa_diff.py know the compiled-in kernels by.
// PL: every instance its own half-spaces (SolveArgs::inst_lin) -- sLin / sTLin are per-ROW tables: one block per row of the wave, filled
// at the top of every tile by the row's own lanes from the instance's blocks; project_halfspace_columns takes the row's base instead of
// the wave's, the sweeps and the iteration loop are the shared form's.  LIN != 0 on the slack-plane form only (solve_kernel_lin_planes
// with the four rows' tables -- which is why these forms are instantiated at KMAX 1 and 2 as well: four [N][3][4][16] tables at N = 10
// are 61 KB); with SOC, HET and every launch form; not HALF, PF, ADAPT or PB.  Run-time instantiated only; bit 3 of the sixth template
// argument (MODE | 8), for the reason given at PB.
// PC: every instance its own cone coefficients (SolveArgs::inst_cones) -- where the cones sit stays the batch's, so the item layout of
// the transposed cone step (item_at) is the shared form's; the coefficient of a lane's item (item_mu) is a per-ROW quantity, loaded at
// the top of every tile from the row's instance, next to the HET table loads.  The last component of an outside projection is always
// the reference's division a / mu: a wave holds four instances' coefficients, and the multiply by 1 / mu that the shared form takes
// when every coefficient of the launch is a power of two would have to be decided per tile by a ballot in front of the iteration
// loop -- the division is correct for any mix and costs only where a cone is active.  SOC forms with HET, UB and every launch form;
// not HALF, PF, PB (box forms), PL or ADAPT.  Run-time instantiated only; bit 4 of the sixth template argument (MODE | 16).
// PD: every instance its own additive disturbance sequence (SolveArgs::dist) -- the plant step of MPC step k hands on fl(x1 + w[k][b])
// instead of x1: ONE double addition on the state lanes, at the two places a plant step is taken (the x0 of the next fused step, the
// x0_next store of the launch's last one).  The value is loaded at the END of a step, behind the iteration loop, so that its latency
// is paid once per MPC step and no register is held through the loop; a step outside the sequence adds nothing at all (wave-uniform
// test), and so does a step that ran no iteration (max_iter = 0: no plant step).  Only x0 moves: the x|u records keep the solver's
// prediction.  With every variant and launch form but HALF, PF and ADAPT; composes with PB, PL and PC.  Run-time instantiated only;
// bit 5 of the sixth template argument (MODE | 32).
// PP: a plant model of its own (SolveArgs::plant: A_p, B_p, f_p per instance, or one for all) -- where a plant step is taken, state row
// j becomes acc = f_p[j]; acc = fma(x0[k], A_p[j][k], acc), k = 0 .. NX-1; acc = fma(u0[k], B_p[j][k], acc), k = 0 .. NU-1 instead of the
// solver's x1: ONE chain, one rounding per term, on the DPP blocks whatever MODE says (the order of the forward pass under MODE 2: a plant
// equal to the model hands on the same bits).  x0 is what the state lanes still hold in slot 0, u0 what the input lanes hold in slot
// 1.  The lane's row is loaded at the END of a step, in blocks of four columns (plant_chain): nothing of it lives through the iteration
// loop.  A disturbance row (PD) is added to the result.  Only x0 moves.  Composes with PD, PB, PL, PC and HET; not HALF, PF or ADAPT.
// Run-time instantiated only; bit 6 of the sixth template argument (MODE | 64).  PD and PP forms write SolveArgs::state_log, if given.
// PM: measurement noise (SolveArgs::meas) -- the x0 record is the plant's TRUE state; MPC step k solves from xm = fl(x0 + v[k][b]) (ONE
// double addition, plant_add; a step outside the sequence: x0 itself, no addition), so X[0], the cone / half-space slack of slot 0 and
// the whole solve see xm, and the plant step behind the iteration loop starts from the true x0 again: plant_step(true x0, u0), then the
// disturbance (PD).  PM implies PP: the launch always supplies a plant block (the model's own where none is installed).  The true state
// is NOT carried through the iteration loop: a state lane stores what every plant step hands on to its own cell of x0_next and reads
// that cell back behind the next step's loop (step 0 reads x0), the index formed behind an empty asm as in `disturbed`; the measurement
// of the NEXT step is formed right there from the value in hand.  A step that ran no iteration takes no plant step: its true state
// stays.  Composes with everything PP composes with.  Run-time instantiated only; bit 7 of the sixth template argument (MODE | 128).
// PE: a fixed-gain state estimator (SolveArgs::est_gain, est_xp, est_log, est_model) between the measurement and the solve.  MPC step k
// solves from xhat = xp + M (xm - xp): e = fl(xm - xp) (ONE subtraction, plant_sub), then row j of M over the row's e on the accumulator
// that starts at xp[j] -- plant_chain<0, NX>, the DPP blocks whatever MODE says -- so X[0], the slack of slot 0 and the whole solve see
// xhat.  Behind the iteration loop the MODEL predicts the next xp from X[0] = xhat and X[1] = u0 (plant_by over est_model: the chain of
// PP), the plant steps the TRUE state as under PM, the next step's measurement is formed and corrected right there: the prediction is
// consumed in registers, est_xp is read at the top of a tile and stored behind the launch's last step only.  A step that ran no
// iteration (max_iter = 0: then no step of the launch runs one) takes neither plant step nor prediction, and the next step's xp is the
// record's.  PE implies PM and PP (a launch without a noise sequence binds an empty one); composes with everything PM composes with.
// Run-time instantiated only; bit 8 of the sixth template argument (MODE | 256).
// PS: a closed-loop score (SolveArgs::score_tab, score_rec, score_step0) at the plant step.  Where a PD / PP / PM form hands on a state
// -- behind the iteration loop of every fused step, and at the x0_next store of the last one -- the row scores z = [xn | u0]: per lane
// d = fl(z - target), s = fl(fl(w * d) * d), e = max(fl(z - hi), fl(lo - z), 0) (score_term: contraction off), the cost one DPP chain
// against ones that starts at the record's cost and adds the row's s in ascending order (score_chain), the violation one row maximum;
// lane 0 reads the record and writes it back.  The record is read and written per step, not carried: on the PM / PE box forms, which sit
// at the register limit, six more registers through the iteration loop would be six more spills in it.  A step that ran no iteration
// takes no plant step and is not scored.  Only the record moves.  PS rides on PD or PP (a launch with neither installed binds an
// empty disturbance sequence, as the state log does); composes with everything they compose with.  Run-time instantiated only; bit 9
// of the sixth template argument (MODE | 512).
// PA: an actuator model (SolveArgs::act, act_step0) between the command and the plant step.  Where a PP form takes a plant step the input
// lanes turn the command uc = u0 (slot 1) into the applied control ua: limits, lag, gain and offset, noise (actuator_limits, actuator_lag,
// actuator_gain, plant_add) against the instance's setup block, each stage only where it is installed -- an absent stage leaves the bits
// alone.  ua takes u0's place in the plant chain and in the score's z, nowhere else: the step log, the x|u record and the estimator's
// prediction keep the command.  Each input lane reads and writes its own cell of the lag's record once per step and stores its entry of the
// actuation log behind the score; whether a lag is installed is wave-uniform (bit 1 of the block pointer).  Everything is formed behind the iteration loop, from
// the kernel-argument segment (late_arg): nothing of it lives through the loop.  A step that ran no iteration takes no plant step and
// runs no stage.  PA implies PP (a launch with no plant installed forms the model's block, as PM does); composes with PD, PM, PE, PS,
// PB / PL / PC and HET; not HALF, PF or ADAPT.  Run-time instantiated only; bit 10 of the sixth template argument (MODE | 1024).
// PQ: a transport delay in front of the actuator's stages (ActuatorLaunch::delay, queue, head).  Inside `applied`, on an input lane whose
// instance has d > 0: the oldest entry of the instance's ring leaves -- it is what the limits see --, the command takes its cell and lane
// NX moves the head: one load and one store per input lane and step, next to the head's.  d = 0 reads and writes nothing and hands the
// command's bits on.  Once per step that takes a plant step, as the lag's record.  PQ rides on PA; bit 12 (MODE | 4096) -- bit 11
// names no form: a name that sets it is refused, as it was before the delay existed (tests/test_actuator_cpu.py asks exactly that).
// PX: a predictor that compensates the delay.  Where a PM / PE form forms the state a step solves from (the top of a tile, behind the
// iteration loop) that state xin is stepped d times by the MODEL over the queue as it stands, oldest first: xs = plant_by(model, xs, q[t])
// -- a run-time loop to the wave's largest d (the four rows of a wave have their own d; a row past its d keeps its xs by a select, so that
// every DPP broadcast of the chain runs under a full EXEC), the input lanes presenting q[t] where the chain reads u0.  Slot 0 of the state
// lanes then holds xs; a PE form keeps xhat in ActuatorLaunch::xhat and reads it back behind the loop for the estimate log and for the
// model's prediction of the next xp, which under PX uses the control that reaches the actuator now (what left the queue), not the
// command.  Nothing of it lives through the iteration loop.  PX rides on PQ and PM; bit 13 (MODE | 8192).
template <int NX, int NU, int N, bool SOC, bool DBG, int MODE_PB, int LIN = 0, bool HET = false, int KMAX = LIN_KMAX, bool ADAPT = false, bool UB = false, bool HALF = false,
          bool PF = false>
__global__ __launch_bounds__(64)
__attribute__((amdgpu_waves_per_eu(LIN != 0 ? solve_kernel_lin_waves(NX, NU, N, SOC, LIN, KMAX, UB, (MODE_PB & 8) != 0) : solve_kernel_waves_per_simd(NX + NU, N, SOC, false, ADAPT),
                                   LIN != 0 ? solve_kernel_lin_waves(NX, NU, N, SOC, LIN, KMAX, UB, (MODE_PB & 8) != 0) : solve_kernel_waves_per_simd(NX + NU, N, SOC, false, ADAPT))))
void admm_solve_kernel(const SolveArgs P) {
    constexpr int MODE = MODE_PB & 3;
    constexpr bool PB = (MODE_PB & 4) != 0;
    constexpr bool PL = (MODE_PB & 8) != 0;
    constexpr bool PC = (MODE_PB & 16) != 0;
    constexpr bool PD = (MODE_PB & 32) != 0;
    constexpr bool PP = (MODE_PB & 64) != 0;
    constexpr bool PM = (MODE_PB & 128) != 0;
    constexpr bool PE = (MODE_PB & 256) != 0;
    constexpr bool PS = (MODE_PB & 512) != 0;
    constexpr bool PA = (MODE_PB & 1024) != 0;
    constexpr bool PQ = (MODE_PB & 4096) != 0;
    constexpr bool PX = (MODE_PB & 8192) != 0;
    static_assert(MODE <= 2 && MODE_PB < 16384 && (MODE_PB & 2048) == 0, "MODE 0 | 1 | 2, + 4: per-instance box, + 8: per-instance half-spaces, + 16: per-instance cone coefficients, + 32: per-instance disturbance, + 64: a plant of its own, + 128: measurement noise, + 256: a state estimator, + 512: a closed-loop score, + 1024: an actuator model, + 4096: a transport delay in front of it, + 8192: a predictor that compensates the delay (2048 names no form)");
    static_assert(!PQ || PA, "a transport delay: a form with an actuator model (PA, bit 10): the queue is popped and pushed inside `applied`");
    static_assert(!PX || (PQ && PM), "a delay predictor: a form with the queue (PQ, bit 12) that solves from something other than the x0 record (PM, bit 7)");
    static_assert(!PA || PP, "an actuator model: a form with a plant block (PP, bit 6): the plant step is a chain over the applied control");
    static_assert(!PA || !ADAPT, "an actuator model: not with adaptive rho (refused)");
    static_assert(!PA || !HALF, "an actuator model: not the half-row form");
    static_assert(!PA || !PF, "an actuator model: not the prefetch form");
    static_assert(!PS || PD || PP, "a closed-loop score: a form that takes its plant step itself (PD, bit 5, or PP, bit 6)");
    static_assert(!PS || !ADAPT, "a closed-loop score: not with adaptive rho (refused)");
    static_assert(!PS || !HALF, "a closed-loop score: not the half-row form");
    static_assert(!PS || !PF, "a closed-loop score: not the prefetch form");
    static_assert(!PE || (PM && PP), "a state estimator: a form that solves from a measured state (PM, bit 7) on a plant block (PP, bit 6)");
    static_assert(!PE || !ADAPT, "a state estimator: not with adaptive rho (refused)");
    static_assert(!PE || !HALF, "a state estimator: not the half-row form");
    static_assert(!PE || !PF, "a state estimator: not the prefetch form");
    static_assert(!PM || PP, "measurement noise: a form with a plant block (PP, bit 6): the true state is stepped through it");
    static_assert(!PM || !ADAPT, "measurement noise: not with adaptive rho (refused)");
    static_assert(!PM || !HALF, "measurement noise: not the half-row form");
    static_assert(!PM || !PF, "measurement noise: not the prefetch form");
    static_assert(!PP || !ADAPT, "a plant of its own: not with adaptive rho (refused)");
    static_assert(!PP || !HALF, "a plant of its own: not the half-row form");
    static_assert(!PP || !PF, "a plant of its own: not the prefetch form");
    static_assert(!PD || !ADAPT, "per-instance disturbance: not with adaptive rho (refused)");
    static_assert(!PD || !HALF, "per-instance disturbance: not the half-row form");
    static_assert(!PD || !PF, "per-instance disturbance: not the prefetch form");
    static_assert(!PC || SOC, "per-instance cone coefficients: a cone variant (SOC)");
    static_assert(!PC || (!PL && !ADAPT), "per-instance cone coefficients: not with per-instance half-spaces (coverage kernel) or adaptive rho (refused)");
    static_assert(!PL || LIN != 0, "per-instance half-spaces: a half-space variant (LIN != 0)");
    static_assert(!PL || !HALF, "per-instance half-spaces: not the half-row form");
    static_assert(!PL || !PF, "per-instance half-spaces: not the prefetch form");
    static_assert(!PL || !ADAPT, "per-instance half-spaces: not with adaptive rho (refused, as on shared half-spaces)");
    static_assert(!PL || !PB, "per-instance half-spaces: not with a per-instance box (that combination runs on the coverage kernel)");
    // the one LDS rule, with the tables counted once per row: a PL form exists where its slack planes and the four rows' tables fit a
    // wave's static LDS; there is no per-knot register form of it (the dispatcher consults the same rule: coverage kernel otherwise)
    static_assert(!PL || solve_kernel_lin_planes(NX, NU, N, SOC, LIN, KMAX, UB, true),
                  "per-instance half-spaces: the slack planes and the four rows' tables must fit the wave's static LDS");
    constexpr bool LS = (LIN & 1) != 0, LT = (LIN & 2) != 0;
    constexpr int NZ = NX + NU;
    static_assert(NZ <= 16, "one instance per 16-lane DPP row");
    constexpr bool FUSED = MODE == 2 && LIN == 0 && fused_shape(NX, NU);              // fused_backward_step(_soc) / fused_forward_step
    // (LIN on the fused blocks -- two / three extra linear-cost terms in the asm statement -- was built and measured: no difference,
    // (12,4,10) + 2 + 2 half-spaces 5.31 ms either way; what the variant pays is its projection step and 208 B/lane of scratch)
    static_assert(!HALF || (NZ <= 8 && FUSED && !SOC && !DBG && !HET && !ADAPT), "half rows: nx+nu <= 8, the plain box kernel on its fused step blocks");
    static_assert(!PF || (MODE == 2 && !SOC && !DBG && LIN == 0 && !HET && !ADAPT), "prefetch form: the plain box kernel");
    static_assert(!PB || (!HALF && !PF), "per-instance box: full rows, not the prefetch form");
    // PB without UB: a wave's static LDS is sPt + the four rows' blocks, 128 NX + 1024 N bytes.  Every shape the kernel holds keeps its
    // waves per SIMD under that: two waves need 6 N + 2 (NX + NU) <= 100, so N <= 16 and eight waves of a CU take at most 8 x 18 KB of its
    // 160 KB; one wave per SIMD ends at N = 37 (the 512-register file), four waves x 38 KB
    static_assert(!PB || UB || 4L * solve_kernel_waves_per_simd(NX + NU, N, SOC, false, ADAPT) * (128 * NX + 1024 * N) <= 160 * 1024,
                  "per-instance box: the rows' bound blocks must leave the shape its waves per SIMD");
    static_assert(!PB || (!SOC && LIN == 0 && !ADAPT), "per-instance box: the box variants (cones, half-spaces and adaptive rho run on the coverage kernel / are refused)");
    constexpr int RL = HALF ? 8 : 16;                                  // lanes of one instance
    constexpr int IPW = 64 / RL;                                       // instances per wave
    constexpr int RECD = N * NZ;                                       // doubles of one instance's record
    constexpr int PF_PIECES = (IPW * RECD * 8 + 1023) / 1024;          // PF: 1-KiB LDS-DMA pieces (64 lanes x 16 B) per array and tile
    constexpr int PF_ARR = PF_PIECES * 128;                            // ... doubles of one array in the tile buffer
    constexpr unsigned long long RMASK = HALF ? 0xFFull : 0xFFFFull;
    const int lane = threadIdx.x & 63;
    const int j = lane & (RL - 1);
    const int grp = lane / RL;
    const bool is_state = j < NX;
    const bool is_input = (j >= NX) && (j < NZ);

    // per-wave LDS copies of the tables that are read with a dynamic index or only once per solve
    __shared__ double sPt[NX * 16];
    __shared__ double sLo[UB ? 1 : (PB ? IPW : 1) * N * 16];   // (UB: the two bounds of a lane live in registers, read from the table once;
    __shared__ double sHi[UB ? 1 : (PB ? IPW : 1) * N * 16];   //  PB: one block per row, filled for every tile)
    __shared__ double sLin[LS ? (PL ? IPW : 1) * 3 * KMAX * 16 : 1];            // (PL: one block per row, filled for every tile from the
    __shared__ double sTLin[LT ? (PL ? IPW : 1) * 3 * N * KMAX * 16 : 1];       //  row's instance: SolveArgs::inst_lin)
    // SOC: the cone slack lives in LDS, not in registers.  Per row and slot three planes of CS cells (lane j: cell j; the lanes beyond
    // NZ share cell NZ):
    //   W   what the next backward sweep adds to the linear cost: vcnew - gc (admm.cpp:269 | :282 | :295).  Between the forward
    //       sweep and the cone step it holds x + gc, the vector the cone step projects (:102-109)
    //   GC  gc | yc (:229 / :234)
    //   VC  vcnew | zcnew of the cells that belong to a (cone, knot) item (the other cells: W holds it, see below)
    // The cone step is transposed -- lane j of pass p owns ONE (cone, knot) item: it gathers the item's three components from W,
    // projects them (one square root / division sequence per pass instead of one per knot) and writes all three planes; the sweeps
    // read W (backward) and GC (forward) one step ahead of their use.  Cells outside every item: the projection is the identity,
    // vcnew = x + gc bit for bit, so gc = 0 and W = x + gc -- what the forward sweep leaves there.  A slot is 3 CS doubles, an ODD
    // number: the item gathers of a pass (stride = one slot) fall into distinct LDS banks.  + a dummy slot whose item (0, 0, 1)
    // the lanes without an item project (onto itself): no EXEC-mask region around the gather / scatter of a pass.
    // SPD: how many sweep steps ahead of its use a cell is read (the ring of SPD + 1 registers per plane)
#ifndef TINYMPC_SOC_PD
#define TINYMPC_SOC_PD 2
#endif
    constexpr int SPD = TINYMPC_SOC_PD, SPR = SPD + 1;
    constexpr int CS = SOC ? ((NZ + 1) | 1) : 1;
    constexpr int SLOT_D = 3 * CS;
    constexpr int PL_GC = CS, PL_VC = 2 * CS;
    __shared__ double sC[SOC ? (4 * N + 1) * SLOT_D : 1];
    __shared__ double sP[ADAPT ? 4 * NX * NX : 1];            // ADAPT: each row's own Pinf, column-major (lane j keeps column j current)
    // ADAPT: the lane tables every adaptation reads (ATAB_AT, ATAB_DK, ATAB_DP), lane-major [table][lane][AKC] so that a lane's
    // coefficients are consecutive (ds_read_b128), and each row's log of rho steps that C1 / C2 still have to take (flush_c)
    constexpr int AKC = NX > NU ? NX : NU;
    // HET && ADAPT: every row has its own instance's tables (SolveArgs::atab is then [batch][ATAB_DOUBLES]).  They are read through
    // L2 at the adaptation itself -- every fifth iteration, three tables of at most 16 x 16 doubles per row -- instead of from four
    // per-row LDS copies (4 x 3 * 16 * AKC doubles: 18 KB per wave at (12,4), which with the 9.5 KB below would leave five waves per CU where the LDS of the
    // shared-family form leaves eight).  LDS per wave of the (12,4,10) form: sPt 1.5 KB + bounds 2 x 1.25 KB + sP 4.5 KB + sDl 1 KB =
    // 9.5 KB, two waves per SIMD as the shared-family ADAPT form.
    constexpr bool HA = HET && ADAPT;
    __shared__ double sTab[(ADAPT && !HET) ? 3 * 16 * AKC : 1];
    __shared__ double sDl[ADAPT ? 4 * ADAPT_LOG : 1];
    if constexpr (ADAPT && !HET)
        for (int e = lane; e < 3 * 16 * AKC; e += 64) {
            const int t = e / (16 * AKC), r = e % (16 * AKC);
            sTab[e] = P.atab[t * 256 + (r % AKC) * 16 + r / AKC];              // ATAB_AT / ATAB_DK / ATAB_DP = 0 / 256 / 512
        }
    if constexpr (LS && !PL) for (int e = lane; e < 3 * KMAX * 16; e += 64) sLin[e] = P.tab[TAB_BOUNDS + 2 * N * 16 + e];
    if constexpr (LT && !PL) for (int e = lane; e < 3 * N * KMAX * 16; e += 64) sTLin[e] = P.tab[TAB_BOUNDS + 2 * N * 16 + 3 * KMAX * 16 + e];
    for (int e = lane; e < NX * 16; e += 64) sPt[e] = P.tab[TAB_PT + e];
    for (int e = lane; e < N * 16; e += 64) {
        if constexpr (!UB && !PB) {
            sLo[e] = P.tab[TAB_BOUNDS + e];
            sHi[e] = P.tab[TAB_BOUNDS + N * 16 + e];
        }
    }
    // this lane's matrix rows
    double mb[NZ], mf1[NX], mf2[NU];
#pragma unroll
    for (int k = 0; k < NZ; ++k) mb[k] = P.tab[TAB_MB + k * 16 + j];
#pragma unroll
    for (int k = 0; k < NX; ++k) mf1[k] = P.tab[TAB_MF1 + k * 16 + j];
#pragma unroll
    for (int k = 0; k < NU; ++k) mf2[k] = P.tab[TAB_MF2 + (NX + k) * 16 + j];
    double cb = P.tab[TAB_VEC + VEC_CB * 16 + j];
    double cf = P.tab[TAB_VEC + VEC_CF * 16 + j];
    double qr = P.tab[TAB_VEC + VEC_QR * 16 + j];
    // (PB: the two masks are formed from the lane index -- the very numbers the table holds, batch_tables.hip -- so that the compiler may
    // form them again where it would otherwise carry or spill them: the per-instance-data form sits at the 256-register limit, and the
    // bounds of a PB form, loaded per tile, cannot be parked in scratch before the tile loop the way the shared ones are)
    const double smask = PB ? (is_state ? 1.0 : 0.0) : P.tab[TAB_VEC + VEC_SMASK * 16 + j];
    const double nim = PB ? (is_input ? -1.0 : 0.0) : P.tab[TAB_VEC + VEC_NIM * 16 + j];
    bool soc_lane = false, proj_lane = false;
    int cone_base = -1, cone_c = 0;
    double socmask = 0.0;
    if constexpr (SOC) {
        socmask = P.tab[TAB_VEC + VEC_SOCFLAG * 16 + j];               // 1.0 on the rows that carry a cone slack
        soc_lane = socmask != 0.0;
        cone_base = (int)P.tab[TAB_VEC + VEC_CONE_BASE * 16 + j];
        cone_c = (cone_base >= 0) ? (j - cone_base) : 0;
        proj_lane = soc_lane && cone_base >= 0;
    }
    // Transposed cone step: the (cone, knot) pairs of a row are dealt out to its lanes, 16 per pass -- lane j of pass p takes
    // item 16 p + j, counted cone by cone (ascending base lane): a state cone has N items (slots 0..N-1), an input cone N-1
    // (slots 1..N-1).  All four rows of a wave share the layout.
    constexpr int SOC_PASSES = SOC ? (soc_item_passes(NX, NU, N) > 0 ? soc_item_passes(NX, NU, N) : 1) : 1;
    int item_at[SOC_PASSES];                                   // LDS index (W plane) of the item's first component; the dummy item for lanes without one
    float item_mu[SOC_PASSES], item_rmu[SOC_PASSES];
    bool mu_pow2 = !PC;                                        // every cone coefficient of the launch is 2^k, |k| <= 60 (wave-uniform): soc_project3 multiplies (PC: never)
    int soc_passes = 0;                                        // passes that hold an item (wave-uniform: a family whose cone is off has none)
    if constexpr (SOC) {
        if (lane < 3) {                                        // the dummy item: W = VC = (0, 0, 1), GC = 0
            sC[4 * N * SLOT_D + lane] = lane == 2 ? 1.0 : 0.0;
            sC[4 * N * SLOT_D + PL_GC + lane] = 0.0;
            sC[4 * N * SLOT_D + PL_VC + lane] = lane == 2 ? 1.0 : 0.0;
        }
        const unsigned heads = (unsigned)(__builtin_amdgcn_ballot_w64(proj_lane && cone_c == 0) & 0xFFFFull);   // row 0 speaks for all
#pragma unroll
        for (int p = 0; p < SOC_PASSES; ++p) {
            int t = p * 16 + j;
            item_at[p] = 4 * N * SLOT_D; item_mu[p] = 1.0f;
            if (heads && p * 16 < soc_items_of(heads, NX, N)) soc_passes = p + 1;
            for (unsigned m = heads; m; m &= m - 1) {
                const int hb = __builtin_ctz(m);
                const int cnt = hb < NX ? N : N - 1;
                if (t >= 0 && t < cnt) {
                    item_at[p] = (grp * N + t + (hb < NX ? 0 : 1)) * SLOT_D + hb;
                    if constexpr (!PC) item_mu[p] = (float)P.tab[TAB_VEC + VEC_CONE_MU * 16 + hb];      // (PC: the row's instance has its own, loaded for every tile)
                    t = -1;
                } else if (t >= 0) t -= cnt;
            }
            item_rmu[p] = 1.0f / item_mu[p];
            if constexpr (!PC) {
                const unsigned mb_ = __float_as_uint(item_mu[p]);
                const bool p2 = (mb_ & 0x807FFFFFu) == 0u && (mb_ >> 23) >= 127u - 60u && (mb_ >> 23) <= 127u + 60u;
                if (__builtin_amdgcn_ballot_w64(!p2) != 0ull) mu_pow2 = false;
            }
        }
    }
    bool lin_lane = false, tlin_lane = false;
    if constexpr (LS) lin_lane = P.tab[TAB_VEC + VEC_LINFLAG * 16 + j] != 0.0;
    if constexpr (LT) tlin_lane = P.tab[TAB_VEC + VEC_TLINFLAG * 16 + j] != 0.0;
    // LIN: the half-space slacks live in LDS -- per set (static | time-varying) two planes of one cell per row and slot: V (x + gl
    // between the forward sweep and the projection step, then vlnew) and G (gl); the backward sweep adds -rho (V - G) (admm.cpp:272
    // ...), read two steps ahead like the cone slack.  The projections are transposed (project_halfspace_columns): a lane holds
    // the box kernel's arrays, nothing per slot but one LDS write, and the variant runs two waves per SIMD.
    // (LSP / LTP: the set's slack in planes; LSR / LTR: in register arrays, projected per knot -- the variant whose planes do not fit)
    constexpr bool LPL = solve_kernel_lin_planes(NX, NU, N, SOC, LIN, KMAX, UB, PL);
    constexpr bool LSP = LS && LPL, LTP = LT && LPL, LSR = LS && !LPL, LTR = LT && !LPL;
    constexpr int CSL = LPL ? ((NZ + 1) | 1) : 1;
    __shared__ double sLV[LSP ? 4 * N * CSL : 1], sLG[LSP ? 4 * N * CSL : 1];
    __shared__ double sTV[LTP ? 4 * N * CSL : 1], sTG[LTP ? 4 * N * CSL : 1];
    double ones[(LSR || LTR) ? 16 : 1];
#pragma unroll
    for (int k = 0; k < ((LSR || LTR) ? 16 : 1); ++k) ones[k] = 1.0;
    bool lin_x_on = false, lin_u_on = false, tlin_x_on = false, tlin_u_on = false;     // which families (uniform over the wave)
    if constexpr (LS) { lin_x_on = P.tab[TAB_VEC + VEC_LINFLAG * 16] != 0.0; lin_u_on = P.tab[TAB_VEC + VEC_LINFLAG * 16 + NX] != 0.0; }
    if constexpr (LT) { tlin_x_on = P.tab[TAB_VEC + VEC_TLINFLAG * 16] != 0.0; tlin_u_on = P.tab[TAB_VEC + VEC_TLINFLAG * 16 + NX] != 0.0; }
    double rho = P.rho;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();   // LDS tables were written by other lanes of this wave

    // UB: slot 1 speaks for every slot (slot 0 of an input lane is the neutral dummy: its box stays (-inf, +inf))
    // (PB: the row's instance has its own, loaded for every tile: rlo_u ... below)
    const double lo_u = PB ? 0.0 : P.tab[TAB_BOUNDS + (N > 1 ? 16 : 0) + j], hi_u = PB ? 0.0 : P.tab[TAB_BOUNDS + N * 16 + (N > 1 ? 16 : 0) + j];
    const double lo_u0 = PB ? 0.0 : P.tab[TAB_BOUNDS + j], hi_u0 = PB ? 0.0 : P.tab[TAB_BOUNDS + N * 16 + j];
    const int sbox = PB ? grp * (N * 16) : 0;                  // PB && !UB: this row's block of sLo / sHi
    // PL: this row's blocks of sLin / sTLin (the shared forms: the wave's one)
    const double* const rLin = sLin + (PL ? grp * (3 * KMAX * 16) : 0);
    const double* const rTLin = sTLin + (PL ? grp * (3 * N * KMAX * 16) : 0);
    // (PF: a plain single-step launch over the whole batch -- no index list, no permutation, no trajectory window: those paths are
    // compiled OUT of the form, because a register-returning load on ANY path between a tile's hand-over and its stores makes the
    // compiler wait for the whole VMEM queue at the join, the next tile's pieces included)
    const int ninst = PF ? P.batch : (P.index ? *P.count : (P.perm ? P.perm_count : P.batch));
    const int ntiles = (ninst + IPW - 1) / IPW;
    const bool resumed = !PF && P.index != nullptr;
    const bool has_traj = !PF && P.traj != nullptr;
    // ---- PREFETCH form: the tile buffer (the launch's dynamic LDS: [x0 piece: 128 doubles][the arrays of pf_mask, PF_ARR each]) and who
    // fills it.  A piece is ONE global_load_lds_dwordx4: lane l's 16 bytes land at piece base + 16 l, so the buffer mirrors the records'
    // own layout [instance][knot][row]; the tile's instances are consecutive (a plain launch).  The last pieces of a tile reach up to
    // 1 KiB past it -- past the END of the array for the last tile: the host allocates every record array and x0 with that much slack
    // (batch_api.hip PF_SLACK_BYTES; nobody reads what those bytes bring).
    extern __shared__ __attribute__((aligned(16))) double sPF[];
    typedef const __attribute__((address_space(1))) void* pf_gptr;
    typedef __attribute__((address_space(3))) void* pf_lptr;
    // Buffer slots (compile-time offsets, so that every buffer read is ONE base register + an immediate): [x0 piece][S0][S1][S2][S3].
    // Warm launches: S0 vnew|znew, S1 g|y, S2 v|z, S3 the reference record when every instance has its own (pf_mask bit 3); cold
    // launches read nothing but the reference record: S0.  EVERY record read of a tile goes through the buffer: one register-returning
    // load left in flight across the hand-over would make the compiler's own wait for it -- which cannot tell the pieces issued behind
    // it apart -- a wait for the next tile's records too, and the prefetch would hide nothing (measured: round 6, first form).
    constexpr int PF_S0 = 128, PF_S1 = PF_S0 + PF_ARR, PF_S2 = PF_S1 + PF_ARR, PF_S3 = PF_S2 + PF_ARR;
    auto pf_issue = [&](const int t) {
        const int tl = P.reverse ? ntiles - 1 - t : t;
        __builtin_amdgcn_global_load_lds((pf_gptr)(P.x0 + ((size_t)tl * (IPW * NX) + (size_t)lane * 2)), (pf_lptr)sPF, 16, 0, 0);
        const size_t t0 = (size_t)tl * (IPW * RECD) + (size_t)lane * 2;
        auto arr = [&](const double* p, const int at) {
#pragma unroll
            for (int q = 0; q < PF_PIECES; ++q) __builtin_amdgcn_global_load_lds((pf_gptr)(p + t0 + q * 128), (pf_lptr)(sPF + at + q * 128), 16, 0, 0);
        };
        if (!P.cold) { arr(P.slack, PF_S0); arr(P.dual, PF_S1); arr(P.slack_prev, PF_S2); }
        if (P.pf_mask & 8) arr(P.ref, P.cold ? PF_S0 : PF_S3);
    };
    unsigned pf_ticket = 0u;                                   // (lane 0) the ticket drawn for the tile after the next one
    const int pf_shard = PF ? (int)(blockIdx.x % (unsigned)(P.pf_shards > 0 ? P.pf_shards : 1)) : 0;
    // (the pointer goes through an empty asm: LLVM's atomic optimizer rewrites an add of a uniform value to a UNIFORM address into one
    // wave-wide add whose result it reads back -- readfirstlane, i.e. a full VMEM wait -- on the spot; a ticket is not needed before the
    // next tile's top, and that is where its wait belongs)
    typedef __attribute__((address_space(1))) unsigned* pf_ctr_t;
    unsigned long long pf_ctr_bits = PF ? (unsigned long long)(P.pf_counter + 16 * pf_shard) : 0ull;
    if constexpr (PF) asm volatile("" : "+v"(pf_ctr_bits));
    const pf_ctr_t pf_ctr = (pf_ctr_t)pf_ctr_bits;
    auto pf_draw = [&]() { return lane == 0 ? __hip_atomic_fetch_add(pf_ctr, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u; };
    const unsigned pf_base = PF ? P.pf_base[pf_shard] : 0u;
    int pf_next = 0, pf_i = 0;                                 // (pf_i: tiles this wave has taken)
    bool pf_first = true;
    // a reference record every instance shares: -(ref x diagonal) and the terminal term are formed ONCE per wave and kept in LDS
    // (one 16-lane row per slot): a tile reads them back instead of carrying ten more doubles per lane from tile to tile
    double* const sQX = sPF + PF_S3;                           // (the slot of the per-instance records: free when the record is shared)
    if constexpr (PF) {
        if ((int)blockIdx.x < ntiles) {
            pf_issue((int)blockIdx.x);
            if (P.pf_static <= 1) pf_ticket = pf_draw();           // (the second tile is a ticketed one already)
        }
        if (P.ref_shared) {
            double rl = 0.0, qxs[N];
#pragma unroll
            for (int s = 0; s < N; ++s) {
                const bool valid = is_state || (is_input && s >= 1);
                const double r = valid ? P.ref[j - (is_input ? NZ : 0) + s * NZ] : 0.0;
                qxs[s] = -(r * qr);
                if (s == N - 1) rl = r;
            }
            double pt[NX];
#pragma unroll
            for (int k = 0; k < NX; ++k) pt[k] = sPt[k * 16 + j];
            double xp = 0.0;
            if constexpr (HALF) ring1_half<0, NX>(xp, rl, pt);
            else xp = ring_sum<MODE, 0, NX>(0.0, rl, pt);
            qxs[N - 1] = is_state ? -xp : qxs[N - 1];          // (terminal_term below, for the shared record)
            if (grp == 0) {
#pragma unroll
                for (int s = 0; s < N; ++s) sQX[s * 16 + j] = qxs[s];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    // Tiles of 4 instances: one per wave (grid = tiles), or -- a follow-up stage of a split solve, fewer waves than tiles -- the wave
    // takes its next tile off the stage's counter the moment it is free (its tiles differ in depth: a fixed stride would make the
    // stage wait for the slot that drew the deepest ones)
    for (int tile = blockIdx.x; tile < ntiles;
         tile = PF ? pf_next : (P.work_counter ? __builtin_amdgcn_readfirstlane(lane == 0 ? atomicAdd(P.work_counter, 1) : 0) + (int)gridDim.x : tile + (int)gridDim.x)) {
        const int slot = (P.reverse ? ntiles - 1 - tile : tile) * IPW + grp;
        // PF: every lane takes its part of the tile out of the buffer (the rows of a last, partial tile: whatever the clamped pieces
        // brought -- they do not use it), then the buffer is handed to the NEXT tile's records: issued here, under the full EXEC mask,
        // in flight while this tile iterates.  Order of this wave's VMEM operations per tile: [reads of the arrays that do not travel
        // through the buffer] [ticket] [the next tile's pieces] ... [this tile's stores].
        double pfVN[PF ? N : 1], pfG[PF ? N : 1], pfVP[PF ? N : 1], pfQXs[PF ? N : 1], pf_x0 = 0.0, pf_rl = 0.0;
        if constexpr (PF) {
            // The tile's records have landed when the wave's own VMEM counter says so -- nothing else orders a ds_read behind a pending
            // LDS-DMA.  A wave's VMEM operations complete in issue order; behind this tile's pieces only the stores of the tile before
            // were issued, among them N each to the vnew|znew and g|y records when the launch writes both: those may stay in flight.
            if (pf_first) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if ((P.store_mask & 6) == 6) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * N <= 63 ? 2 * N : 63) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            pf_first = false;
            if (pf_i + 1 < P.pf_static) pf_next = tile + (int)gridDim.x;
            else {
                unsigned pf_t;                                    // (volatile: the read-back stays HERE, behind the wait above)
                asm volatile("v_readfirstlane_b32 %0, %1" : "=s"(pf_t) : "v"(pf_ticket));
                pf_next = (int)(pf_t - pf_base) * P.pf_shards + pf_shard + (P.pf_static > 1 ? P.pf_static : 1) * (int)gridDim.x;
            }
            const int m = P.pf_mask;
            // this lane's cell of slot 0 in a buffer array (input lanes: knot s-1 at slot s; their slot 0 and the lanes beyond nx+nu read
            // a cell nobody uses: at worst the 16 doubles in FRONT of the array, which the x0 piece covers)
            const int lrow = grp * RECD + (j < NZ ? j - (is_input ? NZ : 0) : 0);
            const bool warm_t = !P.cold;
            pf_x0 = sPF[grp * NX + (is_state ? j : 0)];
#pragma unroll
            for (int s = 0; s < N; ++s) { pfVN[s] = 0.0; pfG[s] = 0.0; pfVP[s] = 0.0; }
            if (warm_t) {
#pragma unroll
                for (int s = 0; s < N; ++s) { pfVN[s] = sPF[PF_S0 + lrow + s * NZ]; pfG[s] = sPF[PF_S1 + lrow + s * NZ]; }
            }
            auto own_ref = [&](const int at) {                    // this instance's own reference record: -(ref x diagonal), admm.cpp:266 / :279
#pragma unroll
                for (int s = 0; s < N; ++s) {
                    const bool valid = is_state || (is_input && s >= 1);
                    const double r = valid ? sPF[at + lrow + s * NZ] : 0.0;
                    pfQXs[s] = -(r * qr);
                    if (s == N - 1) pf_rl = r;
                }
            };
            if (m & 8) { if (warm_t) own_ref(PF_S3); else own_ref(PF_S0); }      // (two call sites: the slot is an immediate in each)
            else {
#pragma unroll
                for (int s = 0; s < N; ++s) pfQXs[s] = sQX[s * 16 + j];
            }
            if (warm_t) {
#pragma unroll
                for (int s = 0; s < N; ++s) pfVP[s] = sPF[PF_S2 + lrow + s * NZ];
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // the buffer's contents are in registers: it is free
            if (pf_next < ntiles) {                               // (a wave stops drawing with its first ticket beyond the batch)
                // the tile after the next one is a ticketed one.  A BRANCH (the empty asm keeps it one): as a select, or assigned on every
                // path, the ticket register -- which may have a draw in flight -- would be touched in every tile, and the compiler waits
                // for the whole VMEM queue before it touches it: the stores of the tile before would never stay in flight
                if (pf_i + 2 >= P.pf_static) {
                    asm volatile("" ::: "memory");
                    pf_ticket = pf_draw();
                }
                pf_issue(pf_next);
            }
            ++pf_i;
        }
        (void)pfVN; (void)pfG; (void)pfVP; (void)pf_rl; (void)pf_x0; (void)pfQXs; (void)pf_first; (void)pf_ticket; (void)sQX; (void)pf_ctr; (void)pf_base; (void)pf_draw; (void)pf_i;
        if (slot < ninst) {
            const int b = PF ? slot : (resumed ? P.index[slot] : (P.perm ? P.perm[slot] : slot));
            const double* het = nullptr;
            if constexpr (HET) {                               // this instance's own cache (A, B, Q, R, rho differ per instance)
                het = P.het_tabs + (size_t)b * TAB_BOUNDS;
#pragma unroll
                for (int k = 0; k < NZ; ++k) mb[k] = het[TAB_MB + k * 16 + j];
#pragma unroll
                for (int k = 0; k < NX; ++k) mf1[k] = het[TAB_MF1 + k * 16 + j];
#pragma unroll
                for (int k = 0; k < NU; ++k) mf2[k] = het[TAB_MF2 + (NX + k) * 16 + j];
                cb = het[TAB_VEC + VEC_CB * 16 + j];
                cf = het[TAB_VEC + VEC_CF * 16 + j];
                qr = het[TAB_VEC + VEC_QR * 16 + j];
                rho = het[TAB_VEC + VEC_RHO * 16 + j];
            }
            // the row's box of a UB form: the wave's (shared box), or -- PB -- this instance's own: [lo | hi][N slots][16 lanes]
            double rlo_u = lo_u, rhi_u = hi_u, rlo_u0 = lo_u0, rhi_u0 = hi_u0;
            if constexpr (PB) {
                // (this lane's entry of slot 0, as ONE offset formed here: split into a per-lane part and a per-instance part, the former
                // is hoisted out of the tile loop and held -- or spilled -- from the kernel's first instruction to its last)
                size_t ib_at = (size_t)b * (2 * N * 16) + j;
                asm volatile("" : "+v"(ib_at));
                const double* ib = P.inst_bounds + ib_at;
                if constexpr (UB) {                            // slot 1 speaks for every slot but an input lane's dummy slot 0
                    rlo_u0 = ib[0]; rhi_u0 = ib[N * 16];
                    rlo_u = ib[N > 1 ? 16 : 0]; rhi_u = ib[N * 16 + (N > 1 ? 16 : 0)];
                } else {                                       // one 128-byte segment per slot and bound, by the row's own lanes
#pragma unroll
                    for (int s = 0; s < N; ++s) { sLo[sbox + s * 16 + j] = ib[s * 16]; sHi[sbox + s * 16 + j] = ib[N * 16 + s * 16]; }
                    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                    __builtin_amdgcn_wave_barrier();
                }
            }
            if constexpr (PL) {
                // the row's own half-space tables, by the row's own lanes: one 128-byte segment per table row, the instance's blocks in
                // the order the form's sets have them (static, then one per slot).  A row without an instance (a partial last tile) is
                // not here: it reads nothing
                constexpr int LBLK = 3 * KMAX * 16;
                size_t il_at = (size_t)b * ((LS ? LBLK : 0) + (LT ? N * LBLK : 0)) + j;
                asm volatile("" : "+v"(il_at));
                const double* il = P.inst_lin + il_at;
                if constexpr (LS) {
#pragma unroll
                    for (int e = 0; e < 3 * KMAX; ++e) sLin[grp * LBLK + e * 16 + j] = il[e * 16];
                }
                if constexpr (LT) {
                    const double* ilt = il + (LS ? LBLK : 0);
                    for (int e = 0; e < 3 * KMAX * N; ++e) sTLin[grp * (N * LBLK) + e * 16 + j] = ilt[e * 16];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if constexpr (PC) {
                // the coefficient of this lane's item in every pass: the item's cone starts at lane hb of the row (item_at holds it: a
                // slot is SLOT_D > 16 doubles), the row's instance keeps its coefficient there.  A lane without an item keeps the dummy's 1.0
                // (one load per pass, all from the row's 128-byte block.  One load per lane and a ds_bpermute per pass was built, too: it
                // costs 4 to 8 B/lane of scratch more in four of the five forms that spill at all, and saves none in any)
                size_t ic_at = (size_t)b * 16;
                asm volatile("" : "+v"(ic_at));
                const double* ic = P.inst_cones + ic_at;
#pragma unroll
                for (int p = 0; p < SOC_PASSES; ++p) {
                    // (through an empty asm: the lane's offset is the same in every tile, and formed once in front of the tile loop it
                    // would be held -- or spilled -- from the kernel's first instruction to its last, as at PB)
                    int at = item_at[p];
                    asm volatile("" : "+v"(at));
                    const bool has = at != 4 * N * SLOT_D;
                    const float own = (float)ic[has ? at % SLOT_D : 0];
                    item_mu[p] = has ? own : 1.0f;
                }
            }
            if constexpr (ADAPT) {                             // this instance's own rho / Kinf / Pinf (they persist from solve to solve)
                rho = P.arho[b];
                const double* aK = P.aK + (size_t)b * (NU * NX);
                if (is_state) {
#pragma unroll
                    for (int k = 0; k < NU; ++k) mb[NX + k] = -aK[k + NU * j];            // -Kinf'[j][k]
#pragma unroll
                    for (int k = 0; k < NX; ++k) sP[grp * NX * NX + k + NX * j] = P.aP[(size_t)b * (NX * NX) + k + NX * j];
                } else if (is_input) {
#pragma unroll
                    for (int k = 0; k < NX; ++k) mf1[k] = -aK[(j - NX) + NU * k];         // -Kinf[j-nx][k]
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            // ADAPT: the lane tables of the adaptation -- the family's, or (HET) this instance's own, re-based for every tile
            const double* atab_i = nullptr;
            if constexpr (HET && ADAPT) atab_i = P.atab + (size_t)b * ATAB_DOUBLES;
            (void)atab_i;
            // record base of this lane: input lanes read knot s-1 at slot s
            const size_t lbase = (size_t)b * (N * NZ) + j - (is_input ? NZ : 0);
            double X[N], G[N], VN[N], VP[N], QX[N], Dn[N - 1];
            // cone slack cells of this lane (W plane of slot 0): sC[cw + s * SLOT_D (+ PL_GC | PL_VC)]
            const int cw = grp * N * SLOT_D + (j < NZ ? j : NZ);
            // PM: what the solver is handed for the true state xt at MPC step `at_step` -- fl(xt + v[meas_step0 + at_step][b]) on a state
            // lane where that row exists (wave-uniform test), else xt as it is
            auto measured = [&](const double xt, const int at_step) -> double {
                const int mk = P.meas_step0 + at_step;
                if ((unsigned)mk >= (unsigned)P.meas_steps || !is_state) return xt;
                int m_b = b;
                asm volatile("" : "+v"(m_b));
                return plant_add(xt, P.meas[((size_t)mk * P.batch + m_b) * NX + j]);
            };
            (void)measured;
            double x0v_in = is_state ? (PF ? pf_x0 : P.x0[(size_t)b * NX + j]) : 0.0;      // tiny_set_x0
            if constexpr (PM) x0v_in = measured(x0v_in, 0);
            // PE: what the solver is handed for the measurement xm under the predicted estimate xp -- row j of the instance's gain over
            // the row's innovation, on the accumulator that starts at xp (the input lanes' rows of the block are zero, and so are their
            // xm and xp).  Called at the top of a tile and behind the iteration loop only; everything it needs is formed there
            auto corrected = [&](const double xm, const double xp) -> double {
                const double e = plant_sub(xm, xp);
                int g_b = b;
                asm volatile("" : "+v"(g_b));
                const unsigned long long raw = reinterpret_cast<unsigned long long>(late_arg<const double>(__builtin_offsetof(SolveArgs, est_gain)));
                const double* gt = reinterpret_cast<const double*>(raw & ~1ull) + ((raw & 1ull) ? (size_t)0 : (size_t)g_b * (NX * 16)) + j;
                double acc = xp;
                plant_chain<0, NX>(acc, e, gt);
                return is_state ? acc : 0.0;
            };
            (void)corrected;
            if constexpr (PE) x0v_in = corrected(x0v_in, is_state ? late_arg<double>(__builtin_offsetof(SolveArgs, est_xp))[(size_t)b * NX + j] : 0.0);
            // PX: what the solver is handed for xin (the x0 record, the measurement or the corrected estimate) under a delay of d steps
            // -- xin stepped d times by the MODEL over the instance's queue as it stands, oldest first: the chain of plant_by, the
            // accumulator starting at f.  The loop runs to the largest d of the wave's rows (the ballot counts the rows of the tile
            // only) and a row past its own d keeps its xs by a select: every lane of a row stays in the chain's DPP broadcasts.  The
            // input lanes present q[t] where the chain reads u0.  d = 0: xin's own bits.  Called where `corrected` is
            auto compensated = [&](const double xin) -> double {
                if constexpr (PX) {
                    int c_b = b;
                    asm volatile("" : "+v"(c_b));
                    const DelayLaunch* const act = delay_launch_of(late_arg<const ActuatorLaunch>(__builtin_offsetof(SolveArgs, act)));
                    const int d = act->delay[c_b], h = act->head[c_b];
                    const unsigned long long raw = reinterpret_cast<unsigned long long>(act->model);
                    const double* const pt = reinterpret_cast<const double*>(raw & ~1ull) + ((raw & 1ull) ? (size_t)0 : (size_t)c_b * ((NZ + 1) * 16)) + j;
                    const double* const q = act->queue + (size_t)c_b * act->d_max * NU + (is_input ? j - NX : 0);
                    double xs = xin;
                    for (int t = 0; __ballot(t < d) != 0ull; ++t) {
                        const bool mine = t < d;
                        const int at = h + t < d ? h + t : h + t - d;              // (the ring: the oldest entry sits at the head)
                        const double qt = (mine && is_input) ? q[(size_t)at * NU] : 0.0;
                        double acc = pt[NZ * 16];
                        plant_chain<0, NX>(acc, xs, pt);
                        plant_chain<NX, NU>(acc, qt, pt + NX * 16);
                        xs = (mine && is_state) ? acc : xs;
                    }
                    return xs;
                } else {
                    return xin;
                }
            };
            (void)compensated;
            // (a PE form keeps xhat in memory while slot 0 holds the predicted state: this lane's own cell, read back behind the loop)
            auto xhat_cell = [&]() -> double* {
                int x_b = b;
                asm volatile("" : "+v"(x_b));
                return delay_launch_of(late_arg<const ActuatorLaunch>(__builtin_offsetof(SolveArgs, act)))->xhat + ((size_t)x_b * NX + (is_state ? j : 0));
            };
            (void)xhat_cell;
            if constexpr (PX) {
                if constexpr (PE) { if (is_state) *xhat_cell() = x0v_in; }
                x0v_in = compensated(x0v_in);
            }
            const int cl = grp * N * CSL + (j < NZ ? j : NZ);  // LIN: this lane's cell of slot 0 (slot s: + s * CSL)
            double VL[LSR ? N : 1], GL[LSR ? N : 1], VT[LTR ? N : 1], GT[LTR ? N : 1];
            double Qd[DBG ? N : 1], Pd[DBG ? N : 1], Dd[DBG ? N : 1];
            double ref_last = 0.0, qx_last_plain = 0.0;
            // ---- load the instance record (coalesced: contiguous NZ*8-byte knot segments)
#pragma unroll
            for (int s = 0; s < N; ++s) {
                const bool valid = is_state || (is_input && s >= 1);
                const size_t off = lbase + s * NZ;
                const bool warm = valid && !P.cold;
                if constexpr (PF) {                          // (what the tile buffer held; a shared reference record: formed once per wave)
                    VN[s] = warm ? pfVN[s] : 0.0;
                    G[s] = warm ? pfG[s] : 0.0;
                    VP[s] = warm ? pfVP[s] : 0.0;
                    QX[s] = pfQXs[s];
                    X[s] = 0.0;
                    if (s == N - 1) ref_last = pf_rl;
                    continue;
                }
                const double r = valid ? (P.ref_shared ? P.ref[off - (size_t)b * (N * NZ)] : load_ref(P.ref + off)) : 0.0;
                VN[s] = warm ? P.slack[off] : 0.0;
                G[s] = warm ? P.dual[off] : 0.0;
                VP[s] = warm ? P.slack_prev[off] : 0.0;
                QX[s] = -(r * qr);                           // admm.cpp:266 / :279
                X[s] = 0.0;
                if (s == N - 1) ref_last = r;
                if constexpr (SOC) {
                    // vcnew = x, zcnew = u of the solve before (admm.cpp:352-357; x[:,0] = x0 is already in place then); gc | yc
                    double vc0 = (warm && soc_lane) ? (resumed ? P.cslack : P.prim)[off] : 0.0;
                    const double gc0 = (warm && soc_lane) ? P.cdual[off] : 0.0;
                    if (s == 0 && is_state && soc_lane && !resumed) vc0 = x0v_in;
                    sC[cw + s * SLOT_D] = vc0 - gc0;
                    sC[cw + s * SLOT_D + PL_GC] = gc0;
                    sC[cw + s * SLOT_D + PL_VC] = vc0;
                }
                if constexpr (LS) {
                    const double vl0 = (warm && lin_lane) ? (resumed ? P.lslack : P.prim)[off] : 0.0;      // admm.cpp:361-365
                    const double gl0 = (warm && lin_lane) ? P.ldual[off] : 0.0;
                    if constexpr (LSP) { sLV[cl + s * CSL] = vl0; sLG[cl + s * CSL] = gl0; } else { VL[s] = vl0; GL[s] = gl0; }
                }
                if constexpr (LT) {
                    const double vt0 = (warm && tlin_lane) ? (resumed ? P.tlslack : P.prim)[off] : 0.0;    // admm.cpp:370-374
                    const double gt0 = (warm && tlin_lane) ? P.tldual[off] : 0.0;
                    if constexpr (LTP) { sTV[cl + s * CSL] = vt0; sTG[cl + s * CSL] = gt0; } else { VT[s] = vt0; GT[s] = gt0; }
                }
                if constexpr (DBG) { Qd[s] = 0.0; Pd[s] = 0.0; Dd[s] = 0.0; }
            }
            double x0v = x0v_in;
            auto terminal_term = [&]() {   // -(Xref[:,N-1]^T Pinf) (admm.cpp:292); only state lanes' ref_last is broadcast
                double pt[NX];
#pragma unroll
                for (int k = 0; k < NX; ++k)
                    pt[k] = ADAPT ? sP[grp * NX * NX + k + NX * (is_state ? j : 0)] : (HET ? het[TAB_PT + k * 16 + j] : sPt[k * 16 + j]);
                double xp = 0.0;
                if constexpr (HALF) ring1_half<0, NX>(xp, ref_last, pt);
                else xp = ring_sum<MODE, 0, NX>(0.0, ref_last, pt);
                qx_last_plain = QX[N - 1];                   // q[:,N-1] uses -Xref*Q, p[:,N-1] the terminal term
                QX[N - 1] = is_state ? -xp : QX[N - 1];
            };
            int ndl = 0;                                       // ADAPT: rho steps logged in sDl and not yet taken by C1 / C2
            auto flush_c = [&](int n) {                        // update_matrices_with_derivatives, rho_benchmark.cpp:196-210 (C1, C2)
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                if (P.aC2 && is_state) {
                    double* c2 = P.aC2 + (size_t)b * (NX * NX) + NX * j;
                    double v[NX], d[NX];
#pragma unroll
                    for (int k = 0; k < NX; ++k) { v[k] = c2[k]; d[k] = P.atab[(HA ? (size_t)b * ATAB_DOUBLES : (size_t)0) + ATAB_DC2 + k * 16 + j]; }
                    for (int i = 0; i < n; ++i) {
                        const double dl = sDl[grp * ADAPT_LOG + i];
#pragma unroll
                        for (int k = 0; k < NX; ++k) v[k] = taylor_step(v[k], dl, d[k]);
                    }
#pragma unroll
                    for (int k = 0; k < NX; ++k) c2[k] = v[k];
                }
                if (P.aC1 && j < NU) {
                    double* c1 = P.aC1 + (size_t)b * (NU * NU) + NU * j;
                    double v[NU], d[NU];
#pragma unroll
                    for (int k = 0; k < NU; ++k) { v[k] = c1[k]; d[k] = P.atab[(HA ? (size_t)b * ATAB_DOUBLES : (size_t)0) + ATAB_DC1 + k * 16 + j]; }
                    for (int i = 0; i < n; ++i) {
                        const double dl = sDl[grp * ADAPT_LOG + i];
#pragma unroll
                        for (int k = 0; k < NU; ++k) v[k] = taylor_step(v[k], dl, d[k]);
                    }
#pragma unroll
                    for (int k = 0; k < NU; ++k) c1[k] = v[k];
                }
            };
            if (!has_traj && !(PF && P.ref_shared)) terminal_term();
            const int traj_k0 = has_traj ? (P.traj_step0 + (P.traj_offsets ? P.traj_offsets[b] : 0)) : 0;

            int iter = 0, solved = 0, checked = 0;
            unsigned acc_iter = 0, acc_solved = 0;
            bool vp_touched = false;                           // v|z differ from what was loaded (a solve that converges at its first check leaves them alone)
            double rp = 0.0, rd = 0.0;
            const int nsteps = PF ? 1 : (P.steps > 1 ? P.steps : 1);
            // PD: what the plant step of MPC step `at_step` hands on for this lane's x1 -- fl(x1 + w[dist_step0 + at_step][b]) on a state
            // lane where that row exists (the test is wave-uniform: a step outside the sequence loads and adds nothing), else x1 as it
            // is.  Called at the END of a step and at the x0_next store, and everything it needs is formed there: nothing of it
            // lives through the iteration loop
            auto disturbed = [&](const double x1, const int at_step) -> double {
                const int dk = P.dist_step0 + at_step;
                if ((unsigned)dk >= (unsigned)P.dist_steps || !is_state) return x1;
                // (the instance index through an empty asm: what is formed from it is the same in every step of a tile, and formed
                // once in front of the step loop it would be held -- or spilled -- through the iteration loop, as at PB and PC.  On
                // the 32-bit index, which is alive anyway, not on the 64-bit offset: that product in front of the asm was hoisted)
                int d_b = b;
                asm volatile("" : "+v"(d_b));
                return plant_add(x1, P.dist[((size_t)dk * P.batch + d_b) * NX + j]);
            };
            (void)disturbed;
            // PP: what the plant hands on for this lane -- the chain above over the row's x0 (slot 0 of the state lanes) and u0 (slot 1 of
            // the input lanes); like `disturbed` called behind the iteration loop only, and everything it needs is formed there
            auto plant_by = [&](const double* const blocks, const double x0_row, const double u0_row) -> double {
                int p_b = b;
                asm volatile("" : "+v"(p_b));
                const unsigned long long raw = reinterpret_cast<unsigned long long>(blocks);
                const double* pt = reinterpret_cast<const double*>(raw & ~1ull) + ((raw & 1ull) ? (size_t)0 : (size_t)p_b * ((NZ + 1) * 16)) + j;
                double acc = pt[NZ * 16];
                plant_chain<0, NX>(acc, x0_row, pt);
                plant_chain<NX, NU>(acc, u0_row, pt + NX * 16);
                return acc;
            };
            auto plant_step = [&](const double x0_row, const double u0_row) -> double { return plant_by(P.plant, x0_row, u0_row); };
            (void)plant_step;
            // PE: the estimate the MODEL predicts from the row's xhat and u0 -- the same chain over SolveArgs::est_model
            auto predicted = [&](const double xhat_row, const double u0_row) -> double {
                const double xn = plant_by(late_arg<const double>(__builtin_offsetof(SolveArgs, est_model)), xhat_row, u0_row);
                return is_state ? xn : 0.0;
            };
            (void)predicted;
            // PM: the true state MPC step `at_step` of this launch started from, re-read behind its iteration loop from where the plant
            // step before put it (this lane's own cell of x0_next; step 0: x0) -- no register carries it through the loop.  x0_next need
            // not be x0 (it is, in every launch the library makes): step 0 reads x0, every later step what the step before it stored to
            // x0_next.  A launch of more than one step always has x0_next (bind_common_args: fused steps imply the plant step); the
            // store in the step loop tests it all the same, as the last step's does, and without it every step reads x0
            auto true_cell = [&]() -> size_t {                 // (this lane's cell of x0 / x0_next, formed where it is used)
                int t_b = b;
                asm volatile("" : "+v"(t_b));
                return (size_t)t_b * NX + j;
            };
            auto true_x0 = [&](const int at_step, const size_t cell) -> double {
                const double* from = (at_step == 0 || !P.x0_next) ? P.x0 : P.x0_next;
                return is_state ? from[cell] : 0.0;
            };
            (void)true_cell; (void)true_x0;
            // PS: the score of the MPC step `at_step` whose plant step handed on `xn_row` (state lanes) under the applied u0 (slot 1 of the
            // input lanes): z = [xn | u0] across the row, the lane-local terms against the instance's setup block, the cost on ONE chain
            // that starts at the record's and takes the row's terms in ascending order, the violation by a row maximum (score_row_max); lane 0 of the
            // row reads and writes the record.  Called behind the iteration loop only, where a plant step was taken, and everything it
            // needs is formed there: the pointers come from the kernel-argument segment, nothing lives through the loop
            auto scored = [&](const double xn_row, const double u0_row, const int at_step) {
                int s_b = b;
                asm volatile("" : "+v"(s_b));
                const unsigned long long raw = reinterpret_cast<unsigned long long>(late_arg<const double>(__builtin_offsetof(SolveArgs, score_tab)));
                const double* st = reinterpret_cast<const double*>(raw & ~1ull) + ((raw & 1ull) ? (size_t)0 : (size_t)s_b * 64) + j;
                const double z = is_state ? xn_row : (is_input ? u0_row : 0.0);
                const ScoreTerm t = score_term(z, st[0], st[16], st[32], st[48]);
                ScoreRecord* const rec = late_arg<ScoreRecord>(__builtin_offsetof(SolveArgs, score_rec)) + s_b;
                double cost = j == 0 ? rec->cost : 0.0;
                score_chain<0, NZ>(cost, t.s);
                const double m = score_row_max(t.e);
                if (j == 0) {
                    rec->cost = cost;
                    if (m > 0.0) {
                        const double worst = rec->worst;
                        const int first = rec->first_violation;
                        rec->worst = fmax(worst, m);
                        rec->violated_steps += 1;
                        if (first < 0) rec->first_violation = late_value<int>(__builtin_offsetof(SolveArgs, score_step0)) + at_step;
                    }
                }
            };
            (void)scored;
            // PA: the control the plant receives at MPC step `at_step` for the command `u0_row` (slot 1 of the input lanes): on an input
            // lane the four stages against the instance's block, elsewhere u0_row as it is (the plant chain and the score read the input
            // lanes only).  Called behind the iteration loop only, ONCE per step that takes a plant step -- it moves the lag's record --
            // and everything it needs is formed there.  A form without PA: the command itself
            // PQ: stage 0, the transport delay -- on an input lane whose instance has d > 0 the oldest entry of its ring is what the stages
            // see, the command takes its cell and lane NX moves the head (every lane of the row has loaded the head by then: one load
            // instruction); d = 0: the command's own bits, nothing read or written.  s0_out: where a PX form with an estimator takes it from
            auto applied = [&](const double u0_row, const int at_step, double* const s0_out = nullptr) -> double {
                if constexpr (PA) {
                    int a_b = b;
                    asm volatile("" : "+v"(a_b));
                    const ActuatorLaunch* const act = late_arg<const ActuatorLaunch>(__builtin_offsetof(SolveArgs, act));
                    const unsigned long long raw = reinterpret_cast<unsigned long long>(act->tab);
                    const int k = late_value<int>(__builtin_offsetof(SolveArgs, act_step0)) + at_step;
                    double ua = u0_row;
                    if constexpr (PQ) {
                        if (is_input) {
                            const DelayLaunch* const dl = delay_launch_of(act);
                            const int d = dl->delay[a_b];
                            if (d > 0) {
                                const int h = dl->head[a_b];
                                double* const cell = dl->queue + (((size_t)a_b * dl->d_max + h) * NU + (j - NX));
                                ua = *cell;
                                *cell = u0_row;
                                // (the pop is safe by a data dependency: this store's value needs the load of h, which every lane of the
                                // row issued in the same instruction.  `compensated` reads the head again behind this store, on OTHER lanes of
                                // the wave: that relies on program order over may-alias pointers and on one wave's stores and loads going
                                // through the same L1 in order -- keep it a fresh load there, never a value read once and carried)
                                if (j == NX) dl->head[a_b] = (h + 1 < d) ? h + 1 : 0;
                            }
                        }
                        if (s0_out) *s0_out = ua;
                    }
                    // (the limits and the gain run on every lane of the row: a lane outside the inputs reads neutral entries, and nothing reads
                    // what it computes.  Only the lag's record, the noise and the log are per input lane)
                    if (raw & ~3ull) {
                        const double* const t = reinterpret_cast<const double*>(raw & ~3ull) + ((raw & 1ull) ? (size_t)0 : (size_t)a_b * 80) + j;
                        ua = actuator_limits(ua, t[0], t[16]);
                        if ((raw & 2ull) && is_input) {
                            double* const a = act->state + ((size_t)a_b * NU + (j - NX));
                            ua = actuator_lag(ua, *a, t[32]);
                            *a = ua;
                        }
                        ua = actuator_gain(ua, t[48], t[64]);
                    }
                    if (is_input) {
                        const size_t cell = (size_t)a_b * NU + (j - NX);
                        if (act->noise && (unsigned)k < (unsigned)act->noise_steps) ua = plant_add(ua, act->noise[(size_t)k * P.batch * NU + cell]);
                    }
                    return ua;
                } else {
                    return u0_row;
                }
            };
            (void)applied;
            // ... and its entry of the actuation log, stored on its own BEHIND the score: next to the other stages the store's address
            // costs the cone PE + PS form the register pair that keeps a loop-invariant conversion out of the iteration loop
            auto act_logged = [&](const double ua, const int at_step) {
                if constexpr (PA) {
                    int l_b = b;
                    asm volatile("" : "+v"(l_b));
                    const ActuatorLaunch* const act = late_arg<const ActuatorLaunch>(__builtin_offsetof(SolveArgs, act));
                    const int k = late_value<int>(__builtin_offsetof(SolveArgs, act_step0)) + at_step;
                    if (act->log && is_input) act->log[(size_t)(k - act->log_step0) * P.batch * NU + (size_t)l_b * NU + (j - NX)] = ua;
                }
            };
            (void)act_logged;
            const int iter_first = resumed ? P.iter_base : 0;  // (a multiple of check_termination: the countdown restarts in phase)
            for (int step = 0; step < nsteps; ++step) {        // closed-loop MPC steps fused in one launch
                X[0] = x0v;                                    // work->x.col(0) = x0
                if (has_traj) {                                // work->Xref = Xref_total.block(0, k, nx, N)
                    if (is_state) {
#pragma unroll
                        for (int s = 0; s < N; ++s) {
                            int kk = traj_k0 + step + s;
                            kk = kk < P.traj_points ? kk : P.traj_points - 1;
                            const double r = P.traj[(size_t)kk * NX + j];
                            QX[s] = -(r * qr);
                            if (s == N - 1) ref_last = r;
                        }
                    }
                    terminal_term();
                }
                if (P.reset_duals) {                           // work->y = 0; work->g = 0
#pragma unroll
                    for (int s = 0; s < N; ++s) G[s] = 0.0;
                }
                if constexpr (SOC) {
                    if (step > 0) {                            // vcnew = x, zcnew = u of the previous solve (admm.cpp:352-357)
#pragma unroll
                        for (int s = 0; s < N; ++s) {
                            const double vc0 = soc_lane ? X[s] : 0.0;
                            sC[cw + s * SLOT_D] = vc0 - sC[cw + s * SLOT_D + PL_GC];
                            sC[cw + s * SLOT_D + PL_VC] = vc0;
                        }
                    }
                }
                if constexpr (LS) {                            // vlnew = x, zlnew = u (admm.cpp:361-365)
                    if (step > 0) {
#pragma unroll
                        for (int s = 0; s < N; ++s) { if constexpr (LSP) sLV[cl + s * CSL] = lin_lane ? X[s] : 0.0; else VL[s] = lin_lane ? X[s] : 0.0; }
                    } else if (is_state && lin_lane && !resumed) { if constexpr (LSP) sLV[cl] = x0v; else VL[0] = x0v; }
                }
                if constexpr (LT) {                            // vlnew_tv = x, zlnew_tv = u (admm.cpp:370-374)
                    if (step > 0) {
#pragma unroll
                        for (int s = 0; s < N; ++s) { if constexpr (LTP) sTV[cl + s * CSL] = tlin_lane ? X[s] : 0.0; else VT[s] = tlin_lane ? X[s] : 0.0; }
                    } else if (is_state && tlin_lane && !resumed) { if constexpr (LTP) sTV[cl] = x0v; else VT[0] = x0v; }
                }
                if constexpr (LPL) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                const int iter0 = iter_first;
                iter = iter0; solved = 0;
                if (resumed && P.check_termination > 0) checked = 1;
                int countdown = P.check_termination;
                // SOC: vcnew - gc of slot i comes out of the W plane two sweep steps before its use (a ring of three registers); the
                // first two of a sweep are read at the end of the iteration before
                double wr[SOC ? SPR : 1];
                bool gcz[SOC_PASSES];                          // SOC: the GC cells of pass p's items are known to be zero (rows only LEAVE a solve)
#pragma unroll
                for (int p = 0; p < SOC_PASSES; ++p) gcz[p] = false;
                if constexpr (SOC) {
#pragma unroll
                    for (int d = 1; d <= SPR && d <= N; ++d) wr[(N - d) % SPR] = sC[cw + (N - d) * SLOT_D];
                }
                for (int it = iter0; it < P.max_iter; ++it) {
                    // LIN: vlnew and gl of slot i come out of their planes two sweep steps before their use (rings of three registers)
                    double lvr[LSP ? SPR : 1], lgr[LSP ? SPR : 1], tvr[LTP ? SPR : 1], tgr[LTP ? SPR : 1];
                    if constexpr (LPL) {
#pragma unroll
                        for (int d = 1; d <= SPR && d <= N; ++d) {
                            if constexpr (LSP) { lvr[(N - d) % SPR] = sLV[cl + (N - d) * CSL]; lgr[(N - d) % SPR] = sLG[cl + (N - d) * CSL]; }
                            if constexpr (LTP) { tvr[(N - d) % SPR] = sTV[cl + (N - d) * CSL]; tgr[(N - d) % SPR] = sTG[cl + (N - d) * CSL]; }
                        }
                    }
                    // vlnew - gl | vlnew_tv - gl_tv of slot s_: from the rings, or the register arrays of the per-knot variant
                    auto lin_w = [&](const int s_) { if constexpr (LSP) return lvr[s_ % SPR] - lgr[s_ % SPR]; else return VL[LSR ? s_ : 0] - GL[LSR ? s_ : 0]; };
                    auto tlin_w = [&](const int s_) { if constexpr (LTP) return tvr[s_ % SPR] - tgr[s_ % SPR]; else return VT[LTR ? s_ : 0] - GT[LTR ? s_ : 0]; };
                    // ---- update_linear_cost (lane-local) fused into the backward sweep.
                    // qv(s): state lanes q_s (s = N-1: the terminal p), input lanes r_{s-1}.
                    double qhi;
                    {
                        double t = fma(-rho, VN[N - 1] - G[N - 1], QX[N - 1]);      // admm.cpp:293 | :280
                        if constexpr (SOC) t = fma(-rho, wr[(N - 1) % SPR], t);     // :295 | :282
                        if constexpr (LS) t = fma(-rho, lin_w(N - 1), t);           // :298 | :285
                        if constexpr (LT) t = fma(-rho, tlin_w(N - 1), t);          // :301 | :288
                        qhi = t;
                        if constexpr (DBG) {
                            double ql = fma(-rho, VN[N - 1] - G[N - 1], qx_last_plain);   // q[:,N-1], :267
                            if constexpr (SOC) ql = fma(-rho, wr[(N - 1) % SPR], ql);       // :269
                            if constexpr (LS) ql = fma(-rho, lin_w(N - 1), ql);             // :272
                            if constexpr (LT) ql = fma(-rho, tlin_w(N - 1), ql);            // :275
                            Qd[N - 1] = is_state ? ql : t;
                            Pd[N - 1] = t;
                        }
                    }
                    double pcur = qhi;                         // p_{N-1} on state lanes
                    // ---- backward_pass_grad, admm.cpp:13-20
                    if constexpr (HALF) {                       // (the wait states of the half-row chains carry the neighbouring steps' lane-local work)
                        double tmpv = VN[N - 2] - G[N - 2];
#pragma unroll
                        for (int i = N - 2; i >= 0; --i) {
                            double qlo, res, dnp, tmpn;
                            constexpr int dummy = 0;
                            const int in = i > 0 ? i - 1 : dummy;
                            fused_backward_step_half<NX, NU>(qlo, res, dnp, tmpn, tmpv, VN[in], G[in], QX[i], rho, smask, cb, nim, cf, pcur, qhi, mb, mb + NX);
                            if (i + 1 <= N - 2) Dn[i + 1] = dnp;                        // fma(p_{i+1} | d_{i+1}, nim, cf)
                            tmpv = tmpn;
                            pcur = res;                                                 // p_i | d_i
                            qhi = qlo;
                        }
                        Dn[0] = fma(pcur, nim, cf);
                    }
#pragma unroll
                    for (int i = N - 2; i >= 0 && !HALF; --i) {
                        if constexpr (SOC) {
                            if (i >= SPD) wr[(i - SPD) % SPR] = sC[cw + (i - SPD) * SLOT_D];      // (slot i + 1's register is free by now)
                        }
                        if constexpr (LSP) { if (i >= SPD) { lvr[(i - SPD) % SPR] = sLV[cl + (i - SPD) * CSL]; lgr[(i - SPD) % SPR] = sLG[cl + (i - SPD) * CSL]; } }
                        if constexpr (LTP) { if (i >= SPD) { tvr[(i - SPD) % SPR] = sTV[cl + (i - SPD) * CSL]; tgr[(i - SPD) % SPR] = sTG[cl + (i - SPD) * CSL]; } }
                        if constexpr (SOC || LPL) __builtin_amdgcn_sched_barrier(0);
                        if constexpr (FUSED) {                  // linear-cost terms + both mat-vec chains in one asm statement (no s_nop)
                            double qlo, res;
                            if constexpr (SOC) fused_backward_step_soc<NX, NU>(qlo, res, VN[i], G[i], QX[i], wr[i % SPR], rho, smask, cb, pcur, qhi, mb, mb + NX);
                            else fused_backward_step<NX, NU>(qlo, res, VN[i], G[i], QX[i], rho, smask, cb, pcur, qhi, mb, mb + NX);
                            pcur = res;                                                 // p_i | d_i
                            Dn[i] = fma(res, nim, cf);
                            if constexpr (DBG) { Qd[i] = qlo; Pd[i] = res; Dd[i + 1] = res; }
                            qhi = qlo;
                            continue;
                        }
                        double qlo = fma(-rho, VN[i] - G[i], QX[i]);                // :267 | :280
                        if constexpr (SOC) qlo = fma(-rho, wr[i % SPR], qlo);       // :269 | :282
                        if constexpr (LS) qlo = fma(-rho, lin_w(i), qlo);           // :272 | :285
                        if constexpr (LT) qlo = fma(-rho, tlin_w(i), qlo);          // :275 | :288
                        // state lanes: q_i + APf + AmBKt p_{i+1} - Kinf' r_i ; input lanes: Quu_inv (B' p_{i+1} + r_i + BPf)
                        const double res = ring_sum2<MODE, NX, NU>(fma(qlo, smask, cb), pcur, mb, qhi, mb + NX);
                        pcur = res;                                                 // p_i | d_i
                        Dn[i] = fma(res, nim, cf);                                  // input lanes: -d_i; state lanes: fdyn (the forward step's constant)
                        if constexpr (DBG) { Qd[i] = qlo; Pd[i] = res; Dd[i + 1] = res; }
                        qhi = qlo;
                    }
                    // ---- forward_pass (admm.cpp:25-32) with update_slack + update_dual + the residual maxima
                    // (admm.cpp:81-135, 219-235, 314-317) of slot i+1 issued right behind the step that produced it:
                    // the lane-local element-wise work (and its LDS bound reads) fills the dependency stalls of
                    // the next step's FMA chain instead of forming a separate, latency-exposed phase.
                    // The 2N subtractions and maxima behind the residuals: short horizons form them inside the termination test, from the
                    // registers, only when the probe lets the test run (said here, not left to the compiler's sinking); long ones keep
                    // the running maxima of the forward sweep
                    constexpr bool LAZY_RES = N <= 12;
                    // the short box loop with nx a multiple of 4 (the quadrotor's): the forward step's B u chain runs in place, g of a
                    // forward step is formed one step late -- where it takes the place of the s_nop hipcc puts between two asm statements
                    // -- and the last slot's clamp is one asm statement.  Elsewhere (long horizons, whose g and x live partly in AGPRs;
                    // the cone variant; the copy form) these cost more wait states and copies than they save: the form of before
                    constexpr bool TIGHT = FUSED && !HALF && LAZY_RES && !SOC && NX % 4 == 0;
                    double pmax = 0.0, dmax = 0.0;
                    auto slot_update = [&](const int s, const double lo, const double hi, const double gcv, const double glv, const double gtv) {
                        const double xi = X[s];
                        const double t = xi + G[s];                                 // :85 / :88
                        const double vn = TIGHT ? vclamp64(lo, hi, t) : vmin64(hi, vmax64(lo, t));   // :91-98
                        if constexpr (!LAZY_RES) {
                            pmax = resid_max<true>(pmax, xi - vn);
                            dmax = resid_max<true>(dmax, VP[s] - vn);
                        }
                        G[s] = t - vn;                      // :222 / :225  g + x - vnew; (g + x) == t bit-for-bit
                        VN[s] = vn;
                        if constexpr (SOC) {
                            // vcnew = x + gc on every row of a family whose cone slack is on (:102-109); gc is 0 on the
                            // other rows, so one FMA against the 0/1 mask does the add and the select.  Projected after the
                            // sweep, one lane per (cone, knot): the cone step below; a cell outside every item keeps this
                            // value as its vcnew, so its gc = (x + gc) - vcnew = 0 (written once per solve, behind the cone step)
                            sC[cw + s * SLOT_D] = fma(xi, socmask, gcv);
                        }
                        // half-space slacks: vlnew = x + gl on the rows of a family whose slack is on (:139 / :144 / :177 / :182), projected
                        // after the sweep, one lane per (knot, family) column (project_halfspace_columns)
                        if constexpr (LSP) sLV[cl + s * CSL] = (lin_lane && (is_state || s >= 1)) ? (xi + glv) : 0.0;
                        if constexpr (LTP) sTV[cl + s * CSL] = (tlin_lane && (is_state || s >= 1)) ? (xi + gtv) : 0.0;
                        if constexpr (LSR || LTR) {
                            // the per-knot form: a'z is a lane-local product summed over the row with the broadcast-FMA chain (against a vector of
                            // ones), separately for the state and the input rows; constraints are applied sequentially, only when violated (:154)
                            auto halfspaces = [&](double z, const double* tabk, const int nk) {
                                for (int k = 0; k < nk; ++k) {
                                    const double a = tabk[k * 16 + j];
                                    const double bk = tabk[KMAX * 16 + k * 16 + j];
                                    const double nn = tabk[2 * KMAX * 16 + k * 16 + j];
                                    const double prod = a * z;
                                    double cs = 0.0, ci = 0.0;
                                    ring1<0, NX>(cs, prod, ones);
                                    ring1<NX, NU>(ci, prod, ones);
                                    const double cv = is_state ? cs : ci;
                                    if (cv > bk) {
#pragma clang fp contract(off)
                                        const double pr = ((cv - bk) / nn) * a;         // the product rounded, as in project_halfspace_columns
                                        z = z - pr;
                                    }
                                }
                                return z;
                            };
                            if constexpr (LSR) {
                                const bool on = lin_lane && (is_state || s >= 1);
                                double vl = on ? (xi + GL[s]) : 0.0;                    // :139 / :144
                                vl = halfspaces(vl, rLin, P.n_lin);
                                GL[s] = on ? ((GL[s] + xi) - vl) : 0.0;                 // :239 / :244
                                VL[s] = on ? vl : 0.0;
                            }
                            if constexpr (LTR) {
                                const bool on = tlin_lane && (is_state || s >= 1);
                                double vt = on ? (xi + GT[s]) : 0.0;                    // :177 / :182
                                vt = halfspaces(vt, rTLin + s * 3 * KMAX * 16, P.n_tlin);
                                GT[s] = on ? ((GT[s] + xi) - vt) : 0.0;                 // :249 / :254
                                VT[s] = on ? vt : 0.0;
                            }
                        }
                    };
                    // Software pipeline: the box bounds of slot i+1 are read from LDS one whole step before
                    // they are used (sched_barrier pins the reads above the step), and slot i's update is
                    // scheduled together with the FMA chain of step i -- both only need x_i.
                    double lo_c = UB ? rlo_u0 : sLo[sbox + j], hi_c = UB ? rhi_u0 : sHi[sbox + j];
                    double gr[SOC ? SPR : 1];                   // SOC: gc of slot i, read from its plane SPD steps ahead
                    if constexpr (SOC) {
#pragma unroll
                        for (int d = 0; d < SPD && d < N; ++d) gr[d % SPR] = sC[cw + d * SLOT_D + PL_GC];
                    } else gr[0] = 0.0;
                    double glr[LSP ? SPR : 1], gtr[LTP ? SPR : 1];   // LIN: gl | gl_tv of slot i, likewise
                    glr[0] = 0.0; gtr[0] = 0.0;
                    if constexpr (LPL) {
#pragma unroll
                        for (int d = 0; d < SPD && d < N; ++d) {
                            if constexpr (LSP) glr[d % SPR] = sLG[cl + d * CSL];
                            if constexpr (LTP) gtr[d % SPR] = sTG[cl + d * CSL];
                        }
                    }
                    double tt_d = 0.0, vn_d = 0.0;              // TIGHT: x + g and vnew of the step before (its g is formed one step late)
#pragma unroll
                    for (int i = 0; i < N - 1; ++i) {
                        const double lo_n = UB ? rlo_u : sLo[sbox + (i + 1) * 16 + j], hi_n = UB ? rhi_u : sHi[sbox + (i + 1) * 16 + j];
                        if constexpr (SOC) { if (i + SPD < N) gr[(i + SPD) % SPR] = sC[cw + (i + SPD) * SLOT_D + PL_GC]; }
                        if constexpr (LSP) { if (i + SPD < N) glr[(i + SPD) % SPR] = sLG[cl + (i + SPD) * CSL]; }
                        if constexpr (LTP) { if (i + SPD < N) gtr[(i + SPD) % SPR] = sTG[cl + (i + SPD) * CSL]; }
                        __builtin_amdgcn_sched_barrier(0);
                        if constexpr (FUSED) {                  // first half of slot i's update in front of the chains (no s_nop)
                            double tt, vn, xn, t = Dn[i];
                            const double xi = X[i];
                            if constexpr (HALF) {
                                double gnew;
                                fused_forward_step_half<NX, NU>(tt, vn, t, xn, gnew, xi, G[i], lo_c, hi_c, mf1, mf2);
                                X[i + 1] = xn;
                                if constexpr (!LAZY_RES) {
                                    pmax = resid_max<true>(pmax, xi - vn);
                                    dmax = resid_max<true>(dmax, VP[i] - vn);
                                }
                                G[i] = gnew;
                                VN[i] = vn;
                                lo_c = lo_n; hi_c = hi_n;
                                continue;
                            }
                            fused_forward_step<NX, NU, TIGHT>(tt, vn, t, xn, xi, G[i], lo_c, hi_c, mf1, mf2);
                            X[i + 1] = xn;
                            if constexpr (!LAZY_RES) {
                                pmax = resid_max<true>(pmax, xi - vn);
                                dmax = resid_max<true>(dmax, VP[i] - vn);
                            }
                            if constexpr (TIGHT) {
                                // g <- (x + g) - vnew of the step BEFORE, pinned between this step's chains and the next step's: an
                                // instruction there that reads none of this step's outputs spares hipcc's s_nop between the two asm
                                // statements, and is the first of the two wait states the next chain's broadcast of x_{i+1} needs
                                __builtin_amdgcn_sched_barrier(0);
                                if (i > 0) G[i - 1] = pinned_sub64(tt_d, vn_d);
                                tt_d = tt; vn_d = vn;
                            } else G[i] = tt - vn;
                            VN[i] = vn;
                            if constexpr (SOC) sC[cw + i * SLOT_D] = fma(xi, socmask, gr[i % SPR]);   // x + gc -> cone step (below); see slot_update
                            lo_c = lo_n; hi_c = hi_n;
                            continue;
                        }
                        const double t = ring_sum<MODE, 0, NX>(Dn[i], X[i], mf1);   // f + A x_i | u_i = -d_i - Kinf x_i
                        X[i + 1] = ring_short<MODE, NX, NU>(t, t, mf2);             // x_{i+1} = (f + A x_i) + B u_i | u_i (slot i+1)
                        slot_update(i, lo_c, hi_c, gr[SOC ? i % SPR : 0], glr[LSP ? i % SPR : 0], gtr[LTP ? i % SPR : 0]);
                        lo_c = lo_n; hi_c = hi_n;
                    }
                    if constexpr (TIGHT && N >= 2) G[N - 2] = tt_d - vn_d;
                    (void)tt_d; (void)vn_d;
                    slot_update(N - 1, lo_c, hi_c, gr[SOC ? (N - 1) % SPR : 0], glr[LSP ? (N - 1) % SPR : 0], gtr[LTP ? (N - 1) % SPR : 0]);
                    if constexpr (LPL) {
                        // ---- half-space projections (admm.cpp:137-211) + their dual update (:239-254), transposed
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        if constexpr (LSP) {
                            if (lin_x_on) project_halfspace_columns<NX, KMAX, 16, 16>(j, grp, N, CSL, 0, 0, sLV, sLG, rLin, 0, P.n_lin);
                            if (lin_u_on) project_halfspace_columns<NU, KMAX, 16, 16>(j, grp, N, CSL, NX, 1, sLV, sLG, rLin, 0, P.n_lin);
                        }
                        if constexpr (LTP) {
                            if (tlin_x_on) project_halfspace_columns<NX, KMAX, 16, 16>(j, grp, N, CSL, 0, 0, sTV, sTG, rTLin, 3 * KMAX * 16, P.n_tlin);
                            if (tlin_u_on) project_halfspace_columns<NU, KMAX, 16, 16>(j, grp, N, CSL, NX, 1, sTV, sTG, rTLin, 3 * KMAX * 16, P.n_tlin);
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                    }
                    // ---- termination_condition, admm.cpp:310-328 (the box residuals: the cone slacks do not enter them)
                    bool conv = false;
                    // The 2N subtractions and maxima behind the four residuals (a tenth of the quadrotor iteration) are only formed when the
                    // test can pass: a row converges only if EVERY entry of its residuals is below the tolerance, so two probe slots decide
                    // first -- slot 1 (x_1 | u_0: where the constraints bite) and the last one.  An entry there at or above its tolerance and
                    // the test is lost whatever the other slots hold (max >= that entry; `x rho` is monotone for rho > 0; a NaN entry is
                    // ignored by the maxima, so it does not count against the probe either).  The probe is skipped -- the full test runs --
                    // on the last test of the launch's iteration budget: the residuals it leaves are the ones the solve reports (:314-317).
                    auto termination = [&]() {
                        if (countdown > 0 && --countdown == 0) {
                            countdown = P.check_termination;
                            checked = 1;
                            constexpr int PS0 = N >= 2 ? 1 : 0, PS1 = N - 1;
                            auto lost = [&](const int s) {              // (`|`, not `||`: four compares and three s_or, no EXEC-mask regions)
                                return (int)(fabs(X[s] - VN[s]) >= P.tol_pri) | (int)(fabs(VP[s] - VN[s]) * rho >= P.tol_dua);
                            };
                            const bool maybe = ((int)!(rho > 0.0) | (int)!(lost(PS0) | lost(PS1))) != 0;
                            // any row all of whose lanes say maybe?  (scalar: AND-fold the ballot over each row's RL bits; rows that have
                            // left the loop are masked off and vote 0)
                            unsigned long long fold = __ballot(maybe);
                            fold &= fold >> 1; fold &= fold >> 2; fold &= fold >> 4;
                            if constexpr (!HALF) fold &= fold >> 8;
                            const bool any_row = (fold & (HALF ? 0x0101010101010101ull : 0x0001000100010001ull)) != 0ull;
                            // INVARIANT: rp / rd -- what d_resid reports and what repack_sort keys on -- are refreshed only by a
                            // FULL test: a row passed the probe, or this is the last test the launch's iteration budget allows.  Every launch
                            // and every stage of a split solve therefore ends on a full test BECAUSE its end is P.max_iter (the stage's cap);
                            // a caller that stopped a launch any other way would read residuals of an earlier iteration.
                            const bool last_test = (P.max_iter - 1 - it) < P.check_termination;
                            if (last_test || any_row) {
                                if constexpr (LAZY_RES) {
#pragma unroll
                                    for (int s = 0; s < N; ++s) {
                                        pmax = resid_max<false>(pmax, X[s] - VN[s]);
                                        dmax = resid_max<false>(dmax, VP[s] - VN[s]);
                                    }
                                }
                                rp = pmax;
                                rd = dmax * rho;
                                const bool ok = (rp < P.tol_pri) && (rd < P.tol_dua);
                                const unsigned long long bal = __ballot(ok);
                                conv = ((bal >> (grp * RL)) & RMASK) == RMASK;
                            }
                        }
                    };
                    if constexpr (SOC) {
                        // ---- cone step (admm.cpp:112-135, 228-235), transposed: x + gc of every slot went to LDS above; lane j
                        // of pass p gathers the three components of its (cone, knot) item, projects them -- ONE square root /
                        // division sequence per pass instead of one per knot -- and writes the item's cells of the three planes.
                        // The termination test needs nothing from it and stands between the first gather and its use.
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        double n0 = sC[item_at[0]], n1 = sC[item_at[0] + 1], n2 = sC[item_at[0] + 2];
                        // the next backward sweep's first terms: on their way together with the gather.  They stay valid unless a pass
                        // below takes its exact path and rewrites W cells (then they are read again)
#pragma unroll
                        for (int d = 1; d <= SPR && d <= N; ++d) wr[(N - d) % SPR] = sC[cw + (N - d) * SLOT_D];
                        termination();
                        bool any_exact = false;
#pragma unroll
                        for (int p = 0; p < SOC_PASSES; ++p) {
                            if (p > 0 && p >= soc_passes) break;            // wave-uniform
                            const int at = item_at[p];
                            if (p > 0) { n0 = sC[at]; n1 = sC[at + 1]; n2 = sC[at + 2]; }
                            const double s0 = n0, s1 = n1, s2 = n2;
                            if (soc_all_inside(s0, s1, s2, item_mu[p])) {
                                // no cone of the wave is active: vcnew = x + gc bit for bit, so gc = (x + gc) - vcnew = 0 and
                                // vcnew - gc = x + gc -- what the forward sweep left in the W plane.  VC takes its copy (for the
                                // write-back); the GC cells are zeroed once, then known to be zero (gcz: of the rows still iterating)
                                sC[at + PL_VC] = s0; sC[at + PL_VC + 1] = s1; sC[at + PL_VC + 2] = s2;
                                if (!gcz[p]) {
                                    sC[at + PL_GC] = 0.0; sC[at + PL_GC + 1] = 0.0; sC[at + PL_GC + 2] = 0.0;
                                    gcz[p] = true;
                                }
                            } else {
                                double r0, r1, r2;
                                soc_project3(s0, s1, s2, item_mu[p], item_rmu[p], mu_pow2, r0, r1, r2);
                                // the item's three cells of every plane (the dummy item: (0, 0, 1) onto itself, from every lane that has none)
                                const double g0 = s0 - r0, g1 = s1 - r1, g2 = s2 - r2;      // :229 / :234  (gc + x) - vcnew
                                sC[at + PL_VC] = r0; sC[at + PL_VC + 1] = r1; sC[at + PL_VC + 2] = r2;
                                sC[at + PL_GC] = g0; sC[at + PL_GC + 1] = g1; sC[at + PL_GC + 2] = g2;
                                sC[at] = r0 - g0; sC[at + 1] = r1 - g1; sC[at + 2] = r2 - g2;   // vcnew - gc: the next backward sweep's term
                                gcz[p] = false;
                                any_exact = true;
                            }
                        }
                        // a cell outside every item: gc = (x + gc) - vcnew = 0 from the solve's first iteration on (whatever the warm start
                        // held there); once per solve, wave-uniform (the rows of a wave open their solves together)
                        if (it == iter0 && !proj_lane) {
#pragma unroll
                            for (int s = 0; s < N; ++s) sC[cw + s * SLOT_D + PL_GC] = 0.0;
                        }
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        if (any_exact) {
#pragma unroll
                            for (int d = 1; d <= SPR && d <= N; ++d) wr[(N - d) % SPR] = sC[cw + (N - d) * SLOT_D];
                        }
                    }
                    iter += 1;                                                      // :394
                    if constexpr (ADAPT) {
                        // ---- adaptive rho, admm.cpp:397-423: every 5th pass of the loop index (after iterations 6, 11, ...).
                        // benchmark_rho_adaptation (rho_benchmark.cpp:207-249) builds dense OSQP-style matrices and multiplies
                        // them out; every entry it multiplies by zero is skipped here, what is left is evaluated block by block:
                        //   rows of A x - z:  u_i - znew_i  and  (A x_i + B u_i - x_{i+1}) - vnew_{i+1}          (:78-102, :144-150)
                        //   P x + q + A' y:   (Q x_i | Pinf x_{N-1}) + Q x_i + (A' g_{i+1} - g_i),  R u_i + R u_i + (y_i + B' g_{i+1})   (:107-168)
                        if (it > 0 && it % 5 == 0) {
                            double at[NX];
#pragma unroll
                            for (int k = 0; k < NX; ++k) at[k] = HA ? atab_i[ATAB_AT + k * 16 + j] : sTab[j * AKC + k];
                            double pri_res = 0.0, ax_max = 0.0, z_max = 0.0, dual_res = 0.0, px_max = 0.0, aty_max = 0.0, q_max = 0.0;
                            double pxq_max = 0.0;              // max |Q x_i|, |R u_i| over the knots before the last: entries of P x AND of q
#pragma unroll
                            for (int i = 0; i < N - 1; ++i) {
                                // primal rows of knot i live in slot i+1: input lanes u_i, state lanes the dynamics defect
                                const double axs = ring_sum<MODE, 0, NX>(0.0, X[i], mf1);            // state lanes: A x_i
                                const double dyn = ring_short<MODE, NX, NU>(axs, is_input ? X[i + 1] : 0.0, mf2) - X[i + 1];
                                const double a = is_state ? dyn : X[i + 1];
                                const double zz = VN[i + 1];
                                const bool on = is_state || is_input;
                                pri_res = fmax(pri_res, on ? fabs(a - zz) : 0.0);
                                ax_max = fmax(ax_max, on ? fabs(a) : 0.0);
                                z_max = fmax(z_max, on ? fabs(zz) : 0.0);
                                // dual rows: state lanes knot i, input lanes knot i (slot i+1); A' g_{i+1} | B' g_{i+1} from one chain
                                const double init = is_state ? (i >= 1 ? -G[i] : 0.0) : G[i + 1];
                                const double aty = ring_sum<MODE, 0, NX>(init, G[i + 1], at);
                                const double xs = is_state ? X[i] : X[i + 1];
                                const double px = qr * xs;                                          // P block = Q | R (:114, :119)
                                dual_res = fmax(dual_res, on ? fabs((px + px) + aty) : 0.0);       // q = Q x | R u (:132, :137)
                                pxq_max = fmax(pxq_max, on ? fabs(px) : 0.0);
                                aty_max = fmax(aty_max, on ? fabs(aty) : 0.0);
                            }
                            {   // last knot (state lanes): P block = the CURRENT Pinf (:112), A' y = -g_{N-1}
                                double prow[NX];
#pragma unroll
                                for (int k = 0; k < NX; ++k) prow[k] = sP[grp * NX * NX + (is_state ? j : 0) + NX * k];   // Pinf[j][k]
                                const double pxl = ring_sum<MODE, 0, NX>(0.0, X[N - 1], prow);
                                const double ql = qr * X[N - 1];
                                const double atyl = -G[N - 1];
                                dual_res = fmax(dual_res, is_state ? fabs((pxl + ql) + atyl) : 0.0);
                                px_max = fmax(pxq_max, is_state ? fabs(pxl) : 0.0);
                                aty_max = fmax(aty_max, is_state ? fabs(atyl) : 0.0);
                                q_max = fmax(pxq_max, is_state ? fabs(ql) : 0.0);                  // q uses Q at the last knot too (:132)
                            }
                            pri_res = grp_max16(pri_res); ax_max = grp_max16(ax_max); z_max = grp_max16(z_max);
                            dual_res = grp_max16(dual_res); px_max = grp_max16(px_max); aty_max = grp_max16(aty_max); q_max = grp_max16(q_max);
                            // predict_rho, rho_benchmark.cpp:174-194
                            const double pri_norm = fmax(ax_max, z_max);
                            const double dual_norm = fmax(fmax(px_max, aty_max), q_max);
                            const double eps = 1e-10;
                            const double normalized_pri = pri_res / (pri_norm + eps);
                            const double normalized_dual = dual_res / (dual_norm + eps);
                            const double ratio = normalized_pri / (normalized_dual + eps);
                            double new_rho = rho * sqrt(ratio);
                            if (P.aclip) new_rho = fmin(fmax(new_rho, P.arho_min), P.arho_max);
                            // update_matrices_with_derivatives, rho_benchmark.cpp:196-210 (the second call at admm.cpp:421 adds 0)
                            const double delta = new_rho - rho;
                            if (is_state) {
#pragma unroll
                                for (int k = 0; k < NU; ++k) mb[NX + k] = -taylor_step(-mb[NX + k], delta, (HA ? atab_i[ATAB_DK + k * 16 + j] : sTab[(16 + j) * AKC + k]));
#pragma unroll
                                for (int k = 0; k < NX; ++k) {
                                    const int e = grp * NX * NX + k + NX * j;
                                    sP[e] = taylor_step(sP[e], delta, (HA ? atab_i[ATAB_DP + k * 16 + j] : sTab[(32 + j) * AKC + k]));
                                }
                            } else if (is_input) {
#pragma unroll
                                for (int k = 0; k < NX; ++k) mf1[k] = -taylor_step(-mf1[k], delta, (HA ? atab_i[ATAB_DK + k * 16 + j] : sTab[(16 + j) * AKC + k]));
                            }
                            if (P.aC1 || P.aC2) {                                           // C1 / C2: logged, applied by flush_c
                                if (j == 0) sDl[grp * ADAPT_LOG + ndl] = delta;
                                if (++ndl == ADAPT_LOG) { flush_c(ndl); ndl = 0; }
                            }
                            rho = new_rho;
                            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                            __builtin_amdgcn_wave_barrier();
                            // p[:,N-1] = -(Xref[:,N-1]' Pinf) - ... is evaluated with the Pinf of the moment (admm.cpp:292)
                            QX[N - 1] = qx_last_plain;
                            terminal_term();
                        }
                    }
                    if constexpr (!SOC) termination();                             // (after the adaptation: it may have moved rho)
                    if (conv) { solved = 1; break; }                                // :431-441 (returns before v = vnew)
#pragma unroll
                    for (int s = 0; s < N; ++s) VP[s] = VN[s];                      // :445-446
                    vp_touched = true;
                }
                acc_iter += (unsigned)(iter - iter0);
                acc_solved += (unsigned)solved;
                // (the logs of a single-step launch: a stretch of a fused launch that batch_dispatch.hip cut up, "step_regroup")
                if (P.iter_log && j == 0) P.iter_log[(size_t)step * P.batch + b] = solved ? iter : -iter;
                if (P.u0_log && is_input) P.u0_log[((size_t)step * P.batch + b) * NU + (j - NX)] = X[1];
                if constexpr (PE) {                            // (the xhat this step solved from: the state lanes still hold it in slot 0)
                    double* const elog = late_arg<double>(__builtin_offsetof(SolveArgs, est_log));
                    if constexpr (PX) { if (elog && is_state) elog[((size_t)step * P.batch + b) * NX + j] = *xhat_cell(); } else      // (slot 0 holds the predicted state)
                    if (elog && is_state) elog[((size_t)step * P.batch + b) * NX + j] = X[0];
                }
                if (nsteps > 1) {
                    // plant step x0 <- A x0 + B u_0 + f (== forward_pass x_1).  Input lanes hold u_0 in slot 1: their
                    // slot 0 is the neutral dummy and must stay 0, or its "slack" would enter the dual residual
                    x0v = is_state ? X[1] : 0.0;
                    if constexpr (PM) {                        // (X[0] is the measurement: the plant starts from the true state, and the next step is handed ITS measurement)
                        if (step + 1 < nsteps) {
                            const size_t cell = true_cell();
                            double xt = true_x0(step, cell);
                            [[maybe_unused]] double est_next = 0.0;             // PE: the xp the next step corrects -- predicted here, or (no iteration ran) the record's
                            if constexpr (PE && !PX) est_next = (iter > iter0) ? predicted(X[0], X[1]) : (is_state ? late_arg<double>(__builtin_offsetof(SolveArgs, est_xp))[cell] : 0.0);
                            double ua = X[1];                                   // (PA: what the plant receives; else the command)
                            if constexpr (PE && PX) {                           // (the model predicts from xhat with what reaches the actuator NOW: what left the queue)
                                double s0 = X[1];
                                if (iter > iter0) {
                                    ua = applied(X[1], step, &s0);
                                    est_next = predicted(is_state ? *xhat_cell() : 0.0, s0);
                                    const double xp = plant_step(xt, ua);
                                    xt = is_state ? xp : 0.0;
                                    if constexpr (PD) xt = disturbed(xt, step);
                                } else {
                                    est_next = is_state ? late_arg<double>(__builtin_offsetof(SolveArgs, est_xp))[cell] : 0.0;
                                }
                            } else
                            if (iter > iter0) {
                                ua = applied(X[1], step);
                                const double xp = plant_step(xt, ua);
                                xt = is_state ? xp : 0.0;
                                if constexpr (PD) xt = disturbed(xt, step);
                            }
                            if (P.x0_next && is_state) P.x0_next[cell] = xt;      // (where true_x0 finds it; a step without a plant step: unchanged)
                            if constexpr (PS) { if (iter > iter0) scored(xt, ua, step); }
                            if constexpr (PA) { if (iter > iter0) act_logged(ua, step); }
                            if (P.state_log && is_state) P.state_log[((size_t)step * P.batch + b) * NX + j] = xt;
                            x0v = measured(xt, step + 1);
                            if constexpr (PE) x0v = corrected(x0v, est_next);
                            if constexpr (PX) {                                 // (the queue as this step's push left it: before the next step's)
                                if constexpr (PE) { if (is_state) *xhat_cell() = x0v; }
                                x0v = compensated(x0v);
                            }
                        }
                    } else {
                    [[maybe_unused]] double ua = X[1];         // (PA: what the plant receives)
                    if constexpr (PA) {                        // (a PP form: the chain over the applied control)
                        if (step + 1 < nsteps && iter > iter0) { ua = applied(X[1], step); const double xp = plant_step(X[0], ua); x0v = is_state ? xp : 0.0; }
                    } else
                    if constexpr (PP) {                        // (likewise; the chain runs on every lane of the row, the input lanes' rows are zero)
                        if (step + 1 < nsteps && iter > iter0) { const double xp = plant_step(X[0], X[1]); x0v = is_state ? xp : 0.0; }
                    }
                    if constexpr (PD) {                        // (a step that ran no iteration -- max_iter = 0 -- took no plant step; the last step's is the x0_next store)
                        if (step + 1 < nsteps && iter > iter0) x0v = disturbed(x0v, step);
                    }
                    if constexpr (PD || PP) {
                        if (P.state_log && step + 1 < nsteps && is_state) P.state_log[((size_t)step * P.batch + b) * NX + j] = x0v;
                    }
                    if constexpr (PS) {                        // (the score of a step that took its plant step: what it handed on, under the u0 it applied)
                        if (step + 1 < nsteps && iter > iter0) scored(x0v, PA ? ua : X[1], step);
                    }
                    if constexpr (PA) {
                        if (step + 1 < nsteps && iter > iter0) act_logged(ua, step);
                    }
                    }
                }
            }

            // ---- write back (coalesced) -------------------------------------------------------
            // FLS: every store instruction writes WHOLE knot segments [x_s ; u_s] (128 bytes = one cache line at nx+nu = 16).  The slot
            // convention -- input lanes hold knot s-1 at slot s -- otherwise makes a store write 96 bytes of one line and 32 of the line
            // before it: partial-line stores, and HBM takes those at three quarters of the rate of whole lines (tools/ubench/
            // ubench_stream_forms.hip -DSLOT_MAJOR=1 -DSPLIT_LINES=1: the copy pattern of a warm solve 5.7 -> 4.4 TB/s, and the
            // PREFETCH form turns from 20 % faster than one tile per wave into 7 % slower).  So the input lanes store the value of their
            // NEXT slot into the segment of the state lanes' slot; the input cells of the last knot (no u_{N-1}: never read, zero since
            // the records were allocated) are written as zero.  Same values at the same addresses: bit-identical records.
            constexpr bool FLS = TINYMPC_FULL_LINE_STORES != 0 && (PF || TINYMPC_FULL_LINE_STORES == 2) && !SOC && LIN == 0 && !DBG;
            if (FLS && (P.store_mask & 32) == 0) {
                if constexpr (FLS) {
                    const size_t seg = (size_t)b * (N * NZ) + j;
                    const bool in_row = j < NZ;
#pragma unroll
                    for (int s = 0; s < N; ++s) {
                        const size_t off = seg + s * NZ;
                        const double xs = is_input ? (s + 1 < N ? X[s + 1 < N ? s + 1 : s] : 0.0) : X[s];
                        const double vs = is_input ? (s + 1 < N ? VN[s + 1 < N ? s + 1 : s] : 0.0) : VN[s];
                        const double gs = is_input ? (s + 1 < N ? G[s + 1 < N ? s + 1 : s] : 0.0) : G[s];
                        const double ps = is_input ? (s + 1 < N ? VP[s + 1 < N ? s + 1 : s] : 0.0) : VP[s];
                        if (in_row) {
                            if (P.store_mask & 1) {
                                // max_iter = 0: the sweeps never ran, x[:,1:] and u keep what they held (only x[:,0] = x0 is set)
                                if (acc_iter > 0) { if constexpr (PF) P.prim[off] = xs; else store_primal(P.prim + off, xs); }
                                else if (s == 0 && is_state) P.prim[off] = xs;
                            }
                            if (P.store_mask & 2) P.slack[off] = vs;
                            if (P.store_mask & 4) P.dual[off] = gs;
                            if ((P.store_mask & 8) && vp_touched) P.slack_prev[off] = ps;   // admm.cpp:431-441 returns before v = vnew
                        }
                    }
                }
            } else
#pragma unroll
            for (int s = 0; s < N; ++s) {
                const bool valid = is_state || (is_input && s >= 1);
                const size_t off = lbase + s * NZ;
                if (valid) {
                    // max_iter = 0: the sweeps never ran, x[:,1:] and u keep what they held (only x[:,0] = x0 is set)
                    // bit 0: the whole x|u trajectory; bit 5: only its first knot (x_0, x_1, u_0: what a closed-loop caller applies)
                    if (((P.store_mask & 1) || ((P.store_mask & 32) && s <= 1)) && (acc_iter > 0 || (s == 0 && is_state))) {
                        // (a cone / half-space variant reads x|u back at the start of the next solve, admm.cpp:352-374: plain store)
                        if constexpr (SOC || LIN != 0) P.prim[off] = X[s];
                        else store_primal(P.prim + off, X[s]);
                    }
                    if (P.store_mask & 2) P.slack[off] = VN[s];
                    if (P.store_mask & 4) P.dual[off] = G[s];
                    if ((P.store_mask & 8) && vp_touched) P.slack_prev[off] = VP[s];   // admm.cpp:431-441 returns before v = vnew
                    if constexpr (SOC) {
                        // a family whose cone switch is off keeps its records (admm.cpp:102-109, 228-235).  vcnew: the VC plane where the
                        // cell belongs to an item (or no iteration ran: what the solve started from), else what the last forward sweep
                        // left in the W plane
                        if (soc_lane && (P.store_mask & 16)) {
                            P.cslack[off] = sC[cw + s * SLOT_D + ((proj_lane || iter <= iter_first) ? PL_VC : 0)];
                            P.cdual[off] = sC[cw + s * SLOT_D + PL_GC];
                        }
                    }
                    if constexpr (LSP) { if (lin_lane && (P.store_mask & 16)) { P.lslack[off] = sLV[cl + s * CSL]; P.ldual[off] = sLG[cl + s * CSL]; } }
                    if constexpr (LTP) { if (tlin_lane && (P.store_mask & 16)) { P.tlslack[off] = sTV[cl + s * CSL]; P.tldual[off] = sTG[cl + s * CSL]; } }
                    if constexpr (LSR) { if (lin_lane && (P.store_mask & 16)) { P.lslack[off] = VL[s]; P.ldual[off] = GL[s]; } }
                    if constexpr (LTR) { if (tlin_lane && (P.store_mask & 16)) { P.tlslack[off] = VT[s]; P.tldual[off] = GT[s]; } }
                    if constexpr (DBG) {
                        if (P.dbg_qr && acc_iter > 0) {
                            P.dbg_qr[off] = Qd[s];                          // work->q | work->r
                            P.dbg_pd[off] = is_state ? Pd[s] : Dd[s];       // work->p | work->d
                        }
                    }
                }
            }
            if constexpr (ADAPT) {
                if (ndl > 0) flush_c(ndl);
                if (j == 0) P.arho[b] = rho;
                if (is_state) {
#pragma unroll
                    for (int k = 0; k < NU; ++k) P.aK[(size_t)b * (NU * NX) + k + NU * j] = -mb[NX + k];
#pragma unroll
                    for (int k = 0; k < NX; ++k) P.aP[(size_t)b * (NX * NX) + k + NX * j] = sP[grp * NX * NX + k + NX * j];
                }
            }
            if constexpr (PM) {                              // (the plant step of the launch's LAST MPC step, from the true state)
                const double xt = true_x0(nsteps - 1, true_cell());
                if constexpr (PE && !PX) {                   // (... and the model's prediction from its xhat: the xp the next launch corrects)
                    if (P.x0_next && acc_iter > 0) {
                        const double xpn = predicted(X[0], X[1]);
                        if (is_state) late_arg<double>(__builtin_offsetof(SolveArgs, est_xp))[(size_t)b * NX + j] = xpn;
                    }
                }
                if (P.x0_next && acc_iter > 0) {
                    [[maybe_unused]] double s0 = X[1];
                    const double ua = applied(X[1], nsteps - 1, (PE && PX) ? &s0 : nullptr);
                    if constexpr (PE && PX) {                // (under the predictor: from the xhat kept in memory, with what left the queue)
                        const double xpn = predicted(is_state ? *xhat_cell() : 0.0, s0);
                        if (is_state) late_arg<double>(__builtin_offsetof(SolveArgs, est_xp))[(size_t)b * NX + j] = xpn;
                    }
                    double xn = plant_step(xt, ua);
                    if constexpr (PD) xn = disturbed(xn, nsteps - 1);
                    if (is_state) P.x0_next[(size_t)b * NX + j] = xn;
                    if (P.state_log && is_state) P.state_log[((size_t)(nsteps - 1) * P.batch + b) * NX + j] = xn;
                    if constexpr (PS) scored(xn, ua, nsteps - 1);
                    if constexpr (PA) act_logged(ua, nsteps - 1);
                } else if (P.state_log && is_state) {
                    P.state_log[((size_t)(nsteps - 1) * P.batch + b) * NX + j] = xt;
                }
            } else
            if constexpr (PD || PP) {                        // (the plant step of the launch's LAST MPC step)
                if (P.x0_next && acc_iter > 0) {
                    double xn = X[1];
                    [[maybe_unused]] double ua = X[1];       // (PA: what the plant receives)
                    if constexpr (PA) { ua = applied(X[1], nsteps - 1); xn = plant_step(X[0], ua); } else
                    if constexpr (PP) xn = plant_step(X[0], X[1]);
                    if constexpr (PD) xn = disturbed(xn, nsteps - 1);
                    if (is_state) P.x0_next[(size_t)b * NX + j] = xn;
                    if (P.state_log && is_state) P.state_log[((size_t)(nsteps - 1) * P.batch + b) * NX + j] = xn;
                    if constexpr (PS) scored(xn, PA ? ua : X[1], nsteps - 1);
                    if constexpr (PA) act_logged(ua, nsteps - 1);
                } else if (P.state_log && is_state) {        // (no plant step: the x0 the launch left in place)
                    P.state_log[((size_t)(nsteps - 1) * P.batch + b) * NX + j] = P.x0[(size_t)b * NX + j];
                }
            } else
            if (P.x0_next && acc_iter > 0 && is_state) P.x0_next[(size_t)b * NX + j] = X[1];     // x1 = A x0 + B u0 + f (needs a forward pass)
            const double ps = grp_maxw<RL>(is_state ? rp : 0.0), pi = grp_maxw<RL>(is_input ? rp : 0.0);
            const double ds = grp_maxw<RL>(is_state ? rd : 0.0), di = grp_maxw<RL>(is_input ? rd : 0.0);
            if (P.next_index) {
                const bool open = j == 0 && !solved;
                const unsigned long long m = __ballot(open);
                if (m) {
                    const int first = __ffsll((long long)m) - 1;
                    int at = 0;
                    if (lane == first) at = atomicAdd(P.next_count, __popcll(m));
                    at = __shfl(at, first);
                    if (open) P.next_index[at + __popcll(m & ((1ull << lane) - 1ull))] = b;
                }
            }
            if (j == 0) {
                P.status[b] = make_int4(iter, solved, solved ? 1 : 11, checked);
                double4 rr = make_double4(ps, pi, ds, di);
                *reinterpret_cast<double4*>(P.resid + (size_t)b * 4) = rr;
                if (P.accum) {
                    if constexpr (PF) {                      // (no value comes back: a persistent wave must not wait for one here)
                        __hip_atomic_fetch_add(&P.accum[b].x, acc_iter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        __hip_atomic_fetch_add(&P.accum[b].y, acc_solved, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else {
                        uint2 ac = P.accum[b];
                        ac.x += acc_iter;
                        ac.y += acc_solved;
                        P.accum[b] = ac;
                    }
                }
            }
        }
    }
}

}  // namespace tinympc_amd
