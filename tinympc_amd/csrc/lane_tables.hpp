// lane_tables.hpp -- WHAT goes where in a lane table: the one statement of which entry of the problem and its cache lane j keeps for
// column k (the layout -- where that lands in memory -- is LaneTab, admm_kernel.hip.h).  Function templates over a "view": a struct
// whose members are called as A(j,k), Kinf(m,j), Qw(j) ... and return the entry of that matrix / vector.  The host builders
// (batch_tables.hip) view Mat / Cache, the Riccati and sensitivity epilogues view the column-major LDS and global arrays they hold,
// so all of them write the same tables by construction.  The products Quu_inv B' (QBt) and Quu_inv BPf (QBPf) are inputs of the
// mapping: each side computes them with its own matrix product.
// Included by batch_tables.hip, batch_helpers.hip, batch_instance.hip, riccati_kernel.hip.h and sensitivity_kernel.hip.h -- never by the two headers that
// are instantiated at run time from their source text (admm_kernel.hip.h, tile_kernel.hip.h).
#pragma once
#include <hip/hip_runtime.h>

namespace tinympc_amd {

// entry (i, j) of a column-major array with leading dimension ld; a vector: ld = 0, entry (i)
struct ColMajor {
    const double* p;
    int ld;
    __host__ __device__ double operator()(int i, int j = 0) const { return p[i + ld * j]; }
};

struct LaneMatrices { double mb, mf1, mf2, pt; };     // TAB_MB / MF1 / MF2 / PT at (column k, lane j); 0.0 where the lane keeps nothing
struct LaneVectors { double cb, cf, qr; };            // VEC_CB / CF / QR of lane j
struct AtabEntries { double at, dk, dp, dc1, dc2; };  // ATAB_AT / DK / DP / DC1 / DC2 at (column k, lane j)

// view: A, B, AmBKt, Pinf, Kinf, Quu_inv, QBt
template <class V>
__host__ __device__ inline LaneMatrices lane_matrices(const V& v, int nx, int nu, int j, int k) {
    LaneMatrices m = {0.0, 0.0, 0.0, 0.0};
    if (j < nx) {                                      // state lanes
        if (k < nx) {
            m.mb = v.AmBKt(j, k);                      // p_i += AmBKt p_{i+1}     (admm.cpp:18)
            m.mf1 = v.A(j, k);                         // x_{i+1} = A x_i ...      (admm.cpp:30)
            m.pt = v.Pinf(k, j);                       // (Xref' Pinf)[j]          (admm.cpp:292)
        } else if (k < nx + nu) {
            m.mb = -v.Kinf(k - nx, j);                 // - Kinf' r_i
            m.mf2 = v.B(j, k - nx);                    // + B u_i
        }
    } else if (j < nx + nu) {                          // input lanes: d_i = Quu_inv (B' p_{i+1} + r_i + BPf)   (admm.cpp:17)
        const int a = j - nx;
        if (k < nx) {
            m.mb = v.QBt(a, k);
            m.mf1 = -v.Kinf(a, k);                     // u_i = -Kinf x_i - d_i     (admm.cpp:29)
        } else if (k < nx + nu) {
            m.mb = v.Quu_inv(a, k - nx);
        }
    }
    return m;
}

// view: APf, f, Qw (state lanes), QBPf, Rw (input lanes)
template <class V>
__host__ __device__ inline LaneVectors lane_vectors(const V& v, int nx, int nu, int j) {
    LaneVectors r = {0.0, 0.0, 0.0};
    if (j < nx) { r.cb = v.APf(j); r.cf = v.f(j); r.qr = v.Qw(j); }
    else if (j < nx + nu) { r.cb = v.QBPf(j - nx); r.qr = v.Rw(j - nx); }
    return r;
}

// ATAB_AT alone (view: A, B): state lanes A[k][j] -- (A' g)_j = sum_k A[k][j] g_k --, input lanes B[k][j-nx]
template <class V>
__host__ __device__ inline double atab_at(const V& v, int nx, int nu, int j, int k) {
    if (k < nx && j < nx) return v.A(k, j);
    if (k < nx && j < nx + nu) return v.B(k, j - nx);
    return 0.0;
}

// view: A, B, dK (nu x nx), dP (nx x nx), dC1 (nu x nu), dC2 (nx x nx)
template <class V>
__host__ __device__ inline AtabEntries atab_entries(const V& v, int nx, int nu, int j, int k) {
    AtabEntries e = {atab_at(v, nx, nu, j, k), 0.0, 0.0, 0.0, 0.0};
    if (j < nx) {
        if (k < nx) { e.dp = v.dP(k, j); e.dc2 = v.dC2(k, j); }
        if (k < nu) e.dk = v.dK(k, j);                 // (their -Kinf' entries)
    } else if (j < nx + nu) {
        if (k < nx) e.dk = v.dK(j - nx, k);
    }
    if (j < nu && k < nu) e.dc1 = v.dC1(k, j);         // C1 is nu x nu: its column j is kept by lane j
    return e;
}

// ---- the box: which element of the caller's bounds lands in (slot, lane) of a bounds block [lo | hi][N slots][lw lanes] -- the block of a
// lane table (LaneTab::BOUNDS) and every instance's block of a per-instance box (SolveArgs::inst_bounds, GeneralArgs::inst_bounds).
// State lanes keep knot `slot` in slot `slot`; input lanes keep knot `slot - 1` (their slot 0 is the neutral dummy of the register
// kernels' slot convention); lanes from nx + nu on, a disabled family and the dummy hold (-inf, +inf).
// family: 0 x_min | x_max [N][nx], 1 u_min | u_max [N - 1][nu], -1 nothing; index: into that family's arrays
struct BoxSource { int family, index; };
__host__ __device__ inline BoxSource box_source(int nx, int nu, int slot, int lane, bool state_on, bool input_on) {
    if (lane < nx) return state_on ? BoxSource{0, slot * nx + lane} : BoxSource{-1, 0};
    if (lane < nx + nu && slot >= 1 && input_on) return BoxSource{1, (slot - 1) * nu + (lane - nx)};
    return BoxSource{-1, 0};
}
struct BoxEntry { double lo, hi; };
// ... and the pair it holds (the four arrays: one instance's, or the family's)
__host__ __device__ inline BoxEntry box_entry(const double* x_min, const double* x_max, const double* u_min, const double* u_max, int nx, int nu, int slot, int lane,
                                              bool state_on, bool input_on) {
    const BoxSource s = box_source(nx, nu, slot, lane, state_on, input_on);
    if (s.family == 0) return {x_min[s.index], x_max[s.index]};
    if (s.family == 1) return {u_min[s.index], u_max[s.index]};
    return {-__builtin_huge_val(), __builtin_huge_val()};
}
// lanes of a per-instance bounds block: whole DPP rows (16 for the shapes of the one-row kernel, 32 for the wide ones of the coverage kernel)
__host__ __device__ constexpr int box_lanes(int nx, int nu) { return 16 * ((nx + nu + 15) / 16); }

// ---- half-spaces: what entry (constraint k, lane) of a block [3][km][lw] -- coefficient | offset | squared norm -- holds: the static
// block and the per-slot blocks of a lane table (LaneTab::lin_offset / tlin_offset) and every instance's blocks of a per-instance set
// (SolveArgs::inst_lin, GeneralArgs::inst_lin).  State lanes keep the state family's row k, input lanes the input family's; an entry
// without a constraint -- k beyond the family's count or km, a lane from nx + nu on, a disabled family -- is blank: coefficient 0, offset
// +inf, norm 1 (cv = 0 > +inf is false: inert).  The squared norm is summed from 0.0 in row order, every product rounded (what
// tests/halfspace_ref.py models).
// One family's half-spaces at one knot, wherever they lie: row k has the entries a[k * rs + c * cs], c < n, and the offset b[k]; the
// next knot's lie ak / bk doubles further on (time-varying sets)
struct HalfspaceRows {
    const double *a, *b;
    int count, n;
    long rs, cs, ak, bk;
    bool on;
    __host__ __device__ HalfspaceRows knot(int i) const {      // (knot -1, an input lane's slot 0: nothing)
        HalfspaceRows r = *this;
        if (i < 0) { r.count = 0; return r; }
        r.a = a + i * ak; r.b = b + i * bk;
        return r;
    }
};
// one instance's arrays of a family as the setters take them: a (count * knots) x n column-major matrix whose row count * knot + k is
// half-space k of that knot, and the offsets [knot][k] (a static set: one knot)
__host__ __device__ inline HalfspaceRows halfspace_caller_rows(const double* a, const double* b, int count, int n, int knots, bool on) {
    return {a, b, count, n, 1, (long)count * knots, count, count, on};
}
struct HalfspaceEntry { double a, b, nn; };
// the family and the column a lane keeps (nullptr: none)
__host__ __device__ inline const HalfspaceRows* halfspace_family(const HalfspaceRows& st, const HalfspaceRows& in, int nx, int nu, int k, int lane, int km, int* c) {
    if (lane >= nx + nu) return nullptr;
    const HalfspaceRows* f = lane < nx ? &st : &in;
    *c = lane < nx ? lane : lane - nx;
    return (f->on && k < f->count && k < km) ? f : nullptr;
}
// the offset alone (an offsets-only update rewrites nothing else)
__host__ __device__ inline double halfspace_offset(const HalfspaceRows& st, const HalfspaceRows& in, int nx, int nu, int k, int lane, int km) {
    int c = 0;
    const HalfspaceRows* f = halfspace_family(st, in, nx, nu, k, lane, km, &c);
    return f ? f->b[k] : __builtin_huge_val();
}
__host__ __device__ inline HalfspaceEntry halfspace_entry(const HalfspaceRows& st, const HalfspaceRows& in, int nx, int nu, int k, int lane, int km) {
#pragma clang fp contract(off)
    int c = 0;
    const HalfspaceRows* f = halfspace_family(st, in, nx, nu, k, lane, km, &c);
    if (!f) return {0.0, __builtin_huge_val(), 1.0};
    double nn = 0.0;
    for (int i = 0; i < f->n; ++i) { const double v = f->a[k * f->rs + i * f->cs]; const double pr = v * v; nn = nn + pr; }
    return {f->a[k * f->rs + c * f->cs], f->b[k], nn};
}
// the smallest power of two that holds `count` half-spaces per knot and family (at least 1): the km of a per-instance set's blocks
__host__ __device__ constexpr int halfspace_pow2(int count) { int km = 1; while (km < count) km *= 2; return km; }

// ---- cones: which cone's coefficient lane j keeps -- VEC_CONE_MU of a lane table and every instance's block [lw] of per-instance
// cone coefficients (SolveArgs::inst_cones).  The three rows of state cone k are the lanes Acx[k] .. Acx[k] + 2, those of input cone k
// the lanes nx + Acu[k] .. + 2; where cones share rows the last one in the caller's order holds the lane (the register kernels, which
// read a cone's coefficient at its first lane, do not run such sets: kernel_path.hpp).  A family that is off keeps nothing.
// family: 0 cx, 1 cu, -1 no cone; index: the cone
struct ConeSource { int family, index; };
__host__ __device__ inline ConeSource cone_source(const int* Acx, int n_state, const int* Acu, int n_input, int nx, int nu, int lane, bool state_on, bool input_on) {
    const bool st = lane < nx;
    if (lane >= nx + nu || !(st ? state_on : input_on)) return ConeSource{-1, 0};
    const int* first = st ? Acx : Acu;
    const int row = st ? lane : lane - nx;
    for (int k = (st ? n_state : n_input) - 1; k >= 0; --k)
        if (row >= first[k] && row < first[k] + 3) return ConeSource{st ? 0 : 1, k};
    return ConeSource{-1, 0};
}
// ... and the coefficient it holds (cx / cu: one instance's, or the family's); 1.0 on a lane without a cone: the coefficient of the
// register kernels' dummy item
__host__ __device__ inline double cone_entry(const double* cx, const double* cu, const int* Acx, int n_state, const int* Acu, int n_input, int nx, int nu, int lane,
                                             bool state_on = true, bool input_on = true) {
    const ConeSource s = cone_source(Acx, n_state, Acu, n_input, nx, nu, lane, state_on, input_on);
    if (s.family == 0) return cx[s.index];
    if (s.family == 1) return cu[s.index];
    return 1.0;
}

// ---- a plant of its own (tiny_batch_set_plant): what entry (column k, lane) of a plant block [nx + nu columns | f_p][16 lanes] holds
// (SolveArgs::plant).  State lane j keeps row j of A_p (columns 0 .. nx-1) and of B_p (columns nx .. nx+nu-1), both column-major as the
// caller gave them, and f_p[j] in the last row of the block (column nx + nu); every other lane 0.  f_p may be null: zero
__host__ __device__ constexpr int plant_block_doubles(int nx, int nu) { return (nx + nu + 1) * 16; }
__host__ __device__ inline double plant_entry(const double* A_p, const double* B_p, const double* f_p, int nx, int nu, int k, int lane) {
    if (lane >= nx) return 0.0;
    if (k < nx) return A_p[lane + nx * k];
    if (k < nx + nu) return B_p[lane + nx * (k - nx)];
    return f_p ? f_p[lane] : 0.0;
}

// ---- a state estimator's innovation gain (tiny_batch_set_estimator): what entry (column c, lane) of a gain block [nx columns][16 lanes]
// holds (SolveArgs::est_gain).  State lane j keeps row j of M, column-major as the caller gave it; every other lane 0
__host__ __device__ constexpr int gain_block_doubles(int nx) { return nx * 16; }
__host__ __device__ inline double gain_entry(const double* M, int nx, int c, int lane) {
    if (lane >= nx || c >= nx) return 0.0;
    return M[lane + nx * c];
}

// ---- a closed-loop score's setup (tiny_batch_set_score): what entry (row r, lane) of a score block [weight | target | lo | hi][16 lanes]
// holds (SolveArgs::score_tab).  Lane c < nx + nu keeps entry c of z = [x | u] of the caller's four arrays; a null target is 0, a null lo
// -inf, a null hi +inf, and so is every lane outside the row (weight 0 there): such a lane adds a zero and violates nothing
__host__ __device__ constexpr int score_block_doubles() { return 4 * 16; }
__host__ __device__ inline double score_entry(const double* weight, const double* target, const double* lo, const double* hi, int nx, int nu, int r, int lane) {
    const bool in = lane < nx + nu;
    if (r == 0) return in ? weight[lane] : 0.0;
    if (r == 1) return (in && target) ? target[lane] : 0.0;
    if (r == 2) return (in && lo) ? lo[lane] : -__builtin_huge_val();
    return (in && hi) ? hi[lane] : __builtin_huge_val();
}

// ---- an actuator model's setup (tiny_batch_set_actuator): what entry (row r, lane) of an actuator block [lo | hi | alpha | gain | offset]
// [16 lanes] holds (ActuatorLaunch::tab).  The lanes are the row's: input c sits on lane nx + c, where the one-row kernel keeps u0.  A null
// array and every lane outside the inputs are neutral: lo -inf, hi +inf, alpha 1, gain 1, offset -0.0 (fma(m, 1, -0.0) is m for every m,
// the sign of a zero included)
__host__ __device__ constexpr int actuator_block_doubles() { return 5 * 16; }
__host__ __device__ inline double actuator_entry(const double* lo, const double* hi, const double* alpha, const double* gain, const double* offset, int nx, int nu, int r,
                                                 int lane) {
    const int c = lane - nx;
    const bool in = c >= 0 && c < nu;
    if (r == 0) return (in && lo) ? lo[c] : -__builtin_huge_val();
    if (r == 1) return (in && hi) ? hi[c] : __builtin_huge_val();
    if (r == 2) return (in && alpha) ? alpha[c] : 1.0;
    if (r == 3) return (in && gain) ? gain[c] : 1.0;
    return (in && offset) ? offset[c] : -0.0;
}

}  // namespace tinympc_amd
