// batch_tables.hip -- the lane tables of the three kernels, built on the host from the batch's cache, bounds, cones and half-spaces:
// build_tables (one-row kernel) and build_tile_tables (tile kernel): one builder over the layout LaneTab (admm_kernel.hip.h);
// build_general_tables (coverage kernel, row-major at GeneralArgs offsets); all take their matrix and vector entries from the one
// mapping of lane_tables.hpp.  build_adaptive_table (ATAB_*), box_is_uniform, upload_tables.  Split off batch_dispatch.hip in round 6
// (one TU held the tables, the helper kernels and the dispatch); declarations: batch_dispatch.hpp.
#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"

#include <algorithm>
#include <cstring>
#include <limits>

namespace tinympc_amd {

// the largest half-space count per knot among the ENABLED families (a disabled family's rows are inert)
int max_enabled_halfspaces(const TinyBatch* b) {
    return std::max({0, b->set.en_state_linear ? b->nsl : 0, b->set.en_input_linear ? b->nil : 0, b->set.en_tv_state_linear ? b->ntsl : 0,
                     b->set.en_tv_input_linear ? b->ntil : 0});
}
// Half-spaces per knot and family the register-resident LIN variants are built for: 4 (compiled in), 8 / 16 / 32
// (instantiated at run time; the tables must still fit the 64 KiB of static LDS), 0 = more than that: coverage kernel.
int lin_kmax(const TinyBatch* b) {
    const int m = max_enabled_halfspaces(b);
    if (m <= LIN_KMAX) return LIN_KMAX;
    // more than the compiled-in variants hold: the table stride doubles (run-time instantiated KMAX = 8, 16, 32) while
    // the tables still fit the wave's static LDS
    const bool tv = b->set.en_tv_state_linear || b->set.en_tv_input_linear;
    const bool st = b->set.en_state_linear || b->set.en_input_linear;
    for (int km = 2 * LIN_KMAX; km <= LIN_KMAX_BIG; km *= 2) {
        if (m > km) continue;
        const long lds = 8L * ((tv ? 3L * b->N * km * 16 : 1) + (st ? 3L * km * 16 : 1) + b->nx * 16 + 2L * b->N * 16);
        return lds <= 63 * 1024 ? km : 0;
    }
    return 0;
}

// the box is the same at every knot -> the UB forms of both register kernels.  The one place that decides it: for the decisions taken
// before a table exists (batch_dispatch.hip) and, through fill_lane_tables, for the launch.  A disabled or never-set box is
// (-inf, +inf) everywhere; every knot is compared with knot 0, knot 0 included: a NaN bound equals nothing and is not uniform
bool box_is_uniform(const TinyBatch* b) {
    if (b->N < 2) return false;
    if (b->ibox.on) return b->ibox.uniform;   // (the same rule over every instance's box, reduced on the device: batch_instance.hip)
    if (!b->have_bounds) return true;
    auto same = [](const std::vector<double>& v, int knots, int n) {
        for (int i = 0; i < knots; ++i)
            for (int j = 0; j < n; ++j)
                if (v[(size_t)i * n + j] != v[j]) return false;
        return true;
    };
    return (!b->set.en_state_bound || (same(b->x_min, b->N, b->nx) && same(b->x_max, b->N, b->nx))) &&
           (!b->set.en_input_bound || (same(b->u_min, b->N - 1, b->nu) && same(b->u_max, b->N - 1, b->nu)));
}

namespace {
// the family's problem data and cache as lane_tables.hpp views them; QBt = Quu_inv B' and QBPf = Quu_inv BPf are the input rows of
// the fused backward step d_i = Quu_inv (B' p_{i+1} + r_i + BPf)   (admm.cpp:17)
struct HostView {
    ColMajor A, B, AmBKt, Pinf, Kinf, Quu_inv, QBt, APf, QBPf, f, Qw, Rw;
    Mat qbt, qbpf;
    explicit HostView(const TinyBatch* b) : qbt(b->cache.Quu_inv * transpose(b->B)), qbpf(b->cache.Quu_inv * b->cache.BPf) {
        auto m = [](const Mat& x) { return ColMajor{x.a.data(), x.r}; };
        const Cache& c = b->cache;
        A = m(b->A); B = m(b->B); AmBKt = m(c.AmBKt); Pinf = m(c.Pinf); Kinf = m(c.Kinf); Quu_inv = m(c.Quu_inv); QBt = m(qbt);
        APf = m(c.APf); QBPf = m(qbpf); f = m(b->f); Qw = {b->Qw.data(), 0}; Rw = {b->Rw.data(), 0};
    }
    HostView(const HostView&) = delete;                // (QBt and QBPf point into this object)
    HostView& operator=(const HostView&) = delete;
};
}  // namespace

// the four shared half-space families as the fill rule views them: the host copies, row-major [k][n] and [knot][k][n]; a disabled family
// is off, and so is every family of a set that is installed per instance (its host copies are empty)
SharedHalfspaces shared_halfspaces(const TinyBatch* b) {
    const int nx = b->nx, nu = b->nu;
    const bool s = !b->ilin.on[0], t = !b->ilin.on[1];
    SharedHalfspaces h;
    h.sx = {b->Alin_x.data(), b->blin_x.data(), s ? b->nsl : 0, nx, nx, 1, 0, 0, s && b->set.en_state_linear};
    h.su = {b->Alin_u.data(), b->blin_u.data(), s ? b->nil : 0, nu, nu, 1, 0, 0, s && b->set.en_input_linear};
    h.tx = {b->tvA_x.data(), b->tvb_x.data(), t ? b->ntsl : 0, nx, nx, 1, (long)b->ntsl * nx, b->ntsl, t && b->set.en_tv_state_linear};
    h.tu = {b->tvA_u.data(), b->tvb_u.data(), t ? b->ntil : 0, nu, nu, 1, (long)b->ntil * nu, b->ntil, t && b->set.en_tv_input_linear};
    return h;
}

// A lane table in the layout T (admm_kernel.hip.h LaneTab) from the batch's cache, bounds, cones and half-spaces.
static void fill_lane_tables(TinyBatch* b, const LaneTab T, std::vector<double>& t) {
    const int nx = b->nx, nu = b->nu, N = b->N, lw = T.lw;
    const int km = std::max(lin_kmax(b), (int)LIN_KMAX);            // stride of the half-space tables
    t.assign(T.doubles(N, km), 0.0);
    double* vec = &t[T.VEC()];
    const HostView view(b);
    for (int j = 0; j < nx + nu; ++j) {
        for (int k = 0; k < nx + nu; ++k) {
            const LaneMatrices m = lane_matrices(view, nx, nu, j, k);
            t[T.MB() + k * lw + j] = m.mb; t[T.MF1() + k * lw + j] = m.mf1; t[T.MF2() + k * lw + j] = m.mf2; t[T.PT() + k * lw + j] = m.pt;
        }
        const LaneVectors v = lane_vectors(view, nx, nu, j);
        vec[VEC_CB * lw + j] = v.cb; vec[VEC_CF * lw + j] = v.cf; vec[VEC_QR * lw + j] = v.qr;
        vec[(j < nx ? VEC_SMASK : VEC_NIM) * lw + j] = j < nx ? 1.0 : -1.0;
    }
    // cones (admm.cpp:102-135): lane flags, first lane and coefficient of the cone a lane belongs to
    for (int j = 0; j < lw; ++j) vec[VEC_CONE_BASE * lw + j] = -1.0;
    const bool s_on = b->set.en_state_soc && !b->Acx.empty(), i_on = b->set.en_input_soc && !b->Acu.empty();
    for (int j = 0; j < nx + nu; ++j) vec[VEC_SOCFLAG * lw + j] = (j < nx ? s_on : i_on) ? 1.0 : 0.0;
    auto cones = [&](const std::vector<int>& first, int lane0) {
        for (size_t k = 0; k < first.size(); ++k)
            for (int c3 = 0; c3 < 3; ++c3) vec[VEC_CONE_BASE * lw + lane0 + first[k] + c3] = lane0 + first[k];
    };
    if (b->set.en_state_soc) cones(b->Acx, 0);
    if (b->set.en_input_soc) cones(b->Acu, nx);
    // (whose coefficient a lane keeps: cone_entry, lane_tables.hpp -- the rule of per-instance coefficients, too; a lane without a
    // cone, or of a family that is off, stays 0.0 here)
    const int ncx = (int)b->Acx.size(), ncu = (int)b->Acu.size();
    const bool sc_on = b->set.en_state_soc != 0, ic_on = b->set.en_input_soc != 0;
    for (int j = 0; j < nx + nu; ++j)
        if (cone_source(b->Acx.data(), ncx, b->Acu.data(), ncu, nx, nu, j, sc_on, ic_on).family >= 0)
            vec[VEC_CONE_MU * lw + j] = cone_entry(b->cx.data(), b->cu.data(), b->Acx.data(), ncx, b->Acu.data(), ncu, nx, nu, j, sc_on, ic_on);
    // linear-constraint slacks exist for a whole family as soon as its switch is on (admm.cpp:138-145, 176-183)
    for (int j = 0; j < nx + nu; ++j) {
        vec[VEC_LINFLAG * lw + j] = (j < nx ? b->set.en_state_linear : b->set.en_input_linear) ? 1.0 : 0.0;
        vec[VEC_TLINFLAG * lw + j] = (j < nx ? b->set.en_tv_state_linear : b->set.en_tv_input_linear) ? 1.0 : 0.0;
    }
    // half-space tables of the LIN variants (admm.cpp:137-211): blocks of [3][km][lw] -- coefficient, offset, squared norm; a block is
    // blank (offset +inf, norm 1) where there is no constraint k; constraints beyond km are dropped (lin_kmax = 0: the coverage kernel runs)
    // (which entry holds what: halfspace_entry, lane_tables.hpp -- the rule of a per-instance set, too; a set installed per instance
    // leaves its blocks here blank: no kernel form reads them)
    auto fill = [&](double* blk, const HalfspaceRows& st, const HalfspaceRows& in) {
        for (int k = 0; k < km; ++k)
            for (int j = 0; j < lw; ++j) {
                const HalfspaceEntry e = halfspace_entry(st, in, nx, nu, k, j, km);
                blk[k * lw + j] = e.a; blk[km * lw + k * lw + j] = e.b; blk[2 * km * lw + k * lw + j] = e.nn;
            }
    };
    const SharedHalfspaces hs = shared_halfspaces(b);
    fill(&t[T.lin_offset(N)], hs.sx, hs.su);
    for (int s = 0; s < N; ++s)                      // state lanes: slot s = knot s; input lanes: slot s = knot s-1
        fill(&t[T.tlin_offset(N, km)] + (size_t)s * 3 * km * lw, hs.tx.knot(s), hs.tu.knot(s - 1));
    // bounds (admm.cpp:91-98): a disabled or never-set box is (-inf, +inf)
    // (which element lands in which slot and lane: box_entry, lane_tables.hpp -- the rule of the per-instance box, too; with one of
    // those installed this block is not read)
    double* lo = &t[T.BOUNDS()];
    double* hi = lo + N * lw;
    const bool state_on = b->set.en_state_bound && b->have_bounds, input_on = b->set.en_input_bound && b->have_bounds;
    for (int s = 0; s < N; ++s)
        for (int j = 0; j < lw; ++j) {
            const BoxEntry e = box_entry(b->x_min.data(), b->x_max.data(), b->u_min.data(), b->u_max.data(), nx, nu, s, j, state_on, input_on);
            lo[s * lw + j] = e.lo; hi[s * lw + j] = e.hi;
        }
    b->bounds_uniform = box_is_uniform(b);
}

// Tables of the one-row kernel (admm_kernel.hip.h) and of the tile kernel (tile_kernel.hip.h; W = 0, half rows, reads the layout of
// W = 1).  Rebuilt whenever cache, bounds, cones or the enable switches change.
void build_tables(TinyBatch* b) { fill_lane_tables(b, ROW_TAB, b->h_tab); }
void build_tile_tables(TinyBatch* b) { fill_lane_tables(b, LaneTab{32, 16 * std::max(1, b->tile->W)}, b->h_ttab); }

// Tables of the coverage kernel (general_kernel.hip.h): row-major [row][nz+1] matrices + vectors + constraints.
void build_general_tables(TinyBatch* b) {
    const int nx = b->nx, nu = b->nu, N = b->N, nz = nx + nu, ld = nz + 1;
    GeneralArgs& g = b->gargs;
    int off = 0;
    auto take = [&](int n) { int o = off; off += n; return o; };
    g.o_mb = take(nz * ld); g.o_mf1 = take(nz * ld); g.o_mf2 = take(nz * ld); g.o_pt = take(nz * ld);
    g.o_cb = take(nz); g.o_cf = take(nz); g.o_qr = take(nz);
    g.o_lo = take(N * nz); g.o_hi = take(N * nz);
    g.o_sc = take(2 * (int)b->Acx.size() + 2); g.o_ic = take(2 * (int)b->Acu.size() + 2);
    g.o_ax = take(b->nsl * nx + 1); g.o_bx = take(b->nsl + 1); g.o_au = take(b->nil * nu + 1); g.o_bu = take(b->nil + 1);
    g.o_tax = take(N * b->ntsl * nx + 1); g.o_tbx = take(N * b->ntsl + 1);
    g.o_tau = take((N - 1) * b->ntil * nu + 1); g.o_tbu = take((N - 1) * b->ntil + 1);
    std::vector<double>& t = b->h_gtab;
    t.assign(off, 0.0);
    const HostView view(b);
    for (int j = 0; j < nz; ++j) {
        for (int k = 0; k < nz; ++k) {
            const LaneMatrices m = lane_matrices(view, nx, nu, j, k);
            t[g.o_mb + j * ld + k] = m.mb; t[g.o_mf1 + j * ld + k] = m.mf1; t[g.o_mf2 + j * ld + k] = m.mf2; t[g.o_pt + j * ld + k] = m.pt;
        }
        const LaneVectors v = lane_vectors(view, nx, nu, j);
        t[g.o_cb + j] = v.cb; t[g.o_cf + j] = v.cf; t[g.o_qr + j] = v.qr;
    }
    const double inf = std::numeric_limits<double>::infinity();
    for (int e = 0; e < N * nz; ++e) { t[g.o_lo + e] = -inf; t[g.o_hi + e] = inf; }
    if (b->set.en_state_bound && b->have_bounds)
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < nx; ++j) { t[g.o_lo + i * nz + j] = b->x_min[(size_t)i * nx + j]; t[g.o_hi + i * nz + j] = b->x_max[(size_t)i * nx + j]; }
    if (b->set.en_input_bound && b->have_bounds)
        for (int i = 0; i < N - 1; ++i)
            for (int a = 0; a < nu; ++a) { t[g.o_lo + i * nz + nx + a] = b->u_min[(size_t)i * nu + a]; t[g.o_hi + i * nz + nx + a] = b->u_max[(size_t)i * nu + a]; }
    for (size_t k = 0; k < b->Acx.size(); ++k) { t[g.o_sc + 2 * k] = b->Acx[k]; t[g.o_sc + 2 * k + 1] = b->cx[k]; }
    for (size_t k = 0; k < b->Acu.size(); ++k) { t[g.o_ic + 2 * k] = b->Acu[k]; t[g.o_ic + 2 * k + 1] = b->cu[k]; }
    std::copy(b->Alin_x.begin(), b->Alin_x.end(), t.begin() + g.o_ax); std::copy(b->blin_x.begin(), b->blin_x.end(), t.begin() + g.o_bx);
    std::copy(b->Alin_u.begin(), b->Alin_u.end(), t.begin() + g.o_au); std::copy(b->blin_u.begin(), b->blin_u.end(), t.begin() + g.o_bu);
    std::copy(b->tvA_x.begin(), b->tvA_x.end(), t.begin() + g.o_tax); std::copy(b->tvb_x.begin(), b->tvb_x.end(), t.begin() + g.o_tbx);
    std::copy(b->tvA_u.begin(), b->tvA_u.end(), t.begin() + g.o_tau); std::copy(b->tvb_u.begin(), b->tvb_u.end(), t.begin() + g.o_tbu);
}

// The ATAB_* lane tables of a shared family (adaptive rho) from the sensitivity tables the caller set or the GPU computed
// (dKinf, dPinf, and dC1 / dC2 where given: column-major); needs nx + nu <= 16 and dKinf / dPinf of the batch's shape.
std::vector<double> build_adaptive_table(const TinyBatch* b) {
    const int nx = b->nx, nu = b->nu;
    const struct {
        ColMajor A, B, dK, dP;
        const std::vector<double>&c1, &c2;
        int nx, nu;
        double dC1(int k, int j) const { return c1.empty() ? 0.0 : c1[k + (size_t)nu * j]; }
        double dC2(int k, int j) const { return c2.empty() ? 0.0 : c2[k + (size_t)nx * j]; }
    } view = {{b->A.a.data(), nx}, {b->B.a.data(), nx}, {b->dKinf.data(), nu}, {b->dPinf.data(), nx}, b->dC1, b->dC2, nx, nu};
    std::vector<double> t(ATAB_DOUBLES, 0.0);
    for (int j = 0; j < nx + nu; ++j)
        for (int k = 0; k < nx + nu; ++k) {
            const AtabEntries a = atab_entries(view, nx, nu, j, k);
            const int e = k * 16 + j;
            t[ATAB_AT + e] = a.at; t[ATAB_DK + e] = a.dk; t[ATAB_DP + e] = a.dp; t[ATAB_DC1 + e] = a.dc1; t[ATAB_DC2 + e] = a.dc2;
        }
    return t;
}

// a host table into its device buffer, which grows when the table has: the old buffer goes once the stream has run dry of its readers.
// The host vectors are pageable: the copy is staged synchronously, so reusing them later is safe
int upload_growing(TinyBatch* b, double** dev, size_t* capacity, const std::vector<double>& host) {
    if (*capacity < host.size()) {
        if (*dev) {
            HIP_TRY(b, hipStreamSynchronize(b->stream));
            (void)hipFree(*dev);
        }
        *dev = nullptr; *capacity = 0;
        HIP_TRY(b, hipMalloc(dev, host.size() * sizeof(double)));
        *capacity = host.size();
    }
    HIP_TRY(b, hipMemcpyAsync(*dev, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
    return TINY_OK;
}
int upload_tables(TinyBatch* b) {
    if (!b->tab_dirty) return TINY_OK;
    build_tables(b);
    if (int rc = upload_growing(b, &b->d_tab, &b->d_tab_doubles, b->h_tab)) return rc;
    b->tab_dirty = false;
    return TINY_OK;
}

}  // namespace tinympc_amd
