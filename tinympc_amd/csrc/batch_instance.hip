// batch_instance.hip -- every instance its own problem data: a box, static and time-varying half-spaces, cone coefficients
// (InstanceBox, InstanceHalfspaces, InstanceCones of batch_impl.hpp).  Per family: the C ABI setter and getter, the drop the shared
// setters of batch_api.hip call, the fill kernel that turns the caller's arrays into what the solve kernels read (fill rules:
// lane_tables.hpp) and the ensure_instance_* that runs it when a setter or an enable switch has left the block out of date.  The
// sequences the families share with the closed-loop stages of batch_closed_loop.hip -- upload, read one instance back -- are defined
// once, at the top.  Declarations: batch_dispatch.hpp.
#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"

#include <algorithm>
#include <limits>

namespace tinympc_amd {

// ---- what the families and the closed-loop stages share (declared in batch_dispatch.hpp) -------------------------------------
unsigned helper_grid(const TinyBatch* b, size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, (size_t)b->num_cus * 16); }

// fresh[i] <- a new device buffer holding parts[i] (host or device memory by flags; a null src: none, fresh[i] stays null), then the
// stream has run dry: the caller may free its arrays and nothing reads the buffers the fresh ones are about to replace.  Everything or
// nothing: on a HIP error every buffer allocated here is freed again and the call fails with `what` in front of the error's text
int upload_fresh(TinyBatch* b, const UploadPart* parts, double** fresh, int n, int flags, const char* what) {
    hipError_t err = hipSuccess;
    for (int i = 0; i < n; ++i) fresh[i] = nullptr;
    for (int i = 0; i < n && err == hipSuccess; ++i) {
        if (!parts[i].src) continue;
        err = hipMalloc(&fresh[i], std::max<size_t>(parts[i].doubles, 1) * sizeof(double));
        if (err == hipSuccess) err = hipMemcpyAsync(fresh[i], parts[i].src, parts[i].doubles * sizeof(double), (flags & TINY_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, b->stream);
    }
    if (err == hipSuccess) err = hipStreamSynchronize(b->stream);
    if (err == hipSuccess) return TINY_OK;
    (void)hipGetLastError();
    for (int i = 0; i < n; ++i) { if (fresh[i]) (void)hipFree(fresh[i]); fresh[i] = nullptr; }
    return fail(b, TINY_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
}
// dst[0 .. n) <- instance `instance` of src [batch][n], after whatever the stream still had to write
int read_instance(TinyBatch* b, double* dst, const double* src, int instance, size_t n) {
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(dst, src + (size_t)instance * n, n * sizeof(double), hipMemcpyDeviceToHost));
    return TINY_OK;
}

// ---- every instance its own box (tiny_batch_set_instance_bounds): the caller's arrays -> [batch][lo | hi][N slots][lw lanes], one thread
// per (instance, slot, lane); which element lands there: box_entry (lane_tables.hpp), nothing else.  The same pass reduces ONE flag,
// box_is_uniform's rule over every instance: an enabled entry that differs from its family's first knot (slot 0 of a state lane, slot 1 of
// an input lane) -- or is a NaN, which differs from itself -- makes the batch not uniform
static __global__ __launch_bounds__(256) void fill_instance_bounds_kernel(double* __restrict__ out, const double* __restrict__ x_min, const double* __restrict__ x_max,
                                                                          const double* __restrict__ u_min, const double* __restrict__ u_max, int batch, int nx, int nu,
                                                                          int N, int lw, int state_on, int input_on, int* __restrict__ not_uniform) {
    const size_t total = (size_t)batch * N * lw;
    bool differs = false;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e % lw), slot = (int)((e / lw) % N);
        const size_t b = e / ((size_t)N * lw);
        const double *xl = x_min + b * N * nx, *xh = x_max + b * N * nx, *ul = u_min + b * (N - 1) * nu, *uh = u_max + b * (N - 1) * nu;
        const BoxEntry v = box_entry(xl, xh, ul, uh, nx, nu, slot, lane, state_on != 0, input_on != 0);
        out[(b * 2 * N + slot) * lw + lane] = v.lo;
        out[(b * 2 * N + N + slot) * lw + lane] = v.hi;
        const int family = box_source(nx, nu, slot, lane, state_on != 0, input_on != 0).family;
        if (family >= 0) {
            const BoxEntry first = box_entry(xl, xh, ul, uh, nx, nu, family == 0 ? 0 : 1, lane, state_on != 0, input_on != 0);
            differs |= (v.lo != first.lo) | (v.hi != first.hi);
        }
    }
    if (differs) atomicOr(not_uniform, 1);
}
static int ensure_instance_bounds(TinyBatch* b) {
    InstanceBox& s = b->ibox;
    if (!s.on || !s.dirty) return TINY_OK;
    const int lw = box_lanes(b->nx, b->nu);
    const size_t total = (size_t)b->batch * b->N * lw;
    if (!s.built) HIP_TRY(b, hipMalloc(&s.built, 2 * total * sizeof(double)));
    if (!s.flag) HIP_TRY(b, hipMalloc(&s.flag, sizeof(int)));
    HIP_TRY(b, hipMemsetAsync(s.flag, 0, sizeof(int), b->stream));
    hipLaunchKernelGGL(fill_instance_bounds_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.built, s.src[0], s.src[1], s.src[2], s.src[3], b->batch,
                       b->nx, b->nu, b->N, lw, b->set.en_state_bound ? 1 : 0, b->set.en_input_bound ? 1 : 0, s.flag);
    HIP_TRY(b, hipGetLastError());
    int not_uniform = 1;
    HIP_TRY(b, hipMemcpyAsync(&not_uniform, s.flag, sizeof(int), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    s.uniform = b->N >= 2 && not_uniform == 0;
    s.dirty = false;
    b->tab_dirty = true;                              // (the UB decision rides on the lane table's flag: box_is_uniform)
    return TINY_OK;
}
// tiny_batch_set_bound_constraints is about to install one box for all: a per-instance one goes, its device arrays (at 65 536 quadrotors:
// 168 MB + the caller's four) freed once the stream has run dry of their readers
int drop_instance_bounds(TinyBatch* b) {
    InstanceBox& s = b->ibox;
    if (!s.on && !s.built && !s.src[0]) return TINY_OK;
    s.on = false; s.dirty = false;
    return drop_buffers(b, s);
}

// ---- every instance its own half-spaces (tiny_batch_set_instance_linear_constraints / ..._tv_...): the caller's arrays -> [batch][the
// enabled sets' blocks: static [3][km][lw], then [N slots][3][km][lw]], one thread per (instance, block, constraint k, lane); what lands
// there: halfspace_entry (lane_tables.hpp), nothing else.  A set that stayed shared is written from its staged host copies, the same for
// every instance (ia = ib = 0).  mode 1 rewrites a family's offsets only -- the closed-loop update, which moves b and keeps A: no
// coefficient is read, no norm summed again
struct InstLinFamily {
    HalfspaceRows rows;              // instance 0's, all knots
    long ia, ib;                     // doubles from one instance's coefficients / offsets to the next one's
    int mode;                        // 0 leave alone, 1 offsets only, 2 everything
};
struct InstLinFill {
    InstLinFamily f[2][2];           // [static | time-varying][state | input]
    double* out;
    int batch, nx, nu, N, lw, km, lv;
    size_t stride;
};
static __global__ __launch_bounds__(256) void fill_instance_linear_kernel(const InstLinFill F) {
    const int nblk = ((F.lv & 1) ? 1 : 0) + ((F.lv & 2) ? F.N : 0);
    const size_t total = (size_t)F.batch * nblk * F.km * F.lw;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e % F.lw), k = (int)((e / F.lw) % F.km), q = (int)((e / ((size_t)F.lw * F.km)) % nblk);
        const size_t inst = e / ((size_t)F.lw * F.km * nblk);
        const int set = ((F.lv & 1) && q == 0) ? 0 : 1, slot = q - (F.lv & 1);
        const int mode = F.f[set][lane < F.nx ? 0 : 1].mode;
        if (mode == 0) continue;
        HalfspaceRows st = F.f[set][0].rows, in = F.f[set][1].rows;
        st.a += inst * F.f[set][0].ia; st.b += inst * F.f[set][0].ib;
        in.a += inst * F.f[set][1].ia; in.b += inst * F.f[set][1].ib;
        if (set == 1) { st = st.knot(slot); in = in.knot(slot - 1); }      // input lanes: slot s = knot s-1
        double* blk = F.out + inst * F.stride + (size_t)q * 3 * F.km * F.lw;
        if (mode == 1) { blk[F.km * F.lw + k * F.lw + lane] = halfspace_offset(st, in, F.nx, F.nu, k, lane, F.km); continue; }
        const HalfspaceEntry v = halfspace_entry(st, in, F.nx, F.nu, k, lane, F.km);
        blk[k * F.lw + lane] = v.a; blk[F.km * F.lw + k * F.lw + lane] = v.b; blk[2 * F.km * F.lw + k * F.lw + lane] = v.nn;
    }
}
int inst_lin_active(const TinyBatch* b) {
    return ((b->ilin.on[0] && (b->set.en_state_linear || b->set.en_input_linear)) ? 1 : 0) |
           ((b->ilin.on[1] && (b->set.en_tv_state_linear || b->set.en_tv_input_linear)) ? 2 : 0);
}
// the block stride of a per-instance set: the smallest power of two that holds the enabled counts (1 and 2 included)
int inst_lin_kmax(const TinyBatch* b) { return halfspace_pow2(max_enabled_halfspaces(b)); }
static int ensure_instance_linear(TinyBatch* b) {
    InstanceHalfspaces& s = b->ilin;
    if (!s.on[0] && !s.on[1]) return TINY_OK;
    if (!s.full && !s.offsets) return TINY_OK;
    const int N = b->N, nx = b->nx, nu = b->nu;
    const int lv = ((b->set.en_state_linear || b->set.en_input_linear) ? 1 : 0) | ((b->set.en_tv_state_linear || b->set.en_tv_input_linear) ? 2 : 0);
    InstLinFill F = {};
    if (s.full) {
        s.lv = lv; s.km = inst_lin_kmax(b);
        s.stride = (size_t)3 * s.km * box_lanes(nx, nu) * ((lv & 1) + ((lv & 2) ? N : 0));
    }
    F.out = nullptr; F.batch = b->batch; F.nx = nx; F.nu = nu; F.N = N; F.lw = box_lanes(nx, nu); F.km = s.km; F.lv = s.lv; F.stride = s.stride;
    if (s.stride == 0 || !inst_lin_active(b)) { s.offsets = 0; return TINY_OK; }      // (nothing a kernel would read; full stays: built when a switch comes on)
    const size_t need = (size_t)b->batch * s.stride;
    if (s.doubles < need) {
        if (s.built) { HIP_TRY(b, hipStreamSynchronize(b->stream)); (void)hipFree(s.built); }
        s.built = nullptr; s.doubles = 0;
        HIP_TRY(b, hipMalloc(&s.built, need * sizeof(double)));
        s.doubles = need;
        s.full = true;
    }
    F.out = s.built;
    // the caller's arrays: per instance an (n x cols) column-major matrix, one ROW per half-space -- time-varying: row n * knot + k
    const int cnt[2][2] = {{b->nsl, b->nil}, {b->ntsl, b->ntil}};
    const bool on[2][2] = {{b->set.en_state_linear != 0, b->set.en_input_linear != 0}, {b->set.en_tv_state_linear != 0, b->set.en_tv_input_linear != 0}};
    for (int set = 0; set < 2; ++set)
        for (int fam = 0; fam < 2; ++fam) {
            if (!s.on[set]) continue;
            const int n = fam ? nu : nx, c = cnt[set][fam];
            const long knots = set ? (fam ? N - 1 : N) : 1;
            InstLinFamily& f = F.f[set][fam];
            f.rows = halfspace_caller_rows(s.src[set][2 * fam], s.src[set][2 * fam + 1], c, n, (int)knots, on[set][fam]);
            f.ia = c * knots * n; f.ib = c * knots;
            f.mode = s.full ? 2 : ((s.offsets >> (2 * set + fam)) & 1);
        }
    // a set that stayed shared while the other one is per instance: its host copies, staged, for every instance (full builds only)
    if (s.full && (!s.on[0] || !s.on[1])) {
        const int set = s.on[0] ? 1 : 0;
        const SharedHalfspaces h = shared_halfspaces(b);
        const HalfspaceRows hr[2] = {set ? h.tx : h.sx, set ? h.tu : h.su};
        const std::vector<double>* src[4] = {set ? &b->tvA_x : &b->Alin_x, set ? &b->tvb_x : &b->blin_x, set ? &b->tvA_u : &b->Alin_u, set ? &b->tvb_u : &b->blin_u};
        std::vector<double> stage;
        size_t at[4];
        for (int i = 0; i < 4; ++i) { at[i] = stage.size(); stage.insert(stage.end(), src[i]->begin(), src[i]->end()); }
        stage.push_back(0.0);
        if (int rc = upload_growing(b, &s.stage, &s.stage_doubles, stage)) return rc;
        for (int fam = 0; fam < 2; ++fam) {
            InstLinFamily& f = F.f[set][fam];
            f.rows = hr[fam];
            f.rows.a = s.stage + at[2 * fam]; f.rows.b = s.stage + at[2 * fam + 1];
            f.ia = 0; f.ib = 0; f.mode = 2;
        }
    }
    const int nblk = ((F.lv & 1) ? 1 : 0) + ((F.lv & 2) ? N : 0);
    hipLaunchKernelGGL(fill_instance_linear_kernel, dim3(helper_grid(b, (size_t)b->batch * nblk * F.km * F.lw)), dim3(256), 0, b->stream, F);
    HIP_TRY(b, hipGetLastError());
    s.full = false; s.offsets = 0;
    return TINY_OK;
}
// a shared setter of set `set` (0 static, 1 time-varying) is about to install one set for all: a per-instance set goes, its arrays
// freed once the stream has run dry of their readers; the other set, if it is per instance, has its blocks rebuilt (they hold both)
int drop_instance_linear(TinyBatch* b, int set) {
    InstanceHalfspaces& s = b->ilin;
    if (s.on[set] && !s.on[1 - set]) {               // (the other set's arrays are null: every buffer there is belongs to this one)
        if (int rc = drop_buffers(b, s)) return rc;
        s.doubles = 0; s.stage_doubles = 0;
    } else if (s.on[set]) {
        HIP_TRY(b, hipSetDevice(b->device));
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        for (double*& p : s.src[set]) { if (p) (void)hipFree(p); p = nullptr; }
    }
    s.on[set] = false;
    s.full = true; s.offsets = 0;
    return TINY_OK;
}

// ---- every instance its own cone coefficients (tiny_batch_set_instance_cone_coefficients): the caller's dense arrays cx [batch][n_state],
// cu [batch][n_input] -> [batch][lw lanes], one thread per (instance, lane); what lands there: cone_entry (lane_tables.hpp), nothing else.
// A family whose array is null takes the shared coefficients, the same for every instance (stride 0)
static __global__ __launch_bounds__(256) void fill_instance_cones_kernel(double* __restrict__ out, const double* __restrict__ cx, const double* __restrict__ cu, long cx_stride,
                                                                         long cu_stride, const int* __restrict__ Acx, int n_state, const int* __restrict__ Acu, int n_input,
                                                                         int batch, int nx, int nu, int lw) {
    const size_t total = (size_t)batch * lw;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e % lw);
        const size_t b = e / lw;
        out[e] = cone_entry(cx + b * cx_stride, cu + b * cu_stride, Acx, n_state, Acu, n_input, nx, nu, lane);
    }
}
bool inst_cones_active(const TinyBatch* b) { return b->icone.on && soc_active(b); }
static int ensure_instance_cones(TinyBatch* b) {
    InstanceCones& s = b->icone;
    if (!s.on || !s.dirty) return TINY_OK;
    const int lw = box_lanes(b->nx, b->nu), ns = (int)b->Acx.size(), ni = (int)b->Acu.size();
    const size_t total = (size_t)b->batch * lw;
    if (!s.built) HIP_TRY(b, hipMalloc(&s.built, total * sizeof(double)));
    if (!s.pos) HIP_TRY(b, hipMalloc(&s.pos, (size_t)(ns + ni + 1) * sizeof(int)));
    // the cone positions and the shared coefficients (of a family that did not get its own), staged; the host vectors are pageable:
    // the copies are staged synchronously
    std::vector<int> pos(b->Acx);
    pos.insert(pos.end(), b->Acu.begin(), b->Acu.end());
    pos.push_back(0);
    std::vector<double> shared(b->cx);
    shared.insert(shared.end(), b->cu.begin(), b->cu.end());
    shared.push_back(1.0);
    HIP_TRY(b, hipMemcpyAsync(s.pos, pos.data(), pos.size() * sizeof(int), hipMemcpyHostToDevice, b->stream));
    if (int rc = upload_growing(b, &s.stage, &s.stage_doubles, shared)) return rc;
    const double* cx = s.src[0] ? s.src[0] : s.stage;
    const double* cu = s.src[1] ? s.src[1] : s.stage + ns;
    hipLaunchKernelGGL(fill_instance_cones_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.built, cx, cu, s.src[0] ? (long)ns : 0L,
                       s.src[1] ? (long)ni : 0L, s.pos, ns, s.pos + ns, ni, b->batch, b->nx, b->nu, lw);
    HIP_TRY(b, hipGetLastError());
    s.dirty = false;
    return TINY_OK;
}
// tiny_batch_set_cone_constraints is about to install one coefficient set for all (and, maybe, other cones): per-instance coefficients
// go, their arrays freed once the stream has run dry of their readers
int drop_instance_cones(TinyBatch* b) {
    InstanceCones& s = b->icone;
    if (!s.on && !s.built && !s.src[0] && !s.src[1]) return TINY_OK;
    if (int rc = drop_buffers(b, s)) return rc;
    s.stage_doubles = 0;
    s.on = false; s.dirty = false;
    return TINY_OK;
}

// ---- what a launch and tiny_batch_update_settings call (batch_dispatch.hpp)
int ensure_instance_data(TinyBatch* b) {
    if (int rc = ensure_instance_bounds(b)) return rc;   // (first: a rebuilt box may change the UB decision, it sets tab_dirty)
    if (int rc = ensure_instance_linear(b)) return rc;
    return ensure_instance_cones(b);
}
void note_instance_data_read(TinyBatch* b) {
    b->ibox.last = b->ibox.on;                        // (every path a per-instance box can take reads it)
    b->ilin.last = inst_lin_active(b);                // (likewise)
    b->icone.last = inst_cones_active(b);
    note_closed_loop_read(b);                         // (the stages at the plant step: batch_closed_loop.hip)
}
void instance_data_settings_changed(TinyBatch* b) {
    if (b->ibox.on) b->ibox.dirty = true;             // (a disabled family is (-inf, +inf) in the array the kernels read)
    b->ilin.full = true;                              // (... and blank in a per-instance set's blocks, whose stride follows the enabled counts)
}

}  // namespace tinympc_amd

using namespace tinympc_amd;

extern "C" {

// every instance its own box.  The caller's arrays are kept on the device as given; what the kernels read is built from them at once
// (ensure_instance_bounds: synchronous, it reads the knot-invariance flag back) and again when an enable switch changes.  The shared box
// is given up only once that has succeeded: a call that fails leaves the batch on the shared box it had (a per-instance box it had
// before is gone: its arrays were being overwritten) -- not transactional, unlike the other two: these are the largest arrays there are
int tiny_batch_set_instance_bounds(TinyBatch* b, const double* x_min, const double* x_max, const double* u_min, const double* u_max, int flags) {
    if (!b) return TINY_ERR_NULL;
    if (!x_min || !x_max || !u_min || !u_max) return fail(b, TINY_ERR_NULL, "null bound pointer");
    if (flags & TINY_BROADCAST) return fail(b, TINY_ERR_ARG, "one box for every instance: tiny_batch_set_bound_constraints");
    HIP_TRY(b, hipSetDevice(b->device));
    InstanceBox& s = b->ibox;
    const size_t n[4] = {(size_t)b->batch * b->N * b->nx, (size_t)b->batch * b->N * b->nx, (size_t)b->batch * (b->N - 1) * b->nu, (size_t)b->batch * (b->N - 1) * b->nu};
    const double* src[4] = {x_min, x_max, u_min, u_max};
    s.on = false;
    for (int i = 0; i < 4; ++i) {
        if (!s.src[i]) HIP_TRY(b, hipMalloc(&s.src[i], std::max<size_t>(n[i], 1) * sizeof(double)));
        HIP_TRY(b, hipMemcpyAsync(s.src[i], src[i], n[i] * sizeof(double), (flags & TINY_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, b->stream));
    }
    s.on = true; s.dirty = true;
    b->tab_dirty = true;
    if (int rc = ensure_instance_bounds(b)) { s.on = false; return rc; }
    b->have_bounds = false;                          // (the latest setter wins: the shared box is gone)
    b->x_min.clear(); b->x_max.clear(); b->u_min.clear(); b->u_max.clear();
    return TINY_OK;
}

int tiny_batch_get_instance_bounds(TinyBatch* b, int instance, double* x_min, double* x_max, double* u_min, double* u_max) {
    if (!b) return TINY_ERR_NULL;
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    const size_t ns = (size_t)b->N * b->nx, ni = (size_t)(b->N - 1) * b->nu;
    double* dst[4] = {x_min, x_max, u_min, u_max};
    const std::vector<double>* shared[4] = {&b->x_min, &b->x_max, &b->u_min, &b->u_max};
    for (int i = 0; i < 4; ++i) {
        if (!dst[i]) continue;
        const size_t n = i < 2 ? ns : ni;
        if (b->ibox.on) { if (int rc = read_instance(b, dst[i], b->ibox.src[i], instance, n)) return rc; continue; }
        const double none = (i & 1) ? std::numeric_limits<double>::infinity() : -std::numeric_limits<double>::infinity();
        for (size_t e = 0; e < n; ++e) dst[i][e] = b->have_bounds ? (*shared[i])[e] : none;      // (never set: (-inf, +inf))
    }
    return TINY_OK;
}

// every instance its own cone coefficients on the cones tiny_batch_set_cone_constraints installed.  The caller's arrays are kept on the
// device as given (the coverage kernel reads them so); the block the one-row kernel reads is built from them in front of the next
// launch (ensure_instance_cones).  Everything that can fail happens before anything installed is touched
int tiny_batch_set_instance_cone_coefficients(TinyBatch* b, const double* cx, const double* cu, int flags) {
    if (!b) return TINY_ERR_NULL;
    if (b->Acx.empty() && b->Acu.empty()) return fail(b, TINY_ERR_ARG, "no cone set installed: tiny_batch_set_cone_constraints first");
    if (flags & TINY_BROADCAST) return fail(b, TINY_ERR_ARG, "one coefficient for every instance: tiny_batch_set_cone_constraints");
    const size_t cnt[2] = {b->Acx.size(), b->Acu.size()};
    const UploadPart parts[2] = {{cnt[0] ? cx : nullptr, (size_t)b->batch * cnt[0]}, {cnt[1] ? cu : nullptr, (size_t)b->batch * cnt[1]}};
    if (!parts[0].src && !parts[1].src) return fail(b, TINY_ERR_ARG, "null coefficient arrays for every cone family that has cones");
    HIP_TRY(b, hipSetDevice(b->device));
    double* fresh[2];
    if (int rc = upload_fresh(b, parts, fresh, 2, flags, "per-instance cone coefficients")) return rc;
    for (int i = 0; i < 2; ++i) {                                        // (the latest setter wins: a family passed as NULL is back on the shared coefficients)
        if (b->icone.src[i]) (void)hipFree(b->icone.src[i]);
        b->icone.src[i] = fresh[i];
    }
    b->icone.on = true; b->icone.dirty = true;
    b->tab_dirty = true;
    return TINY_OK;
}
// what instance `instance` is held to, as set (whatever the switches say); on a shared set, or for a family that kept it: the shared values
int tiny_batch_get_instance_cone_coefficients(TinyBatch* b, int instance, double* cx, double* cu) {
    if (!b) return TINY_ERR_NULL;
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    double* dst[2] = {cx, cu};
    const std::vector<double>* shared[2] = {&b->cx, &b->cu};
    for (int i = 0; i < 2; ++i) {
        const size_t n = shared[i]->size();
        if (!dst[i] || !n) continue;
        if (b->icone.on && b->icone.src[i]) { if (int rc = read_instance(b, dst[i], b->icone.src[i], instance, n)) return rc; }
        else for (size_t k = 0; k < n; ++k) dst[i][k] = (*shared[i])[k];
    }
    return TINY_OK;
}

// every instance its own half-spaces, set 0 (static) or 1 (time-varying).  The caller's arrays are kept on the device as given; what
// the kernels read is built from them in front of the next launch (ensure_instance_linear).  Everything that can fail -- the checks,
// the allocations, the copies -- happens before anything installed is touched: a failed call leaves what was installed.
// A == NULL for every family with a positive count: the offsets-only update (the counts must be the installed ones)
static int set_instance_linear(TinyBatch* b, int set, int n_state, const double* A_x, const double* b_x, int n_input, const double* A_u, const double* b_u,
                               int flags) {
    if (n_state < 0 || n_input < 0) return fail(b, TINY_ERR_DIM, "negative constraint count");
    if (flags & TINY_BROADCAST)
        return fail(b, TINY_ERR_ARG, "one set for every instance: %s", set ? "tiny_batch_set_tv_linear_constraints" : "tiny_batch_set_linear_constraints");
    if ((n_state > 0 && !b_x) || (n_input > 0 && !b_u)) return fail(b, TINY_ERR_NULL, "null offsets with a positive count");
    InstanceHalfspaces& s = b->ilin;
    const int cnt[2] = {n_state, n_input};
    const double* src[4] = {A_x, b_x, A_u, b_u};
    const int have[2] = {set ? b->ntsl : b->nsl, set ? b->ntil : b->nil};
    bool offsets_only[2];
    for (int fam = 0; fam < 2; ++fam) {
        offsets_only[fam] = cnt[fam] > 0 && !src[2 * fam];
        if (offsets_only[fam] && (!s.on[set] || have[0] != n_state || have[1] != n_input))
            return fail(b, TINY_ERR_ARG, "null coefficients: the offsets-only update needs a per-instance set of the same counts installed (%d, %d)", n_state, n_input);
    }
    HIP_TRY(b, hipSetDevice(b->device));
    const size_t knots[2] = {set ? (size_t)b->N : 1, set ? (size_t)b->N - 1 : 1};
    UploadPart parts[4];
    for (int i = 0; i < 4; ++i) {                                        // (a family without half-spaces gets no buffer; one with a zero-sized array does)
        const int fam = i / 2;
        parts[i] = {cnt[fam] ? src[i] : nullptr, (size_t)b->batch * cnt[fam] * knots[fam] * ((i & 1) ? 1 : (fam ? b->nu : b->nx))};
    }
    double* fresh[4];
    if (int rc = upload_fresh(b, parts, fresh, 4, flags, "per-instance half-spaces")) return rc;
    for (int i = 0; i < 4; ++i) {
        if (offsets_only[i / 2] && !(i & 1)) continue;                   // (this family keeps its coefficients)
        if (s.src[set][i]) (void)hipFree(s.src[set][i]);
        s.src[set][i] = fresh[i];
    }
    const bool all_offsets = (offsets_only[0] || cnt[0] == 0) && (offsets_only[1] || cnt[1] == 0) && (cnt[0] > 0 || cnt[1] > 0);
    if (all_offsets) s.offsets |= ((offsets_only[0] ? 1 : 0) | (offsets_only[1] ? 2 : 0)) << (2 * set);
    else s.full = true;
    s.on[set] = true;
    if (set) { b->ntsl = n_state; b->ntil = n_input; b->tvA_x.clear(); b->tvb_x.clear(); b->tvA_u.clear(); b->tvb_u.clear(); }
    else { b->nsl = n_state; b->nil = n_input; b->Alin_x.clear(); b->blin_x.clear(); b->Alin_u.clear(); b->blin_u.clear(); }
    b->tab_dirty = true;
    return TINY_OK;
}
int tiny_batch_set_instance_linear_constraints(TinyBatch* b, int n_state, const double* Alin_x, const double* blin_x, int n_input,
                                               const double* Alin_u, const double* blin_u, int flags) {
    if (!b) return TINY_ERR_NULL;
    return set_instance_linear(b, 0, n_state, Alin_x, blin_x, n_input, Alin_u, blin_u, flags);
}
int tiny_batch_set_instance_tv_linear_constraints(TinyBatch* b, int n_state, const double* tv_Alin_x, const double* tv_blin_x, int n_input,
                                                  const double* tv_Alin_u, const double* tv_blin_u, int flags) {
    if (!b) return TINY_ERR_NULL;
    return set_instance_linear(b, 1, n_state, tv_Alin_x, tv_blin_x, n_input, tv_Alin_u, tv_blin_u, flags);
}
// what instance `instance` is held to by set `tv` (0 static, 1 time-varying), as set -- whatever the switches say -- in the shared
// setter's layout; on a shared set: the shared one.  any pointer may be NULL
int tiny_batch_get_instance_linear_constraints(TinyBatch* b, int instance, int tv, double* A_x, double* b_x, double* A_u, double* b_u) {
    if (!b) return TINY_ERR_NULL;
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    if (tv != 0 && tv != 1) return fail(b, TINY_ERR_ARG, "set %d: 0 static, 1 time-varying", tv);
    const int cnt[2] = {tv ? b->ntsl : b->nsl, tv ? b->ntil : b->nil};
    const size_t rows[2] = {(size_t)cnt[0] * (tv ? b->N : 1), (size_t)cnt[1] * (tv ? b->N - 1 : 1)};
    double* dst[4] = {A_x, b_x, A_u, b_u};
    const std::vector<double>* shared[4] = {tv ? &b->tvA_x : &b->Alin_x, tv ? &b->tvb_x : &b->blin_x, tv ? &b->tvA_u : &b->Alin_u, tv ? &b->tvb_u : &b->blin_u};
    for (int i = 0; i < 4; ++i) {
        if (!dst[i]) continue;
        const size_t r = rows[i / 2], cols = (i & 1) ? 1 : (i / 2 ? b->nu : b->nx);
        if (b->ilin.on[tv]) { if (r * cols) { if (int rc = read_instance(b, dst[i], b->ilin.src[tv][i], instance, r * cols)) return rc; } }
        else for (size_t k = 0; k < r; ++k)                                  // (the host copies are row-major: rows_of)
            for (size_t c = 0; c < cols; ++c) dst[i][c * r + k] = (*shared[i])[k * cols + c];
    }
    return TINY_OK;
}

}  // extern "C"
