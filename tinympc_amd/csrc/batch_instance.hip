// batch_instance.hip -- every instance its own problem data: a box, static and time-varying half-spaces, cone coefficients, a
// disturbance sequence, a plant model with its state log, a measurement-noise sequence, a state estimator, a closed-loop score (InstanceBox, InstanceHalfspaces, InstanceCones, Disturbance, PlantStep, MeasurementNoise, Estimator, Score of batch_impl.hpp).  Per family: the C ABI setter and
// getter, the drop the shared setters of batch_api.hip call, the fill kernel that turns the caller's arrays into what the solve kernels
// read (fill rules: lane_tables.hpp) and the ensure_instance_* that runs it when a setter or an enable switch has left the block out of date.
// The sequences the families share -- upload, drop, read one instance back -- stand once, at the top.  Declarations: batch_dispatch.hpp.
#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"
#include "noise_gen.hpp"

#include <algorithm>
#include <limits>

namespace tinympc_amd {

// ---- what the families share -----------------------------------------------------------------------------------------------
static unsigned helper_grid(const TinyBatch* b, size_t total) { return (unsigned)std::min<size_t>((total + 255) / 256, (size_t)b->num_cus * 16); }

// fresh[i] <- a new device buffer holding parts[i] (host or device memory by flags; a null src: none, fresh[i] stays null), then the
// stream has run dry: the caller may free its arrays and nothing reads the buffers the fresh ones are about to replace.  Everything or
// nothing: on a HIP error every buffer allocated here is freed again and the call fails with `what` in front of the error's text
struct UploadPart { const double* src; size_t doubles; };
static int upload_fresh(TinyBatch* b, const UploadPart* parts, double** fresh, int n, int flags, const char* what) {
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
// every buffer of one family goes, once the stream has run dry of their readers (its flags and sizes: the caller's)
template <class S>
static int drop_buffers(TinyBatch* b, S& s) {
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    free_buffers(s);
    return TINY_OK;
}
// dst[0 .. n) <- instance `instance` of src [batch][n], after whatever the stream still had to write
static int read_instance(TinyBatch* b, double* dst, const double* src, int instance, size_t n) {
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

// ---- every instance its own disturbance at the plant step (tiny_batch_set_disturbance): one sequence for all, seq [n_steps][nx], written
// out as the layout the kernels read, out [n_steps][batch][nx]; one thread per element (enqueued on the batch's stream)
static __global__ __launch_bounds__(256) void expand_disturbance_kernel(double* __restrict__ out, const double* __restrict__ seq, size_t total, int batch, int nx) {
    const size_t row = (size_t)batch * nx;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
        out[e] = seq[(e / row) * nx + e % nx];
}
static int expand_disturbance(TinyBatch* b, double* out, const double* seq, int n_steps, int width) {
    const size_t total = (size_t)n_steps * b->batch * width;
    hipLaunchKernelGGL(expand_disturbance_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, out, seq, total, b->batch, width);
    HIP_TRY(b, hipGetLastError());
    return TINY_OK;
}
// a step-major sequence [n_steps][batch][nx] (TINY_BROADCAST: [n_steps][nx], expanded on the device so that the kernels know one
// layout), copied into S::seq with its counter rewound -- the disturbance and the measurement noise, and with rows of `width` = nu
// entries the actuation noise (0: nx).  Everything that can fail happens before anything installed is touched
template <class S>
static int install_sequence(TinyBatch* b, S& s, const double* w, int n_steps, int flags, const char* what, const char* what_short, int width = 0) {
    if (width <= 0) width = b->nx;
    HIP_TRY(b, hipSetDevice(b->device));
    if (!w || n_steps <= 0) {                                            // remove: freed once the stream has run dry of its readers
        if (s.seq) { if (int rc = drop_buffers(b, s)) return rc; }
        s.steps = 0; s.step = 0; s.generated = false;
        return TINY_OK;
    }
    const size_t row = (size_t)b->batch * width, full = (size_t)n_steps * row;
    if (full / row != (size_t)n_steps || full > (std::numeric_limits<size_t>::max)() / sizeof(double))
        return fail(b, TINY_ERR_ARG, "%s: %d steps of %d instances do not fit an address", what_short, n_steps, b->batch);
    double* fresh = nullptr;
    if (!(flags & TINY_BROADCAST)) {
        const UploadPart given = {w, full};
        if (int rc = upload_fresh(b, &given, &fresh, 1, flags, what)) return rc;
    } else {
        // one sequence for all, staged and expanded.  The expanded buffer is allocated FIRST: a step count no device memory holds fails
        // there, before the stage is sized by it and a byte of the caller's (then far shorter) array is read
        const size_t given = (size_t)n_steps * width;
        double* stage = nullptr;
        hipError_t err = hipMalloc(&fresh, full * sizeof(double));
        int rc = TINY_OK;
        if (err == hipSuccess) err = hipMalloc(&stage, given * sizeof(double));
        if (err == hipSuccess) err = hipMemcpyAsync(stage, w, given * sizeof(double), (flags & TINY_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, b->stream);
        if (err == hipSuccess) rc = expand_disturbance(b, fresh, stage, n_steps, width);
        if (err == hipSuccess && rc == TINY_OK) err = hipStreamSynchronize(b->stream);      // (the caller may free its array; nothing reads the old one any more)
        if (stage) (void)hipFree(stage);
        if (err != hipSuccess || rc != TINY_OK) {
            (void)hipGetLastError();
            if (fresh) (void)hipFree(fresh);
            return rc != TINY_OK ? rc : fail(b, TINY_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
        }
    }
    if (s.seq) (void)hipFree(s.seq);
    s.seq = fresh; s.steps = n_steps; s.step = 0; s.generated = false;
    return TINY_OK;
}
// ---- a sequence generated on the device (tiny_batch_generate_disturbance / ..._measurement_noise): out [n_steps][batch][nx] filled with
// the counter-based normals of noise_gen.hpp -- every entry a pure function of (seed, stream, instance id, row, entry), the same bits as
// tiny_noise_generate gives on the host.  No LDS, no atomics, no scratch; measured, the arithmetic of a pair binds, not the stores
// (profiles/noise_generator.md).
// Diagonal form: one thread per pair (step, instance, p) in the order of the step-major block, so that consecutive threads write
// consecutive addresses: one 16-byte store for an even nx (every pair then starts on a 16-byte boundary), two 8-byte stores otherwise,
// one where the last pair's second half is dropped
static __global__ __launch_bounds__(256) void generate_diagonal_kernel(double* __restrict__ out, const NoiseFill F) {
    const int np = noise_pairs(F.nx);
    const size_t per_step = (size_t)F.batch * np, total = (size_t)F.n_steps * per_step;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int p = (int)(e % np);
        const size_t i = (e / np) % F.batch;
        const uint32_t k = (uint32_t)(e / per_step);
        double two[2];
        noise_diagonal_pair(F, k, i, p, two);
        double* at = out + ((size_t)k * F.batch + i) * F.nx + 2 * p;
        if (!(F.nx & 1)) *reinterpret_cast<double2*>(at) = make_double2(two[0], two[1]);
        else { at[0] = two[0]; if (2 * p + 1 < F.nx) at[1] = two[1]; }
    }
}
// Factor form: one thread per row (step, instance): at most 16 Philox calls, the nx accumulators in registers (noise_factor_row32).  The
// one shared S is read at wave-uniform addresses; a per-instance S is read by each thread from its own block
static __global__ __launch_bounds__(256) void generate_factor_kernel(double* __restrict__ out, const NoiseFill F) {
    const size_t total = (size_t)F.n_steps * F.batch;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x)
        noise_factor_row32(F, (uint32_t)(e / F.batch), e % F.batch, out + e * F.nx);
}
// the checks tiny_batch_generate_* and tiny_noise_generate share: null (fine) or why the spec is refused
static const char* noise_spec_refusal(const TinyNoiseSpec* spec, int nx) {
    if (!spec) return "null spec";
    if (!spec->scale) return "null scale";
    if (spec->n_steps <= 0) return "n_steps <= 0";
    if (spec->id_stride < 1) return "id_stride < 1";
    if (spec->id_base < 0) return "id_base < 0";
    if (spec->flags & ~(TINY_DEVICE | TINY_BROADCAST | TINY_NOISE_FACTOR)) return "flags: TINY_HOST or TINY_DEVICE, with or without TINY_BROADCAST and TINY_NOISE_FACTOR";
    if (nx > 2 * 65536) return "more than 65 536 pairs a row";
    return nullptr;
}
static NoiseFill noise_fill_of(const TinyNoiseSpec* spec, int stream, int batch, int nx, const double* scale, const double* mean) {
    NoiseFill F = {};
    F.seed = spec->seed; F.id_base = (uint64_t)spec->id_base; F.id_stride = (uint64_t)spec->id_stride;
    F.stream = (uint32_t)stream; F.n_steps = spec->n_steps; F.batch = batch; F.nx = nx;
    F.factor = (spec->flags & TINY_NOISE_FACTOR) != 0; F.broadcast = (spec->flags & TINY_BROADCAST) != 0;
    F.scale = scale; F.mean = mean;
    return F;
}
// the generated block takes the place install_sequence gives a caller's: a fresh buffer, complete before it replaces what is installed,
// the counter rewound.  scale and mean are copied to the device for the fill and freed behind it.  Everything that can fail happens
// before anything installed is touched
template <class S>
static int install_generated(TinyBatch* b, S& s, const TinyNoiseSpec* spec, int stream, const char* what, int width = 0) {
    const int nx = width > 0 ? width : b->nx;        // (the row's width: nx, or nu for the actuation noise)
    if (const char* why = noise_spec_refusal(spec, nx)) return fail(b, TINY_ERR_ARG, "%s: %s", what, why);
    if (nx > 32) return fail(b, TINY_ERR_ARG, "%s: width %d (a batch has rows of at most 32 entries: at most 16 pairs a row)", what, nx);
    HIP_TRY(b, hipSetDevice(b->device));
    const size_t row = (size_t)b->batch * nx, full = (size_t)spec->n_steps * row;
    if (full / row != (size_t)spec->n_steps || full > (std::numeric_limits<size_t>::max)() / sizeof(double))
        return fail(b, TINY_ERR_ARG, "%s: %d steps of %d instances do not fit an address", what, spec->n_steps, b->batch);
    const bool factor = (spec->flags & TINY_NOISE_FACTOR) != 0;
    const size_t sets = (spec->flags & TINY_BROADCAST) ? 1 : (size_t)b->batch;
    // the block is allocated FIRST: a step count no device memory holds fails there
    double* fresh = nullptr;
    if (hipMalloc(&fresh, full * sizeof(double)) != hipSuccess) { (void)hipGetLastError(); return fail(b, TINY_ERR_HIP, "%s: out of device memory", what); }
    const UploadPart parts[2] = {{spec->scale, sets * nx * (factor ? nx : 1)}, {spec->mean, sets * nx}};
    double* staged[2];
    if (int rc = upload_fresh(b, parts, staged, 2, spec->flags & TINY_DEVICE, what)) { (void)hipFree(fresh); return rc; }
    const NoiseFill F = noise_fill_of(spec, stream, b->batch, nx, staged[0], staged[1]);
    if (factor) hipLaunchKernelGGL(generate_factor_kernel, dim3(helper_grid(b, (size_t)spec->n_steps * b->batch)), dim3(256), 0, b->stream, fresh, F);
    else hipLaunchKernelGGL(generate_diagonal_kernel, dim3(helper_grid(b, (size_t)spec->n_steps * b->batch * noise_pairs(nx))), dim3(256), 0, b->stream, fresh, F);
    hipError_t err = hipGetLastError();
    if (err == hipSuccess) err = hipStreamSynchronize(b->stream);         // (nothing reads the old sequence any more; the staged arrays may go)
    for (double* p : staged) if (p) (void)hipFree(p);
    if (err != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(fresh);
        return fail(b, TINY_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
    }
    if (s.seq) (void)hipFree(s.seq);
    s.seq = fresh; s.steps = spec->n_steps; s.step = 0; s.generated = true;
    return TINY_OK;
}
// row `step` of instance `instance` of such a sequence, as set: out [nx]
template <class S>
static int read_sequence_row(TinyBatch* b, const S& s, int step, int instance, double* out, const char* none, int width = 0) {
    if (width <= 0) width = b->nx;
    if (!out) return fail(b, TINY_ERR_ARG, "null output");
    if (!s.seq) return fail(b, TINY_ERR_ARG, "%s", none);
    if (step < 0 || step >= s.steps) return fail(b, TINY_ERR_ARG, "step %d of %d", step, s.steps);
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    return read_instance(b, out, s.seq + (size_t)step * b->batch * width, instance, width);
}
bool disturbance_active(const TinyBatch* b) { return b->dist.seq && b->dist.steps > 0 && (b->advance_x0 || b->steps_per_launch > 1); }
// (the kernels count steps in an int; a counter moved beyond +-2^30 is outside every sequence either way)
int dist_step_base(const TinyBatch* b) { return (int)std::clamp<long>(b->dist.step, -(1L << 30), 1L << 30); }

// ---- a plant of its own at the plant step (tiny_batch_set_plant): the caller's A_p | B_p | f_p -> [plants][nx + nu + 1][16 lanes], one
// thread per (plant, column, lane); what lands there: plant_entry (lane_tables.hpp), nothing else.  One plant for all: one block (stride 0)
static __global__ __launch_bounds__(256) void fill_plant_kernel(double* __restrict__ out, const double* __restrict__ A_p, const double* __restrict__ B_p,
                                                                const double* __restrict__ f_p, int plants, int nx, int nu) {
    const int rows = nx + nu + 1;
    const size_t total = (size_t)plants * rows * 16;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e % 16), k = (int)((e / 16) % rows);
        const size_t p = e / ((size_t)16 * rows);
        out[e] = plant_entry(A_p + p * nx * nx, B_p + p * nx * nu, f_p ? f_p + p * nx : nullptr, nx, nu, k, lane);
    }
}
bool plant_active(const TinyBatch* b) { return b->plant.kind != 0 && (b->advance_x0 || b->steps_per_launch > 1); }
bool state_log_active(const TinyBatch* b) { return b->plant.log_on && (b->advance_x0 || b->steps_per_launch > 1); }
bool measurement_active(const TinyBatch* b) { return b->meas.seq && b->meas.steps > 0 && (b->advance_x0 || b->steps_per_launch > 1); }
int meas_step_base(const TinyBatch* b) { return (int)std::clamp<long>(b->meas.step, -(1L << 30), 1L << 30); }
// what a launch steps the state by: the plant installed, else -- a launch under measurement noise, which always goes through a plant
// block -- the batch's own model: every instance's own A | B | f of a tiny_batch_setup_hetero batch, or the shared family's (uploaded once)
struct PlantSource { const double* src[3]; bool per_instance; double* const* built; };
// (the model alone: what a state estimator predicts by, whatever plant is installed)
static PlantSource model_source(const TinyBatch* b) {
    if (b->hetero) return {{b->d_hA, b->d_hB, b->d_hf}, true, &b->meas.model_built};
    return {{b->meas.model[0], b->meas.model[1], b->meas.model[2]}, false, &b->meas.model_built};
}
static PlantSource plant_source(const TinyBatch* b) {
    if (b->plant.kind) return {{b->plant.src[0], b->plant.src[1], b->plant.src[2]}, b->plant.kind == 2, &b->plant.built};
    if (b->hetero) return {{b->d_hA, b->d_hB, b->d_hf}, true, &b->meas.model_built};
    return {{b->meas.model[0], b->meas.model[1], b->meas.model[2]}, false, &b->meas.model_built};
}
static int ensure_model_source(TinyBatch* b, bool under_a_plant = false) {
    if ((b->plant.kind && !under_a_plant) || b->hetero || b->meas.model[0]) return TINY_OK;
    const UploadPart parts[3] = {{b->A.a.data(), b->A.a.size()}, {b->B.a.data(), b->B.a.size()}, {b->f.a.data(), b->f.a.size()}};
    return upload_fresh(b, parts, b->meas.model, 3, TINY_HOST, "model as plant");
}
const double* plant_kernel_pointer(const TinyBatch* b) {
    const PlantSource p = plant_source(b);
    return reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(*p.built) | (p.per_instance ? (uintptr_t)0 : (uintptr_t)1));
}
// (only the one-row kernel's PP forms read the blocks: the launch that binds one asks for them -- a launch without a plant step, and
// the coverage path, which reads the caller's arrays, build and read no block.  Under measurement noise with no plant installed the
// arrays are the model's: a shared family's A | B | f are uploaded once, by whichever path asks first: ensure_model_source)
// the model's own block, made once -- with no plant installed what the PP forms step by, and under a state estimator what predicts,
// next to whatever plant is installed
static int ensure_model_block(TinyBatch* b) {
    if (b->meas.model_built) return TINY_OK;
    if (int rc = ensure_model_source(b, true)) return rc;
    const PlantSource p = model_source(b);
    const int plants = p.per_instance ? b->batch : 1;
    const size_t total = (size_t)plants * plant_block_doubles(b->nx, b->nu);
    HIP_TRY(b, hipMalloc(&b->meas.model_built, total * sizeof(double)));
    hipLaunchKernelGGL(fill_plant_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, b->meas.model_built, p.src[0], p.src[1], p.src[2], plants, b->nx, b->nu);
    HIP_TRY(b, hipGetLastError());
    return TINY_OK;
}
int ensure_plant_blocks(TinyBatch* b) {
    PlantStep& s = b->plant;
    if (!s.kind) return ensure_model_block(b);        // (no plant installed: the model's own block)
    if (!s.dirty) return TINY_OK;
    const int plants = s.kind == 1 ? 1 : b->batch;
    const size_t total = (size_t)plants * plant_block_doubles(b->nx, b->nu);
    if (!s.built) HIP_TRY(b, hipMalloc(&s.built, total * sizeof(double)));
    hipLaunchKernelGGL(fill_plant_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.built, s.src[0], s.src[1], s.src[2], plants, b->nx, b->nu);
    HIP_TRY(b, hipGetLastError());
    s.dirty = false;
    return TINY_OK;
}
int begin_state_log(TinyBatch* b, int rows) {
    PlantStep& s = b->plant;
    s.log_rows = 0;
    if (s.log_steps < rows) {
        if (s.log) { HIP_TRY(b, hipStreamSynchronize(b->stream)); (void)hipFree(s.log); }
        s.log = nullptr; s.log_steps = 0;
        HIP_TRY(b, hipMalloc(&s.log, (size_t)rows * b->batch * b->nx * sizeof(double)));
        s.log_steps = rows;
    }
    s.log_rows = rows;
    return TINY_OK;
}
// the coverage path's plant step: one thread per (instance, state row), the chain of tiny_batch_set_plant in explicit fma()s.  Every
// thread reads x0 and u0 and writes `next`, never x0 itself: the rows of an instance are read by its other threads.  An instance whose
// launch ran no iteration took no plant step: its x0 passes through.  ua: null, or [batch][nu], the applied control under an actuator
// model (coverage_actuator_kernel), read in place of the record's u0
static __global__ __launch_bounds__(256) void coverage_plant_step_kernel(double* __restrict__ next, const double* __restrict__ x0, const double* __restrict__ prim,
                                                                         const double* __restrict__ ua,
                                                                         const int4* __restrict__ status, const double* __restrict__ A_p, const double* __restrict__ B_p,
                                                                         const double* __restrict__ f_p, int per_instance, const double* __restrict__ dist, int batch,
                                                                         int nx, int nu, int N) {
    const size_t total = (size_t)batch * nx;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % nx);
        const size_t bb = e / nx, p = per_instance ? bb : 0;
        if (status[bb].x <= 0) { next[e] = x0[e]; continue; }
        const double *A = A_p + p * nx * nx, *B = B_p + p * nx * nu, *u0 = ua ? ua + bb * nu : prim + bb * N * (nx + nu) + nx;
        double acc = f_p ? f_p[p * nx + j] : 0.0;
        for (int k = 0; k < nx; ++k) acc = fma(x0[bb * nx + k], A[j + nx * k], acc);
        for (int k = 0; k < nu; ++k) acc = fma(u0[k], B[j + nx * k], acc);
        next[e] = dist ? acc + dist[e] : acc;
    }
}
int enqueue_coverage_plant_step(TinyBatch* b, const double* dist_block) {
    PlantStep& s = b->plant;
    if (int rc = ensure_model_source(b)) return rc;
    const PlantSource p = plant_source(b);
    const size_t total = (size_t)b->batch * b->nx;
    if (!s.next) HIP_TRY(b, hipMalloc(&s.next, total * sizeof(double)));
    hipLaunchKernelGGL(coverage_plant_step_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.next, b->d_x0, b->d_prim,
                       b->act.last ? b->act.ua : nullptr, b->d_status, p.src[0], p.src[1],
                       p.src[2], p.per_instance ? 1 : 0, dist_block, b->batch, b->nx, b->nu, b->N);
    HIP_TRY(b, hipGetLastError());
    HIP_TRY(b, hipMemcpyAsync(b->d_x0, s.next, total * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
    return TINY_OK;
}
// the coverage path's measurements of one MPC step: xm[e] = fl(x0[e] + v[e]) over the [batch][nx] block of that step's row -- one
// IEEE addition per element, what plant_add does on the one-row kernel
static __global__ __launch_bounds__(256) void coverage_measurement_kernel(double* __restrict__ xm, const double* __restrict__ x0, const double* __restrict__ v, size_t total) {
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) xm[e] = x0[e] + v[e];
}
int enqueue_coverage_measurement(TinyBatch* b, long step, const double** x0_of_launch) {
    MeasurementNoise& s = b->meas;
    *x0_of_launch = b->d_x0;
    if (step < 0 || step >= s.steps) return TINY_OK;
    const size_t total = (size_t)b->batch * b->nx;
    if (!s.xm) HIP_TRY(b, hipMalloc(&s.xm, total * sizeof(double)));
    hipLaunchKernelGGL(coverage_measurement_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.xm, b->d_x0, s.seq + (size_t)step * total, total);
    HIP_TRY(b, hipGetLastError());
    *x0_of_launch = s.xm;
    return TINY_OK;
}
int enqueue_state_log_row(TinyBatch* b, int row) {
    const size_t total = (size_t)b->batch * b->nx;
    HIP_TRY(b, hipMemcpyAsync(b->plant.log + (size_t)row * total, b->d_x0, total * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
    return TINY_OK;
}

// ---- a state estimator between the measurement and the solve (tiny_batch_set_estimator): the caller's M -> [gains][nx][16 lanes], one
// thread per (gain, column, lane); what lands there: gain_entry (lane_tables.hpp), nothing else.  One gain for all: one block
static __global__ __launch_bounds__(256) void fill_gain_kernel(double* __restrict__ out, const double* __restrict__ M, int gains, int nx) {
    const size_t total = (size_t)gains * nx * 16;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e % 16), c = (int)((e / 16) % nx);
        const size_t g = e / ((size_t)16 * nx);
        out[e] = gain_entry(M + g * nx * nx, nx, c, lane);
    }
}
bool estimator_active(const TinyBatch* b) { return b->est.kind != 0 && (b->advance_x0 || b->steps_per_launch > 1); }
const double* estimator_gain_pointer(const TinyBatch* b) {
    return reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(b->est.built) | (b->est.kind == 2 ? (uintptr_t)0 : (uintptr_t)1));
}
const double* model_kernel_pointer(const TinyBatch* b) {
    const PlantSource p = model_source(b);
    return reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(*p.built) | (p.per_instance ? (uintptr_t)0 : (uintptr_t)1));
}
// (only the one-row kernel's PE forms read the blocks; the coverage path reads the caller's array and the model's arrays)
int ensure_estimator_blocks(TinyBatch* b) {
    Estimator& s = b->est;
    if (int rc = ensure_model_block(b)) return rc;
    if (!s.kind || !s.dirty) return TINY_OK;
    const int gains = s.kind == 1 ? 1 : b->batch;
    const size_t total = (size_t)gains * gain_block_doubles(b->nx);
    if (!s.built) HIP_TRY(b, hipMalloc(&s.built, total * sizeof(double)));
    hipLaunchKernelGGL(fill_gain_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.built, s.src, gains, b->nx);
    HIP_TRY(b, hipGetLastError());
    s.dirty = false;
    return TINY_OK;
}
int begin_estimate_log(TinyBatch* b, int rows) {
    Estimator& s = b->est;
    s.log_rows = 0;
    if (s.log_steps < rows) {
        if (s.log) { HIP_TRY(b, hipStreamSynchronize(b->stream)); (void)hipFree(s.log); }
        s.log = nullptr; s.log_steps = 0;
        HIP_TRY(b, hipMalloc(&s.log, (size_t)rows * b->batch * b->nx * sizeof(double)));
        s.log_steps = rows;
    }
    s.log_rows = rows;
    return TINY_OK;
}
// the coverage path's correction in front of one single-step launch: one thread per (instance, state row), the chain of
// tiny_batch_set_estimator in explicit fma()s over e[c] = fl(xm[c] - xp[c]) -- what plant_sub and plant_chain do on the one-row kernel
static __global__ __launch_bounds__(256) void coverage_correction_kernel(double* __restrict__ xhat, double* __restrict__ log, const double* __restrict__ xm,
                                                                         const double* __restrict__ xp, const double* __restrict__ M, int per_instance, int batch,
                                                                         int nx) {
    const size_t total = (size_t)batch * nx;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % nx);
        const size_t bb = e / nx;
        const double* G = M + (per_instance ? bb : 0) * nx * nx;
        double acc = xp[e];
        for (int c = 0; c < nx; ++c) {
            const double inno = xm[bb * nx + c] - xp[bb * nx + c];
            acc = fma(inno, G[j + nx * c], acc);
        }
        xhat[e] = acc;
        if (log) log[e] = acc;
    }
}
int enqueue_coverage_correction(TinyBatch* b, int log_row, const double** x0_of_launch) {
    Estimator& s = b->est;
    const size_t total = (size_t)b->batch * b->nx;
    if (!s.xhat) HIP_TRY(b, hipMalloc(&s.xhat, total * sizeof(double)));
    double* const log = (s.log && log_row < s.log_rows) ? s.log + (size_t)log_row * total : nullptr;
    hipLaunchKernelGGL(coverage_correction_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.xhat, log, *x0_of_launch, s.xp, s.src, s.kind == 2 ? 1 : 0,
                       b->batch, b->nx);
    HIP_TRY(b, hipGetLastError());
    *x0_of_launch = s.xhat;
    return TINY_OK;
}
// ... and its prediction behind the launch: xp <- the MODEL's step from xhat and the u0 of the x|u record, the chain of
// coverage_plant_step_kernel.  xhat and xp are arrays of their own: a thread may write its xp while others still read xhat.  An instance
// whose launch ran no iteration keeps its xp
static __global__ __launch_bounds__(256) void coverage_prediction_kernel(double* __restrict__ xp, const double* __restrict__ xhat, const double* __restrict__ prim,
                                                                         const int4* __restrict__ status, const double* __restrict__ A_m, const double* __restrict__ B_m,
                                                                         const double* __restrict__ f_m, int per_instance, int batch, int nx, int nu, int N) {
    const size_t total = (size_t)batch * nx;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % nx);
        const size_t bb = e / nx, p = per_instance ? bb : 0;
        if (status[bb].x <= 0) continue;
        const double *A = A_m + p * nx * nx, *B = B_m + p * nx * nu, *u0 = prim + bb * N * (nx + nu) + nx;
        double acc = f_m ? f_m[p * nx + j] : 0.0;
        for (int k = 0; k < nx; ++k) acc = fma(xhat[bb * nx + k], A[j + nx * k], acc);
        for (int k = 0; k < nu; ++k) acc = fma(u0[k], B[j + nx * k], acc);
        xp[e] = acc;
    }
}
int enqueue_coverage_prediction(TinyBatch* b) {
    Estimator& s = b->est;
    if (int rc = ensure_model_source(b, true)) return rc;
    const PlantSource p = model_source(b);
    const size_t total = (size_t)b->batch * b->nx;
    hipLaunchKernelGGL(coverage_prediction_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.xp, s.xhat, b->d_prim, b->d_status, p.src[0], p.src[1], p.src[2],
                       p.per_instance ? 1 : 0, b->batch, b->nx, b->nu, b->N);
    HIP_TRY(b, hipGetLastError());
    return TINY_OK;
}

// ---- a closed-loop score at the plant step (tiny_batch_set_score): the caller's weight | target | lo | hi -> [setups][4][16 lanes], one
// thread per (setup, row, lane); what lands there: score_entry (lane_tables.hpp), nothing else.  One setup for all: one block
static __global__ __launch_bounds__(256) void fill_score_kernel(double* __restrict__ out, const double* __restrict__ weight, const double* __restrict__ target,
                                                                const double* __restrict__ lo, const double* __restrict__ hi, int setups, int nx, int nu) {
    const size_t total = (size_t)setups * score_block_doubles();
    const int nz = nx + nu;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e % 16), r = (int)((e / 16) % 4);
        const size_t g = e / score_block_doubles();
        out[e] = score_entry(weight + g * nz, target ? target + g * nz : nullptr, lo ? lo + g * nz : nullptr, hi ? hi + g * nz : nullptr, nx, nu, r, lane);
    }
}
// a zeroed record: cost 0, worst 0, violated_steps 0, first_violation -1
static __global__ __launch_bounds__(256) void zero_score_kernel(ScoreRecord* __restrict__ rec, int batch) {
    for (int bb = blockIdx.x * blockDim.x + threadIdx.x; bb < batch; bb += gridDim.x * blockDim.x) rec[bb] = ScoreRecord{0.0, 0.0, 0, -1};
}
static int enqueue_zero_score(TinyBatch* b, void* rec) {
    hipLaunchKernelGGL(zero_score_kernel, dim3(helper_grid(b, (size_t)b->batch)), dim3(256), 0, b->stream, static_cast<ScoreRecord*>(rec), b->batch);
    HIP_TRY(b, hipGetLastError());
    return TINY_OK;
}
bool score_active(const TinyBatch* b) { return b->score.kind != 0 && (b->advance_x0 || b->steps_per_launch > 1); }
int score_step_base(const TinyBatch* b) { return (int)std::clamp<long>(b->score.step, -(1L << 30), 1L << 30); }
const double* score_kernel_pointer(const TinyBatch* b) {
    return reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(b->score.built) | (b->score.kind == 2 ? (uintptr_t)0 : (uintptr_t)1));
}
// (only the one-row kernel's PS forms read the blocks; the coverage path reads the caller's arrays)
int ensure_score_blocks(TinyBatch* b) {
    Score& s = b->score;
    if (!s.kind || !s.dirty) return TINY_OK;
    const int setups = s.kind == 1 ? 1 : b->batch;
    const size_t total = (size_t)setups * score_block_doubles();
    if (!s.built) HIP_TRY(b, hipMalloc(&s.built, total * sizeof(double)));
    hipLaunchKernelGGL(fill_score_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.built, s.src[0], s.src[1], s.src[2], s.src[3], setups, b->nx, b->nu);
    HIP_TRY(b, hipGetLastError());
    s.dirty = false;
    return TINY_OK;
}
// the coverage path's score behind one single-step launch and its plant step: one thread per instance, the arithmetic of
// tiny_batch_set_score in its stated order over z = [x0 as handed on | the u0 of the x|u record] -- what score_term, score_chain and the
// row maximum do on the one-row kernel, same bits.  An instance whose launch ran no iteration took no plant step and is not scored
static __global__ __launch_bounds__(256) void coverage_score_kernel(ScoreRecord* __restrict__ rec, const double* __restrict__ x0, const double* __restrict__ prim,
                                                                    const double* __restrict__ ua,
                                                                    const int4* __restrict__ status, const double* __restrict__ weight, const double* __restrict__ target,
                                                                    const double* __restrict__ lo, const double* __restrict__ hi, int per_instance, int step, int batch,
                                                                    int nx, int nu, int N) {
#pragma clang fp contract(off)
    const int nz = nx + nu;
    for (int bb = blockIdx.x * blockDim.x + threadIdx.x; bb < batch; bb += gridDim.x * blockDim.x) {
        if (status[bb].x <= 0) continue;
        const size_t p = per_instance ? (size_t)bb * nz : 0;
        const double *xn = x0 + (size_t)bb * nx, *u0 = ua ? ua + (size_t)bb * nu : prim + (size_t)bb * N * nz + nx;
        ScoreRecord r = rec[bb];
        double m = 0.0;
        for (int c = 0; c < nz; ++c) {
            const double z = c < nx ? xn[c] : u0[c - nx];
            const double d = z - (target ? target[p + c] : 0.0);
            const double wd = weight[p + c] * d;
            const double s = wd * d;
            r.cost = r.cost + s;
            const double over = hi ? z - hi[p + c] : -__builtin_huge_val(), under = lo ? lo[p + c] - z : -__builtin_huge_val();
            m = fmax(m, fmax(over, under));
        }
        if (m > 0.0) {
            r.worst = fmax(r.worst, m);
            r.violated_steps += 1;
            if (r.first_violation < 0) r.first_violation = step;
        }
        rec[bb] = r;
    }
}
int enqueue_coverage_score(TinyBatch* b, long step) {
    Score& s = b->score;
    const int k = (int)std::clamp<long>(step, -(1L << 30), 1L << 30);
    hipLaunchKernelGGL(coverage_score_kernel, dim3(helper_grid(b, (size_t)b->batch)), dim3(256), 0, b->stream, static_cast<ScoreRecord*>(s.rec), b->d_x0, b->d_prim,
                       b->act.last ? b->act.ua : nullptr, b->d_status,
                       s.src[0], s.src[1], s.src[2], s.src[3], s.kind == 2 ? 1 : 0, k, b->batch, b->nx, b->nu, b->N);
    HIP_TRY(b, hipGetLastError());
    return TINY_OK;
}

// ---- an actuator model between the command and the plant step (tiny_batch_set_actuator): the caller's lo | hi | alpha | gain | offset ->
// [setups][5][16 lanes], one thread per (setup, row, lane); what lands there: actuator_entry (lane_tables.hpp), nothing else
static __global__ __launch_bounds__(256) void fill_actuator_kernel(double* __restrict__ out, const double* __restrict__ lo, const double* __restrict__ hi,
                                                                   const double* __restrict__ alpha, const double* __restrict__ gain, const double* __restrict__ offset,
                                                                   int setups, int nx, int nu) {
    const size_t total = (size_t)setups * actuator_block_doubles();
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lane = (int)(e % 16), r = (int)((e / 16) % 5);
        const size_t g = e / actuator_block_doubles() * nu;
        out[e] = actuator_entry(lo ? lo + g : nullptr, hi ? hi + g : nullptr, alpha ? alpha + g : nullptr, gain ? gain + g : nullptr, offset ? offset + g : nullptr, nx, nu, r,
                                lane);
    }
}
// the record the PA forms read, written on the stream: the launches behind it see it, the ones in front of it have read theirs
static __global__ void write_actuator_launch_kernel(ActuatorLaunch* __restrict__ out, const ActuatorLaunch v) { *out = v; }
bool actuator_active(const TinyBatch* b) {
    return (b->act.kind != 0 || (b->anoise.seq && b->anoise.steps > 0)) && (b->advance_x0 || b->steps_per_launch > 1);
}
int actuation_step_base(const TinyBatch* b) { return (int)std::clamp<long>(b->anoise.step, -(1L << 30), 1L << 30); }
int begin_actuation_log(TinyBatch* b, int rows) {
    Actuator& s = b->act;
    s.log_rows = 0;
    if (!s.log_on) return TINY_OK;
    if (s.log_steps < rows) {
        if (s.log) { HIP_TRY(b, hipStreamSynchronize(b->stream)); (void)hipFree(s.log); }
        s.log = nullptr; s.log_steps = 0;
        HIP_TRY(b, hipMalloc(&s.log, (size_t)rows * b->batch * b->nu * sizeof(double)));
        s.log_steps = rows;
    }
    s.log_rows = rows;
    return TINY_OK;
}
// (only the one-row kernel's PA forms read the blocks and the record; the coverage path reads the caller's arrays)
int ensure_actuator_launch(TinyBatch* b, int rows, const ActuatorLaunch** out) {
    Actuator& s = b->act;
    if (s.kind && s.dirty) {
        const int setups = s.kind == 1 ? 1 : b->batch;
        const size_t total = (size_t)setups * actuator_block_doubles();
        if (!s.built) HIP_TRY(b, hipMalloc(&s.built, total * sizeof(double)));
        hipLaunchKernelGGL(fill_actuator_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.built, s.src[0], s.src[1], s.src[2], s.src[3], s.src[4], setups, b->nx,
                           b->nu);
        HIP_TRY(b, hipGetLastError());
        s.dirty = false;
    }
    if (int rc = begin_actuation_log(b, rows)) return rc;
    if (!s.desc) HIP_TRY(b, hipMalloc(&s.desc, sizeof(ActuatorLaunch)));
    ActuatorLaunch v = {};
    v.tab = s.kind ? reinterpret_cast<const double*>(reinterpret_cast<uintptr_t>(s.built) | (s.kind == 2 ? (uintptr_t)0 : (uintptr_t)1) | (s.lag ? (uintptr_t)2 : (uintptr_t)0)) : nullptr;
    v.state = s.lag ? s.state : nullptr;
    v.noise = b->anoise.seq; v.noise_steps = b->anoise.seq ? b->anoise.steps : 0;
    v.log = s.log_on ? s.log : nullptr; v.log_step0 = actuation_step_base(b);
    hipLaunchKernelGGL(write_actuator_launch_kernel, dim3(1), dim3(1), 0, b->stream, static_cast<ActuatorLaunch*>(s.desc), v);
    HIP_TRY(b, hipGetLastError());
    *out = static_cast<const ActuatorLaunch*>(s.desc);
    return TINY_OK;
}
// the coverage path's actuator behind one single-step launch: one thread per (instance, input), the four stages of tiny_batch_set_actuator
// in their stated order over the u0 of the x|u record -- what actuator_limits, actuator_lag, actuator_gain and plant_add do on the
// one-row kernel, same bits.  Writes ua [batch][nu], which the plant and score helpers behind it read in place of u0, the lag's record
// and the log's row.  An instance whose launch ran no iteration takes no plant step: no stage runs, its ua is never read
static __global__ __launch_bounds__(256) void coverage_actuator_kernel(double* __restrict__ ua, double* __restrict__ state, double* __restrict__ log_row,
                                                                       const double* __restrict__ prim, const int4* __restrict__ status, const double* __restrict__ lo,
                                                                       const double* __restrict__ hi, const double* __restrict__ alpha, const double* __restrict__ gain,
                                                                       const double* __restrict__ offset, int installed, int per_instance, const double* __restrict__ noise,
                                                                       int batch, int nx, int nu, int N) {
#pragma clang fp contract(off)
    const size_t total = (size_t)batch * nu;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % nu);
        const size_t bb = e / nu, p = per_instance ? e : (size_t)c;
        if (status[bb].x <= 0) continue;
        double v = prim[bb * N * (nx + nu) + nx + c];
        if (installed) {
            const double l = lo ? lo[p] : -__builtin_huge_val(), h = hi ? hi[p] : __builtin_huge_val();
            v = v < l ? l : (v > h ? h : v);
            if (alpha) {
                const double a = state[e], d = v - a;
                v = __builtin_fma(alpha[p], d, a);
                state[e] = v;
            }
            v = __builtin_fma(v, gain ? gain[p] : 1.0, offset ? offset[p] : -0.0);
        }
        if (noise) v = v + noise[e];
        ua[e] = v;
        if (log_row) log_row[e] = v;
    }
}
int enqueue_coverage_actuator(TinyBatch* b, long step, int log_row) {
    Actuator& s = b->act;
    const size_t total = (size_t)b->batch * b->nu;
    if (!s.ua) HIP_TRY(b, hipMalloc(&s.ua, total * sizeof(double)));
    const double* noise = (b->anoise.seq && step >= 0 && step < b->anoise.steps) ? b->anoise.seq + (size_t)step * total : nullptr;
    hipLaunchKernelGGL(coverage_actuator_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.ua, s.lag ? s.state : nullptr,
                       (s.log_on && s.log && log_row < s.log_rows) ? s.log + (size_t)log_row * total : nullptr, b->d_prim, b->d_status, s.src[0], s.src[1],
                       s.lag ? s.src[2] : nullptr, s.src[3], s.src[4], s.kind ? 1 : 0, s.kind == 2 ? 1 : 0, noise, b->batch, b->nx, b->nu, b->N);
    HIP_TRY(b, hipGetLastError());
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
    b->dist.last = disturbance_active(b);             // (the one-row and the coverage kernel both add it; decide_path keeps such a launch off the tile kernel)
    b->plant.log_rows = 0;                            // (the state log is the LAST solve call's: a launch that logs sizes it anew)
    b->meas.last = measurement_active(b);             // (the one-row kernel's PM forms, or the helper kernel in front of the coverage kernel)
    b->plant.last = plant_active(b);                  // (likewise: the one-row kernel's PP forms, or the helper kernel behind the coverage kernel)
    b->est.last = estimator_active(b);                // (likewise: the one-row kernel's PE forms, or the helper kernels around the coverage kernel)
    b->est.log_rows = 0;                              // (the estimate log is the LAST solve call's, as the state log)
    b->score.last = score_active(b);                  // (likewise: the one-row kernel's PS forms, or the helper kernel behind the coverage kernel)
    b->act.last = actuator_active(b);                 // (likewise: the one-row kernel's PA forms, or the helper kernel behind the coverage kernel)
    b->act.log_rows = 0;                              // (the actuation log is the LAST solve call's, as the state log)
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
// before is gone: its arrays were being overwritten) -- not transactional, unlike the other three: these are the largest arrays there are
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

// every instance its own additive disturbance at the plant step
int tiny_batch_set_disturbance(TinyBatch* b, const double* w, int n_steps, int flags) {
    if (!b) return TINY_ERR_NULL;
    return install_sequence(b, b->dist, w, n_steps, flags, "per-instance disturbance", "disturbance");
}
// measurement noise: what the solver sees of the state at MPC step k is fl(x0 + v[k][i]).  Removing it drops the model's plant block
// and the coverage path's scratch array with it (both are made again by the launch that needs them)
int tiny_batch_set_measurement_noise(TinyBatch* b, const double* v, int n_steps, int flags) {
    if (!b) return TINY_ERR_NULL;
    return install_sequence(b, b->meas, v, n_steps, flags, "measurement noise", "measurement noise");
}
int tiny_batch_get_measurement_noise(TinyBatch* b, int step, int instance, double* v_out) {
    if (!b) return TINY_ERR_NULL;
    return read_sequence_row(b, b->meas, step, instance, v_out, "no measurement-noise sequence installed");
}
// the same two sequences generated on the device from a seed (noise_gen.hpp); installed as the setters install a caller's
int tiny_batch_generate_disturbance(TinyBatch* b, const TinyNoiseSpec* spec) {
    if (!b) return TINY_ERR_NULL;
    return install_generated(b, b->dist, spec, 0, "generated disturbance");
}
int tiny_batch_generate_measurement_noise(TinyBatch* b, const TinyNoiseSpec* spec) {
    if (!b) return TINY_ERR_NULL;
    return install_generated(b, b->meas, spec, 1, "generated measurement noise");
}
// the rows on the host, no GPU touched: out [n_steps][batch][nx] exactly as the device fills them
int tiny_noise_generate(const TinyNoiseSpec* spec, int stream, int batch, int nx, double* out) {
    if (noise_spec_refusal(spec, nx) || (spec->flags & TINY_DEVICE) || !out || batch <= 0 || nx <= 0 || (stream != 0 && stream != 1)) return TINY_ERR_ARG;
    std::vector<double> g((size_t)2 * noise_pairs(nx));
    noise_fill_host(noise_fill_of(spec, stream, batch, nx, spec->scale, spec->mean), out, g.data());
    return TINY_OK;
}
// row `step` of instance `instance`, as set: w_out [nx]
int tiny_batch_get_disturbance(TinyBatch* b, int step, int instance, double* w_out) {
    if (!b) return TINY_ERR_NULL;
    return read_sequence_row(b, b->dist, step, instance, w_out, "no disturbance sequence installed");
}

// a plant of its own at the plant step: A_p [batch][nx*nx], B_p [batch][nx*nu], f_p [batch][nx] or null (TINY_BROADCAST: one of each),
// kept on the device as given; the blocks the one-row kernel reads are built from them in front of the next launch (ensure_plant).
// Everything that can fail happens before anything installed is touched
int tiny_batch_set_plant(TinyBatch* b, const double* A_p, const double* B_p, const double* f_p, int flags) {
    if (!b) return TINY_ERR_NULL;
    HIP_TRY(b, hipSetDevice(b->device));
    PlantStep& s = b->plant;
    if (A_p && !B_p) return fail(b, TINY_ERR_ARG, "plant: A_p without B_p");
    double* fresh[3] = {nullptr, nullptr, nullptr};
    if (A_p) {
        const size_t plants = (flags & TINY_BROADCAST) ? 1 : (size_t)b->batch;
        const UploadPart parts[3] = {{A_p, plants * b->nx * b->nx}, {B_p, plants * b->nx * b->nu}, {f_p, plants * b->nx}};
        if (int rc = upload_fresh(b, parts, fresh, 3, flags, "plant")) return rc;
    } else if (s.kind) HIP_TRY(b, hipStreamSynchronize(b->stream));       // remove: freed once the stream has run dry of its readers
    for (int i = 0; i < 3; ++i) { if (s.src[i]) (void)hipFree(s.src[i]); s.src[i] = fresh[i]; }
    if (s.built) (void)hipFree(s.built);                                 // (its size follows the kind; the state log and `next` stay)
    s.built = nullptr;
    s.kind = !A_p ? 0 : (flags & TINY_BROADCAST) ? 1 : 2;
    s.dirty = s.kind != 0;
    return TINY_OK;
}
// the plant instance `instance` is stepped by, as set: A_p [nx*nx], B_p [nx*nu], f_p [nx] (zero where none was given); any pointer may be NULL
int tiny_batch_get_plant(TinyBatch* b, int instance, double* A_p, double* B_p, double* f_p) {
    if (!b) return TINY_ERR_NULL;
    if (!b->plant.kind) return fail(b, TINY_ERR_ARG, "no plant installed");
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    double* dst[3] = {A_p, B_p, f_p};
    const size_t n[3] = {(size_t)b->nx * b->nx, (size_t)b->nx * b->nu, (size_t)b->nx};
    for (int i = 0; i < 3; ++i) {
        if (!dst[i]) continue;
        if (b->plant.src[i]) { if (int rc = read_instance(b, dst[i], b->plant.src[i], b->plant.kind == 2 ? instance : 0, n[i])) return rc; }
        else std::fill(dst[i], dst[i] + n[i], 0.0);
    }
    return TINY_OK;
}
// the x0 every MPC step of the last solve call handed on (option "state_log"): x0_next [steps][batch][nx]
int tiny_batch_get_state_log(TinyBatch* b, double* x0_next, int steps) {
    if (!b) return TINY_ERR_NULL;
    if (steps <= 0 || steps > b->plant.log_rows || !b->plant.log) return fail(b, TINY_ERR_ARG, "no state log recorded (set_option state_log; advance_x0 or steps_per_launch)");
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if (x0_next) HIP_TRY(b, hipMemcpy(x0_next, b->plant.log, (size_t)steps * b->batch * b->nx * sizeof(double), hipMemcpyDeviceToHost));
    return TINY_OK;
}

// a state estimator between the measurement and the solve: M [batch][nx*nx] column-major (TINY_BROADCAST: one), kept on the device as
// given; the blocks the one-row kernel reads are built from it in front of the next launch (ensure_estimator_blocks).  Installing one
// where none is installed starts the estimate record at the x0 record as it stands; replacing the gain keeps it.  Everything that can
// fail happens before anything installed is touched
int tiny_batch_set_estimator(TinyBatch* b, const double* M, int flags) {
    if (!b) return TINY_ERR_NULL;
    HIP_TRY(b, hipSetDevice(b->device));
    Estimator& s = b->est;
    if (!M) {                                                            // remove: freed once the stream has run dry of its readers
        if (s.kind) { if (int rc = drop_buffers(b, s)) return rc; }
        s.kind = 0; s.dirty = false; s.log_steps = 0; s.log_rows = 0;
        return TINY_OK;
    }
    const size_t gains = (flags & TINY_BROADCAST) ? 1 : (size_t)b->batch, row = (size_t)b->batch * b->nx;
    const UploadPart given = {M, gains * b->nx * b->nx};
    double *fresh = nullptr, *xp = nullptr;
    if (int rc = upload_fresh(b, &given, &fresh, 1, flags, "estimator gain")) return rc;
    if (!s.kind) {                                                       // (the estimate starts at what x0 holds now)
        hipError_t err = hipMalloc(&xp, row * sizeof(double));
        if (err == hipSuccess) err = hipMemcpyAsync(xp, b->d_x0, row * sizeof(double), hipMemcpyDeviceToDevice, b->stream);
        if (err == hipSuccess) err = hipStreamSynchronize(b->stream);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            if (xp) (void)hipFree(xp);
            (void)hipFree(fresh);
            return fail(b, TINY_ERR_HIP, "estimator: %s", hipGetErrorString(err));
        }
        s.xp = xp;
    }
    if (s.src) (void)hipFree(s.src);
    if (s.built) (void)hipFree(s.built);                                 // (its size follows the kind; the estimate, the log and `xhat` stay)
    s.src = fresh; s.built = nullptr;
    s.kind = (flags & TINY_BROADCAST) ? 1 : 2;
    s.dirty = true;
    return TINY_OK;
}
// the gain instance `instance` is corrected by, as set: M_out [nx*nx]
int tiny_batch_get_estimator(TinyBatch* b, int instance, double* M_out) {
    if (!b) return TINY_ERR_NULL;
    if (!b->est.kind) return fail(b, TINY_ERR_ARG, "no estimator installed");
    if (!M_out) return fail(b, TINY_ERR_ARG, "null output");
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    return read_instance(b, M_out, b->est.src, b->est.kind == 2 ? instance : 0, (size_t)b->nx * b->nx);
}
// the predicted estimate: xp [batch][nx] (TINY_BROADCAST: one [nx] for all, expanded on the device).  The fresh record is complete
// before it takes the place of the one installed
int tiny_batch_set_estimate(TinyBatch* b, const double* xp, int flags) {
    if (!b) return TINY_ERR_NULL;
    if (!b->est.kind) return fail(b, TINY_ERR_ARG, "no estimator installed (tiny_batch_set_estimator)");
    if (!xp) return fail(b, TINY_ERR_ARG, "null estimate");
    HIP_TRY(b, hipSetDevice(b->device));
    const size_t row = (size_t)b->batch * b->nx;
    const UploadPart given = {xp, (flags & TINY_BROADCAST) ? (size_t)b->nx : row};
    double* fresh = nullptr;
    if (int rc = upload_fresh(b, &given, &fresh, 1, flags, "estimate")) return rc;
    if (flags & TINY_BROADCAST) {
        double* full = nullptr;
        hipError_t err = hipMalloc(&full, row * sizeof(double));
        int rc = TINY_OK;
        if (err == hipSuccess) rc = expand_disturbance(b, full, fresh, 1, b->nx);
        if (err == hipSuccess && rc == TINY_OK) err = hipStreamSynchronize(b->stream);
        (void)hipFree(fresh);
        if (err != hipSuccess || rc != TINY_OK) {
            (void)hipGetLastError();
            if (full) (void)hipFree(full);
            return rc != TINY_OK ? rc : fail(b, TINY_ERR_HIP, "estimate: %s", hipGetErrorString(err));
        }
        fresh = full;
    }
    if (b->est.xp) (void)hipFree(b->est.xp);
    b->est.xp = fresh;
    return TINY_OK;
}
int tiny_batch_get_estimate(TinyBatch* b, double* xp_out) {
    if (!b) return TINY_ERR_NULL;
    if (!b->est.kind) return fail(b, TINY_ERR_ARG, "no estimator installed (tiny_batch_set_estimator)");
    if (!xp_out) return fail(b, TINY_ERR_ARG, "null output");
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(xp_out, b->est.xp, (size_t)b->batch * b->nx * sizeof(double), hipMemcpyDeviceToHost));
    return TINY_OK;
}
// the xhat every MPC step of the last solve call solved from (option "estimate_log"): xhat [steps][batch][nx]
int tiny_batch_get_estimate_log(TinyBatch* b, double* xhat, int steps) {
    if (!b) return TINY_ERR_NULL;
    if (steps <= 0 || steps > b->est.log_rows || !b->est.log) return fail(b, TINY_ERR_ARG, "no estimate log recorded (set_option estimate_log; tiny_batch_set_estimator; advance_x0 or steps_per_launch)");
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if (xhat) HIP_TRY(b, hipMemcpy(xhat, b->est.log, (size_t)steps * b->batch * b->nx * sizeof(double), hipMemcpyDeviceToHost));
    return TINY_OK;
}

// a closed-loop score at the plant step: weight | target | lo | hi [batch][nx+nu] (TINY_BROADCAST: one [nx+nu] each), kept on the device
// as given; the blocks the one-row kernel reads are built from them in front of the next launch (ensure_score_blocks).  Installing or
// replacing zeroes the record and rewinds the counter.  Everything that can fail happens before anything installed is touched
int tiny_batch_set_score(TinyBatch* b, const double* weight, const double* target, const double* lo, const double* hi, int flags) {
    if (!b) return TINY_ERR_NULL;
    HIP_TRY(b, hipSetDevice(b->device));
    Score& s = b->score;
    if (flags & ~(TINY_DEVICE | TINY_BROADCAST)) return fail(b, TINY_ERR_ARG, "score: flags 0x%x (TINY_HOST or TINY_DEVICE, with or without TINY_BROADCAST)", flags);
    if (!weight) {                                                       // remove: freed once the stream has run dry of its readers
        if (s.kind) { if (int rc = drop_buffers(b, s)) return rc; }
        s.kind = 0; s.dirty = false; s.step = 0;
        return TINY_OK;
    }
    const size_t nz = (size_t)b->nx + b->nu, doubles = ((flags & TINY_BROADCAST) ? 1 : (size_t)b->batch) * nz;
    const UploadPart given[4] = {{weight, doubles}, {target, doubles}, {lo, doubles}, {hi, doubles}};
    double* fresh[4];
    void* rec = s.rec;
    if (!rec) {
        if (hipMalloc(&rec, (size_t)b->batch * sizeof(ScoreRecord)) != hipSuccess) { (void)hipGetLastError(); return fail(b, TINY_ERR_HIP, "score record: out of device memory"); }
    }
    if (int rc = upload_fresh(b, given, fresh, 4, flags, "score setup")) { if (!s.rec) (void)hipFree(rec); return rc; }
    for (int i = 0; i < 4; ++i) { if (s.src[i]) (void)hipFree(s.src[i]); s.src[i] = fresh[i]; }
    if (s.built) (void)hipFree(s.built);                                 // (its size follows the kind)
    s.built = nullptr; s.rec = rec;
    s.kind = (flags & TINY_BROADCAST) ? 1 : 2;
    s.dirty = true; s.step = 0;
    return enqueue_zero_score(b, s.rec);
}
// the setup instance `instance` is scored by, as set (a null target reads as zeros, null limits as -inf / +inf); any output may be null
int tiny_batch_get_score_setup(TinyBatch* b, int instance, double* weight, double* target, double* lo, double* hi) {
    if (!b) return TINY_ERR_NULL;
    const Score& s = b->score;
    if (!s.kind) return fail(b, TINY_ERR_ARG, "no score installed");
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    const size_t nz = (size_t)b->nx + b->nu;
    double* const out[4] = {weight, target, lo, hi};
    const double none[4] = {0.0, 0.0, -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()};
    for (int i = 0; i < 4; ++i) {
        if (!out[i]) continue;
        if (!s.src[i]) { std::fill(out[i], out[i] + nz, none[i]); continue; }
        if (int rc = read_instance(b, out[i], s.src[i], s.kind == 2 ? instance : 0, nz)) return rc;
    }
    return TINY_OK;
}
// the record: cost, worst [batch] doubles, violated_steps, first_violation [batch] ints, on the host; any may be null
int tiny_batch_get_score(TinyBatch* b, double* cost, double* worst, int* violated_steps, int* first_violation) {
    if (!b) return TINY_ERR_NULL;
    if (!b->score.kind) return fail(b, TINY_ERR_ARG, "no score installed (tiny_batch_set_score)");
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    std::vector<ScoreRecord> h((size_t)b->batch);
    HIP_TRY(b, hipMemcpy(h.data(), b->score.rec, h.size() * sizeof(ScoreRecord), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < h.size(); ++i) {
        if (cost) cost[i] = h[i].cost;
        if (worst) worst[i] = h[i].worst;
        if (violated_steps) violated_steps[i] = h[i].violated_steps;
        if (first_violation) first_violation[i] = h[i].first_violation;
    }
    return TINY_OK;
}
// the record zeroed and the counter rewound; the setup stays
int tiny_batch_reset_score(TinyBatch* b) {
    if (!b) return TINY_ERR_NULL;
    if (!b->score.kind) return fail(b, TINY_ERR_ARG, "no score installed (tiny_batch_set_score)");
    HIP_TRY(b, hipSetDevice(b->device));
    b->score.step = 0;
    return enqueue_zero_score(b, b->score.rec);
}

// an actuator model between the command and the plant step: lo | hi | alpha | gain | offset [batch][nu] (TINY_BROADCAST: one [nu] each),
// any may be null, kept on the device as given; the blocks the one-row kernel reads are built from them in front of the next launch
// (ensure_actuator_launch).  Installing a lag where none was installed zeroes its record; replacing the setup keeps it.  Everything that
// can fail -- the limits' check among it -- happens before anything installed is touched
int tiny_batch_set_actuator(TinyBatch* b, const double* lo, const double* hi, const double* alpha, const double* gain, const double* offset, int flags) {
    if (!b) return TINY_ERR_NULL;
    HIP_TRY(b, hipSetDevice(b->device));
    Actuator& s = b->act;
    if (flags & ~(TINY_DEVICE | TINY_BROADCAST)) return fail(b, TINY_ERR_ARG, "actuator: flags 0x%x (TINY_HOST or TINY_DEVICE, with or without TINY_BROADCAST)", flags);
    if (!lo && !hi && !alpha && !gain && !offset) {                      // remove: freed once the stream has run dry of its readers (the log goes with it)
        if (int rc = drop_buffers(b, s)) return rc;
        s.kind = 0; s.lag = false; s.dirty = false; s.log_steps = 0; s.log_rows = 0;
        return TINY_OK;
    }
    const size_t doubles = ((flags & TINY_BROADCAST) ? 1 : (size_t)b->batch) * b->nu;
    const UploadPart given[5] = {{lo, doubles}, {hi, doubles}, {alpha, doubles}, {gain, doubles}, {offset, doubles}};
    double* fresh[5];
    if (int rc = upload_fresh(b, given, fresh, 5, flags, "actuator setup")) return rc;
    auto give_up = [&](int rc) { for (double* p : fresh) if (p) (void)hipFree(p); return rc; };
    if (lo && hi) {                                                      // (read back: the arrays may be the device's)
        std::vector<double> l(doubles), h(doubles);
        if (hipMemcpy(l.data(), fresh[0], doubles * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h.data(), fresh[1], doubles * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) {
            (void)hipGetLastError();
            return give_up(fail(b, TINY_ERR_HIP, "actuator setup: the limits could not be read back"));
        }
        for (size_t i = 0; i < doubles; ++i)
            if (l[i] > h[i]) return give_up(fail(b, TINY_ERR_ARG, "actuator: lo > hi at input %d of setup %zu", (int)(i % b->nu), i / b->nu));
    }
    double* state = s.state;
    if (alpha && !s.lag) {                                               // a lag where none was installed: its record starts at zero
        if (state) { (void)hipFree(state); state = nullptr; }
        hipError_t err = hipMalloc(&state, (size_t)b->batch * b->nu * sizeof(double));
        if (err == hipSuccess) err = hipMemsetAsync(state, 0, (size_t)b->batch * b->nu * sizeof(double), b->stream);
        if (err != hipSuccess) { (void)hipGetLastError(); if (state) (void)hipFree(state); s.state = nullptr; return give_up(fail(b, TINY_ERR_HIP, "actuator state: %s", hipGetErrorString(err))); }
    }
    for (int i = 0; i < 5; ++i) { if (s.src[i]) (void)hipFree(s.src[i]); s.src[i] = fresh[i]; }
    if (s.built) (void)hipFree(s.built);                                 // (its size follows the kind)
    s.built = nullptr; s.state = state;
    s.kind = (flags & TINY_BROADCAST) ? 1 : 2;
    s.lag = alpha != nullptr; s.dirty = true;
    return TINY_OK;
}
// the setup instance `instance` is actuated by, as set, defaults filled in (alpha reads 1 with no lag); any output may be null
int tiny_batch_get_actuator(TinyBatch* b, int instance, double* lo, double* hi, double* alpha, double* gain, double* offset) {
    if (!b) return TINY_ERR_NULL;
    const Actuator& s = b->act;
    if (!s.kind) return fail(b, TINY_ERR_ARG, "no actuator installed");
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    double* const out[5] = {lo, hi, alpha, gain, offset};
    const double none[5] = {-std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(), 1.0, 1.0, -0.0};
    for (int i = 0; i < 5; ++i) {
        if (!out[i]) continue;
        if (!s.src[i]) { std::fill(out[i], out[i] + b->nu, none[i]); continue; }
        if (int rc = read_instance(b, out[i], s.src[i], s.kind == 2 ? instance : 0, b->nu)) return rc;
    }
    return TINY_OK;
}
// the lag's record a [batch][nu] (TINY_BROADCAST: [nu]); TINY_ERR_ARG with no lag installed
int tiny_batch_set_actuator_state(TinyBatch* b, const double* a, int flags) {
    if (!b) return TINY_ERR_NULL;
    if (!b->act.kind || !b->act.lag) return fail(b, TINY_ERR_ARG, "no actuator lag installed (tiny_batch_set_actuator with alpha)");
    if (!a) return fail(b, TINY_ERR_ARG, "null actuator state");
    if (flags & ~(TINY_DEVICE | TINY_BROADCAST)) return fail(b, TINY_ERR_ARG, "actuator state: flags 0x%x (TINY_HOST or TINY_DEVICE, with or without TINY_BROADCAST)", flags);
    HIP_TRY(b, hipSetDevice(b->device));
    const hipMemcpyKind kind = (flags & TINY_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (!(flags & TINY_BROADCAST)) {
        HIP_TRY(b, hipMemcpyAsync(b->act.state, a, (size_t)b->batch * b->nu * sizeof(double), kind, b->stream));
    } else {                                                             // one row for all: staged and expanded, as a broadcast sequence of one step
        double* stage = nullptr;
        HIP_TRY(b, hipMalloc(&stage, (size_t)b->nu * sizeof(double)));
        hipError_t err = hipMemcpyAsync(stage, a, (size_t)b->nu * sizeof(double), kind, b->stream);
        int rc = TINY_OK;
        if (err == hipSuccess) rc = expand_disturbance(b, b->act.state, stage, 1, b->nu);
        if (err == hipSuccess && rc == TINY_OK) err = hipStreamSynchronize(b->stream);
        (void)hipFree(stage);
        if (rc != TINY_OK) return rc;
        if (err != hipSuccess) { (void)hipGetLastError(); return fail(b, TINY_ERR_HIP, "actuator state: %s", hipGetErrorString(err)); }
        return TINY_OK;
    }
    HIP_TRY(b, hipStreamSynchronize(b->stream));                         // (the caller may free its array)
    return TINY_OK;
}
int tiny_batch_get_actuator_state(TinyBatch* b, double* a_out) {
    if (!b) return TINY_ERR_NULL;
    if (!b->act.kind || !b->act.lag) return fail(b, TINY_ERR_ARG, "no actuator lag installed (tiny_batch_set_actuator with alpha)");
    if (!a_out) return fail(b, TINY_ERR_ARG, "null output");
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(a_out, b->act.state, (size_t)b->batch * b->nu * sizeof(double), hipMemcpyDeviceToHost));
    return TINY_OK;
}
// actuation noise: the applied control of MPC step k takes fl(g + n[k][i]) for its last stage; the disturbance setter's rules, width nu
int tiny_batch_set_actuation_noise(TinyBatch* b, const double* n, int n_steps, int flags) {
    if (!b) return TINY_ERR_NULL;
    return install_sequence(b, b->anoise, n, n_steps, flags, "actuation noise", "actuation noise", b->nu);
}
int tiny_batch_get_actuation_noise(TinyBatch* b, int step, int instance, double* n_out) {
    if (!b) return TINY_ERR_NULL;
    return read_sequence_row(b, b->anoise, step, instance, n_out, "no actuation-noise sequence installed", b->nu);
}
// ... generated on the device from a seed (noise_gen.hpp): stream 2, rows of nu entries
int tiny_batch_generate_actuation_noise(TinyBatch* b, const TinyNoiseSpec* spec) {
    if (!b) return TINY_ERR_NULL;
    return install_generated(b, b->anoise, spec, 2, "generated actuation noise", b->nu);
}
// ... and its rows on the host, no GPU touched: out [n_steps][batch][nu] exactly as the device fills them
int tiny_actuation_noise_generate(const TinyNoiseSpec* spec, int batch, int nu, double* out) {
    if (noise_spec_refusal(spec, nu) || (spec->flags & TINY_DEVICE) || !out || batch <= 0 || nu <= 0) return TINY_ERR_ARG;
    std::vector<double> g((size_t)2 * noise_pairs(nu));
    noise_fill_host(noise_fill_of(spec, 2, batch, nu, spec->scale, spec->mean), out, g.data());
    return TINY_OK;
}
// the applied control of every MPC step of the last solve call (option "actuation_log"): ua [steps][batch][nu]
int tiny_batch_get_actuation_log(TinyBatch* b, double* ua, int steps) {
    if (!b) return TINY_ERR_NULL;
    if (steps <= 0 || steps > b->act.log_rows || !b->act.log) return fail(b, TINY_ERR_ARG, "no actuation log recorded (set_option actuation_log; an actuator or actuation noise; advance_x0 or steps_per_launch)");
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if (ua) HIP_TRY(b, hipMemcpy(ua, b->act.log, (size_t)steps * b->batch * b->nu * sizeof(double), hipMemcpyDeviceToHost));
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
