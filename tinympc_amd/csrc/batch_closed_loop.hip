// batch_closed_loop.hip -- the stages at the fused closed-loop plant step: a per-instance disturbance, a plant of its own with the state
// log, measurement noise, a state estimator, a closed-loop score, an actuator model with actuation noise (the state: closed_loop.hpp).
// Per stage: the C ABI setter and getter, the fill kernel that turns the caller's arrays into the lane block the one-row kernel reads
// (fill rules: lane_tables.hpp) and the helper kernel that does the stage's work around a single-step launch of the coverage kernel.
// What a launch does with the stages stands at the end, one hook per place it touches them (declared in batch_dispatch.hpp); the
// sequences shared with batch_instance.hip -- upload_fresh, drop_buffers, read_instance, helper_grid -- are declared there too.
#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"
#include "noise_gen.hpp"

#include <algorithm>
#include <limits>

namespace tinympc_amd {

// ---- what the stages share ---------------------------------------------------------------------------------------------------
// a stage applies to a launch that takes a plant step: advance_x0, or fused steps
static bool takes_plant_step(const TinyBatch* b) { return b->advance_x0 || b->steps_per_launch > 1; }
// a lane block (the plant's, the model's, the gain's, the score's, the actuator's): allocated where missing, then filled on the batch's
// stream -- fill(grid) launches the stage's fill kernel -- and marked up to date
template <class Fill>
static int ensure_built(TinyBatch* b, double*& built, bool& dirty, size_t doubles, Fill fill) {
    if (!built) HIP_TRY(b, hipMalloc(&built, doubles * sizeof(double)));
    fill(dim3(helper_grid(b, doubles)));
    HIP_TRY(b, hipGetLastError());
    dirty = false;
    return TINY_OK;
}
// a stage's setup as set, for one instance: out[i] <- width[i] doubles of src[i] (kind 2: the instance's own, else the one set), or the
// default where the caller gave no array; any output may be null
template <int N>
static int read_setup(TinyBatch* b, double* const (&src)[N], int kind, int instance, const size_t (&width)[N], const double (&defaults)[N], double* const (&out)[N]) {
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    for (int i = 0; i < N; ++i) {
        if (!out[i]) continue;
        if (!src[i]) { std::fill(out[i], out[i] + width[i], defaults[i]); continue; }
        if (int rc = read_instance(b, out[i], src[i], kind == 2 ? instance : 0, width[i])) return rc;
    }
    return TINY_OK;
}
// room for `rows` rows of `width` entries per instance, none written yet (the caller has looked at log.on)
static int begin_log(TinyBatch* b, StepLog& log, int rows, int width) {
    log.rows = 0;
    if (log.capacity < rows) {
        if (log.buf) { HIP_TRY(b, hipStreamSynchronize(b->stream)); (void)hipFree(log.buf); }
        log.buf = nullptr; log.capacity = 0;
        HIP_TRY(b, hipMalloc(&log.buf, (size_t)rows * b->batch * width * sizeof(double)));
        log.capacity = rows;
    }
    log.rows = rows;
    return TINY_OK;
}
// the first `steps` rows of the last solve call's log, on the host (out may be null: the check alone); `none`: the text with no such rows
static int read_log(TinyBatch* b, const StepLog& log, double* out, int steps, int width, const char* none) {
    if (steps <= 0 || steps > log.rows || !log.buf) return fail(b, TINY_ERR_ARG, "%s", none);
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    if (out) HIP_TRY(b, hipMemcpy(out, log.buf, (size_t)steps * b->batch * width * sizeof(double), hipMemcpyDeviceToHost));
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
// layout), copied into s.seq with its counter rewound -- the disturbance and the measurement noise, and with rows of `width` = nu
// entries the actuation noise (0: nx).  Everything that can fail happens before anything installed is touched
static int install_sequence(TinyBatch* b, StepSequence& s, const double* w, int n_steps, int flags, const char* what, const char* what_short, int width = 0) {
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
static int install_generated(TinyBatch* b, StepSequence& s, const TinyNoiseSpec* spec, int stream, const char* what, int width = 0) {
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
static int read_sequence_row(TinyBatch* b, const StepSequence& s, int step, int instance, double* out, const char* none, int width = 0) {
    if (width <= 0) width = b->nx;
    if (!out) return fail(b, TINY_ERR_ARG, "null output");
    if (!s.seq) return fail(b, TINY_ERR_ARG, "%s", none);
    if (step < 0 || step >= s.steps) return fail(b, TINY_ERR_ARG, "step %d of %d", step, s.steps);
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    return read_instance(b, out, s.seq + (size_t)step * b->batch * width, instance, width);
}
static bool disturbance_active(const TinyBatch* b) { return b->dist.seq && b->dist.steps > 0 && takes_plant_step(b); }

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
static bool plant_active(const TinyBatch* b) { return b->plant.kind != 0 && takes_plant_step(b); }
static bool state_log_active(const TinyBatch* b) { return b->plant.log.on && takes_plant_step(b); }
static bool measurement_active(const TinyBatch* b) { return b->meas.seq && b->meas.steps > 0 && takes_plant_step(b); }
// what a launch steps the state by: the plant installed, else -- a launch under measurement noise, which always goes through a plant
// block -- the batch's own model: every instance's own A | B | f of a tiny_batch_setup_hetero batch, or the shared family's (uploaded once)
struct PlantSource { const double* src[3]; bool per_instance; double* const* built; };
// (the model alone: what a state estimator predicts by, whatever plant is installed)
static PlantSource model_source(const TinyBatch* b) {
    if (b->hetero) return {{b->d_hA, b->d_hB, b->d_hf}, true, &b->model.built};
    return {{b->model.src[0], b->model.src[1], b->model.src[2]}, false, &b->model.built};
}
static PlantSource plant_source(const TinyBatch* b) {
    if (b->plant.kind) return {{b->plant.src[0], b->plant.src[1], b->plant.src[2]}, b->plant.kind == 2, &b->plant.built};
    return model_source(b);
}
static int ensure_model_source(TinyBatch* b, bool under_a_plant = false) {
    if ((b->plant.kind && !under_a_plant) || b->hetero || b->model.src[0]) return TINY_OK;
    const UploadPart parts[3] = {{b->A.a.data(), b->A.a.size()}, {b->B.a.data(), b->B.a.size()}, {b->f.a.data(), b->f.a.size()}};
    return upload_fresh(b, parts, b->model.src, 3, TINY_HOST, "model as plant");
}
static const double* block_pointer(const PlantSource& p) { return tagged_block(*p.built, !p.per_instance); }
// (only the one-row kernel's PP forms read the blocks: the launch that binds one asks for them -- a launch without a plant step, and
// the coverage path, which reads the caller's arrays, build and read no block.  Under measurement noise with no plant installed the
// arrays are the model's: a shared family's A | B | f are uploaded once, by whichever path asks first: ensure_model_source)
// the model's own block, made once -- with no plant installed what the PP forms step by, and under a state estimator what predicts,
// next to whatever plant is installed
static int ensure_model_block(TinyBatch* b) {
    if (b->model.built) return TINY_OK;
    if (int rc = ensure_model_source(b, true)) return rc;
    const PlantSource p = model_source(b);
    const int plants = p.per_instance ? b->batch : 1;
    bool missing = true;
    return ensure_built(b, b->model.built, missing, (size_t)plants * plant_block_doubles(b->nx, b->nu), [&](dim3 grid) {
        hipLaunchKernelGGL(fill_plant_kernel, grid, dim3(256), 0, b->stream, b->model.built, p.src[0], p.src[1], p.src[2], plants, b->nx, b->nu);
    });
}
static int ensure_plant_blocks(TinyBatch* b) {
    PlantStep& s = b->plant;
    if (!s.kind) return ensure_model_block(b);        // (no plant installed: the model's own block)
    if (!s.dirty) return TINY_OK;
    const int plants = s.kind == 1 ? 1 : b->batch;
    return ensure_built(b, s.built, s.dirty, (size_t)plants * plant_block_doubles(b->nx, b->nu), [&](dim3 grid) {
        hipLaunchKernelGGL(fill_plant_kernel, grid, dim3(256), 0, b->stream, s.built, s.src[0], s.src[1], s.src[2], plants, b->nx, b->nu);
    });
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
static int enqueue_coverage_plant_step(TinyBatch* b, const double* dist_block) {
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
static int enqueue_coverage_measurement(TinyBatch* b, long step, const double** x0_of_launch) {
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
static int enqueue_state_log_row(TinyBatch* b, int row) {
    const size_t total = (size_t)b->batch * b->nx;
    HIP_TRY(b, hipMemcpyAsync(b->plant.log.buf + (size_t)row * total, b->d_x0, total * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
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
static bool estimator_active(const TinyBatch* b) { return b->est.kind != 0 && takes_plant_step(b); }
// (only the one-row kernel's PE forms read the blocks; the coverage path reads the caller's array and the model's arrays)
static int ensure_estimator_blocks(TinyBatch* b) {
    Estimator& s = b->est;
    if (int rc = ensure_model_block(b)) return rc;
    if (!s.kind || !s.dirty) return TINY_OK;
    const int gains = s.kind == 1 ? 1 : b->batch;
    return ensure_built(b, s.built, s.dirty, (size_t)gains * gain_block_doubles(b->nx), [&](dim3 grid) {
        hipLaunchKernelGGL(fill_gain_kernel, grid, dim3(256), 0, b->stream, s.built, s.src, gains, b->nx);
    });
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
static int enqueue_coverage_correction(TinyBatch* b, int log_row, const double** x0_of_launch) {
    Estimator& s = b->est;
    const size_t total = (size_t)b->batch * b->nx;
    if (!s.xhat) HIP_TRY(b, hipMalloc(&s.xhat, total * sizeof(double)));
    double* const log = (s.log.buf && log_row < s.log.rows) ? s.log.buf + (size_t)log_row * total : nullptr;
    hipLaunchKernelGGL(coverage_correction_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.xhat, log, *x0_of_launch, s.xp, s.src, s.kind == 2 ? 1 : 0,
                       b->batch, b->nx);
    HIP_TRY(b, hipGetLastError());
    *x0_of_launch = s.xhat;
    return TINY_OK;
}
// ... and its prediction behind the launch: xp <- the MODEL's step from xhat and the u0 of the x|u record, the chain of
// coverage_plant_step_kernel.  xhat and xp are arrays of their own: a thread may write its xp while others still read xhat.  An instance
// whose launch ran no iteration keeps its xp.  s0: null, or [batch][nu] -- under delay compensation the control that reaches the actuator
// now (what the actuator helper took off the queue), read in place of the record's u0
static __global__ __launch_bounds__(256) void coverage_prediction_kernel(double* __restrict__ xp, const double* __restrict__ xhat, const double* __restrict__ prim,
                                                                         const double* __restrict__ s0,
                                                                         const int4* __restrict__ status, const double* __restrict__ A_m, const double* __restrict__ B_m,
                                                                         const double* __restrict__ f_m, int per_instance, int batch, int nx, int nu, int N) {
    const size_t total = (size_t)batch * nx;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(e % nx);
        const size_t bb = e / nx, p = per_instance ? bb : 0;
        if (status[bb].x <= 0) continue;
        const double *A = A_m + p * nx * nx, *B = B_m + p * nx * nu, *u0 = s0 ? s0 + bb * nu : prim + bb * N * (nx + nu) + nx;
        double acc = f_m ? f_m[p * nx + j] : 0.0;
        for (int k = 0; k < nx; ++k) acc = fma(xhat[bb * nx + k], A[j + nx * k], acc);
        for (int k = 0; k < nu; ++k) acc = fma(u0[k], B[j + nx * k], acc);
        xp[e] = acc;
    }
}
static int enqueue_coverage_prediction(TinyBatch* b, const double* s0 = nullptr) {
    Estimator& s = b->est;
    if (int rc = ensure_model_source(b, true)) return rc;
    const PlantSource p = model_source(b);
    const size_t total = (size_t)b->batch * b->nx;
    hipLaunchKernelGGL(coverage_prediction_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.xp, s.xhat, b->d_prim, s0, b->d_status, p.src[0], p.src[1], p.src[2],
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
static bool score_active(const TinyBatch* b) { return b->score.kind != 0 && takes_plant_step(b); }
// (only the one-row kernel's PS forms read the blocks; the coverage path reads the caller's arrays)
static int ensure_score_blocks(TinyBatch* b) {
    Score& s = b->score;
    if (!s.kind || !s.dirty) return TINY_OK;
    const int setups = s.kind == 1 ? 1 : b->batch;
    return ensure_built(b, s.built, s.dirty, (size_t)setups * score_block_doubles(), [&](dim3 grid) {
        hipLaunchKernelGGL(fill_score_kernel, grid, dim3(256), 0, b->stream, s.built, s.src[0], s.src[1], s.src[2], s.src[3], setups, b->nx, b->nu);
    });
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
static int enqueue_coverage_score(TinyBatch* b, long step) {
    Score& s = b->score;
    const int k = kernel_step(step);
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
// ... and the part the PQ / PX forms read behind it (Actuator::desc is an ActuatorRecord: both)
static __global__ void write_delay_launch_kernel(DelayLaunch* __restrict__ out, const DelayLaunch v) { *out = v; }
// (a transport delay is stage 0 of the actuator: installed alone it makes the launch an actuated one)
static bool delay_active(const TinyBatch* b) { return b->delay.d_max > 0 && takes_plant_step(b); }
static bool compensation_active(const TinyBatch* b) { return delay_active(b) && b->delay.compensate; }
static bool actuator_active(const TinyBatch* b) { return (b->act.kind != 0 || (b->anoise.seq && b->anoise.steps > 0) || b->delay.d_max > 0) && takes_plant_step(b); }
// begin_log for a log whose switch the begin itself looks at (the actuation log; the other two logs' callers look first): off, no row
static int begin_log_if_on(TinyBatch* b, StepLog& log, int rows, int width) {
    log.rows = 0;
    return log.on ? begin_log(b, log, rows, width) : TINY_OK;
}
// (only the one-row kernel's PA forms read the blocks and the record; the coverage path reads the caller's arrays)
static int ensure_actuator_launch(TinyBatch* b, const PathDecision& D, int rows, const ActuatorLaunch** out) {
    Actuator& s = b->act;
    ActuatorDelay& q = b->delay;
    // (a PX form steps by the model's own block whatever plant is installed; with an estimator it keeps xhat in the coverage path's array)
    if (D.px) { if (int rc = ensure_model_block(b)) return rc; }
    if (D.px && D.pe && !b->est.xhat) HIP_TRY(b, hipMalloc(&b->est.xhat, (size_t)b->batch * b->nx * sizeof(double)));
    if (s.kind && s.dirty) {
        const int setups = s.kind == 1 ? 1 : b->batch;
        if (int rc = ensure_built(b, s.built, s.dirty, (size_t)setups * actuator_block_doubles(), [&](dim3 grid) {
                hipLaunchKernelGGL(fill_actuator_kernel, grid, dim3(256), 0, b->stream, s.built, s.src[0], s.src[1], s.src[2], s.src[3], s.src[4], setups, b->nx, b->nu);
            })) return rc;
    }
    if (int rc = begin_log_if_on(b, s.log, rows, b->nu)) return rc;
    if (!s.desc) HIP_TRY(b, hipMalloc(&s.desc, sizeof(ActuatorRecord)));
    ActuatorLaunch v = {};
    v.tab = s.kind ? tagged_block(s.built, s.kind != 2, s.lag) : nullptr;
    v.state = s.lag ? s.state : nullptr;
    v.noise = b->anoise.seq; v.noise_steps = b->anoise.seq ? b->anoise.steps : 0;
    v.log = s.log.on ? s.log.buf : nullptr; v.log_step0 = kernel_step(b->anoise.step);
    ActuatorRecord* const record = static_cast<ActuatorRecord*>(s.desc);
    hipLaunchKernelGGL(write_actuator_launch_kernel, dim3(1), dim3(1), 0, b->stream, &record->a, v);
    HIP_TRY(b, hipGetLastError());
    if (D.pq) {
        DelayLaunch w = {};
        w.delay = q.d; w.queue = q.queue; w.head = q.head; w.d_max = q.d_max;
        if (D.px) { w.model = block_pointer(model_source(b)); w.xhat = D.pe ? b->est.xhat : nullptr; }
        hipLaunchKernelGGL(write_delay_launch_kernel, dim3(1), dim3(1), 0, b->stream, &record->d, w);
        HIP_TRY(b, hipGetLastError());
    }
    *out = &record->a;
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
                                                                       const int* __restrict__ delay, const int* __restrict__ head, double* __restrict__ queue, int d_max,
                                                                       double* __restrict__ s0, int batch, int nx, int nu, int N) {
#pragma clang fp contract(off)
    const size_t total = (size_t)batch * nu;
    for (size_t e = blockIdx.x * (size_t)blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(e % nu);
        const size_t bb = e / nu, p = per_instance ? e : (size_t)c;
        if (status[bb].x <= 0) continue;
        double v = prim[bb * N * (nx + nu) + nx + c];
        // stage 0, the transport delay: the oldest entry of the instance's ring leaves, the command takes its cell (the head is only
        // read here: the threads of an instance's other inputs read it too -- coverage_queue_head_kernel moves it behind this kernel)
        if (delay && delay[bb] > 0) {
            double* const cell = queue + (bb * d_max + head[bb]) * nu + c;
            const double uc = v;
            v = *cell;
            *cell = uc;
        }
        if (s0) s0[e] = v;
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
// ... and the head of every ring that popped and pushed: one thread per instance, behind the actuator helper
static __global__ __launch_bounds__(256) void coverage_queue_head_kernel(int* __restrict__ head, const int* __restrict__ delay, const int4* __restrict__ status, int batch) {
    for (int bb = blockIdx.x * blockDim.x + threadIdx.x; bb < batch; bb += gridDim.x * blockDim.x) {
        const int d = delay[bb];
        if (status[bb].x <= 0 || d <= 0) continue;
        const int h = head[bb] + 1;
        head[bb] = h < d ? h : 0;
    }
}
static int enqueue_coverage_actuator(TinyBatch* b, long step, int log_row, bool keep_s0) {
    Actuator& s = b->act;
    ActuatorDelay& q = b->delay;
    const size_t total = (size_t)b->batch * b->nu;
    if (!s.ua) HIP_TRY(b, hipMalloc(&s.ua, total * sizeof(double)));
    if (keep_s0 && !q.s0) HIP_TRY(b, hipMalloc(&q.s0, total * sizeof(double)));
    const bool delayed = q.d_max > 0;
    const double* noise = (b->anoise.seq && step >= 0 && step < b->anoise.steps) ? b->anoise.seq + (size_t)step * total : nullptr;
    hipLaunchKernelGGL(coverage_actuator_kernel, dim3(helper_grid(b, total)), dim3(256), 0, b->stream, s.ua, s.lag ? s.state : nullptr,
                       (s.log.on && s.log.buf && log_row < s.log.rows) ? s.log.buf + (size_t)log_row * total : nullptr, b->d_prim, b->d_status, s.src[0], s.src[1],
                       s.lag ? s.src[2] : nullptr, s.src[3], s.src[4], s.kind ? 1 : 0, s.kind == 2 ? 1 : 0, noise, delayed ? q.d : nullptr, q.head, q.queue, q.d_max,
                       keep_s0 ? q.s0 : nullptr, b->batch, b->nx, b->nu, b->N);
    HIP_TRY(b, hipGetLastError());
    if (delayed) {
        hipLaunchKernelGGL(coverage_queue_head_kernel, dim3(helper_grid(b, (size_t)b->batch)), dim3(256), 0, b->stream, q.head, q.d, b->d_status, b->batch);
        HIP_TRY(b, hipGetLastError());
    }
    return TINY_OK;
}
// the coverage path's predictor in front of one single-step launch: one thread per instance, xs <- xin stepped d times by the MODEL over
// the instance's queue as it stands, oldest first -- the chain of coverage_plant_step_kernel in explicit fma()s, what `compensated` does
// on the one-row kernel, same bits.  d = 0: xin's own bits.  (nx <= 31: the two iterates in local arrays)
static __global__ __launch_bounds__(256) void coverage_compensation_kernel(double* __restrict__ xs, const double* __restrict__ xin, const int* __restrict__ delay,
                                                                           const int* __restrict__ head, const double* __restrict__ queue, int d_max,
                                                                           const double* __restrict__ A_m, const double* __restrict__ B_m, const double* __restrict__ f_m,
                                                                           int per_instance, int batch, int nx, int nu) {
    for (int bb = blockIdx.x * blockDim.x + threadIdx.x; bb < batch; bb += gridDim.x * blockDim.x) {
        const size_t p = per_instance ? (size_t)bb : 0;
        const double *A = A_m + p * nx * nx, *B = B_m + p * nx * nu;
        double cur[32], next[32];
        for (int j = 0; j < nx; ++j) cur[j] = xin[(size_t)bb * nx + j];
        const int d = delay[bb], h = head[bb];
        for (int t = 0; t < d; ++t) {
            const int at = h + t < d ? h + t : h + t - d;
            const double* u = queue + ((size_t)bb * d_max + at) * nu;
            for (int j = 0; j < nx; ++j) {
                double acc = f_m ? f_m[p * nx + j] : 0.0;
                for (int k = 0; k < nx; ++k) acc = fma(cur[k], A[j + nx * k], acc);
                for (int k = 0; k < nu; ++k) acc = fma(u[k], B[j + nx * k], acc);
                next[j] = acc;
            }
            for (int j = 0; j < nx; ++j) cur[j] = next[j];
        }
        for (int j = 0; j < nx; ++j) xs[(size_t)bb * nx + j] = cur[j];
    }
}
static int enqueue_coverage_compensation(TinyBatch* b, const double** x0_of_launch) {
    ActuatorDelay& q = b->delay;
    if (b->nx > 32) return fail(b, TINY_ERR_UNSUPPORTED, "delay compensation: nx = %d (the helper kernel holds 32 states)", b->nx);
    if (int rc = ensure_model_source(b, true)) return rc;
    const PlantSource p = model_source(b);
    if (!q.xs) HIP_TRY(b, hipMalloc(&q.xs, (size_t)b->batch * b->nx * sizeof(double)));
    hipLaunchKernelGGL(coverage_compensation_kernel, dim3(helper_grid(b, (size_t)b->batch)), dim3(256), 0, b->stream, q.xs, *x0_of_launch, q.d, q.head, q.queue, q.d_max,
                       p.src[0], p.src[1], p.src[2], p.per_instance ? 1 : 0, b->batch, b->nx, b->nu);
    HIP_TRY(b, hipGetLastError());
    *x0_of_launch = q.xs;
    return TINY_OK;
}

// ---- what a launch does with the stages: one hook per place it touches them (batch_dispatch.hpp) ---------------------------------
void closed_loop_facts(const TinyBatch* b, PathFacts& f) {
    f.disturbance = disturbance_active(b); f.plant = plant_active(b); f.state_log = state_log_active(b);
    f.measurement = measurement_active(b); f.estimator = estimator_active(b); f.score = score_active(b); f.actuator = actuator_active(b);
    f.delay = delay_active(b); f.delay_compensation = compensation_active(b);
}
void note_closed_loop_read(TinyBatch* b) {
    b->dist.last = disturbance_active(b);             // (the one-row and the coverage kernel both add it; decide_path keeps such a launch off the tile kernel)
    b->plant.log.rows = 0;                            // (the state log is the LAST solve call's: a launch that logs sizes it anew)
    b->meas.last = measurement_active(b);             // (the one-row kernel's PM forms, or the helper kernel in front of the coverage kernel)
    b->plant.last = plant_active(b);                  // (likewise: the one-row kernel's PP forms, or the helper kernel behind the coverage kernel)
    b->est.last = estimator_active(b);                // (likewise: the one-row kernel's PE forms, or the helper kernels around the coverage kernel)
    b->est.log.rows = 0;                              // (the estimate log is the LAST solve call's, as the state log)
    b->score.last = score_active(b);                  // (likewise: the one-row kernel's PS forms, or the helper kernel behind the coverage kernel)
    b->act.last = actuator_active(b);                 // (likewise: the one-row kernel's PA forms, or the helper kernel behind the coverage kernel)
    b->act.log.rows = 0;                              // (the actuation log is the LAST solve call's, as the state log)
}
// the one-row launch the decision D sends to a PD ... PA form: what those forms read, bound into the fields that lie over the PREFETCH
// form's and the adaptive-rho ones (the SolveArgs overlays of admm_kernel.hip.h: no such launch takes either)
int bind_closed_loop_args(TinyBatch* b, const PathDecision& D, SolveArgs& a) {
    // every instance its own disturbance: the PD form of whatever the decision chose.  Its three fields lie over pf_base, which
    // only the PREFETCH form reads -- and no PD launch takes that form
    if (D.pd) { a.dist = b->dist.seq; a.dist_steps = b->dist.seq ? b->dist.steps : 0; a.dist_step0 = kernel_step(b->dist.step); }
    // a plant of its own: the PP form of it, whose pointer lies behind those three; and, in either form, the state log
    if (D.pp) {
        if (int rc = ensure_plant_blocks(b)) return rc;
        a.plant = block_pointer(plant_source(b));
    }
    // measurement noise: the PM form of that, whose three fields lie over pf_mask, pf_shards and pf_static -- written by the caller for
    // the PREFETCH form, which no PM launch takes
    if (D.pm) { a.meas = b->meas.seq; a.meas_steps = b->meas.seq ? b->meas.steps : 0; a.meas_step0 = kernel_step(b->meas.step); }
    if ((D.pd || D.pp) && state_log_active(b)) {
        if (int rc = begin_log(b, b->plant.log, a.steps, b->nx)) return rc;
        a.state_log = b->plant.log.buf;
    }
    // a state estimator: the PE form of that, whose four pointers lie over the adaptive-rho ones -- which no PE launch reads
    if (D.pe) {
        if (int rc = ensure_estimator_blocks(b)) return rc;
        a.est_gain = tagged_block(b->est.built, b->est.kind != 2); a.est_model = block_pointer(model_source(b)); a.est_xp = b->est.xp; a.est_log = nullptr;
        if (b->est.log.on) {
            if (int rc = begin_log(b, b->est.log, a.steps, b->nx)) return rc;
            a.est_log = b->est.log.buf;
        }
    }
    // a closed-loop score: the PS form of that, whose three fields lie over the adaptive-rho tables' -- which no PS launch reads
    if (D.ps) {
        if (int rc = ensure_score_blocks(b)) return rc;
        a.score_tab = tagged_block(b->score.built, b->score.kind != 2); a.score_rec = static_cast<ScoreRecord*>(b->score.rec); a.score_step0 = kernel_step(b->score.step);
    }
    // an actuator model: the PA form of that.  Its int sits in the padding behind score_step0, its pointer over arho_max -- which no PA
    // launch reads; what the pointer names is written on the stream here, once per solve call
    if (D.pa) {
        if (int rc = ensure_actuator_launch(b, D, a.steps, &a.act)) return rc;
        a.act_step0 = kernel_step(b->anoise.step);
    }
    return TINY_OK;
}
// a fused launch cut into stretches of MPC steps: every stretch adds, measures, scores and actuates with the rows of ITS steps and logs
// in ITS rows -- by the forms the launch takes (a form it does not take leaves its fields, which lie over others, alone)
void StepBases::capture(const JitKey& k, const SolveArgs& a) {
    pd = k.pd != 0; pm = k.pm != 0; ps = k.ps != 0; pa = k.pa != 0;
    dist0 = pd ? a.dist_step0 : 0; meas0 = pm ? a.meas_step0 : 0; score0 = ps ? a.score_step0 : 0; act0 = pa ? a.act_step0 : 0;
    state_log = (k.pd || k.pp) ? a.state_log : nullptr;
    est_log = k.pe ? a.est_log : nullptr;
}
void StepBases::apply(SolveArgs& a, int done, int batch, int nx) const {
    if (pd) a.dist_step0 = dist0 + done;
    if (pm) a.meas_step0 = meas0 + done;
    if (ps) a.score_step0 = score0 + done;
    if (pa) a.act_step0 = act0 + done;
    if (state_log) a.state_log = state_log + (size_t)done * batch * nx;
    if (est_log) a.est_log = est_log + (size_t)done * batch * nx;
}
// the coverage kernel keeps its state in the HBM records: a fused launch is a loop of single-step launches, and each stage is a helper
// kernel in front of or behind each of them.  In front: the measurements (which the launch takes as its x0), then the estimator's
// correction of them (of x0 itself with no noise).  Behind: the estimator's prediction by the model, the actuator (the applied
// control, which the two behind it read in place of the record's u0), the plant step (by the installed plant or by the model; with
// none of measurement noise, estimator, actuator and plant the launch itself hands x0 on), the state log's row, the score
int coverage_begin(TinyBatch* b, int steps, CoverageLoop& loop) {
    loop.noisy = b->meas.last; loop.filtered = b->est.last; loop.scoring = b->score.last; loop.actuated = b->act.last;
    loop.compensated = loop.actuated && compensation_active(b);
    loop.own_plant = b->plant.last || loop.noisy || loop.filtered || loop.actuated;
    loop.state_log = state_log_active(b);
    if (loop.actuated) { if (int rc = begin_log_if_on(b, b->act.log, steps, b->nu)) return rc; }
    if (loop.state_log) { if (int rc = begin_log(b, b->plant.log, steps, b->nx)) return rc; }
    if (loop.filtered && b->est.log.on) { if (int rc = begin_log(b, b->est.log, steps, b->nx)) return rc; }
    return TINY_OK;
}
int coverage_before_launch(TinyBatch* b, const CoverageLoop& loop, int s, GeneralArgs& a) {
    // every instance its own disturbance: the [batch][nx] block of this step's row (null: a step outside the sequence, or none applies)
    const long dk = b->dist.step + s;
    a.dist = (b->dist.last && dk >= 0 && dk < b->dist.steps) ? b->dist.seq + (size_t)dk * b->batch * b->nx : nullptr;
    if (loop.noisy) { if (int rc = enqueue_coverage_measurement(b, b->meas.step + s, &a.x0)) return rc; }
    if (loop.filtered) { if (!loop.noisy) a.x0 = b->d_x0; if (int rc = enqueue_coverage_correction(b, s, &a.x0)) return rc; }
    // the delay's predictor: the launch solves from the model's prediction over the queue (of the x0 record itself with neither in front)
    if (loop.compensated) { if (!loop.noisy && !loop.filtered) a.x0 = b->d_x0; if (int rc = enqueue_coverage_compensation(b, &a.x0)) return rc; }
    return TINY_OK;
}
int coverage_after_launch(TinyBatch* b, const CoverageLoop& loop, int s, const GeneralArgs& a) {
    // (under delay compensation the prediction uses what the actuator helper took off the queue: it runs behind that helper)
    const bool late_prediction = loop.filtered && loop.compensated;
    if (loop.filtered && !late_prediction) { if (int rc = enqueue_coverage_prediction(b)) return rc; }
    if (loop.actuated) { if (int rc = enqueue_coverage_actuator(b, b->anoise.step + s, s, late_prediction)) return rc; }
    if (late_prediction) { if (int rc = enqueue_coverage_prediction(b, b->delay.s0)) return rc; }
    if (loop.own_plant) { if (int rc = enqueue_coverage_plant_step(b, a.dist)) return rc; }
    if (loop.state_log) { if (int rc = enqueue_state_log_row(b, s)) return rc; }
    if (loop.scoring) { if (int rc = enqueue_coverage_score(b, b->score.step + s)) return rc; }
    return TINY_OK;
}
void advance_closed_loop_counters(TinyBatch* b, int steps) {
    if (b->dist.last) b->dist.step += steps;         // the disturbance moves one row per MPC step
    if (b->meas.last) b->meas.step += steps;         // ... and the measurement noise likewise
    if (b->score.last) b->score.step += steps;       // ... and the score's step counter
    if (b->act.last) b->anoise.step += steps;        // ... and the actuation step counter
}

}  // namespace tinympc_amd

using namespace tinympc_amd;

extern "C" {

// every instance its own additive disturbance at the plant step
int tiny_batch_set_disturbance(TinyBatch* b, const double* w, int n_steps, int flags) {
    if (!b) return TINY_ERR_NULL;
    return install_sequence(b, b->dist, w, n_steps, flags, "per-instance disturbance", "disturbance");
}
// measurement noise: what the solver sees of the state at MPC step k is fl(x0 + v[k][i]).  Removing it drops the coverage path's
// scratch array with it (made again by the launch that needs it; install_sequence has seen the stream run dry).  The model's plant
// block stays: the estimator and the actuator step through it too
int tiny_batch_set_measurement_noise(TinyBatch* b, const double* v, int n_steps, int flags) {
    if (!b) return TINY_ERR_NULL;
    const int rc = install_sequence(b, b->meas, v, n_steps, flags, "measurement noise", "measurement noise");
    if (rc == TINY_OK && !b->meas.seq && b->meas.xm) { (void)hipFree(b->meas.xm); b->meas.xm = nullptr; }
    return rc;
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
    double* const out[3] = {A_p, B_p, f_p};
    const size_t n[3] = {(size_t)b->nx * b->nx, (size_t)b->nx * b->nu, (size_t)b->nx};
    const double none[3] = {0.0, 0.0, 0.0};
    return read_setup(b, b->plant.src, b->plant.kind, instance, n, none, out);
}
// the x0 every MPC step of the last solve call handed on (option "state_log"): x0_next [steps][batch][nx]
int tiny_batch_get_state_log(TinyBatch* b, double* x0_next, int steps) {
    if (!b) return TINY_ERR_NULL;
    return read_log(b, b->plant.log, x0_next, steps, b->nx, "no state log recorded (set_option state_log; advance_x0 or steps_per_launch)");
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
        s.kind = 0; s.dirty = false; s.log.capacity = 0; s.log.rows = 0;
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
    return read_log(b, b->est.log, xhat, steps, b->nx, "no estimate log recorded (set_option estimate_log; tiny_batch_set_estimator; advance_x0 or steps_per_launch)");
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
    if (!b->score.kind) return fail(b, TINY_ERR_ARG, "no score installed");
    const size_t nz = (size_t)b->nx + b->nu, n[4] = {nz, nz, nz, nz};
    double* const out[4] = {weight, target, lo, hi};
    const double none[4] = {0.0, 0.0, -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity()};
    return read_setup(b, b->score.src, b->score.kind, instance, n, none, out);
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
        s.kind = 0; s.lag = false; s.dirty = false; s.log.capacity = 0; s.log.rows = 0;
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
    if (!b->act.kind) return fail(b, TINY_ERR_ARG, "no actuator installed");
    const size_t nu = (size_t)b->nu, n[5] = {nu, nu, nu, nu, nu};
    double* const out[5] = {lo, hi, alpha, gain, offset};
    const double none[5] = {-std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity(), 1.0, 1.0, -0.0};
    return read_setup(b, b->act.src, b->act.kind, instance, n, none, out);
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
// a transport delay in front of the actuator's stages: d [batch] ints (TINY_BROADCAST: one), 0 <= d[i] <= d_max <= TINY_MAX_DELAY.
// Installing or replacing one fills the queue with +0.0 and rewinds every ring; d == NULL or d_max <= 0 removes it.  The values are
// checked on the host (a device array is read back); everything that can fail happens before anything installed is touched
int tiny_batch_set_actuator_delay(TinyBatch* b, const int* d, int d_max, int flags) {
    if (!b) return TINY_ERR_NULL;
    HIP_TRY(b, hipSetDevice(b->device));
    ActuatorDelay& s = b->delay;
    if (flags & ~(TINY_DEVICE | TINY_BROADCAST)) return fail(b, TINY_ERR_ARG, "actuator delay: flags 0x%x (TINY_HOST or TINY_DEVICE, with or without TINY_BROADCAST)", flags);
    if (!d || d_max <= 0) {                                              // remove: freed once the stream has run dry of its readers
        if (s.d_max) { if (int rc = drop_buffers(b, s)) return rc; }
        s.d_max = 0;
        return TINY_OK;
    }
    if (d_max > TINY_MAX_DELAY) return fail(b, TINY_ERR_ARG, "actuator delay: d_max %d (at most TINY_MAX_DELAY = %d)", d_max, TINY_MAX_DELAY);
    const size_t given = (flags & TINY_BROADCAST) ? 1 : (size_t)b->batch;
    std::vector<int> h((size_t)b->batch);
    if (flags & TINY_DEVICE) HIP_TRY(b, hipMemcpy(h.data(), d, given * sizeof(int), hipMemcpyDeviceToHost));
    else std::copy(d, d + given, h.begin());
    if (given == 1) std::fill(h.begin(), h.end(), h[0]);
    for (size_t i = 0; i < h.size(); ++i)
        if (h[i] < 0 || h[i] > d_max) return fail(b, TINY_ERR_ARG, "actuator delay: d = %d at instance %zu (0 .. d_max = %d)", h[i], given == 1 ? (size_t)0 : i, d_max);
    const size_t cells = (size_t)b->batch * d_max * b->nu;
    int *fd = nullptr, *fh = nullptr;
    double* fq = nullptr;
    hipError_t err = hipMalloc(&fd, h.size() * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&fh, h.size() * sizeof(int));
    if (err == hipSuccess) err = hipMalloc(&fq, cells * sizeof(double));
    if (err == hipSuccess) err = hipMemcpyAsync(fd, h.data(), h.size() * sizeof(int), hipMemcpyHostToDevice, b->stream);
    if (err == hipSuccess) err = hipMemsetAsync(fh, 0, h.size() * sizeof(int), b->stream);
    if (err == hipSuccess) err = hipMemsetAsync(fq, 0, cells * sizeof(double), b->stream);          // (+0.0: all bits zero)
    if (err == hipSuccess) err = hipStreamSynchronize(b->stream);       // (h may go; nothing reads the old arrays any more)
    if (err != hipSuccess) {
        (void)hipGetLastError();
        if (fd) (void)hipFree(fd);
        if (fh) (void)hipFree(fh);
        if (fq) (void)hipFree(fq);
        return fail(b, TINY_ERR_HIP, "actuator delay: %s", hipGetErrorString(err));
    }
    free_buffers(s);                                                     // (the scratch arrays come back with the launch that needs them)
    s.d = fd; s.head = fh; s.queue = fq; s.d_max = d_max;
    return TINY_OK;
}
int tiny_batch_get_actuator_delay(TinyBatch* b, int instance, int* d_out) {
    if (!b) return TINY_ERR_NULL;
    if (!b->delay.d_max) return fail(b, TINY_ERR_ARG, "no actuator delay installed (tiny_batch_set_actuator_delay)");
    if (!d_out) return fail(b, TINY_ERR_ARG, "null output");
    if (instance < 0 || instance >= b->batch) return fail(b, TINY_ERR_ARG, "instance %d of %d", instance, b->batch);
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    HIP_TRY(b, hipMemcpy(d_out, b->delay.d + instance, sizeof(int), hipMemcpyDeviceToHost));
    return TINY_OK;
}
// the queue: q [batch][d_max][nu], oldest first (TINY_BROADCAST: [d_max][nu]); every ring is rewound, so that row t of an instance is its
// t-th oldest entry.  The fresh array is complete before it takes the place of the one installed
int tiny_batch_set_actuator_queue(TinyBatch* b, const double* q, int flags) {
    if (!b) return TINY_ERR_NULL;
    ActuatorDelay& s = b->delay;
    if (!s.d_max) return fail(b, TINY_ERR_ARG, "no actuator delay installed (tiny_batch_set_actuator_delay)");
    if (!q) return fail(b, TINY_ERR_ARG, "null actuator queue");
    if (flags & ~(TINY_DEVICE | TINY_BROADCAST)) return fail(b, TINY_ERR_ARG, "actuator queue: flags 0x%x (TINY_HOST or TINY_DEVICE, with or without TINY_BROADCAST)", flags);
    HIP_TRY(b, hipSetDevice(b->device));
    const size_t slice = (size_t)s.d_max * b->nu, cells = (size_t)b->batch * slice;
    const UploadPart given = {q, (flags & TINY_BROADCAST) ? slice : cells};
    double* fresh = nullptr;
    if (int rc = upload_fresh(b, &given, &fresh, 1, flags, "actuator queue")) return rc;
    if (flags & TINY_BROADCAST) {                                        // one slice for all: expanded as a broadcast sequence of one step
        double* full = nullptr;
        hipError_t err = hipMalloc(&full, cells * sizeof(double));
        int rc = TINY_OK;
        if (err == hipSuccess) rc = expand_disturbance(b, full, fresh, 1, (int)slice);
        if (err == hipSuccess && rc == TINY_OK) err = hipStreamSynchronize(b->stream);
        (void)hipFree(fresh);
        if (err != hipSuccess || rc != TINY_OK) {
            (void)hipGetLastError();
            if (full) (void)hipFree(full);
            return rc != TINY_OK ? rc : fail(b, TINY_ERR_HIP, "actuator queue: %s", hipGetErrorString(err));
        }
        fresh = full;
    }
    // (everything fallible is behind us but the rewind itself: where that fails the fresh array goes and the queue installed stays)
    hipError_t err = hipStreamSynchronize(b->stream);                    // (nothing reads the old queue any more)
    if (err == hipSuccess) err = hipMemset(s.head, 0, (size_t)b->batch * sizeof(int));
    if (err != hipSuccess) {
        (void)hipGetLastError();
        (void)hipFree(fresh);
        return fail(b, TINY_ERR_HIP, "actuator queue: %s", hipGetErrorString(err));
    }
    (void)hipFree(s.queue);
    s.queue = fresh;
    return TINY_OK;
}
// ... on the host, oldest first: the first d[i] rows of an instance's slice, +0.0 behind them
int tiny_batch_get_actuator_queue(TinyBatch* b, double* q_out) {
    if (!b) return TINY_ERR_NULL;
    const ActuatorDelay& s = b->delay;
    if (!s.d_max) return fail(b, TINY_ERR_ARG, "no actuator delay installed (tiny_batch_set_actuator_delay)");
    if (!q_out) return fail(b, TINY_ERR_ARG, "null output");
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    const size_t nu = (size_t)b->nu, slice = (size_t)s.d_max * nu;
    std::vector<int> d((size_t)b->batch), head((size_t)b->batch);
    std::vector<double> ring((size_t)b->batch * slice);
    HIP_TRY(b, hipMemcpy(d.data(), s.d, d.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(head.data(), s.head, head.size() * sizeof(int), hipMemcpyDeviceToHost));
    HIP_TRY(b, hipMemcpy(ring.data(), s.queue, ring.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < d.size(); ++i)
        for (int t = 0; t < s.d_max; ++t) {
            const int at = t < d[i] ? (head[i] + t) % d[i] : 0;
            for (size_t c = 0; c < nu; ++c) q_out[i * slice + (size_t)t * nu + c] = t < d[i] ? ring[i * slice + (size_t)at * nu + c] : 0.0;
        }
    return TINY_OK;
}
// the applied control of every MPC step of the last solve call (option "actuation_log"): ua [steps][batch][nu]
int tiny_batch_get_actuation_log(TinyBatch* b, double* ua, int steps) {
    if (!b) return TINY_ERR_NULL;
    return read_log(b, b->act.log, ua, steps, b->nu, "no actuation log recorded (set_option actuation_log; an actuator or actuation noise; advance_x0 or steps_per_launch)");
}
}  // extern "C"
