// batch_helpers.hip -- what the clock-checked dispatch needs besides the solve kernels: the iteration histogram of a solve (its cost
// model is host arithmetic: launch_learner.hpp), the counting sorts behind step_regroup / repack_sort and the lock-step estimate (small
// device kernels of this unit), the per-instance state of adaptive rho, and the buffers all of them allocate on demand.  Split off
// batch_dispatch.hip in round 6; declarations: batch_dispatch.hpp.  (Per-instance problem data and its fill kernels: batch_instance.hip; the closed-loop stages, their fill and coverage helper kernels: batch_closed_loop.hip.)
#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"

#include <algorithm>
#include <cstring>
#include <limits>

namespace tinympc_amd {

// ---- automatic split solves ("repack_after" = -1): histogram of the iteration counts + a cost model ----------------------
static __global__ __launch_bounds__(256) void iter_hist_kernel(const int4* __restrict__ status, int batch, unsigned* __restrict__ hist) {
    __shared__ unsigned h[TinyBatch::HIST_BINS];
    for (int e = threadIdx.x; e < TinyBatch::HIST_BINS; e += blockDim.x) h[e] = 0u;
    __syncthreads();
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < batch; i += gridDim.x * blockDim.x) {
        int it = status[i].x;
        it = it < 0 ? 0 : (it >= TinyBatch::HIST_BINS ? TinyBatch::HIST_BINS - 1 : it);
        atomicAdd(&h[it], 1u);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < TinyBatch::HIST_BINS; e += blockDim.x)
        if (h[e]) atomicAdd(&hist[e], h[e]);
}
SplitModel split_model(const TinyBatch* b) {
    return {b->nx, b->nu, b->N, solve_kernel_waves_per_simd(b->nx + b->nu, b->N, soc_active(b)), b->set.max_iter, std::max(1, b->set.check_termination),
            b->repack_growth >= 2 ? b->repack_growth : 0, b->num_cus};
}

// ---- adaptive rho: per-instance cache state + the lane tables of the adaptation step -----------------------------------
static __global__ void broadcast_vec_kernel(double* __restrict__ dst, const double* __restrict__ src, long n, int per) {
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) dst[i] = src[i % per];
}

// per-instance batch whose caller set ONE set of sensitivity tables: every instance's lane tables <- the family's (ATAB_DK ... ATAB_DC2)
// with ATAB_AT from the instance's own A and B
static __global__ __launch_bounds__(256) void expand_atabs_kernel(double* __restrict__ atabs, const double* __restrict__ atab, const double* __restrict__ A,
                                                                  const double* __restrict__ B, int nx, int nu, int batch) {
    const int e = threadIdx.x, k = e / 16, j = e % 16;
    for (int b = blockIdx.x; b < batch; b += gridDim.x) {
        double* t = atabs + (size_t)b * ATAB_DOUBLES;
        const struct { ColMajor A, B; } view = {{A + (size_t)b * nx * nx, nx}, {B + (size_t)b * nx * nu, nx}};
        t[ATAB_AT + e] = atab_at(view, nx, nu, j, k);
        for (int o = ATAB_DK; o < ATAB_DOUBLES; o += 256) t[o + e] = atab[o + e];
    }
}

// every instance's cache state <- the family's cache (rho, Kinf, Pinf, C1 = Quu_inv, C2 = AmBKt: tiny_api.cpp:375-376); per-instance
// batch: <- the instance's own Riccati output
int adaptive_fresh_state(TinyBatch* b) {
    const int nx = b->nx, nu = b->nu;
    if (b->hetero) {
        const size_t B = b->batch;
        struct { double* dst; const double* src; size_t n; } parts[] = {{b->d_arho, b->d_hrho, B}, {b->d_aK, b->d_hK, B * nu * nx}, {b->d_aP, b->d_hP, B * nx * nx},
                                                                        {b->d_aC1, b->d_hQuu, B * nu * nu}, {b->d_aC2, b->d_hAmBKt, B * nx * nx}};
        for (auto& p : parts) HIP_TRY(b, hipMemcpyAsync(p.dst, p.src, p.n * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        b->astate_fresh = true;
        return TINY_OK;
    }
    std::vector<double> h;
    h.push_back(b->cache.rho);
    h.insert(h.end(), b->cache.Kinf.a.begin(), b->cache.Kinf.a.end());
    h.insert(h.end(), b->cache.Pinf.a.begin(), b->cache.Pinf.a.end());
    h.insert(h.end(), b->cache.Quu_inv.a.begin(), b->cache.Quu_inv.a.end());
    h.insert(h.end(), b->cache.AmBKt.a.begin(), b->cache.AmBKt.a.end());
    double* tmp = nullptr;
    HIP_TRY(b, hipMalloc(&tmp, h.size() * sizeof(double)));
    if (hipMemcpyAsync(tmp, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice, b->stream) != hipSuccess ||
        hipStreamSynchronize(b->stream) != hipSuccess) { (void)hipFree(tmp); return fail(b, TINY_ERR_HIP, "upload of the cache state failed"); }
    struct { double* dst; int per; size_t off; } parts[] = {{b->d_arho, 1, 0}, {b->d_aK, nu * nx, 1}, {b->d_aP, nx * nx, (size_t)1 + nu * nx},
                                                            {b->d_aC1, nu * nu, (size_t)1 + nu * nx + nx * nx},
                                                            {b->d_aC2, nx * nx, (size_t)1 + nu * nx + nx * nx + nu * nu}};
    for (auto& p : parts) {
        hipLaunchKernelGGL(broadcast_vec_kernel, dim3(512), dim3(256), 0, b->stream, p.dst, tmp + p.off, (long)b->batch * p.per, p.per);
        if (hipGetLastError() != hipSuccess) { (void)hipFree(tmp); return fail(b, TINY_ERR_HIP, "broadcast of the cache state failed"); }
    }
    const hipError_t e = hipStreamSynchronize(b->stream);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(b, TINY_ERR_HIP, "broadcast of the cache state failed");
    b->astate_fresh = true;
    return TINY_OK;
}

int ensure_adaptive(TinyBatch* b, bool need_tables) {
    const int nx = b->nx, nu = b->nu;
    const size_t B = b->batch;
    if (!b->d_arho) {
        HIP_TRY(b, hipMalloc(&b->d_arho, B * sizeof(double)));
        HIP_TRY(b, hipMalloc(&b->d_aK, B * nu * nx * sizeof(double)));
        HIP_TRY(b, hipMalloc(&b->d_aP, B * nx * nx * sizeof(double)));
        HIP_TRY(b, hipMalloc(&b->d_aC1, B * nu * nu * sizeof(double)));
        HIP_TRY(b, hipMalloc(&b->d_aC2, B * nx * nx * sizeof(double)));
        HIP_TRY(b, hipMalloc(&b->d_atab, ATAB_DOUBLES * sizeof(double)));
        if (int rc = adaptive_fresh_state(b)) return rc;
        b->atab_dirty = true;
    }
    if (b->hetero && need_tables && !b->d_atabs) HIP_TRY(b, hipMalloc(&b->d_atabs, B * ATAB_DOUBLES * sizeof(double)));
    if (b->hetero && b->sens_inst) return TINY_OK;           // (every instance's own tables: sensitivity_kernel wrote d_atabs)
    if (b->hetero && b->sens_failed && need_tables)
        return fail(b, TINY_ERR_DIM, "adaptive rho is on but tiny_batch_compute_sensitivity failed for at least one instance (steps = -1 in "
                                     "tiny_batch_get_sensitivity_instance): no tables are installed");
    if (b->atab_dirty && need_tables) {
        if ((int)b->dKinf.size() != nu * nx || (int)b->dPinf.size() != nx * nx)
            return fail(b, TINY_ERR_DIM, "adaptive rho is on but the sensitivity tables are not set (tiny_batch_set_sensitivity / tiny_batch_compute_sensitivity)");
        const std::vector<double> t = build_adaptive_table(b);
        HIP_TRY(b, hipMemcpyAsync(b->d_atab, t.data(), t.size() * sizeof(double), hipMemcpyHostToDevice, b->stream));
        if (b->hetero) {
            hipLaunchKernelGGL(expand_atabs_kernel, dim3((unsigned)std::min<size_t>(B, 2048)), dim3(256), 0, b->stream, b->d_atabs, b->d_atab, b->d_hA, b->d_hB, nx, nu, b->batch);
            HIP_TRY(b, hipGetLastError());
        }
        HIP_TRY(b, hipStreamSynchronize(b->stream));
        b->atab_dirty = false;
    }
    return TINY_OK;
}

// histogram of the iteration counts the solve just enqueued leaves in d_status -> pinned host memory, asynchronously (hist_ev)
int enqueue_iteration_histogram(TinyBatch* b) {
    if (!b->d_hist) {
        HIP_TRY(b, hipMalloc(&b->d_hist, TinyBatch::HIST_BINS * sizeof(unsigned)));
        HIP_TRY(b, hipHostMalloc(reinterpret_cast<void**>(&b->h_hist), TinyBatch::HIST_BINS * sizeof(unsigned), hipHostMallocDefault));
        HIP_TRY(b, hipEventCreateWithFlags(&b->hist_ev, hipEventDisableTiming));
    }
    HIP_TRY(b, hipMemsetAsync(b->d_hist, 0, TinyBatch::HIST_BINS * sizeof(unsigned), b->stream));
    hipLaunchKernelGGL(iter_hist_kernel, dim3(64), dim3(256), 0, b->stream, b->d_status, b->batch, b->d_hist);
    HIP_TRY(b, hipGetLastError());
    HIP_TRY(b, hipMemcpyAsync(b->h_hist, b->d_hist, TinyBatch::HIST_BINS * sizeof(unsigned), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipEventRecord(b->hist_ev, b->stream));
    b->hist_pending = true;
    return TINY_OK;
}

// ---- step_regroup: counting sort of the instances by the iteration count of their last solve, largest first (the longest waves
// of a stretch start first, the short ones fill its tail), and the estimate that switches it on
enum { RG_BINS = 1024 };
__device__ __forceinline__ int regroup_key(const int4 st) {
    const int it = st.x < 0 ? -st.x : st.x;
    return it < RG_BINS - 1 ? it : RG_BINS - 1;
}
// (status / perm: of the FIRST instance of the range; `first` = its number in the batch -- what perm holds)
__global__ __launch_bounds__(256) void regroup_hist_kernel(const int4* status, int batch, unsigned* bins) {
    __shared__ unsigned h[RG_BINS];
    for (int i = threadIdx.x; i < RG_BINS; i += blockDim.x) h[i] = 0u;
    __syncthreads();
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < batch; b += gridDim.x * blockDim.x) atomicAdd(&h[regroup_key(status[b])], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < RG_BINS; i += blockDim.x)
        if (h[i]) atomicAdd(&bins[i], h[i]);
}
// bins[k] <- instances with a key above k (one block of RG_BINS threads): where the first instance of key k goes
__global__ __launch_bounds__(RG_BINS) void regroup_scan_kernel(unsigned* bins) {
    __shared__ unsigned s[RG_BINS];
    const int t = threadIdx.x;
    const unsigned own = bins[RG_BINS - 1 - t];
    s[t] = own;
    __syncthreads();
    for (int d = 1; d < RG_BINS; d <<= 1) {
        const unsigned v = t >= d ? s[t - d] : 0u;
        __syncthreads();
        s[t] += v;
        __syncthreads();
    }
    bins[RG_BINS - 1 - t] = s[t] - own;
}
// (a block ranks its 1024 instances in LDS and asks the device-wide counters once per key it holds: the counts of a batch sit in a
// handful of bins, one atomic per instance on those few addresses would serialise the whole pass)
__global__ __launch_bounds__(256) void regroup_scatter_kernel(const int4* status, int batch, int first, unsigned* bins, int* perm) {
    __shared__ unsigned base[RG_BINS], rank[RG_BINS];
    for (int c0 = blockIdx.x * 1024; c0 < batch; c0 += gridDim.x * 1024) {
        for (int i = threadIdx.x; i < RG_BINS; i += 256) { base[i] = 0u; rank[i] = 0u; }
        __syncthreads();
        int key[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int b = c0 + e * 256 + threadIdx.x;
            key[e] = b < batch ? regroup_key(status[b]) : -1;
            if (key[e] >= 0) atomicAdd(&base[key[e]], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < RG_BINS; i += 256)
            if (base[i]) base[i] = atomicAdd(&bins[i], base[i]);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (key[e] >= 0) perm[base[key[e]] + atomicAdd(&rank[key[e]], 1u)] = first + c0 + e * 256 + threadIdx.x;
        __syncthreads();
    }
}
// ---- repack_sort: the open instances of a split solve's stage by their distance from the tolerances.  Key = the larger of
// primal residual / tol_pri and dual residual / tol_dua (d_resid: what the stage before left at its last test), 16 bins per octave
// from 2^-8 up; a residual that is not a positive number (a diverged instance) goes in front with the largest
__device__ __forceinline__ int repack_key(const double* resid, const int b, const double rtp, const double rtd) {
    const double4 r = *reinterpret_cast<const double4*>(resid + (size_t)b * 4);
    const double m = fmax(fmax(r.x, r.y) * rtp, fmax(r.z, r.w) * rtd);
    if (!(m > 0.0) || !(m < 1e300)) return RG_BINS - 1;
    const unsigned long long u = (unsigned long long)__double_as_longlong(m);
    const int k = (int)((u >> 48) & 0x7FFFull) - ((1023 - 8) << 4);        // exponent and the mantissa's top four bits
    return k < 0 ? 0 : (k > RG_BINS - 2 ? RG_BINS - 2 : k);
}
__global__ __launch_bounds__(256) void repack_hist_kernel(const int* list, const int* count, const double* resid, double rtp, double rtd, unsigned* bins) {
    __shared__ unsigned h[RG_BINS];
    for (int i = threadIdx.x; i < RG_BINS; i += blockDim.x) h[i] = 0u;
    __syncthreads();
    const int n = *count;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) atomicAdd(&h[repack_key(resid, list[i], rtp, rtd)], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < RG_BINS; i += blockDim.x)
        if (h[i]) atomicAdd(&bins[i], h[i]);
}
__global__ __launch_bounds__(256) void repack_scatter_kernel(const int* list, const int* count, const double* resid, double rtp, double rtd, unsigned* bins, int* out) {
    __shared__ unsigned base[RG_BINS], rank[RG_BINS];
    const int n = *count;
    for (int c0 = blockIdx.x * 1024; c0 < n; c0 += gridDim.x * 1024) {
        for (int i = threadIdx.x; i < RG_BINS; i += 256) { base[i] = 0u; rank[i] = 0u; }
        __syncthreads();
        int key[4], inst[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int i = c0 + e * 256 + threadIdx.x;
            inst[e] = i < n ? list[i] : -1;
            key[e] = i < n ? repack_key(resid, inst[e], rtp, rtd) : -1;
            if (key[e] >= 0) atomicAdd(&base[key[e]], 1u);
        }
        __syncthreads();
        for (int i = threadIdx.x; i < RG_BINS; i += 256)
            if (base[i]) base[i] = atomicAdd(&bins[i], base[i]);
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (key[e] >= 0) out[base[key[e]] + atomicAdd(&rank[key[e]], 1u)] = inst[e];
        __syncthreads();
    }
}
// what lock step costs a batch whose waves take the instances four by four in their natural order, by the iteration totals each
// instance has accumulated (d_accum): out[0] += rows x the largest total of every group of four, out[1] += the totals
__global__ __launch_bounds__(256) void lockstep_estimate_kernel(const uint2* accum, int batch, unsigned long long* out) {
    unsigned long long m = 0ull, t = 0ull;
    const int groups = (batch + 3) / 4;
    for (int g = blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += gridDim.x * blockDim.x) {
        unsigned mx = 0u; int rows = 0;
        for (int r = 0; r < 4 && 4 * g + r < batch; ++r) {
            const unsigned v = accum[4 * g + r].x;
            mx = v > mx ? v : mx; t += v; ++rows;
        }
        m += (unsigned long long)mx * rows;
    }
    for (int off = 32; off >= 1; off >>= 1) { m += __shfl_xor(m, off); t += __shfl_xor(t, off); }
    if ((threadIdx.x & 63) == 0) { atomicAdd(&out[0], m); atomicAdd(&out[1], t); }
}
// the code object of this unit's helper kernels (histograms, counting sorts) reaches the device when one of them is first asked about:
// done where their buffers are allocated -- in front of the clock of a planned first solve -- instead of inside its first sort
static void preload_helper_kernels(TinyBatch* b) {
    if (b->helpers_loaded) return;
    b->helpers_loaded = true;
    hipFuncAttributes fa;
    if (hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(regroup_hist_kernel)) != hipSuccess) (void)hipGetLastError();
}
int ensure_regroup_buffers(TinyBatch* b, bool second_stream) {
    preload_helper_kernels(b);
    if (!b->d_perm) HIP_TRY(b, hipMalloc(&b->d_perm, (size_t)b->batch * sizeof(int)));
    if (!b->d_rg_bins) HIP_TRY(b, hipMalloc(&b->d_rg_bins, 2 * RG_BINS * sizeof(unsigned)));
    if (second_stream && b->regroup_streams == 2 && !b->stream2) {
        HIP_TRY(b, hipStreamCreateWithFlags(&b->stream2, hipStreamNonBlocking));
        HIP_TRY(b, hipEventCreateWithFlags(&b->rg_fork, hipEventDisableTiming));
        HIP_TRY(b, hipEventCreateWithFlags(&b->rg_join, hipEventDisableTiming));
    }
    return TINY_OK;
}
// d_perm[first ..) <- instances first .. first + count - 1 ordered by the iteration count d_status holds for them, largest first
// (enqueued on `st`; `half` picks the set of counters)
int enqueue_regroup_sort(TinyBatch* b, hipStream_t st, int half, int first, int count) {
    unsigned* bins = b->d_rg_bins + half * RG_BINS;
    HIP_TRY(b, hipMemsetAsync(bins, 0, RG_BINS * sizeof(unsigned), st));
    const int blocks = std::max(1, std::min(256, (count + 1023) / 1024));
    hipLaunchKernelGGL(regroup_hist_kernel, dim3(blocks), dim3(256), 0, st, b->d_status + first, count, bins);
    hipLaunchKernelGGL(regroup_scan_kernel, dim3(1), dim3(RG_BINS), 0, st, bins);
    hipLaunchKernelGGL(regroup_scatter_kernel, dim3(blocks), dim3(256), 0, st, b->d_status + first, count, first, bins, b->d_perm + first);
    HIP_TRY(b, hipGetLastError());
    return TINY_OK;
}
// d_perm <- list[0 .. *count) ordered by repack_key, largest first (on the batch's stream)
int enqueue_repack_sort(TinyBatch* b, const int* list, const int* count) {
    unsigned* bins = b->d_rg_bins;
    HIP_TRY(b, hipMemsetAsync(bins, 0, RG_BINS * sizeof(unsigned), b->stream));
    const int blocks = std::max(1, std::min(128, (b->batch + 1023) / 1024));
    const double rtp = 1.0 / b->set.abs_pri_tol, rtd = 1.0 / b->set.abs_dua_tol;
    hipLaunchKernelGGL(repack_hist_kernel, dim3(blocks), dim3(256), 0, b->stream, list, count, b->d_resid, rtp, rtd, bins);
    hipLaunchKernelGGL(regroup_scan_kernel, dim3(1), dim3(RG_BINS), 0, b->stream, bins);
    hipLaunchKernelGGL(repack_scatter_kernel, dim3(blocks), dim3(256), 0, b->stream, list, count, b->d_resid, rtp, rtd, bins, b->d_perm);
    HIP_TRY(b, hipGetLastError());
    return TINY_OK;
}
int enqueue_lockstep_estimate(TinyBatch* b) {
    if (!b->d_ls) {
        HIP_TRY(b, hipMalloc(&b->d_ls, 2 * sizeof(unsigned long long)));
        HIP_TRY(b, hipHostMalloc(reinterpret_cast<void**>(&b->h_ls), 2 * sizeof(unsigned long long), hipHostMallocDefault));
        HIP_TRY(b, hipEventCreateWithFlags(&b->ls_ev, hipEventDisableTiming));
    }
    HIP_TRY(b, hipMemsetAsync(b->d_ls, 0, 2 * sizeof(unsigned long long), b->stream));
    hipLaunchKernelGGL(lockstep_estimate_kernel, dim3(64), dim3(256), 0, b->stream, b->d_accum, b->batch, b->d_ls);
    HIP_TRY(b, hipGetLastError());
    HIP_TRY(b, hipMemcpyAsync(b->h_ls, b->d_ls, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(b, hipEventRecord(b->ls_ev, b->stream));
    b->ls_pending = true;
    return TINY_OK;
}
void read_lockstep_estimate(TinyBatch* b) {
    b->ls_pending = false;
    b->learn.lockstep_estimate_arrived(b->h_ls[0], b->h_ls[1]);
}

// index lists + per-stage counters of the split solve: [stage] list lengths, [32 + stage] tile counters
int ensure_repack_buffers(TinyBatch* b) {
    if (b->d_repack_index && b->d_repack_count) return TINY_OK;
    preload_helper_kernels(b);
    if (!b->d_repack_index) HIP_TRY(b, hipMalloc(&b->d_repack_index, 2 * (size_t)b->batch * sizeof(int)));
    if (!b->d_repack_count) HIP_TRY(b, hipMalloc(&b->d_repack_count, 2 * 32 * sizeof(int)));
    return TINY_OK;
}

}  // namespace tinympc_amd
