// batch_dispatch.hpp -- what batch_api.hip (the C ABI), batch_dispatch.hip (kernel selection, launch forms), batch_tables.hip (lane
// tables) and batch_helpers.hip (helper kernels, on-demand buffers) share.
#pragma once
#include "batch_impl.hpp"
#include "kernel_path.hpp"
#include "lane_tables.hpp"

#define HIP_TRY(b, expr)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (void)hipGetLastError();   /* reported here: do not let it resurface in a later, unrelated call */ \
            return fail(b, TINY_ERR_HIP, "%s -> %s", #expr, hipGetErrorString(e_));               \
        }                                                                                         \
    } while (0)

namespace tinympc_amd {
// ---- the compiled-in kernels (one translation unit per shape, _gen/registry.inc)
extern const KernelEntry* const* const g_kernel_list;
extern const int g_nkernels;
const TileEntry* find_tile(int nx, int nu, int N);
const KernelEntry* find_kernel(int nx, int nu, int N);
// ---- which kernel serves the batch as it is configured now: decide_path(path_facts(b)) (kernel_path.hpp: the facts and the rules)
PathFacts path_facts(const TinyBatch* b);
bool soc_active(const TinyBatch* b);
// ---- buffers and state the API calls create on demand
int ensure_kpi(TinyBatch* b, double** p);
int ensure_repack_buffers(TinyBatch* b);
int ensure_regroup_buffers(TinyBatch* b, bool second_stream);
int ensure_adaptive(TinyBatch* b, bool need_tables = true);
int adaptive_fresh_state(TinyBatch* b);
int ensure_instance_bounds(TinyBatch* b);   // the per-instance box the kernels read, rebuilt from the caller's arrays when it is out of date (synchronous then)
// every instance its own half-spaces: is such a set installed AND one of its families enabled (bit 0 static, bit 1 time-varying) / the
// blocks the kernels read, rebuilt -- or only their offsets rewritten -- when they are out of date (enqueued on the batch's stream)
int inst_lin_active(const TinyBatch* b);
int ensure_instance_linear(TinyBatch* b);
int inst_lin_kmax(const TinyBatch* b);     // the block stride of a per-instance set: the smallest power of two that holds the enabled counts
// every instance its own cone coefficients: installed AND a cone family on / the block the one-row kernel reads, rebuilt when a setter
// has changed it (enqueued on the batch's stream)
bool inst_cones_active(const TinyBatch* b);
int ensure_instance_cones(TinyBatch* b);
// every instance its own disturbance at the plant step: installed AND the next launch takes a plant step (advance_x0, or fused steps) /
// the row its first MPC step takes, as the kernels' int / a broadcast sequence [n_steps][nx] expanded to [n_steps][batch][nx]
bool disturbance_active(const TinyBatch* b);
int dist_step_base(const TinyBatch* b);
int expand_disturbance(TinyBatch* b, double* out, const double* seq, int n_steps);
int max_enabled_halfspaces(const TinyBatch* b);   // the largest count per knot among the ENABLED half-space families (batch_tables.hip)
// ---- lane tables (batch_tables.hip)
struct SharedHalfspaces { HalfspaceRows sx, su, tx, tu; };   // static state | input, time-varying state | input (lane_tables.hpp)
SharedHalfspaces shared_halfspaces(const TinyBatch* b);
bool box_is_uniform(const TinyBatch* b);     // the box is the same at every knot: the one place that decides it
int lin_kmax(const TinyBatch* b);       // half-spaces per knot and family the LIN variants are built for (4, 8, 16, 32; 0: coverage kernel)
void build_tables(TinyBatch* b);
void build_tile_tables(TinyBatch* b);
void build_general_tables(TinyBatch* b);
std::vector<double> build_adaptive_table(const TinyBatch* b);   // the shared family's ATAB_* tables from dKinf ... dC2 (no HIP call)
int upload_tables(TinyBatch* b);
int upload_growing(TinyBatch* b, double** dev, size_t* capacity, const std::vector<double>& host);   // host table -> device buffer that grows
// ---- helper kernels (batch_helpers.hip)
constexpr int REGROUP_AUTO_MIN_STEPS = 16, REGROUP_AUTO_MIN_BATCH = 4096;
int enqueue_iteration_histogram(TinyBatch* b);
int enqueue_regroup_sort(TinyBatch* b, hipStream_t st, int half, int first, int count);
int enqueue_repack_sort(TinyBatch* b, const int* list, const int* count);
int enqueue_lockstep_estimate(TinyBatch* b);
// ---- launches besides launch_solve (batch_impl.hpp)
int launch_general(TinyBatch* b, int phase = 0);
int launch_riccati(TinyBatch* b, const RiccatiArgs& r, size_t lds_bytes, int grid);
int launch_sensitivity(hipStream_t stream, const SensitivityArgs& s, int grid);
// ---- the clock-checked dispatch: what probes left behind goes to b->learn (launch_learner.hpp: the rules and the cost models)
void learn_from_probe(TinyBatch* b, int max_iter, bool auto_split);
void read_lockstep_estimate(TinyBatch* b);
SplitModel split_model(const TinyBatch* b);          // the cost model's view of the batch as it is configured now
}  // namespace tinympc_amd
