// batch_dispatch.hpp -- what batch_api.hip (the C ABI), batch_dispatch.hip (kernel selection, launch forms), batch_tables.hip (lane
// tables), batch_helpers.hip (helper kernels, on-demand buffers), batch_instance.hip (per-instance problem data) and
// batch_closed_loop.hip (the stages at the fused closed-loop plant step) share.
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
int max_enabled_halfspaces(const TinyBatch* b);   // the largest count per knot among the ENABLED half-space families (batch_tables.hip)
// ---- every instance its own problem data (batch_instance.hip; the state: InstanceBox, InstanceHalfspaces, InstanceCones of batch_impl.hpp)
// what a launch calls: the blocks the kernels read, rebuilt where a setter or an enable switch left them out of date -- the box first and
// synchronously (it may change the UB decision), the other two enqueued on the batch's stream; nothing out of date: a few flag tests, no
// HIP call -- / the `last` flags <- what the kernel about to be launched reads (the closed-loop stages' too: note_closed_loop_read)
int ensure_instance_data(TinyBatch* b);
void note_instance_data_read(TinyBatch* b);
void instance_data_settings_changed(TinyBatch* b);   // tiny_batch_update_settings: what an enable switch leaves out of date
// a shared setter is about to install one box / half-space set (0 static, 1 time-varying) / cone set for all: the per-instance one goes,
// its buffers freed once the stream has run dry of their readers (nothing installed: no HIP call)
int drop_instance_bounds(TinyBatch* b);
int drop_instance_linear(TinyBatch* b, int set);
int drop_instance_cones(TinyBatch* b);
// half-spaces: is a per-instance set installed AND one of its families enabled (bit 0 static, bit 1 time-varying) / the block stride of
// such a set: the smallest power of two that holds the enabled counts.  Cones: installed AND a cone family on
int inst_lin_active(const TinyBatch* b);
int inst_lin_kmax(const TinyBatch* b);
bool inst_cones_active(const TinyBatch* b);
// ---- what batch_instance.hip and batch_closed_loop.hip share (defined in batch_instance.hip)
unsigned helper_grid(const TinyBatch* b, size_t total);      // blocks of 256 threads for a grid-stride helper kernel over `total` elements
struct UploadPart { const double* src; size_t doubles; };
int upload_fresh(TinyBatch* b, const UploadPart* parts, double** fresh, int n, int flags, const char* what);   // fresh device copies, all or nothing
int read_instance(TinyBatch* b, double* dst, const double* src, int instance, size_t n);                       // one instance of src [batch][n], to the host
// frees and nulls every device buffer a family's struct names (the caller has seen the stream run dry of their readers)
template <class S>
void free_buffers(S& s) { s.each_buffer([](auto*& p) { if (p) (void)hipFree(p); p = nullptr; }); }
// every buffer of one family goes, once the stream has run dry of their readers (its flags and sizes: the caller's)
template <class S>
int drop_buffers(TinyBatch* b, S& s) {
    HIP_TRY(b, hipSetDevice(b->device));
    HIP_TRY(b, hipStreamSynchronize(b->stream));
    free_buffers(s);
    return TINY_OK;
}
// ---- the stages at the fused closed-loop plant step (batch_closed_loop.hip; the state: closed_loop.hpp): one hook per place a launch
// touches them.  The not-dirty path of a warm launch is flag tests and no HIP call
void closed_loop_facts(const TinyBatch* b, PathFacts& f);             // the seven facts: a stage is installed AND the launch takes a plant step
void note_closed_loop_read(TinyBatch* b);                             // the `last` flags <- those facts; the three logs are the LAST solve call's: rows = 0
int bind_closed_loop_args(TinyBatch* b, const PathDecision& D, SolveArgs& a);   // the one-row launch: blocks built where out of date, logs sized, the PD ... PA fields of `a`
struct StepBases {                                                    // the four counters and the two log pointers a stretch of MPC steps re-bases
    int dist0 = 0, meas0 = 0, score0 = 0, act0 = 0;
    double *state_log = nullptr, *est_log = nullptr;
    bool pd = false, pm = false, ps = false, pa = false;
    void capture(const JitKey& k, const SolveArgs& a);                // off the arguments as bound, by the forms the launch takes
    void apply(SolveArgs& a, int done, int batch, int nx) const;      // the stretch that starts `done` steps in
};
struct CoverageLoop { bool noisy = false, filtered = false, scoring = false, actuated = false, own_plant = false, state_log = false, compensated = false; };
int coverage_begin(TinyBatch* b, int steps, CoverageLoop& loop);      // which helper kernels the coverage path's single-step launches take; the logs sized
int coverage_before_launch(TinyBatch* b, const CoverageLoop& loop, int s, GeneralArgs& a);        // step s: this step's disturbance block, the measurement, the correction -> a.dist, a.x0
int coverage_after_launch(TinyBatch* b, const CoverageLoop& loop, int s, const GeneralArgs& a);   // step s: prediction, actuator, plant step, state log row, score
void advance_closed_loop_counters(TinyBatch* b, int steps);           // behind a solve call: every counter whose stage applied moves `steps` on
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
