// batch_dispatch.hpp -- what batch_api.hip (the C ABI), batch_dispatch.hip (kernel selection, launch forms), batch_tables.hip (lane
// tables), batch_helpers.hip (helper kernels, on-demand buffers) and batch_instance.hip (per-instance problem data) share.
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
// ---- every instance its own problem data (batch_instance.hip; the state: InstanceBox ... Disturbance of batch_impl.hpp)
// what a launch calls: the blocks the kernels read, rebuilt where a setter or an enable switch left them out of date -- the box first and
// synchronously (it may change the UB decision), the other two enqueued on the batch's stream; nothing out of date: a few flag tests, no
// HIP call -- / the `last` flags <- what the kernel about to be launched reads
int ensure_instance_data(TinyBatch* b);
void note_instance_data_read(TinyBatch* b);
void instance_data_settings_changed(TinyBatch* b);   // tiny_batch_update_settings: what an enable switch leaves out of date
// a shared setter is about to install one box / half-space set (0 static, 1 time-varying) / cone set for all: the per-instance one goes,
// its buffers freed once the stream has run dry of their readers (nothing installed: no HIP call)
int drop_instance_bounds(TinyBatch* b);
int drop_instance_linear(TinyBatch* b, int set);
int drop_instance_cones(TinyBatch* b);
// half-spaces: is a per-instance set installed AND one of its families enabled (bit 0 static, bit 1 time-varying) / the block stride of
// such a set: the smallest power of two that holds the enabled counts.  Cones: installed AND a cone family on.  Disturbance: installed
// AND the next launch takes a plant step (advance_x0, or fused steps) / the row its first MPC step takes, as the kernels' int
int inst_lin_active(const TinyBatch* b);
int inst_lin_kmax(const TinyBatch* b);
bool inst_cones_active(const TinyBatch* b);
bool disturbance_active(const TinyBatch* b);
int dist_step_base(const TinyBatch* b);
// a plant of its own: installed AND the next launch takes a plant step / the state log: switched on AND the next launch takes a plant
// step / the pointer a PP form reads (SolveArgs::plant: bit 0 says "one block for all") / room for `rows` rows of the log, none written
// yet / the coverage path's plant step behind one single-step launch: the new states from x0, the u0 of the x|u record and the plant,
// plus this step's disturbance block (null: none), for the instances whose launch ran an iteration; then x0 <- them / row `row` of the
// log <- x0 as it is now
bool plant_active(const TinyBatch* b);
bool state_log_active(const TinyBatch* b);
int ensure_plant_blocks(TinyBatch* b);          // (the blocks of the PP forms, built where the setter left them out of date; enqueued on the batch's stream)
const double* plant_kernel_pointer(const TinyBatch* b);
int begin_state_log(TinyBatch* b, int rows);
int enqueue_coverage_plant_step(TinyBatch* b, const double* dist_block);
// measurement noise: installed AND the next launch takes a plant step / the counter as the kernels take it / the coverage path's
// measurements of one MPC step, xm <- fl(x0 + row `step` of the sequence): the array the launch takes as its x0 (x0 itself where the
// row lies outside the sequence: nothing is enqueued)
bool measurement_active(const TinyBatch* b);
int meas_step_base(const TinyBatch* b);
int enqueue_coverage_measurement(TinyBatch* b, long step, const double** x0_of_launch);
int enqueue_state_log_row(TinyBatch* b, int row);
// a state estimator: installed AND the next launch takes a plant step / the gain blocks of the PE forms and the MODEL's plant block,
// built where they are missing or out of date / the pointers a PE form reads (SolveArgs::est_gain, est_model: bit 0 says "one block
// for all") / room for `rows` rows of the estimate log / the coverage path's two helper kernels around one single-step launch: in
// front, xhat <- the correction of the measurement `*x0_of_launch` names (x0, or the measurement helper's array) under xp, handed to
// the launch as its x0 and written to row `log_row` of the log; behind, xp <- the model's prediction from xhat and the u0 of the x|u
// record, for the instances whose launch ran an iteration
bool estimator_active(const TinyBatch* b);
int ensure_estimator_blocks(TinyBatch* b);
const double* estimator_gain_pointer(const TinyBatch* b);
const double* model_kernel_pointer(const TinyBatch* b);
int begin_estimate_log(TinyBatch* b, int rows);
int enqueue_coverage_correction(TinyBatch* b, int log_row, const double** x0_of_launch);
int enqueue_coverage_prediction(TinyBatch* b);
// a closed-loop score: installed AND the next launch takes a plant step / the score step counter as the kernels take it / the setup
// blocks of the PS forms, built where they are missing or out of date / the pointer a PS form reads (SolveArgs::score_tab: bit 0 says
// "one block for all") / the coverage path's helper kernel behind one single-step launch and its plant step: the record of every
// instance whose launch ran an iteration takes z = [x0 as handed on | u0] in, as score step `step`
bool score_active(const TinyBatch* b);
int score_step_base(const TinyBatch* b);
int ensure_score_blocks(TinyBatch* b);
const double* score_kernel_pointer(const TinyBatch* b);
int enqueue_coverage_score(TinyBatch* b, long step);
// an actuator model: it or an actuation-noise sequence is installed AND the next launch takes a plant step / the actuation step counter
// as the kernels take it / the setup blocks, the log of `rows` MPC steps and the record the PA forms read (SolveArgs::act), made and
// written on the stream in front of a solve call's first launch / the coverage path's helper kernel behind one single-step launch: the
// applied control of actuation step `step` into Actuator::ua (what the plant and score helpers behind it read), the lag's record and
// row `log_row` of the log / the log sized for a coverage launch
bool actuator_active(const TinyBatch* b);
int actuation_step_base(const TinyBatch* b);
int ensure_actuator_launch(TinyBatch* b, int rows, const ActuatorLaunch** out);
int enqueue_coverage_actuator(TinyBatch* b, long step, int log_row);
int begin_actuation_log(TinyBatch* b, int rows);
// frees and nulls every device buffer a family's struct names (the caller has seen the stream run dry of their readers)
template <class S>
void free_buffers(S& s) { s.each_buffer([](auto*& p) { if (p) (void)hipFree(p); p = nullptr; }); }
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
