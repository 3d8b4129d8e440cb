// launch_learner.hpp -- what the clock has taught the dispatch about ONE batch (plain or split solve with its K and stage schedule, the tile
// kernel's dynamic form for a one-row shape, stretches of MPC steps for a fused launch) and the cost models it consults.  Plain C++17, no
// HIP: tests/dropin/launch_learner_driver.cpp runs every rule on the host.  TinyBatch holds one LaunchLearner (`learn`); events, buffers,
// pending flags and options stay there and come in as arguments.  Other files READ the fields; only these member functions write them.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/tinympc_amd.h"

namespace tinympc_amd {
constexpr int HIST_BINS = 1024;          // bins of an iteration histogram: TinyBatch::HIST_BINS, TinyBatchPlan::hist
// Predicted launch time (arbitrary units: wave-iterations per wave slot) of a solve whose instances need hist[i] iterations,
// four instances per wave in lock step (a wave runs to the slowest of its rows: E[max of 4] under independence), split at
// `cap` (0 = plain) with the stage schedule of launch_solve (cap, 2 cap, 4 cap, ... max_iter).  A stage costs its work
// spread over the wave slots, or -- when it has fewer waves than slots -- the depth of its longest wave at a lone wave's
// pace (half the paired pace), plus a launch and one record reload / store per instance it carries.
inline double predicted_time(const unsigned* hist, int max_iter, int cap, int growth, double slots, double launch_iters, double reload_iters, bool dynamic = false) {
    const int M = std::min(max_iter, HIST_BINS - 1);
    std::vector<double> cum(M + 2, 0.0);                     // cum[i] = instances with iter <= i
    double n = 0.0;
    for (int i = 0; i <= M; ++i) { n += hist[i]; cum[i] = n; }
    if (n <= 0.0) return 0.0;
    auto stage = [&](int lo, int hi, bool first) {           // iterations lo+1 .. hi for the instances with iter > lo
        const double open = first ? n : n - cum[lo];
        if (open <= 0.0) return 0.0;
        double work = 0.0, second = 0.0;                     // E[d], E[d^2] of a wave's depth d: sum_j P(d > j), sum_j (2j+1) P(d > j)
        int depth = 0;
        for (int i = lo; i < hi; ++i) {
            const double F = (cum[i] - (first ? 0.0 : cum[lo])) / open;          // P(iter <= i | open)
            const double p = 1.0 - F * F * F * F;
            work += p;
            second += (2.0 * (i - lo) + 1.0) * p;
            if (p > 1e-12) depth = i + 1 - lo;
        }
        const double waves = open / 4.0, per_slot = waves / slots;
        // a follow-up stage that walks its list with a fixed grid stride: a slot's time is the SUM of its waves' depths, the stage
        // ends with the slowest slot (mean + 2.5 sigma of that sum); the first stage is balanced by the dispatcher, a follow-up
        // stage whose waves draw their tiles from a counter (`dynamic`) ends at most one wave's depth after the mean
        const double imbalance = first ? 0.0 : (dynamic ? std::min(0.5 * depth, 2.5 * sqrt(std::max(second - work * work, 0.0)))
                                                        : 2.5 * sqrt(std::max(per_slot, 1e-9) * std::max(second - work * work, 0.0)));
        const double t = std::max(work * per_slot + imbalance, 0.5 * depth);
        return t + launch_iters + (first ? 0.0 : reload_iters * std::max(1.0, waves / slots));
    };
    if (cap <= 0 || cap >= M) return stage(0, M, true);
    double t = stage(0, cap, true);
    for (long base = cap; base < M; base *= growth) {
        const int hi = (int)std::min<long>(M, base * growth);
        t += stage((int)base, hi, false);
        if (hi >= M) break;
    }
    return t;
}

// one wave-iteration (4 instances) of the one-row kernel in microseconds: its FLOPs at ~75 % of a SIMD's FP64 issue rate (76.8 GFLOP/s
// per SIMD), shared by the waves of the SIMD -- 1.7 us for the quadrotor at two waves (measured 1.64)
inline double wave_iteration_us(int nx, int nu, int N, int wps) {
    const double S = (double)nx * N + (double)nu * (N - 1);
    const double fl = 4.0 * S + 2.0 * nx * nx + 3.0 * nx + (N - 1.0) * (4.0 * nx * nx + 8.0 * nx * nu + 2.0 * nu * nu + 4.0 * nu + 5.0 * nx) + 11.0 * S;
    return 4.0 * fl * wps / (76.8e3 * (wps == 2 ? 0.75 : 0.45));
}
struct SplitChoice { int k; double ratio; int growth; };      // K (0: plain), predicted time of the best split / plain launch, its stage growth
// the K (multiple of check_termination) with the smallest predicted time, 0 when a plain launch is within 5 % of it; wps: the shape's
// solve_kernel_waves_per_simd (admm_kernel.hip.h)
inline SplitChoice choose_split_for(int nx, int nu, int N, int wps, int M, int ct, int gr, int num_cus, const unsigned* hist) {
    const double slots = (double)num_cus * 4.0 * wps;         // wave slots of the chip
    // one wave-iteration in microseconds (above); the fixed costs of a stage in that unit: ~8 us of launch latency, and the record
    // reload + store (2.45 us per wave for the quadrotor's 156 slots)
    const double S = (double)nx * N + (double)nu * (N - 1);
    const double t_it = wave_iteration_us(nx, nu, N, wps);
    const double launch_iters = 8.0 / t_it, reload_iters = 2.45 * (S / 156.0) / t_it;
    const double plain = predicted_time(hist, M, 0, 2, slots, launch_iters, reload_iters);
    double best = plain;
    int best_k = 0, best_gr = gr > 0 ? gr : 2;
    // gr <= 0: the stage schedule is part of the question -- K, 2K, 4K, ... or K, 4K, 16K, ... (fewer launches, deeper lock step)
    const int grs[2] = {gr > 0 ? gr : 2, gr > 0 ? gr : 4};
    for (int gi = 0; gi < (gr > 0 ? 1 : 2); ++gi) {
        for (int k = std::max(ct, 4 - 4 % ct); k <= M / 2; k += ct) {
            if (k > 64 && k % 8) continue;                    // coarser steps far out
            const double t = predicted_time(hist, M, k, grs[gi], slots, launch_iters, reload_iters);
            if (t < best) { best = t; best_k = k; best_gr = grs[gi]; }
        }
    }
    // One check interval of margin: the histogram is the LAST solve's, and being a step late costs next to nothing (measured on config 3,
    // mode 8-9 of 262 144: K = 10 ... 14 within 3 %) while being a step early sends the whole mode through a second launch (K = 9
    // +6 %, K = 8 +60 %)
    if (best_k > 0 && best_k + ct <= M / 2 && predicted_time(hist, M, best_k + ct, best_gr, slots, launch_iters, reload_iters) <= 1.01 * best) best_k += ct;
    return {(plain > 0.0 && best < 0.95 * plain) ? best_k : 0, plain > 0.0 ? best / plain : 1.0, best_gr};
}
struct SplitModel { int nx, nu, N, wps, max_iter, ct, growth, num_cus; };      // choose_split_for's view of a batch (batch_helpers.hip split_model)
inline SplitChoice choose_split(const SplitModel& m, const unsigned* hist) { return choose_split_for(m.nx, m.nu, m.N, m.wps, m.max_iter, m.ct, m.growth, m.num_cus, hist); }
// stretches of `steps` MPC steps: `lead` steps first (0: none), then K steps each; a short remainder joins the stretch before it
inline std::vector<int> regroup_stretches(int steps, int K, int lead) {
    std::vector<int> out;
    int left = steps;
    if (lead > 0 && left > lead) { out.push_back(lead); left -= lead; }
    while (left > 0) {
        int n = std::min(K, left);
        if (left - n > 0 && left - n < (K + 1) / 2) n = left;
        out.push_back(n);
        left -= n;
    }
    return out;
}
inline int regroup_auto_k(int steps) { return std::max(8, (steps + 3) / 4); }
// the two-stream form (halves of the batch half a stretch out of step) only makes sense when more than one stretch is left after the
// lead step: the condition the launch and tiny_step_regroup_plan share
inline bool regroup_two_streams_apply(int steps, int lead, int K) { return steps - lead > K; }

struct LaunchLearner {
    int auto_verdict = 0;                // plain or split solve: 0 undecided, 1 the split was measured faster (kept), -1 measured slower (plain launches from now on)
    int auto_cap = 0, auto_cap_max_iter = 0;   // the K the cost model derived from the last histogram (0 = plain is predicted as fast), the max_iter it holds for
    int auto_growth = 2, growth_alt = 2, growth_verdict = 0;   // the stage schedule in use; the one on trial; 1 = the clock has compared the two
    int auto_probes = 0;                 // timed solves so far (the first one carries one-time costs -- code object load -- and is not used)
    int auto_since = 0;                  // eligible solves since the last verdict: every 32nd one re-opens the question (plain + split timed again)
    int auto_last_cap = 0;               // the cap the timed launch ran with
    double auto_plain_rate = 0.0, auto_split_rate = 0.0;   // ms per instance-iteration of the last plain and the last split launch
    double auto_gain = 0.0;              // predicted time of the split solve / plain solve (diagnostics)
    int tile_verdict = 0, tile_since = 0;        // the dynamic tile form tried on a one-row shape: 1 kept, -1 rejected, 0 open
    double tile_rate = 0.0;
    int regroup_verdict = 0, regroup_since = 0;  // step_regroup: 0 open, 1 on, -1 off (the estimate of the last fused launch decided)
    double lockstep_ratio = 0.0;         // the last estimate (1.0 = rows of a wave agree)
    bool probe_was_tile = false, probe_was_growth = false;   // what the probe in flight tried
    std::vector<unsigned> hist_copy;     // the histogram the schedule in use was derived from (the pinned one is overwritten asynchronously)

    // ---- queries: the decisions that only read the state (the options and pending flags are TinyBatch's)
    bool one_row_settled(int repack_growth) const { return auto_plain_rate > 0.0 && (auto_verdict == -1 || auto_cap == 0 || (auto_verdict == 1 && (growth_verdict != 0 || repack_growth >= 2))); }
    bool tile_probe_wanted(int repack_growth, bool hist_pending) const { return tile_verdict == 0 && one_row_settled(repack_growth) && !hist_pending; }
    bool growth_probe_wanted(bool auto_split, bool hist_pending, int repack_growth, int max_iter) const {      // a kept split asks ONE more question: the other stage schedule
        return auto_split && !hist_pending && auto_verdict == 1 && growth_verdict == 0 && repack_growth < 2 && auto_cap > 0 && auto_cap_max_iter == max_iter && auto_split_rate > 0.0;
    }
    bool auto_probe_wanted(bool auto_split, bool hist_pending, bool growth_probe) const { return (auto_split && !hist_pending && auto_verdict == 0) || growth_probe; }
    int solve_cap(int repack_after, bool auto_split, int max_iter) const {      // (before its rounding to check_termination)
        return repack_after > 0 ? repack_after : ((auto_split && auto_cap_max_iter == max_iter && auto_verdict >= 0 && auto_plain_rate > 0.0) ? auto_cap : 0);
    }
    int stage_growth(int repack_growth) const { return repack_growth >= 2 ? repack_growth : std::max(2, auto_growth); }   // (option 0: the model's schedule, confirmed or overturned by the clock)
    bool fresh() const { return auto_probes == 0 && auto_verdict == 0; }        // no verdict of its own, no imported plan

    // ---- transitions, named for what happened
    // the clock's word on the probe in flight (ms, if have_reading) and the iteration histogram of its solve have arrived
    void probe_arrived(bool have_reading, float ms, const unsigned* hist, int max_iter, const SplitModel& m) {
        double iters = 0.0;
        for (int i = 0; i < HIST_BINS; ++i) iters += (double)i * hist[i];
        if (++auto_probes > 1 && iters > 0.0 && have_reading && ms > 0.0f) {
            const double rate = (double)ms / iters;      // milliseconds per instance-iteration, plain or split
            if (probe_was_tile) {
                // the dynamic slot form of the tile kernel (one-row layout) against the best the one-row kernel did on this batch
                tile_rate = rate;
                const double best = (auto_verdict == 1 && auto_split_rate > 0.0) ? auto_split_rate : auto_plain_rate;
                if (best > 0.0) tile_verdict = rate < 0.97 * best ? 1 : -1;
            } else if (probe_was_growth) {
                // the other stage schedule of a kept split (K, 4K, ... against K, 2K, ...): the cost model ranks them, the clock decides
                if (auto_split_rate > 0.0 && rate < 0.97 * auto_split_rate) { auto_growth = growth_alt; auto_split_rate = rate; }
                growth_verdict = 1;
            } else {
                if (auto_last_cap > 0) auto_split_rate = rate; else auto_plain_rate = rate;
                if (auto_last_cap > 0 && auto_plain_rate > 0.0 && auto_verdict == 0) auto_verdict = auto_split_rate < 0.97 * auto_plain_rate ? 1 : -1;
            }
        }
        if (probe_was_growth) growth_verdict = 1;           // (asked once, whatever became of the reading)
        probe_was_tile = false; probe_was_growth = false;
        if (auto_verdict == 0) rechoose(hist, max_iter, m);      // (a kept split keeps its K; a rejected one stays rejected until the options change)
    }
    // the histogram arrived through the diagnostic read-back instead: the probe's clock reading is dropped with it, the next probe starts clean
    void histogram_read_back(const unsigned* hist, int max_iter, const SplitModel& m) {
        probe_was_tile = probe_was_growth = false;
        if (auto_verdict == 0) rechoose(hist, max_iter, m);      // (a decided batch keeps its K AND the stage schedule the clock chose)
    }
    // Distributions drift: the 32nd eligible solve after a verdict re-opens the questions (the 64th fused one: step_regroup's).  The field
    // lists of the two 32-solve resets and of the option resets below differ (tile_since, auto_split_rate ...): inherited, not designed.
    void one_row_solve_counted(bool auto_split) { if (auto_split && auto_verdict != 0 && ++auto_since >= 32) { auto_since = 0; auto_verdict = 0; growth_verdict = 0; auto_plain_rate = 0.0; tile_verdict = 0; } }
    bool tile_solve_counted() {          // true: both questions are open again, this solve goes back to the one-row kernel
        if (!(tile_verdict == 1 && ++tile_since >= 32)) return false;
        tile_since = 0; tile_verdict = 0; auto_verdict = 0; growth_verdict = 0; auto_plain_rate = 0.0; auto_since = 0;
        return true;
    }
    void fused_solve_counted(bool regroup_auto) { if (regroup_auto && regroup_verdict != 0 && ++regroup_since >= 64) { regroup_since = 0; regroup_verdict = 0; } }
    void repack_after_set() { auto_cap = 0; hist_copy.clear(); auto_verdict = 0; growth_verdict = 0; auto_plain_rate = auto_split_rate = 0.0; auto_probes = 0; }
    void repack_growth_set() { growth_verdict = 0; }
    void step_regroup_set() { regroup_verdict = 0; regroup_since = 0; }
    void lockstep_estimate_arrived(unsigned long long rows_max, unsigned long long total) {   // {4 x sum over waves of the largest iteration total, sum of the totals}
        lockstep_ratio = total > 0ull ? (double)rows_max / (double)total : 1.0;
        if (regroup_verdict == 0) regroup_verdict = lockstep_ratio >= 1.05 ? 1 : -1;
    }
    int growth_probe_on_trial() { growth_alt = auto_growth == 2 ? 4 : 2; probe_was_growth = true; return growth_alt; }   // the other schedule of 2 | 4
    void tile_probe_enqueued() { probe_was_tile = true; }
    void timed_launch_recorded(int cap) { auto_last_cap = cap; }

    // ---- the state as a TinyBatchPlan (its header fields, magic ... check_termination, are tiny_batch_get_plan's / set_plan's)
    void to_plan(TinyBatchPlan* out, int repack_growth) const {
        out->auto_verdict = auto_verdict; out->auto_cap = auto_cap; out->auto_cap_max_iter = auto_cap_max_iter;
        out->auto_growth = auto_growth; out->growth_verdict = growth_verdict; out->auto_probes = auto_probes;
        out->auto_plain_rate = auto_plain_rate; out->auto_split_rate = auto_split_rate; out->auto_gain = auto_gain;
        out->tile_verdict = tile_verdict; out->tile_rate = tile_rate;
        out->regroup_verdict = regroup_verdict; out->lockstep_ratio = lockstep_ratio;
        out->hist_valid = hist_copy.size() == (size_t)HIST_BINS ? 1 : 0;
        if (out->hist_valid) memcpy(out->hist, hist_copy.data(), sizeof(out->hist));
        // open questions: plain-or-split undecided (while a split is on the table), the other stage schedule of a kept split untried
        out->open_questions = ((auto_verdict == 0 && !(auto_plain_rate > 0.0 && auto_cap == 0)) ? 1 : 0) + ((auto_verdict == 1 && growth_verdict == 0 && repack_growth < 2) ? 1 : 0);
    }
    // every field is checked (a plan is a POD read from a file): verdicts in {-1, 0, 1}, counts non-negative, clock
    // readings finite and non-negative.  A plan is advice only -- results never depend on it -- but a corrupt one must not pin a launch form
    static bool plan_in_range(const TinyBatchPlan* in) {
        auto verdict = [](int v) { return v >= -1 && v <= 1; };
        auto rate = [](double v) { return v >= 0.0 && v < 1e300; };
        return !(!verdict(in->auto_verdict) || !verdict(in->tile_verdict) || !verdict(in->regroup_verdict) || !verdict(in->growth_verdict) ||
                 in->auto_cap < 0 || in->auto_cap >= HIST_BINS || (in->auto_growth != 2 && in->auto_growth != 4) || in->auto_cap_max_iter < 0 ||
                 in->auto_probes < 0 || in->batch <= 0 || !rate(in->auto_plain_rate) || !rate(in->auto_split_rate) || !rate(in->auto_gain) || !rate(in->tile_rate) ||
                 !rate(in->lockstep_ratio) || (in->hist_valid != 0 && in->hist_valid != 1));
    }
    // A verdict whose supporting clock reading is missing, or that was made under other settings than the handle's, counts as OPEN
    void from_plan(const TinyBatchPlan* in, bool same_settings, bool far_batch) {
        auto_verdict = (same_settings && !far_batch && in->auto_plain_rate > 0.0 && (in->auto_verdict != 1 || in->auto_split_rate > 0.0)) ? in->auto_verdict : 0;
        auto_cap = in->auto_cap; auto_cap_max_iter = in->auto_cap_max_iter;
        auto_growth = in->auto_growth; growth_verdict = auto_verdict == 1 ? in->growth_verdict : 0; auto_probes = std::max(2, in->auto_probes);
        auto_plain_rate = in->auto_plain_rate; auto_split_rate = in->auto_split_rate; auto_gain = in->auto_gain;
        tile_verdict = (same_settings && !far_batch && (in->tile_verdict != 1 || in->tile_rate > 0.0)) ? in->tile_verdict : 0; tile_rate = in->tile_rate;
        regroup_verdict = far_batch ? 0 : in->regroup_verdict; lockstep_ratio = in->lockstep_ratio;
        if (in->hist_valid) hist_copy.assign(in->hist, in->hist + HIST_BINS); else hist_copy.clear();
        auto_since = tile_since = regroup_since = 0;
        probe_was_tile = false; probe_was_growth = false; auto_last_cap = 0;
    }
private:
    void rechoose(const unsigned* hist, int max_iter, const SplitModel& m) {    // K, predicted gain, schedule and hist_copy from a fresh histogram
        const SplitChoice c = choose_split(m, hist);
        auto_cap = c.k; auto_gain = c.ratio; auto_growth = c.growth; auto_cap_max_iter = max_iter;
        hist_copy.assign(hist, hist + HIST_BINS);
    }
};
}  // namespace tinympc_amd
