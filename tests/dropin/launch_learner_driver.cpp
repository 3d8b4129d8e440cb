// launch_learner_driver.cpp -- the launch-form learner (csrc/launch_learner.hpp) driven by a script, without a GPU.  Stand-alone, one command:
//     hipcc -x c++ -std=c++17 -I tinympc_amd/csrc tests/dropin/launch_learner_driver.cpp -o driver
//     driver < SCRIPT
// The script holds one event per line, named after the learner's transitions, with their arguments; after every line the driver prints
// one line: the event, every field of the learner, the answer of every query, and what the event returned (tests/test_launch_learner_cpu.py
// compares them with tables derived from the rules).  What TinyBatch passes into the learner is the driver's context:
//     ctx key=value ...                         auto_split hist_pending repack_growth repack_after max_iter: the queries' arguments
//     model nx nu N wps max_iter ct growth num_cus    the SplitModel a fresh histogram is judged with
//     hist bin:count ...                        the histogram the next probe_arrived / histogram_read_back delivers (other bins 0)
// Events: probe_arrived have_reading ms max_iter | histogram_read_back max_iter | one_row_solve_counted auto_split | tile_solve_counted |
//     fused_solve_counted regroup_auto | repack_after_set | repack_growth_set | step_regroup_set | lockstep_estimate_arrived rows_max total |
//     growth_probe_on_trial | tile_probe_enqueued | timed_launch_recorded cap | choose_split (the model's answer alone) |
//     plan_import same_settings far_batch [field=value ...]    to_plan of the state, the fields overwritten, plan_in_range asked, and -- when
//                                               it is in range -- from_plan into the same learner, as tiny_batch_set_plan does (no field: a round trip)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "launch_learner.hpp"

using namespace tinympc_amd;

static unsigned long long fnv(const unsigned* h, size_t n) {
    unsigned long long x = 1469598103934665603ull;
    for (size_t i = 0; i < n * sizeof(unsigned); ++i) x = (x ^ reinterpret_cast<const unsigned char*>(h)[i]) * 1099511628211ull;
    return x;
}

int main() {
    LaunchLearner L;
    SplitModel model = {12, 4, 10, 2, 100, 1, 0, 256};
    std::map<std::string, long> ctx = {{"auto_split", 1}, {"hist_pending", 0}, {"repack_growth", 0}, {"repack_after", -1}, {"max_iter", 100}};
    static unsigned hist[HIST_BINS];
    static TinyBatchPlan plan;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string ev, word;
        if (!(in >> ev) || ev[0] == '#') continue;
        std::ostringstream extra;
        auto num = [&]() { double v = 0.0; in >> word; v = strtod(word.c_str(), nullptr); return v; };
        if (ev == "ctx") {
            while (in >> word) ctx.at(word.substr(0, word.find('='))) = atol(word.c_str() + word.find('=') + 1);
        } else if (ev == "model") {
            int* f[] = {&model.nx, &model.nu, &model.N, &model.wps, &model.max_iter, &model.ct, &model.growth, &model.num_cus};
            for (int* p : f) *p = (int)num();
        } else if (ev == "hist") {
            memset(hist, 0, sizeof(hist));
            while (in >> word) hist[atoi(word.c_str())] = (unsigned)strtoul(word.c_str() + word.find(':') + 1, nullptr, 10);
        } else if (ev == "probe_arrived") {
            const bool have = num() != 0.0;
            const float ms = (float)num();
            L.probe_arrived(have, ms, hist, (int)num(), model);
        } else if (ev == "histogram_read_back") L.histogram_read_back(hist, (int)num(), model);
        else if (ev == "one_row_solve_counted") L.one_row_solve_counted(num() != 0.0);
        else if (ev == "tile_solve_counted") extra << " returned=" << (L.tile_solve_counted() ? 1 : 0);
        else if (ev == "fused_solve_counted") L.fused_solve_counted(num() != 0.0);
        else if (ev == "repack_after_set") L.repack_after_set();
        else if (ev == "repack_growth_set") L.repack_growth_set();
        else if (ev == "step_regroup_set") L.step_regroup_set();
        else if (ev == "lockstep_estimate_arrived") {
            auto count = [&]() { in >> word; return strtoull(word.c_str(), nullptr, 10); };
            const unsigned long long rows_max = count(), total = count();
            L.lockstep_estimate_arrived(rows_max, total);
        } else if (ev == "growth_probe_on_trial") extra << " returned=" << L.growth_probe_on_trial();
        else if (ev == "tile_probe_enqueued") L.tile_probe_enqueued();
        else if (ev == "timed_launch_recorded") L.timed_launch_recorded((int)num());
        else if (ev == "choose_split") {
            const SplitChoice c = choose_split(model, hist);
            char buf[96];
            snprintf(buf, sizeof(buf), " k=%d ratio=%.17g growth=%d", c.k, c.ratio, c.growth);
            extra << buf;
        } else if (ev == "plan_import") {
            const bool same = num() != 0.0, far = num() != 0.0;
            memset(&plan, 0, sizeof(plan));
            plan.batch = 1;
            L.to_plan(&plan, (int)ctx["repack_growth"]);
            std::map<std::string, int*> ints = {{"batch", &plan.batch}, {"auto_verdict", &plan.auto_verdict}, {"auto_cap", &plan.auto_cap}, {"auto_cap_max_iter", &plan.auto_cap_max_iter},
                                                {"auto_growth", &plan.auto_growth}, {"growth_verdict", &plan.growth_verdict}, {"auto_probes", &plan.auto_probes},
                                                {"tile_verdict", &plan.tile_verdict}, {"regroup_verdict", &plan.regroup_verdict}, {"hist_valid", &plan.hist_valid}};
            std::map<std::string, double*> dbls = {{"auto_plain_rate", &plan.auto_plain_rate}, {"auto_split_rate", &plan.auto_split_rate}, {"auto_gain", &plan.auto_gain},
                                                   {"tile_rate", &plan.tile_rate}, {"lockstep_ratio", &plan.lockstep_ratio}};
            while (in >> word) {
                const std::string key = word.substr(0, word.find('=')), val = word.substr(word.find('=') + 1);
                if (key == "hist") memcpy(plan.hist, hist, sizeof(hist));          // (hist=1: the plan carries the current histogram)
                else if (ints.count(key)) *ints[key] = atoi(val.c_str());
                else *dbls.at(key) = strtod(val.c_str(), nullptr);                 // (strtod reads nan and inf)
            }
            const bool ok = LaunchLearner::plan_in_range(&plan);
            extra << " in_range=" << (ok ? 1 : 0) << " plan_open_questions=" << plan.open_questions;
            if (ok) L.from_plan(&plan, same, far);
        } else {
            fprintf(stderr, "unknown event %s\n", ev.c_str());
            return 2;
        }
        const int rg = (int)ctx["repack_growth"], mi = (int)ctx["max_iter"];
        const bool as = ctx["auto_split"] != 0, hp = ctx["hist_pending"] != 0;
        memset(&plan, 0, sizeof(plan));
        L.to_plan(&plan, rg);
        const bool gp = L.growth_probe_wanted(as, hp, rg, mi);
        char buf[1024];
        snprintf(buf, sizeof(buf),
                 "event=%s auto_verdict=%d auto_cap=%d auto_cap_max_iter=%d auto_growth=%d growth_alt=%d growth_verdict=%d auto_probes=%d auto_since=%d auto_last_cap=%d "
                 "auto_plain_rate=%.17g auto_split_rate=%.17g auto_gain=%.17g tile_verdict=%d tile_since=%d tile_rate=%.17g regroup_verdict=%d regroup_since=%d "
                 "lockstep_ratio=%.17g probe_was_tile=%d probe_was_growth=%d hist_copy=%zu:%llu "
                 "one_row_settled=%d tile_probe_wanted=%d growth_probe_wanted=%d auto_probe_wanted=%d solve_cap=%d stage_growth=%d fresh=%d open_questions=%d",
                 ev.c_str(), L.auto_verdict, L.auto_cap, L.auto_cap_max_iter, L.auto_growth, L.growth_alt, L.growth_verdict, L.auto_probes, L.auto_since, L.auto_last_cap,
                 L.auto_plain_rate, L.auto_split_rate, L.auto_gain, L.tile_verdict, L.tile_since, L.tile_rate, L.regroup_verdict, L.regroup_since, L.lockstep_ratio,
                 L.probe_was_tile ? 1 : 0, L.probe_was_growth ? 1 : 0, L.hist_copy.size(), L.hist_copy.empty() ? 0ull : fnv(L.hist_copy.data(), L.hist_copy.size()),
                 L.one_row_settled(rg) ? 1 : 0, L.tile_probe_wanted(rg, hp) ? 1 : 0, gp ? 1 : 0, L.auto_probe_wanted(as, hp, gp) ? 1 : 0,
                 L.solve_cap((int)ctx["repack_after"], as, mi), L.stage_growth(rg), L.fresh() ? 1 : 0, plan.open_questions);
        std::cout << buf << extra.str() << "\n";
    }
    return 0;
}
