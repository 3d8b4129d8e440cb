// actuator_path_driver.cpp -- the kernel choice and the one-row variant choice under an actuator model (csrc/kernel_path.hpp
// PathFacts::actuator, csrc/one_row_variant.hpp VariantFacts::pa), asked without a GPU.  The actuator's plant step is a chain over the
// applied control through a plant block, so the sweeps restate its rule on the answer the same facts get with a PLANT installed and the
// fact off.  Stand-alone, the interface of score_path_driver.cpp:
//     hipcc -x c++ -std=c++17 -I tinympc_amd/csrc tests/dropin/actuator_path_driver.cpp -o driver
//     driver path < QUERIES   one line of `fact=value ...` per query (facts not named: 0) -> the decision
//     driver paths            every consistent PathFacts (the tile kernel's own facts but has_tile and prefer_tile left at 0, one stride and one family of
//                             half-spaces, jit_failed left at 0 -- variant_jit_failed closes hipRTC the same way --: the fact meets none of them):
//                             actuator = 0 must not name pa and must answer, field by field, what a PathFacts with the field left at its
//                             default answers; actuator = 1 against the restated rule.  Prints the counts and `violations=`
//     driver variants         choose_one_row_variant over every VariantFacts with pa = 1 (on the PP, the PM and the PE form, each with and
//                             without PD and PS) against the choice with pa = 0
//     driver message          value and text of the refusal
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kernel_path.hpp"
#include "one_row_variant.hpp"

using namespace tinympc_amd;

struct PFact { const char* name; bool PathFacts::*flag; int PathFacts::*number; std::vector<int> values; };
static const std::vector<PFact>& path_facts() {
    using P = PathFacts;
    static const std::vector<PFact> all = {
        {"has_entry", &P::has_entry, nullptr, {0, 1}}, {"entry_plain", &P::entry_plain, nullptr, {0, 1}}, {"entry_klin", &P::entry_klin, nullptr, {0}},
        {"fits_box", &P::fits_box, nullptr, {0, 1}}, {"fits", &P::fits, nullptr, {0, 1}}, {"has_tile", &P::has_tile, nullptr, {0, 1}},
        {"tile_is_jit", &P::tile_is_jit, nullptr, {0}}, {"tile_lin", &P::tile_lin, nullptr, {0}}, {"lin_kmax", nullptr, &P::lin_kmax, {0, 4}},
        {"planes_fit", &P::planes_fit, nullptr, {0, 1}}, {"pl_planes_fit", &P::pl_planes_fit, nullptr, {0, 1}}, {"soc", &P::soc, nullptr, {0, 1}},
        {"lin_families", nullptr, &P::lin_families, {0, 1}}, {"cones_overlap", &P::cones_overlap, nullptr, {0, 1}}, {"hetero", &P::hetero, nullptr, {0, 1}},
        {"tile_ext", &P::tile_ext, nullptr, {0}}, {"adaptive", &P::adaptive, nullptr, {0, 1}}, {"debug", &P::debug, nullptr, {0, 1}},
        {"inst_bounds", &P::inst_bounds, nullptr, {0, 1}}, {"inst_lin", nullptr, &P::inst_lin, {0, 1}}, {"inst_cones", &P::inst_cones, nullptr, {0, 1}},
        {"force_general", &P::force_general, nullptr, {0, 1}}, {"no_jit", &P::no_jit, nullptr, {0, 1}}, {"no_tile", &P::no_tile, nullptr, {0}},
        {"prefer_tile", &P::prefer_tile, nullptr, {0, 1}}, {"jit_failed", &P::jit_failed, nullptr, {0}}, {"variant_jit_failed", &P::variant_jit_failed, nullptr, {0, 1}},
        {"tile_soc_failed", &P::tile_soc_failed, nullptr, {0}}, {"disturbance", &P::disturbance, nullptr, {0, 1}}, {"plant", &P::plant, nullptr, {0, 1}},
        {"state_log", &P::state_log, nullptr, {0, 1}}, {"measurement", &P::measurement, nullptr, {0, 1}},
        {"estimator", &P::estimator, nullptr, {0, 1}}, {"score", &P::score, nullptr, {0, 1}}, {"actuator", &P::actuator, nullptr, {0, 1}},
    };
    return all;
}
static void assign(PathFacts& f, const PFact& k, int v) {
    if (k.flag) f.*k.flag = v != 0;
    else f.*k.number = v;
}
static const char* KERNEL_NAME[] = {"ONE_ROW", "TILE", "COVERAGE"};
static bool same(const PathDecision& a, const PathDecision& b) {
    return a.kernel == b.kernel && a.lin == b.lin && a.pl == b.pl && a.pb == b.pb && a.pc == b.pc && a.pd == b.pd && a.pp == b.pp && a.pm == b.pm && a.pe == b.pe && a.ps == b.ps && a.pa == b.pa && a.refusal == b.refusal &&
           !strcmp(a.rule, b.rule);
}
// the rule, restated: what the same facts get with a plant installed and the fact off, with the PA bit on a one-row answer, "pa" in the
// rule pair's own names and, where the plant's refusal stood in for it, the refusal of the first fact of the order that IS on
static PathDecision expected_with_actuator(const PathFacts& f) {
    PathFacts g = f;
    g.actuator = false; g.plant = true;
    PathDecision d = decide_path(g);
    if (d.kernel == ONE_ROW) d.pa = 1;
    for (const char* form : {"pd", "pp", "pm", "pe", "ps"}) {
        if (d.rule == std::string("one_row:") + form) d.rule = "one_row:pa";
        if (d.rule == std::string("cover:") + form) d.rule = "cover:pa";
    }
    if (d.refusal == REFUSE_ADAPTIVE_PLANT && !f.plant)
        d.refusal = f.state_log ? REFUSE_ADAPTIVE_STATE_LOG : f.measurement ? REFUSE_ADAPTIVE_MEASUREMENT : f.estimator ? REFUSE_ADAPTIVE_ESTIMATOR : f.score ? REFUSE_ADAPTIVE_SCORE : REFUSE_ADAPTIVE_ACTUATOR;
    return d;
}
// (actuator = 0: a PathFacts built without ever naming the field)
static PathFacts without_the_field(const PathFacts& f) {
    PathFacts g;
    for (const PFact& k : path_facts()) {
        if (!strcmp(k.name, "actuator")) continue;
        if (k.flag) g.*k.flag = f.*k.flag;
        else g.*k.number = f.*k.number;
    }
    return g;
}

static int sweep_paths() {
    const std::vector<PFact>& facts = path_facts();
    std::vector<size_t> at(facts.size(), 0);
    long plain = 0, with_actuator = 0, violations = 0, one_row_pa = 0, cover_pa = 0, tile_with_actuator = 0, refused_12 = 0;
    for (;;) {
        PathFacts f;
        for (size_t i = 0; i < facts.size(); ++i) assign(f, facts[i], facts[i].values[at[i]]);
        if (facts_consistent(f)) {
            const PathDecision d = decide_path(f);
            bool ok = true;
            if (f.actuator) {
                ++with_actuator;
                ok = same(d, expected_with_actuator(f)) && kernel_path_code(d, f) == (d.kernel == ONE_ROW ? 3 : 2) &&
                     (d.kernel != ONE_ROW || (d.pa == 1 && d.pp == 1 && d.ps == (f.score ? 1 : 0)));
                if (d.kernel == TILE) ++tile_with_actuator;
                if (!strcmp(d.rule, "one_row:pa")) ++one_row_pa;
                if (!strcmp(d.rule, "cover:pa")) ++cover_pa;
                if (d.refusal == REFUSE_ADAPTIVE_ACTUATOR) ++refused_12;
            } else {
                ++plain;
                const PathFacts g = without_the_field(f);
                ok = d.pa == 0 && d.refusal != REFUSE_ADAPTIVE_ACTUATOR && strcmp(d.rule, "one_row:pa") && strcmp(d.rule, "cover:pa") && same(d, decide_path(g)) &&
                     kernel_path_code(d, f) == kernel_path_code(decide_path(g), g);
            }
            if (!ok && violations++ < 5)
                printf("violation kernel=%s rule=%s pd=%d pp=%d pm=%d pe=%d ps=%d pa=%d refusal=%d\n", KERNEL_NAME[d.kernel], d.rule, d.pd, d.pp, d.pm, d.pe, d.ps, d.pa, (int)d.refusal);
        }
        size_t i = 0;
        for (; i < facts.size(); ++i) {
            if (++at[i] < facts[i].values.size()) break;
            at[i] = 0;
        }
        if (i == facts.size()) break;
    }
    printf("plain=%ld\nwith_actuator=%ld\nviolations=%ld\none_row_pa=%ld\ncover_pa=%ld\ntile_with_actuator=%ld\nrefused_12=%ld\n", plain, with_actuator, violations, one_row_pa,
           cover_pa, tile_with_actuator, refused_12);
    return violations ? 1 : 0;
}

static int sweep_variants() {
    EntrySlots none = {}, full = {};
    full.has_entry = true;
    for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < 2; ++j)
            for (int l = 0; l < 3; ++l) full.k[i][j][l] = true;
        for (int j = 1; j < 4; ++j) full.klin[i][j] = true;
        full.khet[i] = full.khetub[i] = full.kadapt[i] = true;
        full.khalf[i] = full.kpf[i] = full.khalfpf[i] = true;
    }
    full.kub = full.kubsoc = true;
    long with_pa = 0, violations = 0, key_order = 1;
    for (int entry = 0; entry < 2; ++entry)
        for (int bits = 0; bits < (1 << 11); ++bits)
            for (int lin = 0; lin < 4; ++lin)
                for (int mode = 0; mode < 3; ++mode)
                for (int base = 1; base < 7; ++base) {                   // (the PP, the PM and the PE form, each with or without PD, then the same three with PS)
                    VariantFacts f;
                    f.lin = lin; f.dpp_mode = mode;
                    f.pl = bits & 1; f.pb = bits & 2; f.pc = bits & 4; f.pd = bits & 8; f.soc = bits & 16; f.hetero = bits & 32; f.uniform_ub = bits & 64;
                    f.het_ub = bits & 128; f.half_rows = bits & 256; f.prefetch_on = bits & 512; f.single_step = bits & 1024;
                    f.no_ref_window = true; f.default_grid = true;
                    f.lin_kmax = lin ? 4 : 0; f.il_km = f.pl ? 4 : 0;
                    const int form = (base - 1) % 3;
                    f.pp = true; f.pm = form >= 1; f.pe = form >= 2; f.ps = base > 3; f.pa = true;
                    const EntrySlots& s = entry ? full : none;
                    if (!variant_facts_consistent(f, s)) continue;
                    ++with_pa;
                    const VariantChoice c = choose_one_row_variant(f, s);
                    VariantFacts g = f;
                    g.pa = false;
                    const VariantChoice p = choose_one_row_variant(g, s);
                    JitKey a = c.key, b = p.key;
                    const bool bits_ok = a.pa == 1 && b.pa == 0 && a.ps == (f.ps ? 1 : 0) && a.pe == (f.pe ? 1 : 0) && a.pm == (f.pm ? 1 : 0) && a.pp == 1 && a.pd == (f.pd ? 1 : 0);
                    a.pa = b.pa = 0;
                    const bool ok = bits_ok && !(a < b) && !(b < a) && c.slot.slot == SLOT_NONE && c.prefetch.slot == SLOT_NONE && c.fallback.slot == SLOT_NONE &&
                                    c.ipw == 4 && c.ub_form == p.ub_form;
                    if (!ok) ++violations;
                    JitKey lo = c.key, hi = c.key;                       // (the key orders the bit: two forms never share a cache entry)
                    lo.pa = 0;
                    if (!(lo < hi) || (hi < lo)) key_order = 0;
                }
    printf("with_pa=%ld\nviolations=%ld\nkey_order=%ld\n", with_pa, violations, key_order);
    return violations ? 1 : 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "paths") return sweep_paths();
    if (mode == "variants") return sweep_variants();
    if (mode == "message") {
        printf("%d %s\n", (int)REFUSE_ADAPTIVE_SCORE, path_refusal_message(REFUSE_ADAPTIVE_SCORE));
        printf("%d %s\n", (int)REFUSE_ADAPTIVE_ACTUATOR, path_refusal_message(REFUSE_ADAPTIVE_ACTUATOR));
        return 0;
    }
    if (mode == "path") {
        std::string line;
        while (std::getline(std::cin, line)) {
            PathFacts f;
            std::istringstream words(line);
            std::string w;
            while (words >> w) {
                const size_t eq = w.find('=');
                bool known = false;
                for (const PFact& k : path_facts())
                    if (eq != std::string::npos && w.substr(0, eq) == k.name) { assign(f, k, atoi(w.c_str() + eq + 1)); known = true; }
                if (!known) { fprintf(stderr, "unknown fact %s\n", w.c_str()); return 2; }
            }
            const PathDecision d = decide_path(f);
            printf("kernel=%s lin=%d pl=%d pb=%d pc=%d pd=%d pp=%d pm=%d pe=%d ps=%d pa=%d refusal=%d rule=%s code=%d consistent=%d\n", KERNEL_NAME[d.kernel], d.lin, d.pl, d.pb, d.pc, d.pd, d.pp,
                   d.pm, d.pe, d.ps, d.pa, (int)d.refusal, d.rule, kernel_path_code(d, f), facts_consistent(f) ? 1 : 0);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s path | paths | variants | message\n", argv[0]);
    return 2;
}
