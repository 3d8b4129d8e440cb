// disturbance_path_driver.cpp -- the kernel choice and the one-row variant choice with a per-instance disturbance at the plant step
// (csrc/kernel_path.hpp PathFacts::disturbance, csrc/one_row_variant.hpp VariantFacts::pd) asked without a GPU, and both compared with
// the headers of the commit BEFORE the feature for every combination that does not use it.  Stand-alone:
//     mkdir parent && git show <parent>:tinympc_amd/csrc/kernel_path.hpp > parent/kernel_path.hpp      (and one_row_variant.hpp)
//     hipcc -x c++ -std=c++17 -I tinympc_amd/csrc -I . tests/dropin/disturbance_path_driver.cpp -o driver
//     driver paths       sweeps every consistent PathFacts.  disturbance = 0: decide_path and kernel_path_code against the parent's, prints
//                        `parent_compared=` and `parent_differ=`; disturbance = 1: one line per (kernel, lin, pl, pb, pc, pd, refusal, rule,
//                        code) with its count, and `violations=`: combinations whose answer is not the rule restated below ON THE
//                        PARENT'S decision for the same facts with the tile kernel switched off
//     driver variants    the same for choose_one_row_variant over every entry pattern: pd = 0 against the parent's choice, pd = 1 one line
//                        per distinct choice
//     driver path < QUERIES     one line of `fact=value ...` per query (facts not named: 0) -> the decision
//     driver message     the value and text of REFUSE_ADAPTIVE_DISTURBANCE (exit 1 if an earlier text is not the parent's)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "kernel_path.hpp"
#include "one_row_variant.hpp"
#define tinympc_amd tinympc_amd_parent
#include "parent/kernel_path.hpp"
#include "parent/one_row_variant.hpp"
#undef tinympc_amd

namespace cur = tinympc_amd;
namespace old = tinympc_amd_parent;

struct PFact { const char* name; bool cur::PathFacts::*flag; int cur::PathFacts::*number; std::vector<int> values; };
static const std::vector<PFact>& path_facts() {
    using P = cur::PathFacts;
    static const std::vector<PFact> all = {
        {"has_entry", &P::has_entry, nullptr, {0, 1}}, {"entry_plain", &P::entry_plain, nullptr, {0, 1}}, {"entry_klin", &P::entry_klin, nullptr, {0, 1}},
        {"fits_box", &P::fits_box, nullptr, {0, 1}}, {"fits", &P::fits, nullptr, {0, 1}}, {"has_tile", &P::has_tile, nullptr, {0, 1}},
        {"tile_is_jit", &P::tile_is_jit, nullptr, {0, 1}}, {"tile_lin", &P::tile_lin, nullptr, {0, 1}}, {"lin_kmax", nullptr, &P::lin_kmax, {0, 4, 8, 16, 32}},
        {"planes_fit", &P::planes_fit, nullptr, {0, 1}}, {"pl_planes_fit", &P::pl_planes_fit, nullptr, {0, 1}}, {"soc", &P::soc, nullptr, {0, 1}},
        {"lin_families", nullptr, &P::lin_families, {0, 1, 2, 3}}, {"cones_overlap", &P::cones_overlap, nullptr, {0, 1}}, {"hetero", &P::hetero, nullptr, {0, 1}},
        {"tile_ext", &P::tile_ext, nullptr, {0, 1}}, {"adaptive", &P::adaptive, nullptr, {0, 1}}, {"debug", &P::debug, nullptr, {0, 1}},
        {"inst_bounds", &P::inst_bounds, nullptr, {0, 1}}, {"inst_lin", nullptr, &P::inst_lin, {0, 1, 2, 3}}, {"inst_cones", &P::inst_cones, nullptr, {0, 1}},
        {"force_general", &P::force_general, nullptr, {0, 1}}, {"no_jit", &P::no_jit, nullptr, {0, 1}}, {"no_tile", &P::no_tile, nullptr, {0, 1}},
        {"prefer_tile", &P::prefer_tile, nullptr, {0, 1}}, {"jit_failed", &P::jit_failed, nullptr, {0, 1}}, {"variant_jit_failed", &P::variant_jit_failed, nullptr, {0, 1}},
        {"tile_soc_failed", &P::tile_soc_failed, nullptr, {0, 1}}, {"disturbance", &P::disturbance, nullptr, {0, 1}},
    };
    return all;
}
static void assign(cur::PathFacts& f, const PFact& k, int v) {
    if (k.flag) f.*k.flag = v != 0;
    else f.*k.number = v;
}
static old::PathFacts parent_facts(const cur::PathFacts& f) {
    old::PathFacts p;
    p.has_entry = f.has_entry; p.entry_plain = f.entry_plain; p.entry_klin = f.entry_klin; p.fits_box = f.fits_box; p.fits = f.fits; p.has_tile = f.has_tile;
    p.tile_is_jit = f.tile_is_jit; p.tile_lin = f.tile_lin; p.lin_kmax = f.lin_kmax; p.planes_fit = f.planes_fit; p.pl_planes_fit = f.pl_planes_fit; p.soc = f.soc;
    p.lin_families = f.lin_families; p.cones_overlap = f.cones_overlap; p.hetero = f.hetero; p.tile_ext = f.tile_ext; p.adaptive = f.adaptive; p.debug = f.debug;
    p.inst_bounds = f.inst_bounds; p.inst_lin = f.inst_lin; p.inst_cones = f.inst_cones; p.force_general = f.force_general; p.no_jit = f.no_jit; p.no_tile = f.no_tile;
    p.prefer_tile = f.prefer_tile; p.jit_failed = f.jit_failed; p.variant_jit_failed = f.variant_jit_failed; p.tile_soc_failed = f.tile_soc_failed;
    return p;
}
static const char* KERNEL_NAME[] = {"ONE_ROW", "TILE", "COVERAGE"};
static std::string answer(const char* kernel, int lin, int pl, int pb, int pc, int pd, int refusal, const char* rule, int code) {
    char text[256];
    snprintf(text, sizeof(text), "kernel=%s lin=%d pl=%d pb=%d pc=%d pd=%d refusal=%d rule=%s code=%d", kernel, lin, pl, pb, pc, pd, refusal, rule, code);
    return text;
}
// (a decision as plain numbers: the sweep compares and counts a few hundred million of them)
struct Answer {
    int kernel, lin, pl, pb, pc, pd, refusal, code;
    const char* rule;
    bool same(const Answer& o) const {
        return kernel == o.kernel && lin == o.lin && pl == o.pl && pb == o.pb && pc == o.pc && pd == o.pd && refusal == o.refusal && code == o.code && !strcmp(rule, o.rule);
    }
    bool operator<(const Answer& o) const {
        const int a[8] = {kernel, lin, pl, pb, pc, pd, refusal, code}, b[8] = {o.kernel, o.lin, o.pl, o.pb, o.pc, o.pd, o.refusal, o.code};
        for (int i = 0; i < 8; ++i)
            if (a[i] != b[i]) return a[i] < b[i];
        return rule < o.rule;                                            // (by address: equal texts at two addresses are merged when printed)
    }
    std::string text() const { return answer(KERNEL_NAME[kernel], lin, pl, pb, pc, pd, refusal, rule, code); }
};
static Answer path_answer(const cur::PathDecision& d, const cur::PathFacts& f) {
    return Answer{(int)d.kernel, d.lin, d.pl, d.pb, d.pc, d.pd, (int)d.refusal, cur::kernel_path_code(d, f), d.rule};
}
// the rule pair of the disturbance, restated on the PARENT's decision: ask the parent with the tile kernel switched off.  A coverage
// answer stays what it is.  A one-row answer becomes the PD form of that very form (PB / PL / PC keep their rule's name, every other
// one is "one_row:pd") where a PD form may be made -- the shape fits, hipRTC may be tried, no force_general, no debug outputs, no
// adaptive rho --, else "cover:pd".  Refusals: whatever the parent refuses keeps its value; adaptive rho alone is refused with the new one
static Answer expected_with_disturbance(const cur::PathFacts& f) {
    old::PathFacts pf = parent_facts(f);
    pf.no_tile = true;
    const old::PathDecision p = old::decide_path(pf);
    const int refusal = !f.adaptive ? 0 : (int)p.refusal ? (int)p.refusal : (int)cur::REFUSE_ADAPTIVE_DISTURBANCE;
    if ((int)p.kernel == (int)cur::COVERAGE) return Answer{(int)cur::COVERAGE, 0, 0, 0, 0, 0, refusal, 2, p.rule};
    const bool hiprtc = !f.no_jit && !f.jit_failed && !f.variant_jit_failed;
    if (!(f.fits && hiprtc && !f.force_general && !f.debug && !f.adaptive)) return Answer{(int)cur::COVERAGE, 0, 0, 0, 0, 0, refusal, 2, "cover:pd"};
    return Answer{(int)cur::ONE_ROW, p.lin, p.pl, p.pb, p.pc, 1, refusal, 3, (p.pl || p.pb || p.pc) ? p.rule : "one_row:pd"};
}

struct VFact { const char* name; bool cur::VariantFacts::*flag; int cur::VariantFacts::*number; std::vector<int> values; };
static const std::vector<VFact>& variant_facts() {
    using V = cur::VariantFacts;
    static const std::vector<VFact> all = {
        {"lin", nullptr, &V::lin, {0, 1, 2, 3}}, {"pl", &V::pl, nullptr, {0, 1}}, {"pb", &V::pb, nullptr, {0, 1}}, {"pc", &V::pc, nullptr, {0, 1}},
        {"pd", &V::pd, nullptr, {0, 1}},
        {"soc", &V::soc, nullptr, {0, 1}}, {"debug", &V::debug, nullptr, {0, 1}}, {"dpp_mode", nullptr, &V::dpp_mode, {-1, 0, 1, 2, 3}},
        {"hetero", &V::hetero, nullptr, {0, 1}}, {"adaptive", &V::adaptive, nullptr, {0, 1}}, {"lin_kmax", nullptr, &V::lin_kmax, {0, 4, 8, 16, 32}},
        {"il_km", nullptr, &V::il_km, {0, 1, 4, 32}}, {"uniform_ub", &V::uniform_ub, nullptr, {0, 1}}, {"het_ub", &V::het_ub, nullptr, {0, 1}},
        {"half_rows", &V::half_rows, nullptr, {0, 1}}, {"no_jit", &V::no_jit, nullptr, {0, 1}}, {"variant_jit_failed", &V::variant_jit_failed, nullptr, {0, 1}},
        {"prefetch_on", &V::prefetch_on, nullptr, {0, 1}}, {"single_step", &V::single_step, nullptr, {0, 1}}, {"no_ref_window", &V::no_ref_window, nullptr, {0, 1}},
        {"default_grid", &V::default_grid, nullptr, {0, 1}},
    };
    return all;
}
static old::VariantFacts parent_facts(const cur::VariantFacts& f) {
    old::VariantFacts p;
    p.lin = f.lin; p.pl = f.pl; p.pb = f.pb; p.pc = f.pc; p.soc = f.soc; p.debug = f.debug; p.dpp_mode = f.dpp_mode; p.hetero = f.hetero; p.adaptive = f.adaptive;
    p.lin_kmax = f.lin_kmax; p.il_km = f.il_km; p.uniform_ub = f.uniform_ub; p.het_ub = f.het_ub; p.half_rows = f.half_rows; p.no_jit = f.no_jit;
    p.variant_jit_failed = f.variant_jit_failed; p.prefetch_on = f.prefetch_on; p.single_step = f.single_step; p.no_ref_window = f.no_ref_window;
    p.default_grid = f.default_grid;
    return p;
}
// the slot patterns that exist (kernel_entry.hpp): none, KERNELS_LEAN, KERNELS_FOR, each with or without the shape-dependent slots
template <class Slots>
static Slots slots_of(int entry, int half, int pf, int halfpf) {
    Slots s;
    if (entry == 0) return s;
    s.has_entry = true;
    s.k[0][0][2] = s.kub = true;
    for (int i = 0; i < 2 && entry == 2; ++i) {
        for (int j = 0; j < 2; ++j)
            for (int l = 0; l < 3; ++l) s.k[i][j][l] = true;
        for (int j = 1; j < 4; ++j) s.klin[i][j] = true;
        s.khet[i] = s.khetub[i] = s.kadapt[i] = s.kubsoc = true;
    }
    for (int i = 0; i < 2; ++i) { s.khalf[i] = half != 0; s.kpf[i] = pf != 0; s.khalfpf[i] = halfpf != 0; }
    return s;
}
template <class Ref>
static std::string slot_name(const Ref& r) {
    static const char* NAME[] = {"NONE", "K", "KUB", "KUBSOC", "KLIN", "KHET", "KHETUB", "KADAPT", "KHALF", "KPF", "KHALFPF"};
    return std::string(NAME[(int)r.slot]) + "[" + std::to_string(r.i) + "][" + std::to_string(r.j) + "][" + std::to_string(r.l) + "]";
}
template <class Choice>
static std::string variant_answer(const Choice& c, int pd) {
    const auto& k = c.key;
    char text[320];
    snprintf(text, sizeof(text), "soc=%d dbg=%d mode=%d lin=%d het=%d kmax=%d adapt=%d ub=%d pb=%d pl=%d pc=%d pd=%d slot=%s ipw=%d prefetch=%s ub_form=%d fallback=%s", k.soc,
             k.dbg, k.mode, k.lin, k.het, k.kmax, k.adapt, k.ub, k.pb, k.pl, k.pc, pd, slot_name(c.slot).c_str(), c.ipw, slot_name(c.prefetch).c_str(), c.ub_form ? 1 : 0,
             slot_name(c.fallback).c_str());
    return text;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "message") {
        printf("%d %s\n", (int)cur::REFUSE_ADAPTIVE_DISTURBANCE, cur::path_refusal_message(cur::REFUSE_ADAPTIVE_DISTURBANCE));
        for (int r = 0; r < (int)cur::REFUSE_ADAPTIVE_DISTURBANCE; ++r)
            if (strcmp(cur::path_refusal_message((cur::PathRefusal)r), old::path_refusal_message((old::PathRefusal)r))) return 1;      // (the other texts are the parent's)
        return 0;
    }
    if (mode == "paths") {
        const std::vector<PFact>& dims = path_facts();
        std::vector<size_t> at(dims.size(), 0);
        cur::PathFacts f;
        for (const PFact& k : dims) assign(f, k, k.values[0]);
        std::map<Answer, long> seen;
        long compared = 0, differ = 0, violations = 0, with_disturbance = 0;
        for (bool more = true; more;) {
            if (cur::facts_consistent(f)) {
                const cur::PathDecision d = cur::decide_path(f);
                if (!f.disturbance) {
                    const old::PathFacts pf = parent_facts(f);
                    const old::PathDecision p = old::decide_path(pf);
                    ++compared;
                    if (!old::facts_consistent(pf) || (int)p.kernel != (int)d.kernel || p.lin != d.lin || p.pl != d.pl || p.pb != d.pb || p.pc != d.pc || d.pd != 0 ||
                        (int)p.refusal != (int)d.refusal || strcmp(p.rule, d.rule) || old::kernel_path_code(p, pf) != cur::kernel_path_code(d, f))
                        ++differ;
                } else {
                    const Answer got = path_answer(d, f);
                    ++with_disturbance;
                    ++seen[got];
                    if (!got.same(expected_with_disturbance(f))) ++violations;
                }
            }
            more = false;
            for (size_t i = 0; i < dims.size() && !more; ++i) {           // the next combination: an odometer over the value lists
                if (++at[i] < dims[i].values.size()) more = true;
                else at[i] = 0;
                assign(f, dims[i], dims[i].values[at[i]]);
            }
        }
        std::map<std::string, long> count;
        for (const auto& kv : seen) count[kv.first.text()] += kv.second;
        for (const auto& kv : count) printf("%s count=%ld\n", kv.first.c_str(), kv.second);
        printf("parent_compared=%ld\nparent_differ=%ld\nwith_disturbance=%ld\nviolations=%ld\n", compared, differ, with_disturbance, violations);
        return 0;
    }
    if (mode == "variants") {
        const std::vector<VFact>& dims = variant_facts();
        std::map<std::string, long> count;
        long compared = 0, differ = 0, with_pd = 0, base_differs = 0;
        for (int entry = 0; entry < 3; ++entry)
            for (int shape = 0; shape < (entry ? 8 : 1); ++shape) {
                const cur::EntrySlots s = slots_of<cur::EntrySlots>(entry, shape & 1, (shape >> 1) & 1, (shape >> 2) & 1);
                const old::EntrySlots ps = slots_of<old::EntrySlots>(entry, shape & 1, (shape >> 1) & 1, (shape >> 2) & 1);
                std::vector<size_t> at(dims.size(), 0);
                cur::VariantFacts f;
                for (const VFact& k : dims) { if (k.flag) f.*k.flag = k.values[0] != 0; else f.*k.number = k.values[0]; }
                for (bool more = true; more;) {
                    if (cur::variant_facts_consistent(f, s)) {
                        const cur::VariantChoice c = cur::choose_one_row_variant(f, s);
                        if (!f.pd) {
                            const old::VariantFacts pf = parent_facts(f);
                            ++compared;
                            if (!old::variant_facts_consistent(pf, ps) || c.key.pd != 0 || variant_answer(c, 0) != variant_answer(old::choose_one_row_variant(pf, ps), 0)) ++differ;
                        } else {
                            ++with_pd;
                            // the form PD rides on: what the parent keys for the same facts (but for UB, which a PD form takes where the
                            // compiled-in rung would have: printed, checked by the caller)
                            const old::VariantChoice b = old::choose_one_row_variant(parent_facts(f), ps);
                            if (b.key.soc != c.key.soc || b.key.dbg != c.key.dbg || b.key.mode != c.key.mode || b.key.lin != c.key.lin || b.key.het != c.key.het ||
                                b.key.kmax != c.key.kmax || b.key.adapt != c.key.adapt || b.key.pb != c.key.pb || b.key.pl != c.key.pl || b.key.pc != c.key.pc)
                                ++base_differs;
                            ++count["entry=" + std::to_string(entry) + " hetero=" + std::to_string(f.hetero ? 1 : 0) + " base_ub_form=" + std::to_string(b.ub_form ? 1 : 0) + " " +
                                    variant_answer(c, c.key.pd)];
                        }
                    }
                    more = false;
                    for (size_t i = 0; i < dims.size() && !more; ++i) {
                        if (++at[i] < dims[i].values.size()) more = true;
                        else at[i] = 0;
                        const int v = dims[i].values[at[i]];
                        if (dims[i].flag) f.*dims[i].flag = v != 0; else f.*dims[i].number = v;
                    }
                }
            }
        for (const auto& kv : count) printf("%s count=%ld\n", kv.first.c_str(), kv.second);
        printf("parent_compared=%ld\nparent_differ=%ld\nwith_pd=%ld\nbase_differs=%ld\n", compared, differ, with_pd, base_differs);
        // the key order: pd is the fifteenth field compared
        cur::JitKey a = {}, b = {};
        b.pd = 1;
        printf("key_order=%d\n", (a < b && !(b < a)) ? 1 : 0);
        return 0;
    }
    if (mode == "path") {
        std::string line;
        while (std::getline(std::cin, line)) {
            std::istringstream in(line);
            cur::PathFacts f;
            std::string word;
            while (in >> word) {
                const std::string name = word.substr(0, word.find('='));
                const PFact* hit = nullptr;
                for (const PFact& k : path_facts())
                    if (name == k.name) hit = &k;
                if (!hit || word.find('=') == std::string::npos) { fprintf(stderr, "unknown fact %s\n", word.c_str()); return 2; }
                assign(f, *hit, atoi(word.c_str() + word.find('=') + 1));
            }
            printf("%s consistent=%d\n", path_answer(cur::decide_path(f), f).text().c_str(), cur::facts_consistent(f) ? 1 : 0);
        }
        return 0;
    }
    fprintf(stderr, "usage: %s paths | variants | path | message\n", argv[0]);
    return 2;
}
