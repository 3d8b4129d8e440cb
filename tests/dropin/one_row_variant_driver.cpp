// one_row_variant_driver.cpp -- which instantiation a launch on the one-row kernel runs (csrc/one_row_variant.hpp: VariantFacts,
// EntrySlots, choose_one_row_variant) asked without a GPU.  Stand-alone, one command:
//     hipcc -x c++ -std=c++17 -I tinympc_amd/csrc tests/dropin/one_row_variant_driver.cpp -o driver
//     driver < QUERIES                 one line of `fact=value ...` per query; a fact that is not named is 0 (VariantFacts' own default)
//     driver sweep [fact=value ...]    every consistent combination (variant_facts_consistent) of all facts but the ones fixed on the command line
// The compiled-in entry is given by four words that are never swept: entry=0 none, 1 the KERNELS_LEAN pattern (k[0][0][2] and kub),
// 2 the KERNELS_FOR pattern (every slot), and half=, pf=, halfpf= for the shape-dependent slots khalf[], kpf[], khalfpf[] (both of each).
// A query prints the choice on one line: the key fields, slot, ipw, prefetch, ub_form, fallback (a slot as NAME[i][j][l]) and
// consistent.  The sweep prints one line per distinct choice with the number of combinations that gave it, and `total=`
// (tests/test_one_row_variant_cpu.py compares both with the function restated in numpy).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "one_row_variant.hpp"

using namespace tinympc_amd;

struct Query { VariantFacts f; int entry = 0, half = 0, pf = 0, halfpf = 0; };
// every fact by name, with the values a sweep gives it (the entry words: their one value)
struct Fact { const char* name; bool VariantFacts::*flag; int VariantFacts::*number; int Query::*entry; std::vector<int> values; };
static const std::vector<Fact>& facts() {
    using V = VariantFacts;
    static const std::vector<Fact> all = {
        {"lin", nullptr, &V::lin, nullptr, {0, 1, 2, 3}}, {"pl", &V::pl, nullptr, nullptr, {0, 1}}, {"pb", &V::pb, nullptr, nullptr, {0, 1}},
        {"soc", &V::soc, nullptr, nullptr, {0, 1}}, {"debug", &V::debug, nullptr, nullptr, {0, 1}}, {"dpp_mode", nullptr, &V::dpp_mode, nullptr, {-1, 0, 1, 2, 3}},
        {"hetero", &V::hetero, nullptr, nullptr, {0, 1}}, {"adaptive", &V::adaptive, nullptr, nullptr, {0, 1}},
        {"lin_kmax", nullptr, &V::lin_kmax, nullptr, {0, 4, 8, 16, 32}}, {"il_km", nullptr, &V::il_km, nullptr, {0, 1, 4, 32}},
        {"uniform_ub", &V::uniform_ub, nullptr, nullptr, {0, 1}}, {"het_ub", &V::het_ub, nullptr, nullptr, {0, 1}}, {"half_rows", &V::half_rows, nullptr, nullptr, {0, 1}},
        {"no_jit", &V::no_jit, nullptr, nullptr, {0, 1}}, {"variant_jit_failed", &V::variant_jit_failed, nullptr, nullptr, {0, 1}},
        {"prefetch_on", &V::prefetch_on, nullptr, nullptr, {0, 1}}, {"single_step", &V::single_step, nullptr, nullptr, {0, 1}},
        {"no_ref_window", &V::no_ref_window, nullptr, nullptr, {0, 1}}, {"default_grid", &V::default_grid, nullptr, nullptr, {0, 1}},
        {"entry", nullptr, nullptr, &Query::entry, {0}}, {"half", nullptr, nullptr, &Query::half, {0}}, {"pf", nullptr, nullptr, &Query::pf, {0}},
        {"halfpf", nullptr, nullptr, &Query::halfpf, {0}},
    };
    return all;
}
static void assign(Query& q, const Fact& k, int v) {
    if (k.flag) q.f.*k.flag = v != 0;
    else if (k.number) q.f.*k.number = v;
    else q.*k.entry = v;
}
// `fact=value` words -> (fact, value); an unknown name ends the program
static std::vector<std::pair<const Fact*, int>> parse(std::istream& in) {
    std::vector<std::pair<const Fact*, int>> out;
    std::string word;
    while (in >> word) {
        const std::string name = word.substr(0, word.find('='));
        const Fact* hit = nullptr;
        for (const Fact& k : facts())
            if (name == k.name) hit = &k;
        if (!hit || word.find('=') == std::string::npos) { fprintf(stderr, "unknown fact %s\n", word.c_str()); exit(2); }
        out.push_back({hit, atoi(word.c_str() + word.find('=') + 1)});
    }
    return out;
}
// the slot patterns that exist (kernel_entry.hpp): none, KERNELS_LEAN, KERNELS_FOR, each with or without the shape-dependent slots
static EntrySlots slots_of(const Query& q) {
    EntrySlots s;
    if (q.entry == 0) return s;
    s.has_entry = true;
    s.k[0][0][2] = s.kub = true;
    for (int i = 0; i < 2 && q.entry == 2; ++i) {
        for (int j = 0; j < 2; ++j)
            for (int l = 0; l < 3; ++l) s.k[i][j][l] = true;
        for (int j = 1; j < 4; ++j) s.klin[i][j] = true;
        s.khet[i] = s.khetub[i] = s.kadapt[i] = s.kubsoc = true;
    }
    for (int i = 0; i < 2; ++i) { s.khalf[i] = q.half != 0; s.kpf[i] = q.pf != 0; s.khalfpf[i] = q.halfpf != 0; }
    return s;
}
static std::string slot_name(const SlotRef& r) {
    static const char* NAME[] = {"NONE", "K", "KUB", "KUBSOC", "KLIN", "KHET", "KHETUB", "KADAPT", "KHALF", "KPF", "KHALFPF"};
    const int indices = r.slot == SLOT_K ? 3 : r.slot == SLOT_KLIN ? 2 : (r.slot == SLOT_NONE || r.slot == SLOT_KUB || r.slot == SLOT_KUBSOC) ? 0 : 1;
    const int at[3] = {r.i, r.j, r.l};
    std::string out = NAME[r.slot];
    for (int i = 0; i < indices; ++i) out += "[" + std::to_string(at[i]) + "]";
    return out;
}
static std::string answer(const VariantChoice& c) {
    const JitKey& k = c.key;
    char text[256];
    snprintf(text, sizeof(text), "soc=%d dbg=%d mode=%d lin=%d het=%d kmax=%d adapt=%d ub=%d pb=%d pl=%d slot=%s ipw=%d prefetch=%s ub_form=%d fallback=%s", k.soc, k.dbg, k.mode,
             k.lin, k.het, k.kmax, k.adapt, k.ub, k.pb, k.pl, slot_name(c.slot).c_str(), c.ipw, slot_name(c.prefetch).c_str(), c.ub_form ? 1 : 0, slot_name(c.fallback).c_str());
    return text;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "sweep") {
        std::string fixed;
        for (int i = 2; i < argc; ++i) fixed += std::string(argv[i]) + " ";
        std::istringstream in(fixed);
        std::vector<Fact> dims = facts();
        for (const auto& kv : parse(in))
            for (Fact& k : dims)
                if (std::string(k.name) == kv.first->name) k.values = {kv.second};
        std::map<std::string, long> count;
        std::vector<size_t> at(dims.size(), 0);
        Query q;
        long total = 0;
        for (const Fact& k : dims) assign(q, k, k.values[0]);
        const EntrySlots s = slots_of(q);                                  // (the entry words have one value each)
        for (bool more = true; more;) {
            if (variant_facts_consistent(q.f, s)) {
                count[answer(choose_one_row_variant(q.f, s))]++;
                ++total;
            }
            more = false;
            for (size_t i = 0; i < dims.size() && !more; ++i) {           // the next combination: an odometer over the value lists
                if (++at[i] < dims[i].values.size()) more = true;
                else at[i] = 0;
                assign(q, dims[i], dims[i].values[at[i]]);
            }
        }
        for (const auto& kv : count) printf("%s count=%ld\n", kv.first.c_str(), kv.second);
        printf("total=%ld\n", total);
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        Query q;
        for (const auto& kv : parse(in)) assign(q, *kv.first, kv.second);
        const EntrySlots s = slots_of(q);
        printf("%s consistent=%d\n", answer(choose_one_row_variant(q.f, s)).c_str(), variant_facts_consistent(q.f, s) ? 1 : 0);
    }
    return 0;
}
