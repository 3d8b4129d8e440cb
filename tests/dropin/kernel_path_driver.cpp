// kernel_path_driver.cpp -- the kernel choice (csrc/kernel_path.hpp: PathFacts, decide_path, kernel_path_code) asked without a GPU.
// Stand-alone, one command:
//     hipcc -x c++ -std=c++17 -I tinympc_amd/csrc tests/dropin/kernel_path_driver.cpp -o driver
//     driver < QUERIES                 one line of `fact=value ...` per query; a fact that is not named is 0 (PathFacts' own default)
//     driver sweep [fact=value ...]    every consistent combination (facts_consistent) of all facts but the ones fixed on the command line
// A query prints one line: kernel lin pl pb refusal rule code consistent.  The sweep prints one line per (kernel, lin, pl, pb, refusal,
// rule, code) that occurs, with the number of combinations that gave it, and `total=` (tests/test_kernel_path_cpu.py compares both with
// the rules restated in numpy).  messages: the refusal table, one `index text` per line.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <tuple>
#include <vector>

#include "kernel_path.hpp"

using namespace tinympc_amd;

// every fact by name, with the values a sweep gives it
struct Fact { const char* name; bool PathFacts::*flag; int PathFacts::*number; std::vector<int> values; };
static const std::vector<Fact>& facts() {
    static const std::vector<Fact> all = {
        {"has_entry", &PathFacts::has_entry, nullptr, {0, 1}}, {"entry_plain", &PathFacts::entry_plain, nullptr, {0, 1}}, {"entry_klin", &PathFacts::entry_klin, nullptr, {0, 1}},
        {"fits_box", &PathFacts::fits_box, nullptr, {0, 1}}, {"fits", &PathFacts::fits, nullptr, {0, 1}}, {"has_tile", &PathFacts::has_tile, nullptr, {0, 1}},
        {"tile_is_jit", &PathFacts::tile_is_jit, nullptr, {0, 1}}, {"tile_lin", &PathFacts::tile_lin, nullptr, {0, 1}}, {"lin_kmax", nullptr, &PathFacts::lin_kmax, {0, 4, 8, 16, 32}},
        {"planes_fit", &PathFacts::planes_fit, nullptr, {0, 1}}, {"pl_planes_fit", &PathFacts::pl_planes_fit, nullptr, {0, 1}}, {"soc", &PathFacts::soc, nullptr, {0, 1}},
        {"lin_families", nullptr, &PathFacts::lin_families, {0, 1, 2, 3}}, {"cones_overlap", &PathFacts::cones_overlap, nullptr, {0, 1}}, {"hetero", &PathFacts::hetero, nullptr, {0, 1}},
        {"tile_ext", &PathFacts::tile_ext, nullptr, {0, 1}}, {"adaptive", &PathFacts::adaptive, nullptr, {0, 1}}, {"debug", &PathFacts::debug, nullptr, {0, 1}},
        {"inst_bounds", &PathFacts::inst_bounds, nullptr, {0, 1}}, {"inst_lin", nullptr, &PathFacts::inst_lin, {0, 1, 2, 3}}, {"force_general", &PathFacts::force_general, nullptr, {0, 1}},
        {"no_jit", &PathFacts::no_jit, nullptr, {0, 1}}, {"no_tile", &PathFacts::no_tile, nullptr, {0, 1}}, {"prefer_tile", &PathFacts::prefer_tile, nullptr, {0, 1}},
        {"jit_failed", &PathFacts::jit_failed, nullptr, {0, 1}}, {"variant_jit_failed", &PathFacts::variant_jit_failed, nullptr, {0, 1}},
        {"tile_soc_failed", &PathFacts::tile_soc_failed, nullptr, {0, 1}},
    };
    return all;
}
static void assign(PathFacts& f, const Fact& k, int v) {
    if (k.flag) f.*k.flag = v != 0;
    else f.*k.number = v;
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
static const char* KERNEL_NAME[] = {"ONE_ROW", "TILE", "COVERAGE"};

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "messages") {
        for (size_t i = 0; i < sizeof(PATH_REFUSAL_MESSAGE) / sizeof(PATH_REFUSAL_MESSAGE[0]); ++i) printf("%zu %s\n", i, PATH_REFUSAL_MESSAGE[i]);
        return 0;
    }
    if (argc > 1 && std::string(argv[1]) == "sweep") {
        std::string fixed;
        for (int i = 2; i < argc; ++i) fixed += std::string(argv[i]) + " ";
        std::istringstream in(fixed);
        std::vector<Fact> dims = facts();
        for (const auto& kv : parse(in))
            for (Fact& k : dims)
                if (k.name == kv.first->name) k.values = {kv.second};
        std::map<std::tuple<int, int, int, int, int, std::string, int>, long> count;
        std::vector<size_t> at(dims.size(), 0);
        PathFacts f;
        long total = 0;
        for (const Fact& k : dims) assign(f, k, k.values[0]);
        for (bool more = true; more;) {
            if (facts_consistent(f)) {
                const PathDecision d = decide_path(f);
                count[{(int)d.kernel, d.lin, d.pl, d.pb, (int)d.refusal, d.rule, kernel_path_code(d, f)}]++;
                ++total;
            }
            more = false;
            for (size_t i = 0; i < dims.size() && !more; ++i) {           // the next combination: an odometer over the value lists
                if (++at[i] < dims[i].values.size()) more = true;
                else at[i] = 0;
                assign(f, dims[i], dims[i].values[at[i]]);
            }
        }
        for (const auto& kv : count)
            printf("kernel=%s lin=%d pl=%d pb=%d refusal=%d rule=%s code=%d count=%ld\n", KERNEL_NAME[std::get<0>(kv.first)], std::get<1>(kv.first), std::get<2>(kv.first),
                   std::get<3>(kv.first), std::get<4>(kv.first), std::get<5>(kv.first).c_str(), std::get<6>(kv.first), kv.second);
        printf("total=%ld\n", total);
        return 0;
    }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        PathFacts f;
        for (const auto& kv : parse(in)) assign(f, *kv.first, kv.second);
        const PathDecision d = decide_path(f);
        printf("kernel=%s lin=%d pl=%d pb=%d refusal=%d rule=%s code=%d consistent=%d\n", KERNEL_NAME[d.kernel], d.lin, d.pl, d.pb, (int)d.refusal, d.rule, kernel_path_code(d, f),
               facts_consistent(f) ? 1 : 0);
    }
    return 0;
}
