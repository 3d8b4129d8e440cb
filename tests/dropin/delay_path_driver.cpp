// delay_path_driver.cpp -- the kernel choice and the one-row variant choice under a transport delay and its predictor (csrc/kernel_path.hpp
// PathFacts::delay / delay_compensation, PathDecision::pq / px; csrc/one_row_variant.hpp VariantFacts::pq / px), asked without a GPU.
// With both facts off every decision must be what the rules gave before the delay existed: kernel_path_before_delay.hpp is a frozen copy
// of those rules in a namespace of its own, compiled into this program next to the header of today.  Stand-alone:
//     hipcc -x c++ -std=c++17 -I tinympc_amd/csrc -I tests/dropin tests/dropin/delay_path_driver.cpp -o driver
//     driver paths      every consistent PathFacts over 22 facts, the two new ones among them: both off -> field by
//                       field the frozen rules' answer, pq = px = 0; delay on -> the answer of the same facts without it (compensation: with
//                       the measurement fact on, which it forces), plus pq (and px), the names and the refusal unchanged
//     driver variants   choose_one_row_variant with pq / px on against the choice without: the same key but for the two bits
//     driver path < QUERIES   one line of `fact=value ...` per query -> the decision
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "kernel_path.hpp"
#include "kernel_path_before_delay.hpp"
#include "one_row_variant.hpp"

namespace now = tinympc_amd;
namespace old = kernel_path_before_delay;

static const char* const NAMES[] = {"has_entry", "entry_plain", "fits_box", "fits", "has_tile", "lin_kmax", "planes_fit", "pl_planes_fit", "soc", "lin_families", "cones_overlap",
                                    "hetero", "adaptive", "debug", "inst_bounds", "inst_lin", "inst_cones", "force_general", "no_jit", "prefer_tile", "variant_jit_failed",
                                    "disturbance", "plant", "state_log", "measurement", "estimator", "score", "actuator", "delay", "delay_compensation"};
constexpr int NFACTS = sizeof(NAMES) / sizeof(NAMES[0]), COMMON = NFACTS - 2;
// the facts both headers know, by name (lin_kmax: 0 or 4)
template <class F>
static void fill_common(F& f, const int* v) {
    f.has_entry = v[0]; f.entry_plain = v[1]; f.fits_box = v[2]; f.fits = v[3]; f.has_tile = v[4]; f.lin_kmax = v[5]; f.planes_fit = v[6]; f.pl_planes_fit = v[7];
    f.soc = v[8]; f.lin_families = v[9]; f.cones_overlap = v[10]; f.hetero = v[11]; f.adaptive = v[12]; f.debug = v[13]; f.inst_bounds = v[14]; f.inst_lin = v[15];
    f.inst_cones = v[16]; f.force_general = v[17]; f.no_jit = v[18]; f.prefer_tile = v[19]; f.variant_jit_failed = v[20]; f.disturbance = v[21]; f.plant = v[22];
    f.state_log = v[23]; f.measurement = v[24]; f.estimator = v[25]; f.score = v[26]; f.actuator = v[27];
}
static now::PathFacts facts_of(const int* v) {
    now::PathFacts f;
    fill_common(f, v);
    f.delay = v[28]; f.delay_compensation = v[29];
    return f;
}
static const char* KERNEL_NAME[] = {"ONE_ROW", "TILE", "COVERAGE"};
static bool same_as_before(const now::PathDecision& a, const old::PathDecision& b) {
    return (int)a.kernel == (int)b.kernel && a.lin == b.lin && a.pl == b.pl && a.pb == b.pb && a.pc == b.pc && a.pd == b.pd && a.pp == b.pp && a.pm == b.pm && a.pe == b.pe &&
           a.ps == b.ps && a.pa == b.pa && (int)a.refusal == (int)b.refusal && !strcmp(a.rule, b.rule) && a.pq == 0 && a.px == 0 &&
           !strcmp(now::path_refusal_message(a.refusal), old::path_refusal_message(b.refusal));
}
static bool same(const now::PathDecision& a, const now::PathDecision& b) {
    return a.kernel == b.kernel && a.lin == b.lin && a.pl == b.pl && a.pb == b.pb && a.pc == b.pc && a.pd == b.pd && a.pp == b.pp && a.pm == b.pm && a.pe == b.pe && a.ps == b.ps &&
           a.pa == b.pa && a.pq == b.pq && a.px == b.px && a.refusal == b.refusal && !strcmp(a.rule, b.rule);
}

static int sweep_paths() {
    int v[NFACTS] = {};
    long off = 0, delayed = 0, compensated = 0, violations = 0, one_row_pq = 0, one_row_px = 0, cover = 0, refused = 0;
    // (swept: 22 of the facts; entry_plain follows has_entry, the planes fit wherever half-spaces are on, and prefer_tile, inst_lin, hetero,
    // cones_overlap and state_log stay 0 -- the new facts meet none of them: tests/dropin/actuator_path_driver.cpp sweeps those against the actuator)
    static const int SWEPT[] = {0, 2, 3, 4, 5, 8, 9, 12, 13, 14, 16, 17, 18, 20, 21, 22, 24, 25, 26, 27, 28, 29};
    constexpr int NSWEPT = sizeof(SWEPT) / sizeof(SWEPT[0]);
    for (long code = 0; code < (1L << NSWEPT); ++code) {
        for (int i = 0; i < NFACTS; ++i) v[i] = 0;
        for (int i = 0; i < NSWEPT; ++i) v[SWEPT[i]] = (int)((code >> i) & 1);
        v[5] *= 4;
        v[1] = v[0]; v[6] = v[5] != 0; v[7] = v[9];
        const now::PathFacts f = facts_of(v);
        if (!now::facts_consistent(f)) continue;
        const now::PathDecision d = now::decide_path(f);
        bool ok;
        if (!f.delay) {
            ++off;
            old::PathFacts g;
            fill_common(g, v);
            const old::PathDecision e = old::decide_path(g);
            ok = old::facts_consistent(g) && same_as_before(d, e) && now::kernel_path_code(d, f) == old::kernel_path_code(e, g);
        } else {
            ++delayed;
            if (f.delay_compensation) ++compensated;
            now::PathFacts g = f, h = f;
            g.delay = g.delay_compensation = false; h.delay = h.delay_compensation = false;
            if (f.delay_compensation) g.measurement = true;                  // (what the predictor forces: pm, and through it pp)
            now::PathDecision e = now::decide_path(g);
            e.refusal = now::decide_path(h).refusal;                         // (the forced bit is no installed stage: it refuses nothing)
            if (e.kernel == now::ONE_ROW) { e.pq = 1; e.px = f.delay_compensation ? 1 : 0; }
            ok = same(d, e) && now::kernel_path_code(d, f) == (d.kernel == now::ONE_ROW ? 3 : 2) && d.kernel != now::TILE &&
                 (d.kernel != now::ONE_ROW || (d.pa == 1 && d.pp == 1 && (!f.delay_compensation || d.pm == 1))) &&
                 (!f.adaptive || d.refusal != now::REFUSE_NONE);
            if (d.kernel == now::ONE_ROW && d.pq) ++one_row_pq;
            if (d.kernel == now::ONE_ROW && d.px) ++one_row_px;
            if (d.kernel == now::COVERAGE) ++cover;
            if (d.refusal == now::REFUSE_ADAPTIVE_ACTUATOR) ++refused;
        }
        if (!ok && violations++ < 5)
            printf("violation code=%ld kernel=%s rule=%s pp=%d pm=%d pa=%d pq=%d px=%d refusal=%d\n", code, KERNEL_NAME[d.kernel], d.rule, d.pp, d.pm, d.pa, d.pq, d.px, (int)d.refusal);
    }
    printf("off=%ld\ndelayed=%ld\ncompensated=%ld\nviolations=%ld\none_row_pq=%ld\none_row_px=%ld\ncover=%ld\nrefused_12=%ld\n", off, delayed, compensated, violations, one_row_pq,
           one_row_px, cover, refused);
    return violations ? 1 : 0;
}

static int sweep_variants() {
    using namespace tinympc_amd;
    const EntrySlots none = {};
    long with_pq = 0, violations = 0;
    for (int bits = 0; bits < (1 << 9); ++bits)
        for (int form = 0; form < 3; ++form)                             // (on the PP, the PM and the PE form)
            for (int px = 0; px < 2; ++px) {
                VariantFacts f;
                f.pb = bits & 1; f.pc = bits & 2; f.pd = bits & 4; f.soc = bits & 8; f.hetero = bits & 16; f.uniform_ub = bits & 32; f.het_ub = bits & 64; f.ps = bits & 128;
                f.single_step = bits & 256; f.no_ref_window = true; f.default_grid = true;
                f.pp = true; f.pm = form >= 1; f.pe = form >= 2; f.pa = true; f.pq = true; f.px = px != 0;
                if (!variant_facts_consistent(f, none)) continue;
                ++with_pq;
                const VariantChoice c = choose_one_row_variant(f, none);
                VariantFacts g = f;
                g.pq = g.px = false;
                const VariantChoice p = choose_one_row_variant(g, none);
                JitKey a = c.key, b = p.key;
                bool ok = a.pq == 1 && a.px == px && b.pq == 0 && b.px == 0 && a.pa == 1 && (!px || a.pm == 1);
                JitKey lo = c.key;
                lo.pq = lo.px = 0;
                ok = ok && (lo < c.key) && !(c.key < lo);                   // (the key orders the bits: two forms never share a cache entry)
                a.pq = a.px = 0;
                ok = ok && !(a < b) && !(b < a) && c.slot.slot == SLOT_NONE && c.prefetch.slot == SLOT_NONE && c.ipw == 4 && c.ub_form == p.ub_form;
                if (!ok) ++violations;
            }
    // a PX form without the PM bit, a PQ form without the PA bit: not what batch_dispatch.hip can produce
    VariantFacts bad;
    bad.pp = true; bad.pa = true; bad.pq = true; bad.px = true;
    if (variant_facts_consistent(bad, none)) ++violations;
    bad.pm = true; bad.pa = false;
    if (variant_facts_consistent(bad, none)) ++violations;
    printf("with_pq=%ld\nviolations=%ld\n", with_pq, violations);
    return violations ? 1 : 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "paths") return sweep_paths();
    if (mode == "variants") return sweep_variants();
    if (mode == "path") {
        std::string line;
        while (std::getline(std::cin, line)) {
            int v[NFACTS] = {};
            std::istringstream words(line);
            std::string w;
            while (words >> w) {
                const size_t eq = w.find('=');
                bool known = false;
                for (int i = 0; i < NFACTS; ++i)
                    if (eq != std::string::npos && w.substr(0, eq) == NAMES[i]) { v[i] = atoi(w.c_str() + eq + 1); known = true; }
                if (!known) { fprintf(stderr, "unknown fact %s\n", w.c_str()); return 2; }
            }
            const now::PathFacts f = facts_of(v);
            const now::PathDecision d = now::decide_path(f);
            printf("kernel=%s pd=%d pp=%d pm=%d pe=%d ps=%d pa=%d pq=%d px=%d refusal=%d rule=%s code=%d consistent=%d\n", KERNEL_NAME[d.kernel], d.pd, d.pp, d.pm, d.pe, d.ps, d.pa,
                   d.pq, d.px, (int)d.refusal, d.rule, now::kernel_path_code(d, f), now::facts_consistent(f) ? 1 : 0);
        }
        return 0;
    }
    (void)COMMON;
    fprintf(stderr, "usage: %s path | paths | variants\n", argv[0]);
    return 2;
}
