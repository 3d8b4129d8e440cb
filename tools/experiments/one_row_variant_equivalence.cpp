// one_row_variant_equivalence.cpp -- one-time check that choose_one_row_variant (csrc/one_row_variant.hpp) answers what
// build_one_row_launch answered before it: the parent's key assembly, ladder, HALF upgrade, PREFETCH mapping, fallback condition and
// last_ub expression stand below VERBATIM (between the two marks; only `steps`, `a` and `lin_kmax` are stand-ins), over a fake entry
// whose filled slots are distinct non-null tokens.  Compared over every consistent fact combination and every slot pattern: key,
// resolved token, ipw, PREFETCH token, last_ub (run-time instantiation taken as succeeding) and the fallback token.
//     hipcc -x c++ -std=c++17 -I tinympc_amd/csrc tools/experiments/one_row_variant_equivalence.cpp -o equivalence && ./equivalence
#include <cstdio>
#include <cstring>
#include <map>
#include <string>

#include "one_row_variant.hpp"

using namespace tinympc_amd;

typedef const char* SolveKernel;
struct KernelEntry {
    SolveKernel k[2][2][3], klin[2][4], khet[2], khetub[2], kadapt[2], kub, kubsoc, khalf[2], kpf[2], khalfpf[2];
};
struct TinyBatch {
    const KernelEntry* kernel;
    int nx = 4, nu = 2, N = 10, dpp_mode, il_km, half_rows, prefetch, grid_waves_per_cu;
    bool debug, hetero, adaptive, bounds_uniform, use_ub, het_ub, no_jit, variant_jit_failed;
    int shared_kmax;
    bool last_half, last_ub;
};
struct Decision { int lin, pl, pb; };
struct Args { const void* traj; };
static const int LIN_KMAX = 4;
static int lin_kmax(const TinyBatch* b) { return b->shared_kmax; }

struct Parent { JitKey jk; SolveKernel k, kpf, fallback; int ipw; bool last_ub; const char* rung; };
static Parent parent(TinyBatch* b, const Decision& D, bool soc, int steps, const Args& a) {
    Parent P{};
    const char* rung = "none";
    SolveKernel kpf = nullptr;
    // ======== the parent's text
    const int mode = (b->dpp_mode >= 0 && b->dpp_mode <= 2) ? b->dpp_mode : 0;
    JitKey jk;
    jk = JitKey{b->nx, b->nu, b->N, soc ? 1 : 0, b->debug ? 1 : 0, mode, 0, b->hetero ? 1 : 0, LIN_KMAX, 0};
    if (D.lin) {
        jk.lin = D.lin;
        jk.kmax = lin_kmax(b);
        if (D.pl) { jk.pl = 1; jk.kmax = b->il_km; }
    }
    if (b->adaptive) {
        jk.adapt = 1;
    }
    if (jk.lin || jk.het || jk.adapt) jk.mode = 2;   // those variants exist on the single-chain FMA blocks only
    if (D.pb) {
        jk.pb = 1;
        jk.ub = (b->bounds_uniform && b->use_ub && (!b->hetero || b->het_ub)) ? 1 : 0;
    }
    SolveKernel k = nullptr;
    if (b->kernel && !jk.pb && !jk.pl) {
        if (jk.adapt) { rung = "kadapt"; k = (jk.soc || jk.het) ? nullptr : b->kernel->kadapt[jk.dbg]; }
        else if (!jk.lin && !jk.het && !jk.dbg && jk.mode == 2 && b->bounds_uniform && b->use_ub) { rung = "kub"; k = jk.soc ? b->kernel->kubsoc : b->kernel->kub; }
        else if (!jk.lin && !jk.het) { rung = "k"; k = b->kernel->k[jk.soc][jk.dbg][jk.mode]; }
        else if (jk.lin && !jk.het && !jk.dbg && jk.kmax == LIN_KMAX) { rung = "klin"; k = b->kernel->klin[jk.soc][jk.lin]; }
        else if (jk.het && !jk.lin && !jk.dbg) {
            if (b->het_ub && b->bounds_uniform && b->use_ub && b->kernel->khetub[jk.soc]) { rung = "khetub"; k = b->kernel->khetub[jk.soc]; }
            else if (b->het_ub && b->bounds_uniform && b->use_ub && !b->no_jit && !b->variant_jit_failed) { rung = "hetub_jit"; jk.ub = 1; }
            else { rung = "khet"; k = b->kernel->khet[jk.soc]; }
        }
    }
    int ipw = 4;
    if (k && b->kernel && b->half_rows != 0 && (k == b->kernel->kub || k == b->kernel->k[0][0][2])) {
        SolveKernel kh = b->kernel->khalf[k == b->kernel->kub ? 1 : 0];
        if (kh) { k = kh; ipw = 8; }
    }
    b->last_half = ipw == 8;
    if (k && b->kernel && b->prefetch != 0 && steps == 1 && !a.traj && b->grid_waves_per_cu == 0) {
        SolveKernel c = nullptr;
        if (k == b->kernel->kub) c = b->kernel->kpf[1];
        else if (k == b->kernel->k[0][0][2]) c = b->kernel->kpf[0];
        else if (k == b->kernel->khalf[1]) c = b->kernel->khalfpf[1];
        else if (k == b->kernel->khalf[0] && b->kernel->khalf[0]) c = b->kernel->khalfpf[0];
        if (c) kpf = c;
    }
    const bool jit_fn = !k;                          // (run-time instantiation taken as succeeding; its failure is P.fallback)
    if (jk.ub && !jk.pb && b->kernel && b->kernel->khet[jk.soc]) P.fallback = k ? nullptr : b->kernel->khet[jk.soc];
    b->last_ub = jit_fn ? jk.ub != 0
                        : (b->kernel && (k == b->kernel->kub || k == b->kernel->kubsoc || k == b->kernel->khetub[0] || k == b->kernel->khetub[1] || k == b->kernel->khalf[1]));
    // ======== end of the parent's text
    P.jk = jk; P.k = k; P.kpf = kpf; P.ipw = ipw; P.last_ub = b->last_ub; P.rung = rung;
    return P;
}

// the fake entry of a slot pattern: a filled slot holds its own name
static char g_names[64][16];
static int g_nnames = 0;
static SolveKernel token(bool filled, const char* fmt, int i = 0, int j = 0, int l = 0) {
    if (!filled) return nullptr;
    snprintf(g_names[g_nnames], sizeof(g_names[0]), fmt, i, j, l);
    return g_names[g_nnames++];
}
static KernelEntry fake_entry(const EntrySlots& s) {
    KernelEntry e{};
    g_nnames = 0;
    for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < 2; ++j)
            for (int l = 0; l < 3; ++l) e.k[i][j][l] = token(s.k[i][j][l], "K[%d][%d][%d]", i, j, l);
        for (int j = 0; j < 4; ++j) e.klin[i][j] = token(s.klin[i][j], "KLIN[%d][%d]", i, j);
        e.khet[i] = token(s.khet[i], "KHET[%d]", i); e.khetub[i] = token(s.khetub[i], "KHETUB[%d]", i); e.kadapt[i] = token(s.kadapt[i], "KADAPT[%d]", i);
        e.khalf[i] = token(s.khalf[i], "KHALF[%d]", i); e.kpf[i] = token(s.kpf[i], "KPF[%d]", i); e.khalfpf[i] = token(s.khalfpf[i], "KHALFPF[%d]", i);
    }
    e.kub = token(s.kub, "KUB"); e.kubsoc = token(s.kubsoc, "KUBSOC");
    return e;
}
static SolveKernel slot_token(const KernelEntry* e, const SlotRef& r) { return e ? slot_value(*e, r) : nullptr; }

int main() {
    long compared = 0, disagreements = 0;
    std::map<std::string, long> rungs, resolved;
    static const int MODES[] = {-1, 0, 1, 2, 3}, KM[] = {0, 4, 8, 16, 32}, IKM[] = {0, 1, 4, 32};
    int patterns = 0;
    for (int entry = 0; entry < 3; ++entry)
        for (int opt = 0; opt < 8; ++opt) {
            EntrySlots s;
            if (entry) {
                s.has_entry = s.k[0][0][2] = s.kub = true;
                for (int i = 0; i < 2 && entry == 2; ++i) {
                    for (int j = 0; j < 2; ++j)
                        for (int l = 0; l < 3; ++l) s.k[i][j][l] = true;
                    for (int j = 1; j < 4; ++j) s.klin[i][j] = true;
                    s.khet[i] = s.khetub[i] = s.kadapt[i] = s.kubsoc = true;
                }
            }
            for (int i = 0; i < 2; ++i) { s.khalf[i] = opt & 1; s.kpf[i] = (opt & 2) != 0; s.khalfpf[i] = (opt & 4) != 0; }
            if (!variant_facts_consistent(VariantFacts{}, s)) continue;
            ++patterns;
            const KernelEntry e = fake_entry(s);
            for (long bits = 0; bits < (1L << 15); ++bits)
                for (int lin = 0; lin < 4; ++lin)
                    for (int mode : MODES)
                        for (int km : KM)
                            for (int ikm : IKM) {
                                VariantFacts f;
                                int at = 0;
                                auto bit = [&]() { return ((bits >> at++) & 1) != 0; };
                                f.lin = lin; f.dpp_mode = mode; f.lin_kmax = km; f.il_km = ikm;
                                f.pl = bit(); f.pb = bit(); f.soc = bit(); f.debug = bit(); f.hetero = bit(); f.adaptive = bit(); f.uniform_ub = bit(); f.het_ub = bit();
                                f.half_rows = bit(); f.no_jit = bit(); f.variant_jit_failed = bit(); f.prefetch_on = bit(); f.single_step = bit(); f.no_ref_window = bit();
                                f.default_grid = bit();
                                if (!variant_facts_consistent(f, s)) continue;
                                TinyBatch b{};
                                b.kernel = entry ? &e : nullptr;
                                b.nx = 4; b.nu = 2; b.N = 10;
                                b.dpp_mode = mode; b.il_km = ikm; b.shared_kmax = km; b.half_rows = f.half_rows ? -1 : 0; b.prefetch = f.prefetch_on ? -1 : 0;
                                b.grid_waves_per_cu = f.default_grid ? 0 : 2;
                                b.debug = f.debug; b.hetero = f.hetero; b.adaptive = f.adaptive; b.bounds_uniform = f.uniform_ub; b.use_ub = true; b.het_ub = f.het_ub;
                                b.no_jit = f.no_jit; b.variant_jit_failed = f.variant_jit_failed;
                                const Args a{f.no_ref_window ? nullptr : (const void*)&b};
                                const Parent P = parent(&b, Decision{f.lin, f.pl, f.pb}, f.soc, f.single_step ? 1 : 3, a);
                                const VariantChoice c = choose_one_row_variant(f, s);
                                JitKey key = c.key;
                                key.nx = b.nx; key.nu = b.nu; key.N = b.N;
                                const bool same = !(key < P.jk) && !(P.jk < key) && slot_token(b.kernel, c.slot) == P.k && c.ipw == P.ipw &&
                                                  slot_token(b.kernel, c.prefetch) == P.kpf && c.ub_form == P.last_ub && slot_token(b.kernel, c.fallback) == P.fallback &&
                                                  (c.ipw == 8) == b.last_half;
                                ++compared;
                                if (!same && ++disagreements <= 10)
                                    printf("DISAGREE entry=%d opt=%d bits=%ld lin=%d mode=%d km=%d ikm=%d: parent k=%s kpf=%s ipw=%d ub=%d fb=%s\n", entry, opt, bits, lin, mode, km, ikm,
                                           P.k ? P.k : "-", P.kpf ? P.kpf : "-", P.ipw, (int)P.last_ub, P.fallback ? P.fallback : "-");
                                rungs[P.rung]++;
                                resolved[std::string(P.k ? P.k : "jit") + (P.kpf ? std::string("+") + P.kpf : "")]++;
                            }
        }
    printf("patterns=%d compared=%ld disagreements=%ld\n", patterns, compared, disagreements);
    for (const auto& kv : rungs) printf("rung %s %ld\n", kv.first.c_str(), kv.second);
    for (const auto& kv : resolved) printf("resolved %s %ld\n", kv.first.c_str(), kv.second);
    return disagreements ? 1 : 0;
}
