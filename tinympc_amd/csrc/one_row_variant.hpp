// one_row_variant.hpp -- which instantiation of admm_solve_kernel a launch on the one-row kernel runs, once decide_path (kernel_path.hpp)
// has said "one-row kernel, lin / pl / pb": ONE function (choose_one_row_variant) over a flat set of facts (VariantFacts) and the flags
// of the slots the shape's compiled-in entry holds (EntrySlots; batch_dispatch.hip entry_slots is the only code that reads them off a
// KernelEntry).  The answer is the complete key of the instantiation, the compiled-in slot that serves it by NAME (or: instantiate at
// run time), instances per wave, the PREFETCH slot, whether the form is a UB form and the slot to fall back to -- nothing downstream
// compares kernel pointers to find out what was chosen.  Plain C++17, no HIP, no allocation: once per launch_solve call;
// tests/dropin/one_row_variant_driver.cpp runs it on the host.  The rungs in order and what they inherit: profiles/one_row_variant.md
#pragma once

namespace tinympc_amd {

struct JitKey {
    int nx, nu, N, soc, dbg, mode, lin, het, kmax, adapt;
    int ub = 0;               // the knot-invariant-bounds form (round 5: for the per-instance-data variant, which is only compiled in without it)
    int pb = 0;               // every instance its own box (admm_kernel.hip.h PB): run-time instantiated only
    int pl = 0;               // every instance its own half-spaces (admm_kernel.hip.h PL): run-time instantiated only, kmax from 1
    int pc = 0;               // every instance its own cone coefficients (admm_kernel.hip.h PC): run-time instantiated only, with soc
    int pd = 0;               // every instance its own disturbance at the plant step (admm_kernel.hip.h PD): run-time instantiated only
    int pp = 0;               // a plant of its own at the plant step (admm_kernel.hip.h PP): run-time instantiated only
    int pm = 0;               // the solve runs from a measured state, the plant from the true one (admm_kernel.hip.h PM): run-time instantiated only, with pp
    int pe = 0;               // a state estimator between the measurement and the solve (admm_kernel.hip.h PE): run-time instantiated only, with pm and pp
    int ps = 0;               // a closed-loop score at the plant step (admm_kernel.hip.h PS): run-time instantiated only, with pd or pp
    int pa = 0;               // an actuator model between the command and the plant step (admm_kernel.hip.h PA): run-time instantiated only, with pp
    int pq = 0;               // a transport delay in front of the actuator's stages (admm_kernel.hip.h PQ): run-time instantiated only, with pa
    int px = 0;               // the solve runs from the model's prediction over the delay's queue (admm_kernel.hip.h PX): run-time instantiated only, with pq and pm
    bool operator<(const JitKey& o) const {
        const int a[22] = {nx, nu, N, soc, dbg, mode, lin, het, kmax, adapt, ub, pb, pl, pc, pd, pp, pm, pe, ps, pa, pq, px},
                  b[22] = {o.nx, o.nu, o.N, o.soc, o.dbg, o.mode, o.lin, o.het, o.kmax, o.adapt, o.ub, o.pb, o.pl, o.pc, o.pd, o.pp, o.pm, o.pe, o.ps, o.pa, o.pq, o.px};
        for (int i = 0; i < 22; ++i)
            if (a[i] != b[i]) return a[i] < b[i];
        return false;
    }
};

constexpr int VARIANT_LIN_KMAX = 4;      // admm_kernel.hip.h LIN_KMAX (batch_dispatch.hip asserts it): the stride the compiled-in half-space variants have

// which slots of a KernelEntry (kernel_entry.hpp) are filled; the same names and indices.  KERNELS_FOR fills everything from k to
// kubsoc (klin[][0] excepted: LIN = 0 is no half-space variant), KERNELS_LEAN only k[0][0][2] and kub; khalf / kpf / khalfpf depend on
// the shape under both
struct EntrySlots {
    bool has_entry = false;
    bool k[2][2][3] = {};      // [soc][dbg][mode]
    bool klin[2][4] = {};      // [soc][lin]
    bool khet[2] = {}, khetub[2] = {};      // [soc]
    bool kadapt[2] = {};       // [dbg]
    bool kub = false, kubsoc = false;
    bool khalf[2] = {}, kpf[2] = {}, khalfpf[2] = {};      // [ub]
};

enum OneRowSlot { SLOT_NONE = 0, SLOT_K, SLOT_KUB, SLOT_KUBSOC, SLOT_KLIN, SLOT_KHET, SLOT_KHETUB, SLOT_KADAPT, SLOT_KHALF, SLOT_KPF, SLOT_KHALFPF };
struct SlotRef {               // a slot with its indices in the order of the entry's declaration (SLOT_K: i j l, SLOT_KLIN: i j, the other arrays: i)
    OneRowSlot slot = SLOT_NONE;
    int i = 0, j = 0, l = 0;
    bool is(OneRowSlot s, int i_ = 0, int j_ = 0, int l_ = 0) const { return slot == s && i == i_ && j == j_ && l == l_; }
};
// what the slot holds: a flag of EntrySlots or a kernel of KernelEntry (the same member names); SLOT_NONE: false / nullptr
template <class Entry>
inline auto slot_value(const Entry& e, const SlotRef& r) -> decltype(e.kub) {
    switch (r.slot) {
    case SLOT_K: return e.k[r.i][r.j][r.l];
    case SLOT_KUB: return e.kub;
    case SLOT_KUBSOC: return e.kubsoc;
    case SLOT_KLIN: return e.klin[r.i][r.j];
    case SLOT_KHET: return e.khet[r.i];
    case SLOT_KHETUB: return e.khetub[r.i];
    case SLOT_KADAPT: return e.kadapt[r.i];
    case SLOT_KHALF: return e.khalf[r.i];
    case SLOT_KPF: return e.kpf[r.i];
    case SLOT_KHALFPF: return e.khalfpf[r.i];
    default: return {};
    }
}
inline bool slot_present(const EntrySlots& s, const SlotRef& r) { return slot_value(s, r); }

struct VariantFacts {
    // ---- from the path decision
    int lin = 0;                       // the LIN template value (0: no half-space variant)
    bool pl = false, pb = false;       // the per-instance half-space / box form
    bool pc = false;                   // the per-instance cone-coefficient form
    bool pd = false;                   // the per-instance disturbance form: any of the above, or none, with bit 5
    bool pp = false;                   // the form with a plant of its own: likewise, with bit 6 (with or without bit 5)
    bool pm = false;                   // the measured-state form: bit 7, always with bit 6
    bool pe = false;                   // the state-estimator form: bit 8, always with bits 7 and 6
    bool ps = false;                   // the closed-loop-score form: bit 9, always with bit 5 or bit 6
    bool pa = false;                   // the actuator-model form: bit 10, always with bit 6
    bool pq = false;                   // the transport-delay form: bit 12, always with bit 10 (bit 11 names no form)
    bool px = false;                   // the delay-predictor form: bit 13, always with bits 12 and 7
    // ---- from the problem
    bool soc = false, debug = false;
    int dpp_mode = 0;                  // option "dpp_mode" as set (values outside 0..2 count as 0)
    bool hetero = false, adaptive = false;
    int lin_kmax = 0;                  // table stride of the shared half-spaces (asked with lin != 0 only)
    int il_km = 0;                     // ... of the per-instance blocks (pl only)
    bool uniform_ub = false;           // bounds_uniform && use_ub: the box is knot-invariant and the UB forms are allowed
    // ---- options and what failed earlier
    bool het_ub = false, half_rows = false, no_jit = false, variant_jit_failed = false;
    // ---- the launch, as far as the PREFETCH form asks
    bool prefetch_on = false;          // option "prefetch" != 0
    bool single_step = false;          // steps == 1
    bool no_ref_window = false;        // no reference-trajectory window
    bool default_grid = false;         // option "grid_waves_per_cu" == 0
};

// what batch_dispatch.hip can produce (a necessary condition, not a tight one): the sweep of tests/dropin/one_row_variant_driver.cpp
// counts these combinations only.  decide_path gives pl with half-spaces only, pb for the plain box launch only, both only where
// run-time instantiation may be tried, and refuses adaptive rho with either and with half-spaces; pc for a cone launch without
// half-spaces, a per-instance box or debug outputs only, under the same two conditions.
inline bool variant_facts_consistent(const VariantFacts& f, const EntrySlots& s) {
    auto stride = [](int km) { return km == 4 || km == 8 || km == 16 || km == 32; };
    const bool rest = s.k[0][0][0];    // every slot but k[0][0][2], kub and the shape-dependent ones: KERNELS_FOR fills them all, KERNELS_LEAN none
    bool slots_ok = s.has_entry ? (s.kub && s.k[0][0][2]) : !(s.kub || s.k[0][0][2] || rest);
    for (int i = 0; i < 2; ++i) {
        for (int j = 0; j < 2; ++j)
            for (int l = 0; l < 3; ++l) slots_ok = slots_ok && (s.k[i][j][l] == rest || (i == 0 && j == 0 && l == 2));
        for (int j = 1; j < 4; ++j) slots_ok = slots_ok && s.klin[i][j] == rest;
        slots_ok = slots_ok && !s.klin[i][0] && s.khet[i] == rest && s.khetub[i] == rest && s.kadapt[i] == rest;
        slots_ok = slots_ok && (s.has_entry || !(s.khalf[i] || s.kpf[i] || s.khalfpf[i])) && (!s.khalfpf[i] || s.khalf[i]);
    }
    slots_ok = slots_ok && s.kubsoc == rest && s.khalf[0] == s.khalf[1] && s.kpf[0] == s.kpf[1] && s.khalfpf[0] == s.khalfpf[1];
    return slots_ok && f.lin >= 0 && f.lin <= 3 && (!f.pl || f.lin) && !(f.pb && (f.pl || f.soc || f.lin || f.debug)) && !(f.pl && f.debug) &&
           !((f.pb || f.pl) && (f.no_jit || f.variant_jit_failed)) && !(f.adaptive && (f.pb || f.pl || f.lin)) &&
           (f.lin ? (f.pl ? f.lin_kmax == 0 || stride(f.lin_kmax) : stride(f.lin_kmax)) : f.lin_kmax == 0) &&
           (f.pl ? f.il_km >= 1 && f.il_km <= 32 : f.il_km == 0) &&
           !(f.pc && (!f.soc || f.pb || f.pl || f.lin || f.debug || f.adaptive || f.no_jit || f.variant_jit_failed)) &&
           !((f.pd || f.pp) && (f.debug || f.adaptive || f.no_jit || f.variant_jit_failed)) &&     // (decide_path: a PD / PP form only where hipRTC may be tried)
           !(f.pm && !f.pp) &&                                                                     // (... and a PM form is a PP form)
           !(f.pe && !f.pm) &&                                                                     // (... and a PE form is a PM form)
           !(f.ps && !(f.pd || f.pp)) &&                                                           // (... and a PS form is a PD or a PP form)
           !(f.pa && !f.pp) &&                                                                     // (... and a PA form is a PP form)
           !(f.pq && !f.pa) && !(f.px && !(f.pq && f.pm));                                         // (... a PQ form a PA form, a PX form a PQ and a PM form)
}

struct VariantChoice {
    JitKey key = {};           // every field but nx, nu, N (0: the caller's)
    SlotRef slot;              // the compiled-in instantiation that serves; SLOT_NONE: instantiate `key` at run time
    int ipw = 4;               // instances per wave: 8 in the HALF form
    SlotRef prefetch;          // the PREFETCH form of `slot` for a launch that can take it; SLOT_NONE: none
    bool ub_form = false;      // the form keeps the knot-invariant box in registers
    SlotRef fallback;          // the compiled-in slot that serves (with key.ub = 0) if `key` cannot be instantiated; SLOT_NONE: none
};

// the compiled-in slot of a box / cone launch without half-spaces, per-instance data or adaptive rho: the UB form where the box is
// knot-invariant (no debug outputs, single-chain FMA blocks), else k[soc][dbg][mode] -- a UB slot that is empty is NOT replaced by k[][][]
inline SlotRef plain_slot(bool soc, bool dbg, int mode, bool uniform_ub) {
    if (!dbg && mode == 2 && uniform_ub) return SlotRef{soc ? SLOT_KUBSOC : SLOT_KUB};
    return SlotRef{SLOT_K, soc ? 1 : 0, dbg ? 1 : 0, mode};
}
inline int clamped_dpp_mode(int dpp_mode) { return (dpp_mode >= 0 && dpp_mode <= 2) ? dpp_mode : 0; }

inline VariantChoice choose_one_row_variant(const VariantFacts& f, const EntrySlots& s) {
    VariantChoice c;
    JitKey& k = c.key;
    const int soc = f.soc ? 1 : 0, dbg = f.debug ? 1 : 0;
    // ---- the key: <SOC, DBG, MODE, LIN, HET, KMAX, ADAPT, UB, PB, PL, PC>
    k.soc = soc; k.dbg = dbg; k.mode = clamped_dpp_mode(f.dpp_mode);
    k.lin = f.lin; k.het = f.hetero ? 1 : 0; k.adapt = f.adaptive ? 1 : 0;
    k.pl = (f.lin && f.pl) ? 1 : 0;                                      // (the PL form rides on a half-space variant, at the blocks' own stride)
    k.kmax = !f.lin ? VARIANT_LIN_KMAX : k.pl ? f.il_km : f.lin_kmax;
    if (k.lin || k.het || k.adapt) k.mode = 2;                           // those variants exist on the single-chain FMA blocks only
    if (f.pb) { k.pb = 1; k.ub = (f.uniform_ub && (!f.hetero || f.het_ub)) ? 1 : 0; }
    // (the PC form rides on the cone variant -- full rows, no PREFETCH slot --, on its UB form where the compiled-in rungs below would take one)
    if (f.pc && f.soc) { k.pc = 1; k.ub = (!dbg && k.mode == 2 && f.uniform_ub && (!f.hetero || f.het_ub)) ? 1 : 0; }
    // ---- the rungs: which compiled-in slot holds that key (PB, PL and PC are run-time instantiated only: the entry is not asked)
    // (the PD form of whatever the key is by now -- full rows, no PREFETCH slot --, on the UB form where the compiled-in rungs below would
    // take one: their conditions, asked of the key, since no rung is)
    if (f.pd || f.pp) {                                                  // (PP: PD's rule, bit for bit)
        k.pd = f.pd ? 1 : 0; k.pp = f.pp ? 1 : 0; k.pm = (f.pp && f.pm) ? 1 : 0; k.pe = (k.pm && f.pe) ? 1 : 0; k.ps = f.ps ? 1 : 0; k.pa = (f.pp && f.pa) ? 1 : 0;
        k.pq = (k.pa && f.pq) ? 1 : 0; k.px = (k.pq && k.pm && f.px) ? 1 : 0;
        if (!k.pb && !k.pc && !k.lin && !k.adapt && !dbg && k.mode == 2) k.ub = (f.uniform_ub && (!f.hetero || f.het_ub)) ? 1 : 0;
    }
    SlotRef want;
    if (s.has_entry && !k.pb && !k.pl && !k.pc && !k.pd && !k.pp) {
        if (k.adapt) { if (!k.soc && !k.het) want = SlotRef{SLOT_KADAPT, dbg}; }      // (with a cone or per-instance data: run-time instantiated, jit_prebuilt.txt)
        else if (!k.lin && !k.het) want = plain_slot(f.soc, f.debug, k.mode, f.uniform_ub);
        else if (k.lin && !k.het && !dbg && k.kmax == VARIANT_LIN_KMAX) want = SlotRef{SLOT_KLIN, soc, k.lin};
        else if (k.het && !k.lin && !dbg) {
            // per-instance data with a knot-invariant box: the UB form of the HET variant, compiled in for the shapes with the full
            // variant set, instantiated at run time for the others (the form without it serves if that fails); "het_ub" = 0: without
            const bool ub = f.het_ub && f.uniform_ub;
            if (ub && s.khetub[soc]) want = SlotRef{SLOT_KHETUB, soc};
            else if (ub && !f.no_jit && !f.variant_jit_failed) { k.ub = 1; c.fallback = SlotRef{SLOT_KHET, soc}; }
            else want = SlotRef{SLOT_KHET, soc};
        }
    }
    if (slot_present(s, want)) c.slot = want;
    if (!slot_present(s, c.fallback)) c.fallback = SlotRef{};
    // ---- HALF rows (nx+nu <= 8): the plain box launch takes the form that puts two instances into a DPP row, eight per wave
    if (f.half_rows && (c.slot.is(SLOT_KUB) || c.slot.is(SLOT_K, 0, 0, 2))) {
        const SlotRef half{SLOT_KHALF, c.slot.is(SLOT_KUB) ? 1 : 0};
        if (slot_present(s, half)) { c.slot = half; c.ipw = 8; }
    }
    // ---- the PREFETCH form: a plain single-step launch over the whole batch, where the variant has the form
    if (f.prefetch_on && f.single_step && f.no_ref_window && f.default_grid) {
        SlotRef pf;
        if (c.slot.is(SLOT_KUB)) pf = SlotRef{SLOT_KPF, 1};
        else if (c.slot.is(SLOT_K, 0, 0, 2)) pf = SlotRef{SLOT_KPF, 0};
        else if (c.slot.slot == SLOT_KHALF) pf = SlotRef{SLOT_KHALFPF, c.slot.i};
        if (slot_present(s, pf)) c.prefetch = pf;
    }
    c.ub_form = c.slot.slot == SLOT_NONE ? k.ub != 0
                                         : (c.slot.slot == SLOT_KUB || c.slot.slot == SLOT_KUBSOC || c.slot.slot == SLOT_KHETUB || c.slot.is(SLOT_KHALF, 1));
    return c;
}

}  // namespace tinympc_amd
