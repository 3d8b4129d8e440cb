// kernel_path_before_delay.hpp -- a frozen copy, in a namespace of its own, of csrc/kernel_path.hpp as it stood before the transport
// delay: tests/dropin/delay_path_driver.cpp compares today's decisions with its.  From here on the header's own text:
// kernel_path.hpp -- which kernel a solve runs on (the one-row register kernel, the tile kernel or the coverage kernel), which half-space /
// per-instance form of the one-row kernel it takes and which combinations with adaptive rho are refused: ONE ordered list of rules
// (decide_path) over a flat set of facts (PathFacts; batch_dispatch.hip path_facts is the only code that reads them off a handle).
// Plain C++17, no HIP: tests/dropin/kernel_path_driver.cpp runs every rule on the host.  The decision is made once per launch_solve
// call and is not kept on the handle: any setter can change a fact.  The rules, their order and their oddities: profiles/kernel_path.md
#pragma once

namespace kernel_path_before_delay {

struct PathFacts {
    // ---- what the shape allows (with the cone / debug / FMA-block mode that are on)
    bool has_entry = false;        // kernel_dims.txt holds the shape: a compiled-in one-row entry exists
    bool entry_plain = false;      // ... and it holds the box / cone variant asked for (LEAN shapes: <box, no debug, mode 2> and the UB form only)
    bool entry_klin = false;       // ... and the half-space variant klin[cone][lin_families]
    bool fits_box = false;         // jit_shape_fits without a cone: run-time instantiation can make a one-row kernel for the shape
    bool fits = false;             // jit_shape_fits with the cone that is on
    bool has_tile = false;         // a tile entry exists (tile_dims.txt, or a tile shape chosen at run time:)
    bool tile_is_jit = false;
    bool tile_lin = false;         // the tile kernel's half-space variant exists for the families and counts that are on
    int lin_kmax = 0;              // table stride of the shared half-spaces: 4 (compiled in), 8 / 16 / 32 (run-time instantiated), 0: too many (or none on)
    bool planes_fit = false;       // the one-row variant's slack planes fit a wave's LDS at that stride
    bool pl_planes_fit = false;    // ... and, at the per-instance blocks' stride (<= 32), with the four rows' own tables (the PL form)
    // ---- settings
    bool soc = false;              // a cone family is on
    int lin_families = 0;          // half-space sets that are on: bit 0 static, bit 1 time-varying
    bool cones_overlap = false;    // cones of an enabled family share rows
    bool hetero = false;           // per-instance problem data
    bool tile_ext = false;         // reference window / reset_duals / one_shot: bit 0 of the tile kernel's EXT value
    bool adaptive = false;
    bool debug = false;
    bool inst_bounds = false;      // every instance its own box
    int inst_lin = 0;              // ... its own half-spaces: the sets installed AND on (a subset of lin_families)
    bool inst_cones = false;       // ... its own cone coefficients: installed AND a cone family on
    // ---- options
    bool force_general = false, no_jit = false, no_tile = false, prefer_tile = false;
    // ---- what failed earlier on this handle
    bool jit_failed = false;            // the shape's one-row kernel could not be instantiated
    bool variant_jit_failed = false;    // a variant outside the compiled-in set could not
    bool tile_soc_failed = false;       // a cone / half-space / EXT form of the tile kernel could not
    // ---- the plant (appended: every decision with it off is what it was)
    bool disturbance = false;           // a per-instance disturbance sequence is installed AND the launch takes a plant step
    bool plant = false;                 // a plant of its own is installed AND the launch takes a plant step
    bool state_log = false;             // the state log is on AND the launch takes a plant step
    bool measurement = false;           // a measurement-noise sequence is installed AND the launch takes a plant step
    bool estimator = false;             // a state estimator is installed AND the launch takes a plant step
    bool score = false;                 // a closed-loop score is installed AND the launch takes a plant step
    bool actuator = false;              // an actuator model or an actuation-noise sequence is installed AND the launch takes a plant step
};

// what path_facts can produce: the sweep of tests/dropin/kernel_path_driver.cpp counts these combinations only
inline bool facts_consistent(const PathFacts& f) {
    const bool km_ok = f.lin_kmax == 0 || f.lin_kmax == 4 || f.lin_kmax == 8 || f.lin_kmax == 16 || f.lin_kmax == 32;
    return km_ok && f.lin_families >= 0 && f.lin_families <= 3 && (f.inst_lin & ~f.lin_families) == 0 &&
           (f.lin_families || f.lin_kmax == 0) &&                                   // a stride only with a family on
           (!f.planes_fit || f.lin_kmax != 0) && (!f.pl_planes_fit || f.lin_families) &&
           (!f.entry_plain || f.has_entry) && (!f.entry_klin || (f.has_entry && f.lin_families)) &&
           (!f.fits || f.fits_box) && (f.soc || f.fits == f.fits_box) &&             // a cone costs registers
           (!f.tile_is_jit || f.has_tile) && (!f.tile_lin || (f.has_tile && f.lin_kmax != 0)) &&
           (!f.cones_overlap || f.soc) && (!f.inst_cones || f.soc);
}

enum KernelPath { ONE_ROW = 0, TILE = 1, COVERAGE = 2 };
// what adaptive rho does not combine with, and the texts callers read through tiny_batch_last_error: PATH_REFUSAL_MESSAGE is indexed by
// the enumerator.  The values are the order the refusals were added in; the order they are REPORTED in is decide_path's
enum PathRefusal { REFUSE_NONE = 0, REFUSE_ADAPTIVE_INSTANCE_BOX, REFUSE_ADAPTIVE_HALFSPACES, REFUSE_ADAPTIVE_OVERLAPPING_CONES, REFUSE_ADAPTIVE_NO_REGISTER_FORM,
                   REFUSE_ADAPTIVE_INSTANCE_CONES, REFUSE_ADAPTIVE_DISTURBANCE, REFUSE_ADAPTIVE_PLANT, REFUSE_ADAPTIVE_STATE_LOG, REFUSE_ADAPTIVE_MEASUREMENT,
                   REFUSE_ADAPTIVE_ESTIMATOR, REFUSE_ADAPTIVE_SCORE, REFUSE_ADAPTIVE_ACTUATOR };
constexpr const char* PATH_REFUSAL_MESSAGE[] = {
    "",
    "adaptive rho does not combine with per-instance bounds (tiny_batch_set_instance_bounds): a per-instance box "
    "with a moving cache would need the coverage kernel, which does not take adaptive rho",
    // (per-instance or shared half-spaces; also what the one-row launch answers to one_shot and repack_after > 0: build_one_row_launch)
    "adaptive rho does not combine with heterogeneous data / half-spaces / one_shot / repack_after",
    "overlapping cones run on the coverage kernel: no adaptive rho with them",
    "adaptive rho needs the register-resident kernel (nx+nu <= 16, horizon within the register file)",
    "adaptive rho does not combine with per-instance cone coefficients (tiny_batch_set_instance_cone_coefficients): the adaptive cone "
    "form has no per-instance coefficients, and the coverage kernel does not take adaptive rho",
    "adaptive rho does not combine with a per-instance disturbance",
    "adaptive rho does not combine with a plant of its own at the plant step (tiny_batch_set_plant)",
    "adaptive rho does not combine with the state log (option state_log)",
    "adaptive rho does not combine with measurement noise (tiny_batch_set_measurement_noise)",
    "adaptive rho does not combine with a state estimator (tiny_batch_set_estimator)",
    "adaptive rho does not combine with a closed-loop score (tiny_batch_set_score)",
    "adaptive rho does not combine with an actuator model (tiny_batch_set_actuator)",
};
static_assert(sizeof(PATH_REFUSAL_MESSAGE) / sizeof(PATH_REFUSAL_MESSAGE[0]) == REFUSE_ADAPTIVE_ACTUATOR + 1, "one text per refusal");
inline const char* path_refusal_message(PathRefusal r) { return PATH_REFUSAL_MESSAGE[r]; }

struct PathDecision {
    KernelPath kernel;
    int lin;                       // ONE_ROW: the LIN template value of the launch (0: no half-space variant)
    int pl, pb;                    // ONE_ROW: the per-instance half-space / box form
    PathRefusal refusal;           // launch_solve reports it instead of launching; tiny_batch_kernel_path answers all the same
    const char* rule;              // the rule that decided
    int pc = 0;                    // ONE_ROW: the per-instance cone-coefficient form
    int pd = 0;                    // ONE_ROW: the per-instance disturbance form (of whatever form the fields above name)
    int pp = 0;                    // ONE_ROW: the form with a plant of its own (likewise; with or without pd)
    int pm = 0;                    // ONE_ROW: the form that solves from a measured state (likewise; always with pp)
    int pe = 0;                    // ONE_ROW: the form with a state estimator in front of the solve (likewise; always with pm and pp)
    int ps = 0;                    // ONE_ROW: the form that scores what the plant step hands on (likewise; always with pd or pp)
    int pa = 0;                    // ONE_ROW: the form with an actuator model between the command and the plant step (likewise; always with pp)
};

// a one-row kernel exists for the shape: compiled in (counted even under no_jit), or one that run-time instantiation can make
inline bool one_row_form_exists(const PathFacts& f) { return f.has_entry || (!f.no_jit && !f.jit_failed && f.fits); }

inline PathDecision decide_path(const PathFacts& f) {
    const bool regs = one_row_form_exists(f);
    const bool hiprtc = !f.no_jit && !f.jit_failed && !f.variant_jit_failed;      // run-time instantiation of a one-row variant may be tried
    const int lf = f.lin_families;
    // refusals, in the order they are reported; the rules below answer for a refused combination too
    const PathRefusal refusal = !f.adaptive        ? REFUSE_NONE
                                : f.inst_bounds    ? REFUSE_ADAPTIVE_INSTANCE_BOX
                                : f.inst_lin       ? REFUSE_ADAPTIVE_HALFSPACES
                                : f.inst_cones     ? REFUSE_ADAPTIVE_INSTANCE_CONES
                                : f.cones_overlap  ? REFUSE_ADAPTIVE_OVERLAPPING_CONES
                                : !regs            ? REFUSE_ADAPTIVE_NO_REGISTER_FORM
                                : lf               ? REFUSE_ADAPTIVE_HALFSPACES          // shared ones, whether or not a one-row variant exists
                                : f.disturbance    ? REFUSE_ADAPTIVE_DISTURBANCE         // (last: every combination refused before keeps its text)
                                : f.plant          ? REFUSE_ADAPTIVE_PLANT
                                : f.state_log      ? REFUSE_ADAPTIVE_STATE_LOG
                                : f.measurement    ? REFUSE_ADAPTIVE_MEASUREMENT
                                : f.estimator      ? REFUSE_ADAPTIVE_ESTIMATOR
                                : f.score          ? REFUSE_ADAPTIVE_SCORE
                                : f.actuator       ? REFUSE_ADAPTIVE_ACTUATOR
                                                   : REFUSE_NONE;
    auto tile = [&](const char* rule) { return PathDecision{TILE, 0, 0, 0, refusal, rule, 0, 0, 0, 0, 0, 0, 0}; };
    auto cover = [&](const char* rule) { return PathDecision{COVERAGE, 0, 0, 0, refusal, rule, 0, 0, 0, 0, 0, 0, 0}; };
    // the stages at the fused closed-loop plant step: ONE rule, applied to whatever one-row answer the rules below give -- the PD ... PA
    // form of that very form (PB, PL and PC forms take the bits and keep their rule's name; every other one-row answer is
    // "one_row:<form>"), run-time instantiated only: where hipRTC may not be tried, with debug outputs, under force_general and with
    // adaptive rho (refused) the coverage kernel answers, "cover:<form>".  A coverage answer stays what it is, the tile kernel is not
    // asked.  Which facts force which bits on, and the precedence of the name: profiles/kernel_path.md
    const bool closed_loop = f.disturbance || f.plant || f.state_log || f.measurement || f.estimator || f.score || f.actuator;
    const bool pd_form = f.fits && hiprtc && !f.force_general && !f.debug && !f.adaptive;
    const bool pe = f.estimator, pm = f.measurement || pe, pa = f.actuator, pp = f.plant || pm || pa, pd = f.disturbance || ((f.state_log || f.score) && !pp);
    const bool ps = f.score;
    struct FormRules { const char *cover, *one_row; };
    static constexpr FormRules FORMS[] = {{"cover:pd", "one_row:pd"}, {"cover:pp", "one_row:pp"}, {"cover:pm", "one_row:pm"},
                                          {"cover:pe", "one_row:pe"}, {"cover:ps", "one_row:ps"}, {"cover:pa", "one_row:pa"}};
    const FormRules& form = FORMS[pa ? 5 : ps ? 4 : pe ? 3 : pm ? 2 : pp ? 1 : 0];       // (the name's precedence: pa, ps, pe, pm, pp, pd)
    auto one_row = [&](int lin, int pl, int pb, const char* rule, int pc = 0) {
        if (!pd && !pp) return PathDecision{ONE_ROW, lin, pl, pb, refusal, rule, pc, 0, 0, 0, 0, 0, 0};
        if (!pd_form) return cover(form.cover);
        return PathDecision{ONE_ROW, lin, pl, pb, refusal, (pl || pb || pc) ? rule : form.one_row, pc, pd ? 1 : 0, pp ? 1 : 0, pm ? 1 : 0, pe ? 1 : 0, ps ? 1 : 0, pa ? 1 : 0};
    };
    // why the one-row kernel has no variant for the SHARED half-spaces that are on (nullptr: it has one, or none is on)
    const char* no_lin = !lf                                                                  ? nullptr
                         : !regs                                                              ? "cover:no_register_form"
                         : f.force_general                                                    ? "cover:force_general"
                         : f.variant_jit_failed && f.debug                                    ? "cover:halfspaces_debug_without_hiprtc"
                         : f.lin_kmax == 0                                                    ? "cover:too_many_halfspaces"
                         : f.lin_kmax > 4 && (f.no_jit || f.variant_jit_failed)               ? "cover:wide_halfspaces_without_hiprtc"
                         : f.variant_jit_failed && f.has_entry && !f.hetero && !f.entry_klin  ? "cover:lean_halfspaces_without_hiprtc"
                                                                                              : nullptr;
    // the tile kernel can run this launch (it has no per-instance box or half-spaces, no adaptive rho, no debug outputs; its cone /
    // half-space / EXT forms and every form of a shape outside tile_dims.txt are run-time instantiated; EXT forms are for the shapes
    // the one-row kernel does not hold)
    const bool ext = f.tile_ext || f.hetero;
    const bool tile_can = f.has_tile && !f.no_tile && !f.force_general && !f.debug && !(lf && !f.tile_lin) && !closed_loop &&
                          !((f.tile_is_jit || f.soc || lf || ext) && (f.no_jit || f.tile_soc_failed)) && !(ext && regs);

    // ---- the rules, in order
    // cones that share rows are projected one after the other: the coverage kernel only
    if (f.cones_overlap) return cover("cones_overlap");
    // every instance its own box: the one-row kernel's PB form of the plain box variant, run-time instantiated only (a compiled-in
    // entry is not asked); everything else on the coverage kernel
    if (f.inst_bounds) return (f.fits_box && !f.soc && !lf && !f.debug && !f.force_general && hiprtc) ? one_row(0, 0, 1, "one_row:pb") : cover("cover:pb");
    // every instance its own half-spaces: the PL form, run-time instantiated only, where its planes and the four rows' tables fit
    if (f.inst_lin && f.inst_cones) return cover("cover:pc_with_halfspaces");      // (PL and PC keep their pointers in one place: no form has both)
    if (f.inst_lin) {
        const bool pl_form = f.fits && !f.debug && !f.force_general && hiprtc && f.pl_planes_fit;
        if (f.adaptive) return one_row(pl_form ? lf : 0, pl_form ? 1 : 0, 0, "one_row:pl_adaptive");      // (refused)
        return pl_form ? one_row(lf, 1, 0, "one_row:pl") : cover("cover:pl");
    }
    // every instance its own cone coefficients: the PC form of the cone variant, run-time instantiated only, with or without per-instance
    // problem data; with shared half-spaces, on a tile-kernel shape and everywhere else on the coverage kernel (adaptive rho: refused)
    if (f.inst_cones) return (f.fits && !lf && !f.debug && !f.force_general && hiprtc) ? one_row(0, 0, 0, "one_row:pc", 1) : cover("cover:pc");
    // adaptive rho lives on the one-row kernel only (without a register form, or with shared half-spaces: refused)
    if (f.adaptive) return one_row(no_lin ? 0 : lf, 0, 0, "one_row:adaptive");
    if (tile_can && !regs) return tile("tile:no_register_form");
    if (tile_can && f.prefer_tile) return tile("tile:prefer_tile");
    if (tile_can && no_lin) return tile("tile:no_one_row_halfspace_variant");
    // (the one-row variant would run its per-knot form there, at one wave per SIMD)
    if (tile_can && lf && !f.planes_fit) return tile("tile:planes_do_not_fit_one_row");
    if (lf) return no_lin ? cover(no_lin) : one_row(lf, 0, 0, "one_row:halfspaces");
    // per-instance problem data (in front of the LEAN-shape rule: a LEAN shape's per-instance variant is tried even where its plain one is not)
    if (f.hetero) return (f.force_general || !regs || f.variant_jit_failed) ? cover("cover:per_instance_data") : one_row(0, 0, 0, "one_row:per_instance_data");
    // a cone / debug / dpp-mode variant outside the compiled-in set of a LEAN shape that run-time instantiation could not make either
    if (f.variant_jit_failed && f.has_entry && !f.entry_plain) return cover("cover:lean_variant_without_hiprtc");
    if (!regs) return cover("cover:no_register_form");
    if (f.force_general) return cover("cover:force_general");
    return one_row(0, 0, 0, "one_row:plain");
}

// tiny_batch_kernel_path: 0 the one-row kernel, compiled in; 1 the tile kernel; 2 the coverage kernel; 3 the one-row kernel, instantiated at
// run time (every form with a per-instance box, half-space set, cone coefficients, disturbance, plant, measurement noise, state estimator, closed-loop score or actuator model is); 4 the tile kernel, instantiated at run time
inline int kernel_path_code(const PathDecision& d, const PathFacts& f) {
    if (d.kernel == TILE) return f.tile_is_jit ? 4 : 1;
    if (d.kernel == COVERAGE) return 2;
    return (f.has_entry && !f.inst_bounds && !f.inst_lin && !d.pc && !d.pd && !d.pp) ? 0 : 3;
}

}  // namespace kernel_path_before_delay
