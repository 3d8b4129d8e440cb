"""CPU: which kernel a solve runs on, which form of the one-row kernel it takes and what adaptive rho is refused (csrc/kernel_path.hpp),
checked on the rule list itself.  It is plain C++ without a HIP call, so tests/dropin/kernel_path_driver.cpp answers for any set of facts
and counts the answers over every consistent combination of them.  The expected answers below are restated from the rules
(profiles/kernel_path.md lists them in order), not read off the driver: the GPU suite pins the choice only at the shapes and settings
its tests happen to use."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("kernel_path") / "driver")
    csrc = os.path.join(ROOT, "tinympc_amd", "csrc")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", csrc, os.path.join(ROOT, "tests", "dropin", "kernel_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def words(line):
    r = dict(w.split("=", 1) for w in line.split())
    return {k: (v if k in ("kernel", "rule") else int(v)) for k, v in r.items()}


@pytest.fixture(scope="module")
def ask(driver):
    def run(*queries):
        """each query: a dict of facts (unnamed facts are 0) -> the driver's answer as a dict; every query must be a consistent set"""
        lines = [" ".join("%s=%d" % kv for kv in q.items()) for q in queries]
        out = subprocess.run([driver], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
        assert len(out) == len(lines)
        rows = [words(ln) for ln in out]
        assert all(r.pop("consistent") == 1 for r in rows), [q for q, ln in zip(queries, out) if "consistent=0" in ln]
        return rows
    return run


def decision(kernel, rule, code, lin=0, pl=0, pb=0, refusal=0):
    return dict(kernel=kernel, lin=lin, pl=pl, pb=pb, refusal=refusal, rule=rule, code=code)


# shapes: what kernel_dims.txt holds with its full variant set / what only run-time instantiation serves / a tile-kernel shape
FULL = dict(has_entry=1, entry_plain=1, fits_box=1, fits=1)
JIT = dict(fits_box=1, fits=1)
TILE_ONLY = dict(has_tile=1)
# shared static half-spaces, four per knot, on a FULL shape whose entry holds the variant
LIN = dict(FULL, entry_klin=1, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1)
PLAIN_ANSWER = decision("ONE_ROW", "one_row:plain", 0)


def check(ask, cases):
    """cases: (facts, expected decision); all of them in one run of the driver"""
    got = ask(*[c[0] for c in cases])
    for (facts, want), have in zip(cases, got):
        assert have == want, (facts, have, want)


def test_rule_01_cones_that_share_rows_go_to_the_coverage_kernel(ask):
    """Rule 1 stands in front of everything; without it the per-instance box rule, next in order, answers."""
    base = dict(FULL, soc=1, cones_overlap=1, inst_bounds=1, has_tile=1, prefer_tile=1)
    check(ask, [(base, decision("COVERAGE", "cones_overlap", 2)),
                (dict(base, cones_overlap=0), decision("COVERAGE", "cover:pb", 2))])


def test_rule_02_per_instance_box_one_row_only_where_every_term_holds(ask):
    """Rule 2: the PB form is run-time instantiated only, for the plain box variant: each term alone sends the box to the coverage kernel.  A
    compiled-in entry is not asked (the answer is 3 on a compiled-in shape, and a shape with an entry that run-time instantiation does not
    hold stays on the coverage kernel).  Without the box the per-instance half-space rule is next."""
    base = dict(JIT, inst_bounds=1)
    one_row = decision("ONE_ROW", "one_row:pb", 3, pb=1)
    cover = decision("COVERAGE", "cover:pb", 2)
    offenders = [dict(fits_box=0, fits=0), dict(soc=1), dict(lin_families=1, lin_kmax=4), dict(debug=1), dict(force_general=1), dict(no_jit=1), dict(jit_failed=1),
                 dict(variant_jit_failed=1)]
    check(ask, [(base, one_row), (dict(FULL, inst_bounds=1), one_row), (dict(has_entry=1, entry_plain=1, inst_bounds=1), cover)] +
          [(dict(base, **o), cover) for o in offenders] +
          [(dict(base, has_tile=1, prefer_tile=1), one_row),                                  # (the tile kernel has no per-instance box)
           (dict(LIN, inst_bounds=1, inst_lin=1), cover),
           (dict(LIN, inst_lin=1), decision("ONE_ROW", "one_row:pl", 3, lin=1, pl=1))])


def test_rule_03_per_instance_halfspaces_one_row_only_where_every_term_holds(ask):
    """Rule 3: the PL form, run-time instantiated only, where its planes and the four rows' tables fit.  Adaptive rho stands in FRONT of the form's
    terms: the combination is refused, the answer stays the one-row kernel (path code 3) whether or not the form exists.  Without a
    per-instance set the shared half-space rules answer."""
    base = dict(JIT, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1, inst_lin=1)
    one_row = decision("ONE_ROW", "one_row:pl", 3, lin=1, pl=1)
    cover = decision("COVERAGE", "cover:pl", 2)
    offenders = [dict(soc=1, fits=0), dict(debug=1), dict(force_general=1), dict(no_jit=1), dict(jit_failed=1), dict(variant_jit_failed=1), dict(pl_planes_fit=0)]
    check(ask, [(base, one_row), (dict(LIN, inst_lin=1), one_row), (dict(base, soc=1), one_row), (dict(base, hetero=1), one_row),
                (dict(base, lin_families=3, inst_lin=2), decision("ONE_ROW", "one_row:pl", 3, lin=3, pl=1)),
                (dict(base, planes_fit=0, has_tile=1, tile_lin=1, prefer_tile=1), one_row)] +                # (the tile kernel has no per-instance half-spaces)
          [(dict(base, **o), cover) for o in offenders] +
          [(dict(base, adaptive=1), decision("ONE_ROW", "one_row:pl_adaptive", 3, lin=1, pl=1, refusal=2))] +
          [(dict(base, adaptive=1, **o), decision("ONE_ROW", "one_row:pl_adaptive", 3, refusal=2)) for o in offenders] +
          [(dict(base, inst_lin=0), decision("ONE_ROW", "one_row:halfspaces", 3, lin=1))])


def test_rule_04_adaptive_rho_stays_on_the_one_row_kernel(ask):
    """Rule 4: in front of the tile rules and of the half-space rules.  Shared half-spaces that are ON are refused (2) whether the one-row
    kernel has a variant for them (lin = lin_families) or not (lin = 0: too many per knot, force_general, a wide set without run-time
    instantiation) -- without the refusal the second kind ran the adaptive kernel with the half-spaces dropped.  A set that is installed
    but switched off is no fact at all (lin_families counts enabled sets), and without a register form that text (4) comes first."""
    wide = dict(LIN, lin_kmax=8, entry_klin=0)
    check(ask, [(dict(FULL, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 0)),
                (dict(FULL, adaptive=1, has_tile=1, prefer_tile=1), decision("ONE_ROW", "one_row:adaptive", 0)),
                (dict(FULL, has_tile=1, prefer_tile=1), decision("TILE", "tile:prefer_tile", 1)),
                (dict(FULL, adaptive=1, force_general=1), decision("ONE_ROW", "one_row:adaptive", 0)),
                (dict(LIN, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 0, lin=1, refusal=2)),
                (dict(LIN, adaptive=1, lin_families=2), decision("ONE_ROW", "one_row:adaptive", 0, lin=2, refusal=2)),
                (dict(LIN, adaptive=1, lin_families=3), decision("ONE_ROW", "one_row:adaptive", 0, lin=3, refusal=2)),
                (dict(wide, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 0, lin=1, refusal=2)),
                (dict(LIN, adaptive=1, lin_kmax=0, planes_fit=0), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=1, lin_families=3, lin_kmax=0, planes_fit=0), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=1, force_general=1), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(wide, adaptive=1, no_jit=1), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(wide, adaptive=1, variant_jit_failed=1), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=1, debug=1, variant_jit_failed=1), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=1, entry_klin=0, variant_jit_failed=1), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=1, has_tile=1, tile_lin=1, prefer_tile=1), decision("ONE_ROW", "one_row:adaptive", 0, lin=1, refusal=2)),
                (dict(LIN, adaptive=1, lin_families=0, lin_kmax=0, planes_fit=0, pl_planes_fit=0, entry_klin=0), decision("ONE_ROW", "one_row:adaptive", 0)),
                (dict(LIN, adaptive=0, lin_kmax=0, planes_fit=0), decision("COVERAGE", "cover:too_many_halfspaces", 2)),
                (dict(TILE_ONLY, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 3, refusal=4)),
                (dict(TILE_ONLY, adaptive=1, lin_families=1, lin_kmax=4, tile_lin=1), decision("ONE_ROW", "one_row:adaptive", 3, refusal=4))])


def test_rule_05_tile_kernel_for_a_shape_without_a_register_form(ask):
    """Rule 5, and every term of `the tile kernel can run this launch` as its sole offender: the next rule that answers is the last but
    two, `no register form`.  A compiled-in entry counts as a register form even under no_jit."""
    tile = decision("TILE", "tile:no_register_form", 1)
    cover = decision("COVERAGE", "cover:no_register_form", 2)
    halfspaces = dict(TILE_ONLY, lin_families=2, lin_kmax=8, tile_lin=1)
    check(ask, [(TILE_ONLY, tile), (dict(TILE_ONLY, tile_is_jit=1), decision("TILE", "tile:no_register_form", 4)),
                (dict(TILE_ONLY, no_jit=1), tile), (dict(TILE_ONLY, tile_soc_failed=1), tile), (dict(TILE_ONLY, variant_jit_failed=1, jit_failed=1), tile),
                (dict(TILE_ONLY, soc=1), tile), (dict(TILE_ONLY, hetero=1), tile), (dict(TILE_ONLY, tile_ext=1), tile), (halfspaces, tile),
                (dict(TILE_ONLY, fits_box=1, fits=1, no_jit=1), tile), (dict(TILE_ONLY, fits_box=1, fits=1, jit_failed=1), tile),
                (dict(TILE_ONLY, has_tile=0), cover), (dict(TILE_ONLY, no_tile=1), cover), (dict(TILE_ONLY, force_general=1), cover), (dict(TILE_ONLY, debug=1), cover),
                (dict(halfspaces, tile_lin=0), cover), (dict(halfspaces, no_jit=1), cover), (dict(halfspaces, tile_soc_failed=1), cover)] +
          [(dict(TILE_ONLY, **{need: 1, off: 1}), cover if need != "hetero" else decision("COVERAGE", "cover:per_instance_data", 2))
           for need in ("tile_is_jit", "soc", "hetero", "tile_ext") for off in ("no_jit", "tile_soc_failed")] +
          [(dict(TILE_ONLY, has_entry=1, entry_plain=1, no_jit=1), PLAIN_ANSWER)])


def test_rule_06_prefer_tile(ask):
    """Rule 6: a shape both kernels hold goes to the tile kernel on request -- but the EXT forms are for the shapes the one-row kernel does
    not hold."""
    base = dict(FULL, has_tile=1, prefer_tile=1)
    check(ask, [(base, decision("TILE", "tile:prefer_tile", 1)), (dict(base, prefer_tile=0), PLAIN_ANSWER), (dict(base, no_tile=1), PLAIN_ANSWER),
                (dict(base, debug=1), PLAIN_ANSWER), (dict(base, tile_ext=1), PLAIN_ANSWER), (dict(base, soc=1, no_jit=1), PLAIN_ANSWER),
                (dict(base, soc=1, tile_soc_failed=1), PLAIN_ANSWER), (dict(base, soc=1), decision("TILE", "tile:prefer_tile", 1)),
                (dict(base, hetero=1), decision("ONE_ROW", "one_row:per_instance_data", 0)),
                (dict(base, force_general=1), decision("COVERAGE", "cover:force_general", 2))])


def test_rules_07_08_halfspaces_the_one_row_kernel_cannot_hold_go_to_the_tile_kernel(ask):
    """Rules 7 and 8: no one-row variant, or one whose slack planes do not fit a wave's LDS -- only with force_general off (it stands in
    `the tile kernel can run this launch`), and only where the tile kernel's own variant exists."""
    base = dict(LIN, lin_kmax=8, has_tile=1, tile_lin=1)
    one_row = decision("ONE_ROW", "one_row:halfspaces", 0, lin=1)
    check(ask, [(base, one_row),
                (dict(base, variant_jit_failed=1), decision("TILE", "tile:no_one_row_halfspace_variant", 1)),
                (dict(base, variant_jit_failed=1, tile_lin=0), decision("COVERAGE", "cover:wide_halfspaces_without_hiprtc", 2)),
                (dict(base, planes_fit=0), decision("TILE", "tile:planes_do_not_fit_one_row", 1)),
                (dict(base, planes_fit=0, has_tile=0, tile_lin=0), one_row),
                (dict(base, planes_fit=0, tile_lin=0), one_row),
                (dict(base, planes_fit=0, no_tile=1), one_row),
                (dict(base, planes_fit=0, force_general=1), decision("COVERAGE", "cover:force_general", 2)),
                (dict(base, planes_fit=0, no_jit=1), decision("COVERAGE", "cover:wide_halfspaces_without_hiprtc", 2))])


def test_rule_09_shared_halfspaces_why_the_one_row_kernel_has_no_variant(ask):
    """Rule 9 and the ordered list of reasons behind it, each as the sole offender; with none the one-row kernel takes lin_families."""
    one_row = decision("ONE_ROW", "one_row:halfspaces", 0, lin=1)

    def cover(why):
        return decision("COVERAGE", "cover:" + why, 2)
    lean = dict(LIN, entry_klin=0, variant_jit_failed=1)
    check(ask, [(LIN, one_row), (dict(LIN, lin_families=3), decision("ONE_ROW", "one_row:halfspaces", 0, lin=3)),
                (dict(lin_families=1, lin_kmax=4, planes_fit=1), cover("no_register_form")),
                (dict(LIN, force_general=1), cover("force_general")),
                (dict(LIN, force_general=1, lin_kmax=0, planes_fit=0), cover("force_general")),
                (dict(LIN, debug=1), one_row), (dict(LIN, variant_jit_failed=1), one_row),
                (dict(LIN, debug=1, variant_jit_failed=1), cover("halfspaces_debug_without_hiprtc")),
                (dict(LIN, debug=1, variant_jit_failed=1, lin_kmax=0, planes_fit=0), cover("halfspaces_debug_without_hiprtc")),
                (dict(LIN, lin_kmax=0, planes_fit=0), cover("too_many_halfspaces")),
                (dict(LIN, lin_kmax=0, planes_fit=0, no_jit=1), cover("too_many_halfspaces")),
                (dict(LIN, no_jit=1), one_row)] +
          [(dict(LIN, lin_kmax=km), one_row) for km in (8, 16, 32)] +
          [(dict(LIN, lin_kmax=km, **{off: 1}), cover("wide_halfspaces_without_hiprtc")) for km in (8, 16, 32) for off in ("no_jit", "variant_jit_failed")] +
          [(dict(LIN, lin_kmax=8, jit_failed=1), one_row),
           (lean, cover("lean_halfspaces_without_hiprtc")), (dict(lean, variant_jit_failed=0), one_row), (dict(lean, hetero=1), one_row),
           (dict(lean, has_entry=0, entry_plain=0), decision("ONE_ROW", "one_row:halfspaces", 3, lin=1)),
           (dict(lean, lin_kmax=8), cover("wide_halfspaces_without_hiprtc"))])


def test_rules_10_11_per_instance_data_stands_in_front_of_the_lean_shape_rule(ask):
    """Rule 10 (per-instance problem data) and rule 11 (a variant outside a LEAN shape's compiled-in set that could not be instantiated)."""
    lean_missing = dict(FULL, entry_plain=0, variant_jit_failed=1)
    check(ask, [(dict(FULL, hetero=1), decision("ONE_ROW", "one_row:per_instance_data", 0)),
                (dict(JIT, hetero=1), decision("ONE_ROW", "one_row:per_instance_data", 3)),
                (dict(FULL, hetero=1, force_general=1), decision("COVERAGE", "cover:per_instance_data", 2)),
                (dict(FULL, hetero=1, variant_jit_failed=1), decision("COVERAGE", "cover:per_instance_data", 2)),
                (dict(hetero=1), decision("COVERAGE", "cover:per_instance_data", 2)),
                (dict(lean_missing, hetero=1), decision("COVERAGE", "cover:per_instance_data", 2)),
                (lean_missing, decision("COVERAGE", "cover:lean_variant_without_hiprtc", 2)),
                (dict(lean_missing, variant_jit_failed=0), PLAIN_ANSWER), (dict(lean_missing, entry_plain=1), PLAIN_ANSWER),
                (dict(lean_missing, has_entry=0), decision("ONE_ROW", "one_row:plain", 3)),
                (dict(lean_missing, force_general=1), decision("COVERAGE", "cover:lean_variant_without_hiprtc", 2))])


def test_rules_12_13_no_register_form_force_general_and_the_plain_launch(ask):
    """Rules 12 to 14: without a register form, or with force_general, the coverage kernel; else the one-row kernel's plain launch."""
    cover = decision("COVERAGE", "cover:no_register_form", 2)
    check(ask, [({}, cover), (dict(JIT, no_jit=1), cover), (dict(JIT, jit_failed=1), cover), (dict(fits_box=1, soc=1), cover),
                (dict(JIT, force_general=1), decision("COVERAGE", "cover:force_general", 2)), (dict(no_jit=1, force_general=1), cover),
                (dict(FULL, force_general=1), decision("COVERAGE", "cover:force_general", 2)),
                (JIT, decision("ONE_ROW", "one_row:plain", 3)), (dict(JIT, variant_jit_failed=1), decision("ONE_ROW", "one_row:plain", 3)),
                (FULL, PLAIN_ANSWER), (dict(FULL, soc=1, fits=0), PLAIN_ANSWER), (dict(FULL, no_jit=1, jit_failed=1, debug=1, tile_ext=1), PLAIN_ANSWER)])


# the texts as launch_solve and build_one_row_launch reported them before the table existed (callers and tests read tiny_batch_last_error)
MESSAGES = ["",
            "adaptive rho does not combine with per-instance bounds (tiny_batch_set_instance_bounds): a per-instance box with a moving cache would need the coverage "
            "kernel, which does not take adaptive rho",
            "adaptive rho does not combine with heterogeneous data / half-spaces / one_shot / repack_after",
            "overlapping cones run on the coverage kernel: no adaptive rho with them",
            "adaptive rho needs the register-resident kernel (nx+nu <= 16, horizon within the register file)",
            # ... and the eight that came with the per-instance cone coefficients and the closed-loop stages, indexed by their refusal
            "adaptive rho does not combine with per-instance cone coefficients (tiny_batch_set_instance_cone_coefficients): the adaptive cone form has no per-instance "
            "coefficients, and the coverage kernel does not take adaptive rho",
            "adaptive rho does not combine with a per-instance disturbance",
            "adaptive rho does not combine with a plant of its own at the plant step (tiny_batch_set_plant)",
            "adaptive rho does not combine with the state log (option state_log)",
            "adaptive rho does not combine with measurement noise (tiny_batch_set_measurement_noise)",
            "adaptive rho does not combine with a state estimator (tiny_batch_set_estimator)",
            "adaptive rho does not combine with a closed-loop score (tiny_batch_set_score)",
            "adaptive rho does not combine with an actuator model (tiny_batch_set_actuator)"]


def test_refusals_in_their_order_and_their_messages(driver, ask):
    """What adaptive rho does not combine with: a per-instance box (1), per-instance half-spaces (2), overlapping cones (3), no register form
    (4), shared half-spaces that are on (2 again, LAST: every combination one of the four in front refuses keeps that text), reported in
    that order; nothing is refused without adaptive rho.  The kernel and the path code are answered all the same: a per-instance box
    can answer 2 (or 3), per-instance half-spaces answer 3."""
    out = subprocess.run([driver, "messages"], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert out == ["%d %s" % (i, m) if m else "%d " % i for i, m in enumerate(MESSAGES)]
    everything = dict(LIN, soc=1, cones_overlap=1, inst_bounds=1, inst_lin=1, adaptive=1)
    check(ask, [(everything, decision("COVERAGE", "cones_overlap", 2, refusal=1)),
                (dict(everything, inst_bounds=0), decision("COVERAGE", "cones_overlap", 2, refusal=2)),
                (dict(everything, inst_bounds=0, inst_lin=0), decision("COVERAGE", "cones_overlap", 2, refusal=3)),
                (dict(soc=1, cones_overlap=1, adaptive=1), decision("COVERAGE", "cones_overlap", 2, refusal=3)),
                (dict(adaptive=1), decision("ONE_ROW", "one_row:adaptive", 3, refusal=4)),
                (dict(JIT, adaptive=1, no_jit=1), decision("ONE_ROW", "one_row:adaptive", 3, refusal=4)),
                (dict(FULL, adaptive=1, no_jit=1), decision("ONE_ROW", "one_row:adaptive", 0)),
                (dict(JIT, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 3)),
                (dict(everything, adaptive=0), decision("COVERAGE", "cones_overlap", 2)),
                (dict(JIT, inst_bounds=1, adaptive=1), decision("ONE_ROW", "one_row:pb", 3, pb=1, refusal=1)),
                (dict(JIT, soc=1, inst_bounds=1, adaptive=1), decision("COVERAGE", "cover:pb", 2, refusal=1)),
                (dict(LIN, inst_lin=1, adaptive=1), decision("ONE_ROW", "one_row:pl_adaptive", 3, lin=1, pl=1, refusal=2)),
                (dict(LIN, inst_lin=1, adaptive=1, force_general=1), decision("ONE_ROW", "one_row:pl_adaptive", 3, refusal=2)),
                # shared half-spaces behind each of the four: the text in front stays
                (dict(LIN, inst_bounds=1, adaptive=1), decision("COVERAGE", "cover:pb", 2, refusal=1)),
                (dict(LIN, soc=1, cones_overlap=1, adaptive=1), decision("COVERAGE", "cones_overlap", 2, refusal=3)),
                (dict(lin_families=1, lin_kmax=4, planes_fit=1, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 3, refusal=4)),
                (dict(JIT, lin_families=1, lin_kmax=4, planes_fit=1, adaptive=1, no_jit=1), decision("ONE_ROW", "one_row:adaptive", 3, refusal=4)),
                # ... and alone: with a variant, and in the three cases without one
                (dict(LIN, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 0, lin=1, refusal=2)),
                (dict(JIT, lin_families=2, lin_kmax=16, planes_fit=1, adaptive=1), decision("ONE_ROW", "one_row:adaptive", 3, lin=2, refusal=2)),
                (dict(LIN, adaptive=1, lin_kmax=0, planes_fit=0), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=1, force_general=1), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=1, lin_kmax=8, no_jit=1), decision("ONE_ROW", "one_row:adaptive", 0, refusal=2)),
                (dict(LIN, adaptive=0, lin_kmax=8, no_jit=1), decision("COVERAGE", "cover:wide_halfspaces_without_hiprtc", 2))])


def test_the_five_path_codes(ask):
    """tiny_batch_kernel_path: 0 one-row compiled in, 1 tile, 2 coverage, 3 one-row instantiated at run time -- every per-instance box or
    half-space form is, on a compiled-in shape too --, 4 tile instantiated at run time."""
    got = ask(FULL, dict(FULL, has_tile=1, prefer_tile=1), {}, JIT, dict(FULL, inst_bounds=1), dict(LIN, inst_lin=1), dict(TILE_ONLY, tile_is_jit=1),
              dict(FULL, has_tile=1, tile_is_jit=1))
    assert [g["code"] for g in got] == [0, 1, 2, 3, 3, 3, 4, 0]


# ---- the sweep: the ordered rule list restated over arrays, one element per consistent combination of facts
FREE = ("hetero", "tile_ext", "adaptive", "debug", "inst_bounds", "force_general", "no_jit", "no_tile", "prefer_tile", "jit_failed", "variant_jit_failed", "tile_soc_failed")
# The whole consistent space has 113 million elements: each sweep fixes five of the twelve facts that no consistency rule names -- together
# the two let every fact vary, against every value of all the facts the consistency rules tie together
SLICES = [dict(tile_ext=0, no_tile=0, prefer_tile=0, jit_failed=0, tile_soc_failed=0),
          dict(adaptive=0, debug=0, inst_bounds=0, force_general=0, variant_jit_failed=0)]


def consistent_space(fixed):
    """dict fact -> array, broadcastable to (tied facts, free facts): facts_consistent restated"""
    tied = []
    for lf, il, km, planes, plp in itertools.product(range(4), range(4), (0, 4, 8, 16, 32), (0, 1), (0, 1)):
        if il & ~lf or (km and not lf) or (planes and not km) or (plp and not lf):
            continue
        for entry, plain, klin in itertools.product((0, 1), repeat=3):
            if (plain and not entry) or (klin and not (entry and lf)):
                continue
            for tile, tjit, tlin in itertools.product((0, 1), repeat=3):
                if (tjit and not tile) or (tlin and not (tile and km)):
                    continue
                for soc, fb, fits, overlap in itertools.product((0, 1), repeat=4):
                    if (fits and not fb) or (not soc and fits != fb) or (overlap and not soc):
                        continue
                    tied.append((lf, il, km, planes, plp, entry, plain, klin, tile, tjit, tlin, soc, fb, fits, overlap))
    tied = np.array(tied, dtype=np.int8)
    names = "lin_families inst_lin lin_kmax planes_fit pl_planes_fit has_entry entry_plain entry_klin has_tile tile_is_jit tile_lin soc fits_box fits cones_overlap".split()
    f = {n: tied[:, i][:, None] for i, n in enumerate(names)}
    free = [n for n in FREE if n not in fixed]
    grid = np.array(list(itertools.product((0, 1), repeat=len(free))), dtype=np.int8)
    for i, n in enumerate(free):
        f[n] = grid[:, i][None, :]
    for n, v in fixed.items():
        f[n] = np.int8(v)
    return f, (len(tied), len(grid))


def restated_rules(f, shape):
    """-> per element the index of the rule that decides; the rules' names and kernels; per element lin, pl, pb, refusal, code"""
    B = {k: np.asarray(v) != 0 for k, v in f.items()}
    lf = np.asarray(f["lin_families"]).astype(np.int64)
    km = np.asarray(f["lin_kmax"])
    il = np.asarray(f["inst_lin"]) != 0
    regs = B["has_entry"] | (~B["no_jit"] & ~B["jit_failed"] & B["fits"])
    hiprtc = ~B["no_jit"] & ~B["jit_failed"] & ~B["variant_jit_failed"]
    lin_on = lf != 0
    gaps = [("cover:no_register_form", ~regs), ("cover:force_general", B["force_general"]), ("cover:halfspaces_debug_without_hiprtc", B["variant_jit_failed"] & B["debug"]),
            ("cover:too_many_halfspaces", km == 0), ("cover:wide_halfspaces_without_hiprtc", (km > 4) & (B["no_jit"] | B["variant_jit_failed"])),
            ("cover:lean_halfspaces_without_hiprtc", B["variant_jit_failed"] & B["has_entry"] & ~B["hetero"] & ~B["entry_klin"])]
    no_lin = lin_on & np.logical_or.reduce([np.broadcast_to(g, shape) for _, g in gaps])
    ext = B["tile_ext"] | B["hetero"]
    tile_can = (B["has_tile"] & ~B["no_tile"] & ~B["force_general"] & ~B["debug"] & ~(lin_on & ~B["tile_lin"]) &
                ~((B["tile_is_jit"] | B["soc"] | lin_on | ext) & (B["no_jit"] | B["tile_soc_failed"])) & ~(ext & regs))
    pb_form = B["fits_box"] & ~B["soc"] & ~lin_on & ~B["debug"] & ~B["force_general"] & hiprtc
    pl_form = B["fits"] & ~B["debug"] & ~B["force_general"] & hiprtc & B["pl_planes_fit"]
    ONE, TILE, COVER = "ONE_ROW", "TILE", "COVERAGE"
    rules = [(B["cones_overlap"], COVER, "cones_overlap"),
             (B["inst_bounds"] & pb_form, ONE, "one_row:pb"), (B["inst_bounds"], COVER, "cover:pb"),
             (il & B["adaptive"], ONE, "one_row:pl_adaptive"), (il & pl_form, ONE, "one_row:pl"), (il, COVER, "cover:pl"),
             (B["adaptive"], ONE, "one_row:adaptive"),
             (tile_can & ~regs, TILE, "tile:no_register_form"), (tile_can & B["prefer_tile"], TILE, "tile:prefer_tile"),
             (tile_can & no_lin, TILE, "tile:no_one_row_halfspace_variant"), (tile_can & lin_on & ~B["planes_fit"], TILE, "tile:planes_do_not_fit_one_row"),
             (lin_on & ~no_lin, ONE, "one_row:halfspaces")] + [(lin_on & g, COVER, name) for name, g in gaps] + \
            [(B["hetero"] & (B["force_general"] | ~regs | B["variant_jit_failed"]), COVER, "cover:per_instance_data"), (B["hetero"], ONE, "one_row:per_instance_data"),
             (B["variant_jit_failed"] & B["has_entry"] & ~B["entry_plain"], COVER, "cover:lean_variant_without_hiprtc"),
             (~regs, COVER, "cover:no_register_form"), (B["force_general"], COVER, "cover:force_general"),
             (np.ones((), bool), ONE, "one_row:plain")]
    which = np.select([np.broadcast_to(c, shape) for c, _, _ in rules], range(len(rules)))
    name = [r[2] for r in rules]
    kernel = np.array([(ONE, TILE, COVER).index(r[1]) for r in rules])[which]
    takes_lin = np.array([n in ("one_row:halfspaces", "one_row:pl") for n in name])[which] | \
        (np.array([n == "one_row:adaptive" for n in name])[which] & ~no_lin) | (np.array([n == "one_row:pl_adaptive" for n in name])[which] & pl_form)
    lin = np.where(takes_lin, lf, 0)
    pl = np.array([n.startswith("one_row:pl") for n in name])[which] & (lin != 0)
    pb = np.array([n == "one_row:pb" for n in name])[which]
    refusal = np.select([np.broadcast_to(c, shape) for c in (~B["adaptive"], B["inst_bounds"], il, B["cones_overlap"], ~regs, lin_on)], [0, 1, 2, 3, 4, 2], 0)
    code = np.where(kernel == 1, np.where(B["tile_is_jit"], 4, 1), np.where(kernel == 2, 2, np.where(B["has_entry"] & ~B["inst_bounds"] & ~il, 0, 3)))
    return which, name, [r[1] for r in rules], lin, pl, pb, refusal, code


@pytest.mark.parametrize("fixed", SLICES, ids=lambda s: "+".join(s))
def test_sweep_every_consistent_combination_counts_agree(driver, fixed):
    f, shape = consistent_space(fixed)
    which, name, kernel_of, lin, pl, pb, refusal, code = restated_rules(f, shape)
    assert shape[0] == 3449 * 8 and shape[1] == 128          # (3449 tied half-space / entry / tile combinations x 8 of cone and fit)
    key = ((((which * 4 + lin) * 2 + pl) * 2 + pb) * 5 + refusal) * 5 + code
    keys, counts = np.unique(key, return_counts=True)
    want = {}
    for k, c in zip(keys.tolist(), counts.tolist()):
        k, cd = divmod(k, 5)
        k, rf = divmod(k, 5)
        k, b = divmod(k, 2)
        k, p = divmod(k, 2)
        w, ln = divmod(k, 4)
        want[(kernel_of[w], ln, p, b, rf, name[w], cd)] = want.get((kernel_of[w], ln, p, b, rf, name[w], cd), 0) + c      # (two rules share a name with a reason of rule 9)
    out = subprocess.run([driver, "sweep"] + ["%s=%d" % kv for kv in fixed.items()], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[-1] == "total=%d" % (shape[0] * shape[1])
    have = {}
    for ln in out[:-1]:
        r = words(ln)
        have[(r["kernel"], r["lin"], r["pl"], r["pb"], r["refusal"], r["rule"], r["code"])] = r["count"]
    assert have == want
