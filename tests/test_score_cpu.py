"""CPU: the per-instance closed-loop score at the plant step (tiny_batch_set_score), as far as it can be checked without a GPU -- the
exported entry points, their ctypes mirror and their NULL returns; the reference's arithmetic; the visibility conditions of every case
the GPU tests use, from the reference and the oracle loops alone; score_entry against a dense restatement; the path and variant rules
(tests/dropin/score_path_driver.cpp) and the refusal's text and position; the argument block's fixed layout; that the PS forms of the
one-row kernel (run-time instantiated only) compile for gfx950 and that names with ADAPT, HALF, PF or without a PD / PP bit are refused
by name; and that the bit adds nothing to the iteration loop."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plant_cases as pc
import score_cases as scs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

NEW_SYMBOLS = ("tiny_batch_set_score", "tiny_batch_get_score_setup", "tiny_batch_get_score", "tiny_batch_reset_score", "tiny_group_set_score")
PD, PP, PM, PE, PS = 32, 64, 128, 256, 512         # bits 5 .. 9 of the kernel's MODE argument


def ps_name(nx, nu, N, soc=False, mode=2, lin=0, het=False, kmax=4, adapt=False, ub=False, half=False, pf=False):
    b = lambda v: "true" if v else "false"
    tail = ", %s, %s, %s" % (b(ub), b(half), b(pf)) if (half or pf) else (", true" if ub else "")
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, %d, %s, %d, %s%s>" % (nx, nu, N, b(soc), mode, lin, b(het), kmax, b(adapt), tail)


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_set_score(None, None, None, None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_score_setup(None, 0, None, None, None, None) == tm.ERR_NULL
    assert L.tiny_batch_get_score(None, None, None, None, None) == tm.ERR_NULL
    assert L.tiny_batch_reset_score(None) == tm.ERR_NULL
    assert L.tiny_group_set_score(None, None, None, None, None, tm.HOST) == tm.ERR_NULL
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        for name in ("set_score", "set_score_device", "get_score", "reset_score"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(tm.TinyBatchSolver.get_score_setup)
    for word in ("z = [xn | u0]", "three separate", "ONE running sum", "score_step", "last_score", "first_violation = k", "Out of scope: a moving target",
                 "adaptive rho does not combine with a closed-loop score"):
        assert word in header, word


def test_the_reference_rounds_three_times_per_term_in_ascending_order():
    one = lambda z, w, tg=None, lo=None, hi=None, **how: scs.score_step(scs.ZERO, np.array(z, dtype=float), (np.array(w, dtype=float), tg, lo, hi), 3, **how)
    # d, w * d and (w * d) * d are each rounded: (1 + 2^-30)^2 loses its last bit, and the sum is not one fma
    x = 1.0 + 2.0 ** -30
    assert one([x], [1.0])[0] == x * x
    a = one([1.0, x], [-1.0, 1.0])[0]                                        # (-1 + x^2: the bit the product dropped would survive the fused addition)
    assert a == -1.0 + x * x == 2.0 ** -29 and one([1.0, x], [-1.0, 1.0], fused=True)[0] == 2.0 ** -29 + 2.0 ** -60
    # ascending order: 2^53 + 1 + 1 stays 2^53 from the left and moves from the right
    big = [2.0 ** 53, 1.0, 1.0]
    assert one([1.0] * 3, big)[0] == 2.0 ** 53 and one([1.0] * 3, big, order=(2, 1, 0))[0] == 2.0 ** 53 + 2.0
    # the violation: the larger side, never negative; the counter's value where the first one falls; no limits: nothing
    z = np.array([1.0, -2.0, 0.5])
    r = one(z, [1.0] * 3, lo=np.array([-1.0, -1.5, 0.0]), hi=np.array([0.75, 0.0, 1.0]))
    assert r[1:] == (0.5, 1, 3)
    assert one(z, [1.0] * 3)[1:] == (0.0, 0, -1) and one(z, [1.0] * 3, lo=z - 1.0, hi=z + 1.0)[1:] == (0.0, 0, -1)
    # over steps: the record accumulates, a step that took no plant step is skipped and still counted
    xs, us = np.array([[1.0], [3.0], [0.0]]), np.array([[0.0], [0.0], [0.0]])
    s = (np.array([1.0, 1.0]), None, None, np.array([2.0, 1.0]))
    assert scs.score_reference(xs, us, s) == (10.0, 1.0, 1, 1)
    assert scs.score_reference(xs, us, s, k0=7) == (10.0, 1.0, 1, 8)
    assert scs.score_reference(xs, us, s, scored=[True, False, True]) == (1.0, 0.0, 0, -1)
    assert scs.score_reference(xs[2:], us[2:], s, k0=2, rec=scs.score_reference(xs[:2], us[:2], s)) == scs.score_reference(xs, us, s)


@pytest.mark.parametrize("name", scs.ALL_CASES)
def test_the_cases_of_the_gpu_tests_meet_their_conditions(name):
    scs.check_case(name)
    assert scs.T == 5
    assert [(pc.CASES[n]["shape"], pc.CASES[n]["B"]) for n in scs.ORACLE_CASES] == [((4, 2, 10), 13), ((5, 3, 7), 11), ((12, 4, 10), 2)]
    assert [pc.CASES[n]["shape"] for n in scs.EDGE_CASES] == [(15, 1, 3), (1, 15, 3)]
    assert pc.CASES[scs.COMPOSE_CASE]["shape"] == (6, 3, 10) and pc.CASES[scs.COVER_CASE]["shape"] == (20, 8, 10)


# ---- score_entry --------------------------------------------------------------------------------------------------------------------------
def test_score_entry_against_a_dense_restatement(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    prog = ('#include <hip/hip_runtime.h>\n#include <cstdio>\n#include <vector>\n#include "%s"\nusing namespace tinympc_amd;\n'
            'int main() { if (score_block_doubles() != 64) return 1;\n'
            ' for (int nx : {1, 5, 12, 15}) for (int nu : {1, 3, 4, 15}) { if (nx + nu > 16) continue; const int nz = nx + nu;\n'
            '  std::vector<double> a(4 * nz); for (int i = 0; i < 4 * nz; ++i) a[i] = 1000.0 * nx + 100.0 * nu + i + 0.5;\n'
            '  for (int given = 0; given < 8; ++given) for (int r = 0; r < 4; ++r) for (int lane = 0; lane < 16; ++lane)\n'
            '   printf("%%d %%d %%d %%d %%d %%.17g\\n", nx, nu, given, r, lane, score_entry(a.data(), (given & 1) ? a.data() + nz : nullptr, (given & 2) ? a.data() + 2 * nz : nullptr,\n'
            '          (given & 4) ? a.data() + 3 * nz : nullptr, nx, nu, r, lane)); }\n'
            '  return 0; }\n' % os.path.join(CSRC, "lane_tables.hpp"))
    exe, cpp = str(tmp_path / "score"), tmp_path / "score.cpp"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, "-x", "hip", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    rows = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()]
    shapes = [(nx, nu) for nx in (1, 5, 12, 15) for nu in (1, 3, 4, 15) if nx + nu <= 16]
    assert len(rows) == len(shapes) * 8 * 4 * 16 and (15, 1) in shapes and (1, 15) in shapes
    outside = (0.0, 0.0, -np.inf, np.inf)
    for nx, nu, given, r, lane, val in rows:
        nx, nu, given, r, lane, val = int(nx), int(nu), int(given), int(r), int(lane), float(val)
        nz = nx + nu
        dense = (1000.0 * nx + 100.0 * nu + np.arange(4 * nz) + 0.5).reshape(4, nz)    # weight | target | lo | hi over z = [x | u], as given
        have = r == 0 or (given >> (r - 1)) & 1
        assert val == (dense[r, lane] if (lane < nz and have) else outside[r]), (nx, nu, given, r, lane, val)


# ---- the path and the variant choice ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("score_path") / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "dropin", "score_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _lines(exe, mode, stdin=None):
    out = subprocess.run([exe, mode], input=stdin, check=True, capture_output=True, text=True, timeout=1800).stdout.splitlines()
    return [dict(w.split("=", 1) for w in ln.split()) for ln in out]


BOX = dict(fits_box=1, fits=1, score=1)
CONE = dict(BOX, soc=1)
LIN = dict(BOX, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1)


def test_path_rules_under_a_score(driver):
    # facts -> (kernel, rule, (lin, pl, pb, pc, pd, pp, pm, pe, ps), path code, refusal)
    cases = [
        (BOX, ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),                                     # nothing else installed: the PD form, empty sequence
        (dict(BOX, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),  # a compiled-in entry is not asked
        (CONE, ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (LIN, ("ONE_ROW", "one_row:ps", (1, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, hetero=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, state_log=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, disturbance=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, plant=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 0, 1, 0, 0, 1), 3, 0)),                       # with a plant: the PP form, no empty sequence
        (dict(BOX, plant=1, disturbance=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 1, 0, 0, 1), 3, 0)),
        (dict(BOX, measurement=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 0, 1, 1, 0, 1), 3, 0)),
        (dict(BOX, estimator=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 0, 1, 1, 1, 1), 3, 0)),
        (dict(BOX, estimator=1, measurement=1, plant=1, disturbance=1, state_log=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 1, 1, 1, 1), 3, 0)),
        # composition with the per-instance rules: their forms take the bits and keep their rule
        (dict(BOX, inst_bounds=1), ("ONE_ROW", "one_row:pb", (0, 0, 1, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(LIN, inst_lin=1), ("ONE_ROW", "one_row:pl", (1, 1, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(CONE, inst_cones=1), ("ONE_ROW", "one_row:pc", (0, 0, 0, 1, 1, 0, 0, 0, 1), 3, 0)),
        # ... and a coverage answer stays coverage; where no PS form can be made: cover:ps
        (dict(CONE, cones_overlap=1), ("COVERAGE", "cones_overlap", (0,) * 9, 2, 0)),
        (dict(BOX, force_general=1), ("COVERAGE", "cover:force_general", (0,) * 9, 2, 0)),
        (dict(BOX, debug=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 0)),
        (dict(BOX, no_jit=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 0)),
        (dict(BOX, variant_jit_failed=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 0)),
        # never the tile kernel while the fact is on: its shapes run on the coverage kernel
        (dict(score=1, has_tile=1), ("COVERAGE", "cover:no_register_form", (0,) * 9, 2, 0)),
        (dict(BOX, has_tile=1, prefer_tile=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(has_tile=1), ("TILE", "tile:no_register_form", (0,) * 9, 1, 0)),
        # adaptive rho: refused with the fact's own value, reported last; what was refused before keeps its value
        (dict(BOX, adaptive=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 11)),
        (dict(BOX, adaptive=1, estimator=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 10)),
        (dict(BOX, adaptive=1, measurement=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 9)),
        (dict(BOX, adaptive=1, state_log=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 8)),
        (dict(BOX, adaptive=1, plant=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 7)),
        (dict(BOX, adaptive=1, disturbance=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 6)),
        (dict(BOX, adaptive=1, inst_bounds=1), ("COVERAGE", "cover:ps", (0,) * 9, 2, 1)),
        # the fact off: the answers without the feature
        (dict(fits_box=1, fits=1), ("ONE_ROW", "one_row:plain", (0,) * 9, 3, 0)),
        (dict(fits_box=1, fits=1, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:plain", (0,) * 9, 0, 0)),
        (dict(fits_box=1, fits=1, adaptive=1), ("ONE_ROW", "one_row:adaptive", (0,) * 9, 3, 0)),
        (dict(fits_box=1, fits=1, estimator=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1, 0), 3, 0)),
        (dict(fits_box=1, fits=1, state_log=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0, 0, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, estimator=1, adaptive=1), ("COVERAGE", "cover:pe", (0,) * 9, 2, 10)),
    ]
    stdin = "".join(" ".join("%s=%d" % kv for kv in f.items()) + "\n" for f, _ in cases)
    got = _lines(driver, "path", stdin)
    assert len(got) == len(cases)
    for (f, (kernel, rule, forms, code, refusal)), g in zip(cases, got):
        assert (g["kernel"], g["rule"], int(g["code"]), int(g["refusal"]), g["consistent"]) == (kernel, rule, code, refusal, "1"), (f, g)
        assert tuple(int(g[k]) for k in ("lin", "pl", "pb", "pc", "pd", "pp", "pm", "pe", "ps")) == forms, (f, g)
    p = subprocess.run([driver, "message"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.splitlines() == [
        "10 adaptive rho does not combine with a state estimator (tiny_batch_set_estimator)",
        "11 adaptive rho does not combine with a closed-loop score (tiny_batch_set_score)"], p.stdout
    # the value behind the estimator's, and with both facts on (or any earlier one) the earlier refusal is answered
    both = _lines(driver, "path", "".join(" ".join("%s=%d" % kv for kv in dict(BOX, adaptive=1, **on).items()) + "\n"
                                          for on in ({}, dict(estimator=1), dict(measurement=1, estimator=1))))
    assert [int(g["refusal"]) for g in both] == [11, 10, 9]


def test_path_and_variant_sweeps_follow_the_state_logs_rule(driver):
    tail = {k: int(v) for r in _lines(driver, "paths") if len(r) == 1 for k, v in r.items()}
    assert tail["violations"] == 0 and tail["tile_with_score"] == 0, tail
    assert min(tail["plain"], tail["with_score"], tail["one_row_ps"], tail["cover_ps"], tail["refused_11"]) > 1000, tail
    tail = {k: int(v) for r in _lines(driver, "variants") if len(r) == 1 for k, v in r.items()}
    assert tail["with_ps"] > 1000 and tail["violations"] == 0 and tail["key_order"] == 1, tail


def test_the_argument_block_keeps_its_size_and_the_new_fields_lie_over_the_adaptive_rho_tables(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    fields = ("arho", "est_gain", "aC1", "est_model", "aC2", "score_tab", "atab", "score_rec", "arho_min", "score_step0", "arho_max", "aclip", "ref_shared", "pf_mask", "meas",
              "pf_counter", "dist", "plant", "state_log")
    prog = ('#include <cstdio>\n#include "%s"\nusing tinympc_amd::SolveArgs;\nint main() { printf("%%zu %%zu", sizeof(SolveArgs), sizeof(tinympc_amd::ScoreRecord));\n%s printf("\\n"); return 0; }\n'
            % (os.path.join(CSRC, "admm_kernel.hip.h"), "".join('printf(" %%zu", __builtin_offsetof(SolveArgs, %s));\n' % f for f in fields)))
    exe, cpp = str(tmp_path / "layout"), tmp_path / "layout.hip"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    words = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(w) for w in words] == [472, 24, 304, 304, 328, 328, 336, 336, 344, 344, 352, 352, 360, 368, 372, 416, 416, 432, 440, 456, 464], words
    text = open(os.path.join(CSRC, "admm_kernel.hip.h")).read()
    assert ('static_assert(sizeof(SolveArgs) == 472 && __builtin_offsetof(SolveArgs, het_tabs) == 208 && __builtin_offsetof(SolveArgs, pf_mask) == 416 &&\n'
            '              __builtin_offsetof(SolveArgs, pf_counter) == 432 && __builtin_offsetof(SolveArgs, pf_base) == 440, "SolveArgs: size and offsets are fixed");') in text
    assert ('static_assert(__builtin_offsetof(SolveArgs, arho) == 304 && __builtin_offsetof(SolveArgs, est_gain) == 304 && __builtin_offsetof(SolveArgs, est_xp) == 312 &&\n'
            '              __builtin_offsetof(SolveArgs, est_log) == 320 && __builtin_offsetof(SolveArgs, est_model) == 328 && __builtin_offsetof(SolveArgs, aC1) == 328 &&\n'
            '              __builtin_offsetof(SolveArgs, aC2) == 336 && __builtin_offsetof(SolveArgs, atab) == 344, "SolveArgs: the estimator\'s pointers share the adaptive-rho ones\' place");') in text
    assert "__builtin_offsetof(SolveArgs, score_tab) == 336" in text and "__builtin_offsetof(SolveArgs, score_step0) == 352" in text


# ---- the PS forms ------------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import tinympc_amd as tm
out = []
for name in sys.argv[2:]:
    try:
        n, hit = tm.jit_compile(name)
        out.append({"name": name, "bytes": n})
    except RuntimeError as e:
        out.append({"name": name, "error": str(e)[:3000]})
print(json.dumps(out))
'''

# the forms the issue names -- the (12,4,10) box (knot-invariant: UB) and the (6,3,10) cone, on the PD form with an empty sequence and
# on the PE form --, (5,3,7), and a per-instance-data form
PLAIN, FULL = 2 | PD | PS, 2 | PD | PP | PM | PE | PS
PS_VARIANTS = [ps_name(12, 4, 10, mode=PLAIN, ub=True), ps_name(6, 3, 10, soc=True, mode=PLAIN), ps_name(12, 4, 10, mode=2 | PP | PM | PE | PS, ub=True),
               ps_name(6, 3, 10, soc=True, mode=FULL), ps_name(5, 3, 7, mode=2 | PP | PS, ub=True), ps_name(12, 4, 10, mode=PLAIN, het=True, ub=True)]


def test_ps_variants_compile_and_names_with_adapt_half_or_pf_are_refused():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    refused = [(ps_name(6, 3, 10, mode=2 | PS), "a closed-loop score: a form that takes its plant step itself (PD, bit 5, or PP, bit 6)"),
               (ps_name(6, 3, 10, mode=PLAIN, adapt=True), "not with adaptive rho"),
               (ps_name(4, 2, 10, mode=PLAIN, half=True), "not the half-row form"),
               (ps_name(12, 4, 10, mode=PLAIN, pf=True), "not the prefetch form")]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PS_VARIANTS + [n for n, _ in refused], capture_output=True, text=True, timeout=3000, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    good, bad = res[:len(PS_VARIANTS)], res[len(PS_VARIANTS):]
    assert [r["name"] for r in good] == PS_VARIANTS
    assert not [r for r in good if "error" in r], [r for r in good if "error" in r]
    assert all(r["bytes"] > 1000 for r in good)
    for r, (_, text) in zip(bad, refused):
        assert "error" in r and text in r["error"], r


BOX_T = ("12", "4", "10", "false", "false", "MODE", "0", "false", "4", "false", "true")
CONE_T = ("6", "3", "10", "true", "false", "MODE")


@pytest.mark.parametrize("targs,base", [(BOX_T, 2 | PD), (CONE_T, 2 | PD), (BOX_T, 2 | PP | PM | PE), (CONE_T, 2 | PP | PM | PE)], ids=["box-pd", "cone-pd", "box-pe", "cone-pe"])
def test_the_bit_adds_nothing_to_the_iteration_loop(targs, base, tmp_path):
    """the assembly hipcc emits for the PS form and for the same form without the bit, through tools/isa_loop_stats.py (the fused column
    blocks, as the library is built): the iteration loop holds no more FP64, LDS, VMEM or scratch instructions, and it is no longer: the
    totals differ by s_nops at the most.  (Seen when this was written: on the forms with nothing else installed and on the box PE form
    the loops are the same but for one s_nop; on the (6,3,10) cone PE form hipcc re-forms `lane & 48`, which the termination probe
    reads, inside the loop in the place of one s_nop 0 -- one VALU instruction for one s_nop, the same number of issue slots.)"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    spec = importlib.util.spec_from_file_location("isa_loop_stats", os.path.join(ROOT, "tools", "isa_loop_stats.py"))
    ils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ils)
    loops = {}
    for mode in (base | PS, base):
        args = list(targs)
        args[5] = str(mode)
        src, out = tmp_path / ("u%d.hip" % mode), str(tmp_path / ("u%d.s" % mode))
        src.write_text("#define TINYMPC_FUSED_NX %s\n#define TINYMPC_FUSED_NU %s\n#include \"%s/kernel_entry.hpp\"\n#include \"%s/tile_kernel.hip.h\"\n"
                       "namespace tinympc_amd { template __global__ void admm_solve_kernel<%s>(const SolveArgs); }\n" % (args[0], args[1], CSRC, CSRC, ", ".join(args)))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", str(src), "-o", out], check=True, capture_output=True, timeout=1200)
        (sym, lines, loop, meta), = ils.analyse(out)
        assert loop, sym
        body = lines[loop[0]:loop[1] + 1]
        count = {}
        for ins in body:
            count[ils.classify(ins)] = count.get(ils.classify(ins), 0) + 1
        loops[mode] = count
        print(mode, len(body), count, meta)
    ps, plain = loops[base | PS], loops[base]
    assert ps.get("scratch", 0) == 0 and plain.get("scratch", 0) == 0, (ps, plain)
    for kind in ("fp64", "lds", "vmem"):
        assert ps.get(kind, 0) <= plain.get(kind, 0), (kind, ps, plain)
    assert sum(ps.values()) <= sum(plain.values()) and sum(plain.values()) - sum(ps.values()) <= plain.get("nop/wait", 0), (ps, plain)
