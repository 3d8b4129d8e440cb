"""CPU: measurement noise at the plant step of a closed loop (tiny_batch_set_measurement_noise), as far as it can be checked without a
GPU -- the exported entry points and their NULL returns; the oracle-side conditions of every case the GPU tests use; the path and variant
rules (tests/dropin/measurement_path_driver.cpp) and the refusal text; the argument block's fixed layout; that the PM forms of the one-row
kernel (run-time instantiated only) compile for gfx950 and that a name without the PP bit or with ADAPT is refused by name."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import measurement_cases as mc
import plant_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

NEW_SYMBOLS = ("tiny_batch_set_measurement_noise", "tiny_batch_get_measurement_noise", "tiny_group_set_measurement_noise")
PD, PP, PM = 32, 64, 128                           # bits 5, 6 and 7 of the kernel's MODE argument


def pm_name(nx, nu, N, soc=False, mode=2, lin=0, het=False, kmax=4, adapt=False, ub=False):
    b = lambda v: "true" if v else "false"
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, %d, %s, %d, %s%s>" % (nx, nu, N, b(soc), mode, lin, b(het), kmax, b(adapt), ", true" if ub else "")


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_set_measurement_noise(None, None, 0, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_measurement_noise(None, 0, 0, None) == tm.ERR_NULL
    assert L.tiny_group_set_measurement_noise(None, None, 0, tm.HOST) == tm.ERR_NULL
    for name in ("set_measurement_noise", "get_measurement_noise", "set_measurement_noise_device"):
        assert callable(getattr(tm.TinyBatchSolver, name)), name
    assert callable(tm.TinyGroupSolver.set_measurement_noise)
    for word in ("TRUE state", "estimator or filter", "measurement_step", "last_measurement_noise"):
        assert word in header, word


@pytest.mark.parametrize("name", mc.ORACLE_CASES)
def test_the_cases_of_the_gpu_tests_meet_their_conditions(name):
    mc.check_case(name)
    c, v = pc.case(name), mc.noise(name)
    assert v.shape == (mc.T, c["B"], c["nx"]) and mc.T == 5
    assert np.all(np.abs(v) >= 0.5 * mc.AMPLITUDE) and np.all(np.abs(v) <= mc.AMPLITUDE) and mc.AMPLITUDE == 0.05
    assert [(pc.CASES[n]["shape"], pc.CASES[n]["B"]) for n in mc.ORACLE_CASES] == [((4, 2, 10), 13), ((5, 3, 7), 11), ((12, 4, 10), 2)]


# ---- the path and the variant choice ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("measurement_path") / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "dropin", "measurement_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _lines(exe, mode, stdin=None):
    out = subprocess.run([exe, mode], input=stdin, check=True, capture_output=True, text=True, timeout=900).stdout.splitlines()
    return [dict(w.split("=", 1) for w in ln.split()) for ln in out]


BOX = dict(fits_box=1, fits=1, measurement=1)
CONE = dict(BOX, soc=1)
LIN = dict(BOX, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1)


def test_path_rules_under_measurement_noise(driver):
    # facts -> (kernel, rule, (lin, pl, pb, pc, pd, pp, pm), path code, refusal)
    cases = [
        (BOX, ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1), 3, 0)),                                           # the fact forces pp on
        (dict(BOX, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1), 3, 0)),        # a compiled-in entry is not asked
        (CONE, ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1), 3, 0)),
        (LIN, ("ONE_ROW", "one_row:pm", (1, 0, 0, 0, 0, 1, 1), 3, 0)),
        (dict(BOX, hetero=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1), 3, 0)),
        (dict(BOX, plant=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1), 3, 0)),                            # with a plant installed: the same form
        (dict(BOX, disturbance=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 1, 1, 1), 3, 0)),                      # with a disturbance: all three bits
        (dict(BOX, plant=1, disturbance=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 1, 1, 1), 3, 0)),
        (dict(BOX, state_log=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1), 3, 0)),                        # the PP form writes the log itself
        # composition with the per-instance rules: their forms take the bits and keep their rule
        (dict(BOX, inst_bounds=1), ("ONE_ROW", "one_row:pb", (0, 0, 1, 0, 0, 1, 1), 3, 0)),
        (dict(LIN, inst_lin=1), ("ONE_ROW", "one_row:pl", (1, 1, 0, 0, 0, 1, 1), 3, 0)),
        (dict(CONE, inst_cones=1), ("ONE_ROW", "one_row:pc", (0, 0, 0, 1, 0, 1, 1), 3, 0)),
        # ... and a coverage answer stays coverage; where no PM form can be made: cover:pm
        (dict(CONE, cones_overlap=1), ("COVERAGE", "cones_overlap", (0, 0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, force_general=1), ("COVERAGE", "cover:force_general", (0, 0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, debug=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, no_jit=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, variant_jit_failed=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 0)),
        # never the tile kernel while the fact is on: its shapes run on the coverage kernel
        (dict(measurement=1, has_tile=1), ("COVERAGE", "cover:no_register_form", (0, 0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, has_tile=1, prefer_tile=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1), 3, 0)),
        (dict(has_tile=1), ("TILE", "tile:no_register_form", (0, 0, 0, 0, 0, 0, 0), 1, 0)),
        # adaptive rho: refused with the fact's own value; what was refused before keeps its value
        (dict(BOX, adaptive=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 9)),
        (dict(BOX, adaptive=1, state_log=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 8)),
        (dict(BOX, adaptive=1, plant=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 7)),
        (dict(BOX, adaptive=1, disturbance=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 6)),
        (dict(BOX, adaptive=1, inst_bounds=1), ("COVERAGE", "cover:pm", (0, 0, 0, 0, 0, 0, 0), 2, 1)),
        # the fact off: the answers without the feature
        (dict(fits_box=1, fits=1), ("ONE_ROW", "one_row:plain", (0, 0, 0, 0, 0, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:plain", (0, 0, 0, 0, 0, 0, 0), 0, 0)),
        (dict(fits_box=1, fits=1, adaptive=1), ("ONE_ROW", "one_row:adaptive", (0, 0, 0, 0, 0, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, disturbance=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, plant=1), ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1, 0), 3, 0)),
        (dict(fits_box=1, fits=1, state_log=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, plant=1, adaptive=1), ("COVERAGE", "cover:pp", (0, 0, 0, 0, 0, 0, 0), 2, 7)),
    ]
    stdin = "".join(" ".join("%s=%d" % kv for kv in f.items()) + "\n" for f, _ in cases)
    got = _lines(driver, "path", stdin)
    assert len(got) == len(cases)
    for (f, (kernel, rule, forms, code, refusal)), g in zip(cases, got):
        assert (g["kernel"], g["rule"], int(g["code"]), int(g["refusal"]), g["consistent"]) == (kernel, rule, code, refusal, "1"), (f, g)
        assert tuple(int(g[k]) for k in ("lin", "pl", "pb", "pc", "pd", "pp", "pm")) == forms, (f, g)
    p = subprocess.run([driver, "message"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.splitlines() == [
        "9 adaptive rho does not combine with measurement noise (tiny_batch_set_measurement_noise)"], p.stdout


def test_path_and_variant_sweeps_follow_the_plants_rule(driver):
    tail = {k: int(v) for r in _lines(driver, "paths") if len(r) == 1 for k, v in r.items()}
    assert tail["violations"] == 0 and tail["tile_with_measurement"] == 0, tail
    assert min(tail["plain"], tail["with_measurement"], tail["one_row_pm"], tail["cover_pm"], tail["refused_9"]) > 1000, tail
    tail = {k: int(v) for r in _lines(driver, "variants") if len(r) == 1 for k, v in r.items()}
    assert tail["with_pm"] > 1000 and tail["violations"] == 0 and tail["key_order"] == 1, tail


def test_the_argument_block_keeps_its_size_and_the_new_fields_lie_over_the_prefetch_forms_ints(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    prog = ('#include <cstdio>\n#include "%s"\nusing tinympc_amd::SolveArgs;\nint main() { printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(SolveArgs), '
            '__builtin_offsetof(SolveArgs, pf_mask), __builtin_offsetof(SolveArgs, meas), __builtin_offsetof(SolveArgs, meas_steps), '
            '__builtin_offsetof(SolveArgs, meas_step0), __builtin_offsetof(SolveArgs, pf_counter), __builtin_offsetof(SolveArgs, dist)); return 0; }\n'
            % os.path.join(CSRC, "admm_kernel.hip.h"))
    exe, cpp = str(tmp_path / "layout"), tmp_path / "layout.hip"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    words = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(w) for w in words] == [472, 416, 416, 424, 428, 432, 440], words
    text = open(os.path.join(CSRC, "admm_kernel.hip.h")).read()
    assert ('static_assert(sizeof(SolveArgs) == 472 && __builtin_offsetof(SolveArgs, het_tabs) == 208 && __builtin_offsetof(SolveArgs, pf_mask) == 416 &&\n'
            '              __builtin_offsetof(SolveArgs, pf_counter) == 432 && __builtin_offsetof(SolveArgs, pf_base) == 440, "SolveArgs: size and offsets are fixed");') in text


# ---- the PM forms ------------------------------------------------------------------------------------------------------------------------
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

# the forms the GPU tests launch: (4,2,10), (5,3,7), (12,4,10) box (knot-invariant: UB), (12,4,10) per-instance data, (6,3,10) with a
# disturbance, with PB, a cone and a half-space variant, dpp_mode 0, the PL and PC forms
BASE = 2 | PP | PM
PM_VARIANTS = [pm_name(4, 2, 10, mode=BASE, ub=True), pm_name(5, 3, 7, mode=BASE, ub=True), pm_name(12, 4, 10, mode=BASE, ub=True),
               pm_name(12, 4, 10, mode=BASE, het=True, ub=True), pm_name(6, 3, 10, mode=BASE | PD, ub=True), pm_name(6, 3, 10, mode=BASE | 4, ub=True),
               pm_name(6, 3, 10, soc=True, mode=BASE), pm_name(6, 3, 10, mode=BASE, lin=1), pm_name(6, 3, 10, mode=0 | PP | PM),
               pm_name(6, 3, 10, mode=BASE | 8, lin=1, kmax=2), pm_name(6, 3, 10, soc=True, mode=BASE | 16)]


def test_pm_variants_compile_and_names_without_pp_or_with_adapt_are_refused():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    refused = [(pm_name(6, 3, 10, mode=2 | PM), "measurement noise: a form with a plant block (PP, bit 6)"),
               (pm_name(6, 3, 10, mode=BASE, adapt=True), "measurement noise: not with adaptive rho")]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PM_VARIANTS + [n for n, _ in refused], capture_output=True, text=True, timeout=3000, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    good, bad = res[:len(PM_VARIANTS)], res[len(PM_VARIANTS):]
    assert [r["name"] for r in good] == PM_VARIANTS
    assert not [r for r in good if "error" in r], [r for r in good if "error" in r]
    assert all(r["bytes"] > 1000 for r in good)
    for r, (_, text) in zip(bad, refused):
        assert "error" in r and text in r["error"], r
