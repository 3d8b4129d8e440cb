"""CPU: a plant model of its own at the plant step (tiny_batch_set_plant) and the state log, as far as they can be checked without a GPU --
the exported entry points and their NULL returns; the reference plant step of tests/plant_cases.py against exact rational arithmetic;
the oracle-side conditions of every case the GPU tests use; the path and variant rules (tests/dropin/plant_path_driver.cpp) and the
refusal texts; the argument block's fixed layout; that the PP forms of the one-row kernel (run-time instantiated only) compile for
gfx950 and that an ADAPT, HALF or PF name carrying the bit is refused by name."""
import json
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

import plant_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

NEW_SYMBOLS = ("tiny_batch_set_plant", "tiny_batch_get_plant", "tiny_batch_get_state_log", "tiny_group_set_plant")
PD, PP = 32, 64                                    # bits 5 and 6 of the kernel's MODE argument


def pp_name(nx, nu, N, soc=False, mode=2, lin=0, het=False, kmax=4, adapt=False, ub=False, tail=""):
    b = lambda v: "true" if v else "false"
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, %d, %s, %d, %s%s%s>" % (nx, nu, N, b(soc), mode, lin, b(het), kmax, b(adapt), ", true" if ub else "", tail)


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_set_plant(None, None, None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_plant(None, 0, None, None, None) == tm.ERR_NULL
    assert L.tiny_batch_get_state_log(None, None, 1) == tm.ERR_NULL
    assert L.tiny_group_set_plant(None, None, None, None, tm.HOST) == tm.ERR_NULL
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        assert callable(cls.set_plant) and callable(cls.get_plant) and callable(cls.state_log)
    assert callable(tm.TinyBatchSolver.set_plant_device)


def test_the_reference_plant_step_is_the_chain_rounded_once_per_term():
    rng = np.random.default_rng(5)
    nx, nu = 5, 3
    A, B, f, x0, u0 = rng.normal(0, 1, (nx, nx)), rng.normal(0, 1, (nx, nu)), rng.normal(0, 1, nx), rng.normal(0, 1, nx), rng.normal(0, 1, nu)
    got = pc.plant_step(A, B, f, x0, u0)
    for j in range(nx):
        acc = Fraction(f[j])
        for k in range(nx):
            acc = Fraction(float(Fraction(x0[k]) * Fraction(A[j, k]) + acc))
        for k in range(nu):
            acc = Fraction(float(Fraction(u0[k]) * Fraction(B[j, k]) + acc))
        assert got[j] == float(acc)
    assert np.allclose(got, f + A @ x0 + B @ u0, rtol=1e-12, atol=1e-14)
    e = 2.0 ** -27                                                   # (1 + e)^2 - 1 = 2e + e^2 exactly; a rounded product loses the e^2
    assert pc.fma(1.0 + e, 1.0 + e, -1.0) == 2.0 ** -26 + 2.0 ** -54 != (1.0 + e) * (1.0 + e) - 1.0
    assert np.array_equal(pc.plant_step(A, B, None, x0, u0), pc.plant_step(A, B, np.zeros(nx), x0, u0))


@pytest.mark.parametrize("name", pc.ORACLE_CASES + pc.EDGE_CASES)
def test_the_cases_of_the_gpu_tests_meet_their_conditions(name):
    pc.check_case(name)
    c = pc.case(name)
    for p, m in zip(c["plant"], c["model"]):
        assert p.shape == m.shape and np.all(p != m)
        assert np.max(np.abs(p - m)) < 0.06 * max(1.0, np.max(np.abs(m)))       # a few percent


def test_the_batches_end_in_tiles_of_one_three_and_two_rows_and_the_shapes_are_the_three_kinds():
    assert [(pc.CASES[n]["shape"], pc.CASES[n]["B"]) for n in pc.ORACLE_CASES] == [((4, 2, 10), 13), ((5, 3, 7), 11), ((12, 4, 10), 2)]
    assert [pc.CASES[n]["B"] % 4 for n in pc.ORACLE_CASES] == [1, 3, 2] and pc.T == 5
    dims = [tuple(int(w) for w in ln.split()[:3]) for ln in open(os.path.join(CSRC, "kernel_dims.txt")) if ln.strip() and not ln.startswith("#") and ln.split()[0].isdigit()]
    assert (5, 3, 7) not in dims and 5 % 4 != 0


# ---- the path and the variant choice ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("plant_path") / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "dropin", "plant_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _lines(exe, mode, stdin=None):
    out = subprocess.run([exe, mode], input=stdin, check=True, capture_output=True, text=True, timeout=900).stdout.splitlines()
    return [dict(w.split("=", 1) for w in ln.split()) for ln in out]


BOX = dict(fits_box=1, fits=1, plant=1)
CONE = dict(BOX, soc=1)
LIN = dict(BOX, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1)


def test_path_rules_with_a_plant_and_with_the_state_log(driver):
    # facts -> (kernel, rule, (lin, pl, pb, pc, pd, pp), path code, refusal)
    cases = [
        (BOX, ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1), 3, 0)),        # a compiled-in entry is not asked
        (dict(BOX, hetero=1), ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1), 3, 0)),
        (CONE, ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1), 3, 0)),
        (LIN, ("ONE_ROW", "one_row:pp", (1, 0, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, disturbance=1), ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 1, 1), 3, 0)),                      # with a disturbance: both bits
        (dict(BOX, state_log=1), ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1), 3, 0)),                        # the PP form writes the log itself
        # composition with the per-instance rules: their forms take the bit and keep their rule
        (dict(BOX, inst_bounds=1), ("ONE_ROW", "one_row:pb", (0, 0, 1, 0, 0, 1), 3, 0)),
        (dict(LIN, inst_lin=1), ("ONE_ROW", "one_row:pl", (1, 1, 0, 0, 0, 1), 3, 0)),
        (dict(CONE, inst_cones=1), ("ONE_ROW", "one_row:pc", (0, 0, 0, 1, 0, 1), 3, 0)),
        # ... and a coverage answer stays coverage; where no PP form can be made: cover:pp
        (dict(CONE, cones_overlap=1), ("COVERAGE", "cones_overlap", (0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, force_general=1), ("COVERAGE", "cover:force_general", (0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, debug=1), ("COVERAGE", "cover:pp", (0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, no_jit=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pp", (0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, variant_jit_failed=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pp", (0, 0, 0, 0, 0, 0), 2, 0)),
        # never the tile kernel while the fact is on: its shapes run on the coverage kernel
        (dict(plant=1, has_tile=1), ("COVERAGE", "cover:no_register_form", (0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(state_log=1, has_tile=1), ("COVERAGE", "cover:no_register_form", (0, 0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, has_tile=1, prefer_tile=1), ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1), 3, 0)),
        (dict(has_tile=1), ("TILE", "tile:no_register_form", (0, 0, 0, 0, 0, 0), 1, 0)),
        # adaptive rho: refused with the plant's own value; what was refused before keeps its value
        (dict(BOX, adaptive=1), ("COVERAGE", "cover:pp", (0, 0, 0, 0, 0, 0), 2, 7)),
        (dict(BOX, adaptive=1, disturbance=1), ("COVERAGE", "cover:pp", (0, 0, 0, 0, 0, 0), 2, 6)),
        (dict(BOX, adaptive=1, inst_bounds=1), ("COVERAGE", "cover:pp", (0, 0, 0, 0, 0, 0), 2, 1)),
        (dict(fits_box=1, fits=1, state_log=1, adaptive=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0, 0), 2, 8)),
        # the state log alone rides on the PD form (an empty sequence)
        (dict(fits_box=1, fits=1, state_log=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0), 3, 0)),
        (dict(fits_box=1, fits=1, state_log=1, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0), 3, 0)),
        # the facts off: the answers without the feature
        (dict(fits_box=1, fits=1), ("ONE_ROW", "one_row:plain", (0, 0, 0, 0, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:plain", (0, 0, 0, 0, 0, 0), 0, 0)),
        (dict(fits_box=1, fits=1, adaptive=1), ("ONE_ROW", "one_row:adaptive", (0, 0, 0, 0, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, disturbance=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0), 3, 0)),
    ]
    stdin = "".join(" ".join("%s=%d" % kv for kv in f.items()) + "\n" for f, _ in cases)
    got = _lines(driver, "path", stdin)
    assert len(got) == len(cases)
    for (f, (kernel, rule, forms, code, refusal)), g in zip(cases, got):
        assert (g["kernel"], g["rule"], int(g["code"]), int(g["refusal"]), g["consistent"]) == (kernel, rule, code, refusal, "1"), (f, g)
        assert tuple(int(g[k]) for k in ("lin", "pl", "pb", "pc", "pd", "pp")) == forms, (f, g)
    p = subprocess.run([driver, "message"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.splitlines() == [
        "7 adaptive rho does not combine with a plant of its own at the plant step (tiny_batch_set_plant)",
        "8 adaptive rho does not combine with the state log (option state_log)"], p.stdout


def test_path_and_variant_sweeps_follow_pds_rule(driver):
    tail = {k: int(v) for r in _lines(driver, "paths") if len(r) == 1 for k, v in r.items()}
    assert tail["violations"] == 0 and tail["tile_with_plant"] == 0, tail
    assert min(tail["plain"], tail["with_plant"], tail["with_log"], tail["one_row_pp"], tail["cover_pp"]) > 1000, tail
    tail = {k: int(v) for r in _lines(driver, "variants") if len(r) == 1 for k, v in r.items()}
    assert tail["with_pp"] > 1000 and tail["violations"] == 0 and tail["key_order"] == 1, tail


def test_the_argument_block_keeps_its_size_and_the_new_fields_fill_the_room_behind_the_disturbance(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    prog = ('#include <cstdio>\n#include "%s"\nusing tinympc_amd::SolveArgs;\nint main() { printf("%%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(SolveArgs), '
            '__builtin_offsetof(SolveArgs, pf_base), __builtin_offsetof(SolveArgs, dist), __builtin_offsetof(SolveArgs, dist_step0), '
            '__builtin_offsetof(SolveArgs, plant), __builtin_offsetof(SolveArgs, state_log)); return 0; }\n' % os.path.join(CSRC, "admm_kernel.hip.h"))
    exe, cpp = str(tmp_path / "layout"), tmp_path / "layout.hip"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    words = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(w) for w in words] == [472, 440, 440, 452, 456, 464], words


# ---- the PP forms ------------------------------------------------------------------------------------------------------------------------
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
# disturbance, with PB, a cone and a half-space variant; dpp_mode 0; the PL and PC forms
PP_VARIANTS = [pp_name(4, 2, 10, mode=2 | PP, ub=True), pp_name(5, 3, 7, mode=2 | PP, ub=True), pp_name(12, 4, 10, mode=2 | PP, ub=True),
               pp_name(12, 4, 10, mode=2 | PP, het=True, ub=True), pp_name(6, 3, 10, mode=2 | PD | PP, ub=True), pp_name(6, 3, 10, mode=2 | 4 | PP, ub=True),
               pp_name(6, 3, 10, soc=True, mode=2 | PP), pp_name(6, 3, 10, mode=2 | PP, lin=1), pp_name(6, 3, 10, mode=0 | PP),
               # every instance its own half-spaces (PL, two per knot) and cone coefficients (PC), with and without the disturbance bit
               pp_name(6, 3, 10, mode=2 | 8 | PP, lin=1, kmax=2), pp_name(6, 3, 10, mode=2 | 8 | PD | PP, lin=1, kmax=2),
               pp_name(6, 3, 10, soc=True, mode=2 | 16 | PP), pp_name(6, 3, 10, soc=True, mode=2 | 16 | PD | PP)]


def test_pp_variants_compile_and_adapt_half_and_pf_names_are_refused():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    refused = [(pp_name(6, 3, 10, mode=2 | PP, adapt=True), "a plant of its own: not with adaptive rho"),
               (pp_name(4, 2, 10, mode=2 | PP, tail=", false, true"), "a plant of its own: not the half-row form"),
               (pp_name(6, 3, 10, mode=2 | PP, tail=", false, false, true"), "a plant of its own: not the prefetch form")]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PP_VARIANTS + [n for n, _ in refused], capture_output=True, text=True, timeout=3000, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    good, bad = res[:len(PP_VARIANTS)], res[len(PP_VARIANTS):]
    assert [r["name"] for r in good] == PP_VARIANTS
    assert not [r for r in good if "error" in r], [r for r in good if "error" in r]
    assert all(r["bytes"] > 1000 for r in good)
    for r, (_, text) in zip(bad, refused):
        assert "error" in r and text in r["error"], r
