"""CPU: the fixed-gain state estimator at the plant step of a closed loop (tiny_batch_set_estimator), as far as it can be checked without
a GPU -- the exported entry points and their NULL returns; the reference correction; the oracle-side conditions of every case the GPU
tests use; gain_entry against a dense restatement; the path and variant rules (tests/dropin/estimator_path_driver.cpp, the interface of
the measurement driver) and the refusal text and position; the argument block's fixed layout; that the PE forms of the one-row kernel
(run-time instantiated only) compile for gfx950, that a name without the PM bit or with ADAPT is refused by name, and that their
iteration loop touches no scratch."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import estimator_cases as ec
import measurement_cases as mc
import plant_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

NEW_SYMBOLS = ("tiny_batch_set_estimator", "tiny_batch_get_estimator", "tiny_batch_set_estimate", "tiny_batch_get_estimate", "tiny_batch_get_estimate_log",
               "tiny_group_set_estimator", "tiny_group_set_estimate")
PD, PP, PM, PE = 32, 64, 128, 256                  # bits 5 .. 8 of the kernel's MODE argument


def pe_name(nx, nu, N, soc=False, mode=2, lin=0, het=False, kmax=4, adapt=False, ub=False):
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
    assert L.tiny_batch_set_estimator(None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_estimator(None, 0, None) == tm.ERR_NULL
    assert L.tiny_batch_set_estimate(None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_estimate(None, None) == tm.ERR_NULL
    assert L.tiny_batch_get_estimate_log(None, None, 1) == tm.ERR_NULL
    assert L.tiny_group_set_estimator(None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_group_set_estimate(None, None, tm.HOST) == tm.ERR_NULL
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        for name in ("set_estimator", "set_estimator_device", "get_estimator", "set_estimate", "get_estimate", "estimate_log"):
            assert callable(getattr(cls, name)), (cls, name)
    for word in ("TRUE state", "M = L*C", "C v = v_y", "estimate_log", "last_estimator", "ONE chain, ascending c"):
        assert word in header, word


def test_the_reference_correction_is_the_chain_rounded_once_per_term():
    rng = np.random.default_rng(5)
    for nx in (1, 4, 12):
        M, xp, xm = rng.normal(size=(nx, nx)), rng.normal(size=nx), rng.normal(size=nx)
        got = ec.correct(M, xp, xm)
        e = xm - xp
        assert np.allclose(got, xp + M @ e, rtol=0, atol=1e-13)
        acc = float(xp[nx - 1])
        for c in range(nx):
            acc = pc.fma(e[c], M[nx - 1, c], acc)
        assert got[nx - 1] == acc
        assert np.array_equal(ec.correct(np.zeros((nx, nx)), xp, xm), xp)          # M = 0 closes the sensor off
        assert np.array_equal(ec.correct(1e6 * M, xp, xp), xp)                     # e = 0: any finite M
    # one rounding per term, not one at the end and not two per term
    assert ec.correct(np.array([[2.0 ** -53]]), np.array([1.0]), np.array([2.0]))[0] == 1.0
    assert ec.correct(np.array([[1.0 + 2.0 ** -30]]), np.array([0.0]), np.array([1.0 + 2.0 ** -30]))[0] == pc.fma(1.0 + 2.0 ** -30, 1.0 + 2.0 ** -30, 0.0)


@pytest.mark.parametrize("name", ec.ORACLE_CASES + ec.EDGE_CASES)
def test_the_cases_of_the_gpu_tests_meet_their_conditions(name):
    ec.check_case(name)
    c, M, xp0 = pc.case(name), ec.gain(name), ec.estimate(name)
    B, nx = c["B"], c["nx"]
    assert M.shape == (B, nx, nx) and xp0.shape == (B, nx) and ec.T == 5
    d = np.abs(M[:, np.arange(nx), np.arange(nx)])
    off = np.abs(M[:, ~np.eye(nx, dtype=bool)]) * nx / 2
    assert np.all((d >= 0.4) & (d <= 0.8)) and (off.size == 0 or np.all((off >= 0.05 - 1e-15) & (off <= 0.15 + 1e-15)))
    gap = np.abs(xp0 - c["x0"])
    assert np.all((gap >= 0.05 - 1e-12) & (gap <= 0.1 + 1e-12))
    assert [(pc.CASES[n]["shape"], pc.CASES[n]["B"]) for n in ec.ORACLE_CASES] == [((4, 2, 10), 13), ((5, 3, 7), 11), ((12, 4, 10), 2)]
    assert [pc.CASES[n]["shape"] for n in ec.EDGE_CASES] == [(15, 1, 3), (1, 15, 3)]
    assert all(np.all(p != m) for p, m in zip(c["plant"], mc.model_of(c)))         # the case's perturbed plant


# ---- gain_entry ---------------------------------------------------------------------------------------------------------------------------
def test_gain_entry_against_a_dense_restatement(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    prog = ('#include <hip/hip_runtime.h>\n#include <cstdio>\n#include <vector>\n#include "%s"\nusing namespace tinympc_amd;\n'
            'int main() { for (int nx : {1, 5, 12, 15, 16}) { std::vector<double> M(nx * nx); for (int i = 0; i < nx * nx; ++i) M[i] = 1000.0 * nx + i + 0.5;\n'
            '  if (gain_block_doubles(nx) != nx * 16) return 1;\n'
            '  for (int c = 0; c < nx; ++c) for (int lane = 0; lane < 16; ++lane) printf("%%d %%d %%d %%.17g\\n", nx, c, lane, gain_entry(M.data(), nx, c, lane)); }\n'
            '  return 0; }\n' % os.path.join(CSRC, "lane_tables.hpp"))
    exe, cpp = str(tmp_path / "gain"), tmp_path / "gain.cpp"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, "-x", "hip", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    rows = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()]
    assert len(rows) == sum(nx * 16 for nx in (1, 5, 12, 15, 16))
    for nx, c, lane, val in rows:
        nx, c, lane, val = int(nx), int(c), int(lane), float(val)
        M = (1000.0 * nx + np.arange(nx * nx) + 0.5).reshape(nx, nx).T             # column-major as given: M[j, c] = flat[j + nx * c]
        assert val == (M[lane, c] if lane < nx else 0.0), (nx, c, lane, val)       # state lane j keeps row j; the input lanes' rows are zero


# ---- the path and the variant choice ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("estimator_path") / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "dropin", "estimator_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _lines(exe, mode, stdin=None):
    out = subprocess.run([exe, mode], input=stdin, check=True, capture_output=True, text=True, timeout=1800).stdout.splitlines()
    return [dict(w.split("=", 1) for w in ln.split()) for ln in out]


BOX = dict(fits_box=1, fits=1, estimator=1)
CONE = dict(BOX, soc=1)
LIN = dict(BOX, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1)


def test_path_rules_under_an_estimator(driver):
    # facts -> (kernel, rule, (lin, pl, pb, pc, pd, pp, pm, pe), path code, refusal)
    cases = [
        (BOX, ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),                                        # the fact forces pm and pp on
        (dict(BOX, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),     # a compiled-in entry is not asked
        (CONE, ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),
        (LIN, ("ONE_ROW", "one_row:pe", (1, 0, 0, 0, 0, 1, 1, 1), 3, 0)),
        (dict(BOX, hetero=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),
        (dict(BOX, measurement=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),                   # with noise installed: the same form
        (dict(BOX, plant=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),
        (dict(BOX, disturbance=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 1, 1, 1, 1), 3, 0)),                   # with a disturbance: all four bits
        (dict(BOX, plant=1, disturbance=1, measurement=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 1, 1, 1, 1), 3, 0)),
        (dict(BOX, state_log=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),                     # the PP form writes the log itself
        # composition with the per-instance rules: their forms take the bits and keep their rule
        (dict(BOX, inst_bounds=1), ("ONE_ROW", "one_row:pb", (0, 0, 1, 0, 0, 1, 1, 1), 3, 0)),
        (dict(LIN, inst_lin=1), ("ONE_ROW", "one_row:pl", (1, 1, 0, 0, 0, 1, 1, 1), 3, 0)),
        (dict(CONE, inst_cones=1), ("ONE_ROW", "one_row:pc", (0, 0, 0, 1, 0, 1, 1, 1), 3, 0)),
        # ... and a coverage answer stays coverage; where no PE form can be made: cover:pe
        (dict(CONE, cones_overlap=1), ("COVERAGE", "cones_overlap", (0,) * 8, 2, 0)),
        (dict(BOX, force_general=1), ("COVERAGE", "cover:force_general", (0,) * 8, 2, 0)),
        (dict(BOX, debug=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 0)),
        (dict(BOX, no_jit=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 0)),
        (dict(BOX, variant_jit_failed=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 0)),
        # never the tile kernel while the fact is on: its shapes run on the coverage kernel
        (dict(estimator=1, has_tile=1), ("COVERAGE", "cover:no_register_form", (0,) * 8, 2, 0)),
        (dict(BOX, has_tile=1, prefer_tile=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1), 3, 0)),
        (dict(has_tile=1), ("TILE", "tile:no_register_form", (0,) * 8, 1, 0)),
        # adaptive rho: refused with the fact's own value, reported last; what was refused before keeps its value
        (dict(BOX, adaptive=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 10)),
        (dict(BOX, adaptive=1, measurement=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 9)),
        (dict(BOX, adaptive=1, state_log=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 8)),
        (dict(BOX, adaptive=1, plant=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 7)),
        (dict(BOX, adaptive=1, disturbance=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 6)),
        (dict(BOX, adaptive=1, inst_bounds=1), ("COVERAGE", "cover:pe", (0,) * 8, 2, 1)),
        # the fact off: the answers without the feature
        (dict(fits_box=1, fits=1), ("ONE_ROW", "one_row:plain", (0,) * 8, 3, 0)),
        (dict(fits_box=1, fits=1, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:plain", (0,) * 8, 0, 0)),
        (dict(fits_box=1, fits=1, adaptive=1), ("ONE_ROW", "one_row:adaptive", (0,) * 8, 3, 0)),
        (dict(fits_box=1, fits=1, measurement=1), ("ONE_ROW", "one_row:pm", (0, 0, 0, 0, 0, 1, 1, 0), 3, 0)),
        (dict(fits_box=1, fits=1, plant=1), ("ONE_ROW", "one_row:pp", (0, 0, 0, 0, 0, 1, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, state_log=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, measurement=1, adaptive=1), ("COVERAGE", "cover:pm", (0,) * 8, 2, 9)),
    ]
    stdin = "".join(" ".join("%s=%d" % kv for kv in f.items()) + "\n" for f, _ in cases)
    got = _lines(driver, "path", stdin)
    assert len(got) == len(cases)
    for (f, (kernel, rule, forms, code, refusal)), g in zip(cases, got):
        assert (g["kernel"], g["rule"], int(g["code"]), int(g["refusal"]), g["consistent"]) == (kernel, rule, code, refusal, "1"), (f, g)
        assert tuple(int(g[k]) for k in ("lin", "pl", "pb", "pc", "pd", "pp", "pm", "pe")) == forms, (f, g)
    p = subprocess.run([driver, "message"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.splitlines() == [
        "9 adaptive rho does not combine with measurement noise (tiny_batch_set_measurement_noise)",
        "10 adaptive rho does not combine with a state estimator (tiny_batch_set_estimator)"], p.stdout
    # appended behind the measurement's: the next value, and with both facts on (or any earlier one) the earlier refusal is answered
    both = _lines(driver, "path", "".join(" ".join("%s=%d" % kv for kv in dict(BOX, adaptive=1, **on).items()) + "\n"
                                          for on in ({}, dict(measurement=1), dict(state_log=1, measurement=1))))
    assert [int(g["refusal"]) for g in both] == [10, 9, 8]


def test_path_and_variant_sweeps_follow_the_measurements_rule(driver):
    tail = {k: int(v) for r in _lines(driver, "paths") if len(r) == 1 for k, v in r.items()}
    assert tail["violations"] == 0 and tail["tile_with_estimator"] == 0, tail
    assert min(tail["plain"], tail["with_estimator"], tail["one_row_pe"], tail["cover_pe"], tail["refused_10"]) > 1000, tail
    tail = {k: int(v) for r in _lines(driver, "variants") if len(r) == 1 for k, v in r.items()}
    assert tail["with_pe"] > 1000 and tail["violations"] == 0 and tail["key_order"] == 1, tail


def test_the_argument_block_keeps_its_size_and_the_new_pointers_lie_over_the_adaptive_rho_ones(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    fields = ("arho", "est_gain", "aK", "est_xp", "aP", "est_log", "aC1", "est_model", "aC2", "atab", "arho_min", "pf_mask", "meas", "pf_counter", "dist", "plant", "state_log")
    prog = ('#include <cstdio>\n#include "%s"\nusing tinympc_amd::SolveArgs;\nint main() { printf("%%zu", sizeof(SolveArgs));\n%s printf("\\n"); return 0; }\n'
            % (os.path.join(CSRC, "admm_kernel.hip.h"), "".join('printf(" %%zu", __builtin_offsetof(SolveArgs, %s));\n' % f for f in fields)))
    exe, cpp = str(tmp_path / "layout"), tmp_path / "layout.hip"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    words = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(w) for w in words] == [472, 304, 304, 312, 312, 320, 320, 328, 328, 336, 344, 352, 416, 416, 432, 440, 456, 464], words
    text = open(os.path.join(CSRC, "admm_kernel.hip.h")).read()
    assert ('static_assert(sizeof(SolveArgs) == 472 && __builtin_offsetof(SolveArgs, het_tabs) == 208 && __builtin_offsetof(SolveArgs, pf_mask) == 416 &&\n'
            '              __builtin_offsetof(SolveArgs, pf_counter) == 432 && __builtin_offsetof(SolveArgs, pf_base) == 440, "SolveArgs: size and offsets are fixed");') in text
    assert "__builtin_offsetof(SolveArgs, est_gain) == 304" in text and "__builtin_offsetof(SolveArgs, est_model) == 328" in text


# ---- the PE forms ------------------------------------------------------------------------------------------------------------------------
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

# the forms the issue names: (12,4,10) box (knot-invariant: UB), the (6,3,10) cone, (5,3,7), and a per-instance-data form
BASE = 2 | PP | PM | PE
PE_VARIANTS = [pe_name(12, 4, 10, mode=BASE, ub=True), pe_name(6, 3, 10, soc=True, mode=BASE), pe_name(5, 3, 7, mode=BASE, ub=True),
               pe_name(12, 4, 10, mode=BASE, het=True, ub=True)]


def test_pe_variants_compile_and_names_without_pm_or_with_adapt_are_refused():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    refused = [(pe_name(6, 3, 10, mode=2 | PP | PE), "a state estimator: a form that solves from a measured state (PM, bit 7)"),
               (pe_name(6, 3, 10, mode=2 | PE), "a state estimator: a form that solves from a measured state (PM, bit 7)"),
               (pe_name(6, 3, 10, mode=BASE, adapt=True), "a state estimator: not with adaptive rho")]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PE_VARIANTS + [n for n, _ in refused], capture_output=True, text=True, timeout=3000, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    good, bad = res[:len(PE_VARIANTS)], res[len(PE_VARIANTS):]
    assert [r["name"] for r in good] == PE_VARIANTS
    assert not [r for r in good if "error" in r], [r for r in good if "error" in r]
    assert all(r["bytes"] > 1000 for r in good)
    for r, (_, text) in zip(bad, refused):
        assert "error" in r and text in r["error"], r


@pytest.mark.parametrize("targs", [("12", "4", "10", "false", "false", str(BASE), "0", "false", "4", "false", "true"), ("6", "3", "10", "true", "false", str(BASE))])
def test_the_iteration_loop_of_a_pe_form_touches_no_scratch_and_no_memory_the_pm_form_does_not(targs, tmp_path):
    """the assembly hipcc emits for the PE form and for the PM form it is derived from, through tools/isa_loop_stats.py (the fused column
    blocks, as the library is built): the iteration loop holds no scratch instruction and no more LDS or VMEM instructions"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    spec = importlib.util.spec_from_file_location("isa_loop_stats", os.path.join(ROOT, "tools", "isa_loop_stats.py"))
    ils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ils)
    loops = {}
    for mode in (BASE, BASE & ~PE):
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
    pe, pm = loops[BASE], loops[BASE & ~PE]
    assert pe.get("scratch", 0) == 0 and pm.get("scratch", 0) == 0, (pe, pm)
    assert pe.get("lds", 0) <= pm.get("lds", 0) and pe.get("vmem", 0) <= pm.get("vmem", 0), (pe, pm)
