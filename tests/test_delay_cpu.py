"""CPU: the transport delay in front of the actuator and the predictor that compensates it (tiny_batch_set_actuator_delay and its
neighbours, option "delay_compensation"), as far as it can be checked without a GPU -- the reference conditions of every case the GPU
tests use, from the reference and the oracle loops alone; the reference's own arithmetic; the exported entry points, their ctypes mirror
and their NULL returns; the path and variant rules (tests/dropin/delay_path_driver.cpp, built here against a frozen copy of the rules
as they stood before the delay); the launch record's layout; and that the PQ and PX forms of the one-row kernel compile for gfx950
while names that violate their asserts are refused."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import delay_cases as dl
import plant_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
BATCH_SYMBOLS = ("tiny_batch_set_actuator_delay", "tiny_batch_get_actuator_delay", "tiny_batch_set_actuator_queue", "tiny_batch_get_actuator_queue")
GROUP_SYMBOLS = ("tiny_group_set_actuator_delay", "tiny_group_set_actuator_queue")
PP, PM, PA, PQ, PX = 64, 128, 1024, 4096, 8192      # bits 6, 7, 10, 12, 13 of the kernel's MODE argument (bit 11 names no form)


@pytest.mark.parametrize("name", dl.ALL_CASES)
def test_the_cases_of_the_gpu_tests_meet_the_reference_conditions(name):
    dl.check_case(name)
    assert dl.T == 8 and dl.D_MAX == 3 and dl.delays(name).tolist() == [i % 4 for i in range(pc.case(name)["B"])]
    assert not np.any(dl.zero_queue(name)) and dl.zero_queue(name).shape == (pc.case(name)["B"], 3, pc.case(name)["nu"])


def test_an_estimator_that_predicts_with_the_command_under_compensation_is_visible():
    dl.check_estimator_case()


def test_the_reference_pops_before_it_pushes_and_predicts_oldest_first():
    q = [np.array([1.0]), np.array([2.0])]
    s0, after = dl.fifo(q, 2, np.array([3.0]))
    assert s0.tolist() == [1.0] and [r.tolist() for r in after] == [[2.0], [3.0]]
    s0, after = dl.fifo([], 0, np.array([-0.0]))
    assert after == [] and s0[0] == 0.0 and np.signbit(s0[0])        # (d = 0: the command's own bits)
    s0, _ = dl.fifo(q, 2, np.array([3.0]), "push_before_pop")
    assert s0.tolist() == [2.0]
    assert dl.fifo([np.array([1.0])], 1, np.array([3.0]), "push_before_pop")[0].tolist() == [3.0]
    # x <- 0.5 + 2 x + u: the order of the entries matters
    model = (np.array([[2.0]]), np.array([[1.0]]), np.array([0.5]))
    assert dl.predict(model, np.array([1.0]), q, 2).tolist() == [2 * (2 * 1.0 + 1.0 + 0.5) + 2.0 + 0.5]
    assert dl.predict(model, np.array([1.0]), q, 2, "newest_first").tolist() == [2 * (2 * 1.0 + 2.0 + 0.5) + 1.0 + 0.5]
    assert dl.predict(model, np.array([1.0]), q, 0).tolist() == [1.0]
    plant = (np.array([[3.0]]), np.array([[1.0]]), np.array([0.0]))
    assert dl.predict(model, np.array([1.0]), q, 1, "predict_with_plant", plant).tolist() == [4.0]


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in BATCH_SYMBOLS + GROUP_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
        assert name in (tm.BATCH_SYMBOLS if name in BATCH_SYMBOLS else tm.GROUP_SYMBOLS), name
    assert "#define TINY_MAX_DELAY 8" in header and tm.MAX_DELAY == 8
    L = tm.lib()
    dp = np.zeros(4).ctypes.data_as(C.POINTER(C.c_double))
    one = C.c_int(0)
    assert L.tiny_batch_set_actuator_delay(None, None, 0, tm.HOST) == tm.ERR_NULL and L.tiny_batch_get_actuator_delay(None, 0, C.byref(one)) == tm.ERR_NULL
    assert L.tiny_batch_set_actuator_queue(None, None, tm.HOST) == tm.ERR_NULL and L.tiny_batch_get_actuator_queue(None, dp) == tm.ERR_NULL
    assert L.tiny_group_set_actuator_delay(None, None, 0, tm.HOST) == tm.ERR_NULL and L.tiny_group_set_actuator_queue(None, None, tm.HOST) == tm.ERR_NULL
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        for name in ("set_actuator_delay", "set_actuator_queue", "get_actuator_queue"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("set_actuator_delay_device", "get_actuator_delay", "set_actuator_queue_device"):
        assert callable(getattr(tm.TinyBatchSolver, name)), name
    for word in ("delay -> limits -> lag -> gain -> noise", "delay_compensation", "actuator_delay", "xs = f + A xs + B q[t]", "BEFORE this step's push",
                 "Out of scope: per-input delays; fractional delays; a delay on the measurement side"):
        assert word in header, word


# ---- the path and variant rules --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("delay_path") / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, "-I", os.path.join(ROOT, "tests", "dropin"), os.path.join(ROOT, "tests", "dropin", "delay_path_driver.cpp"),
                    "-o", exe], check=True)
    return exe


def counts(out):
    return {k: int(v) for k, v in (ln.split("=") for ln in out.splitlines() if ln.count("=") == 1 and " " not in ln)}


def test_with_the_facts_off_every_decision_is_what_it_was_and_with_them_on_the_bits_ride_on_the_actuators_rule(driver):
    p = subprocess.run([driver, "paths"], capture_output=True, text=True)
    n = counts(p.stdout)
    assert p.returncode == 0 and n["violations"] == 0, p.stdout
    assert n["off"] > 100000 and n["delayed"] > 100000 and n["compensated"] * 2 == n["delayed"]
    assert n["one_row_pq"] > 0 and n["one_row_px"] * 2 == n["one_row_pq"] and n["cover"] > 0 and n["refused_12"] > 0
    p = subprocess.run([driver, "variants"], capture_output=True, text=True)
    n = counts(p.stdout)
    assert p.returncode == 0 and n["violations"] == 0 and n["with_pq"] > 100, p.stdout


def ask(driver, *queries):
    p = subprocess.run([driver, "path"], input="\n".join(queries) + "\n", capture_output=True, text=True, check=True)
    return [dict(w.split("=", 1) for w in ln.split()) for ln in p.stdout.strip().splitlines()]


def test_path_rules_under_a_delay(driver):
    base = "fits=1 fits_box=1 actuator=1 delay=1"
    plain, comp, est, forced, nojit, adaptive, adaptive_comp, alone = ask(
        driver, base, base + " delay_compensation=1", base + " delay_compensation=1 estimator=1 score=1", base + " delay_compensation=1 force_general=1",
        base + " no_jit=1 has_entry=1 entry_plain=1", base + " adaptive=1", base + " delay_compensation=1 adaptive=1 measurement=1", "fits=1 fits_box=1 delay_compensation=1")
    assert (plain["kernel"], plain["rule"], plain["pp"], plain["pm"], plain["pa"], plain["pq"], plain["px"], plain["code"]) == ("ONE_ROW", "one_row:pa", "1", "0", "1", "1", "0", "3")
    assert (comp["kernel"], comp["rule"], comp["pp"], comp["pm"], comp["pe"], comp["pa"], comp["pq"], comp["px"], comp["code"]) == ("ONE_ROW", "one_row:pa", "1", "1", "0", "1", "1", "1", "3")
    assert (est["rule"], est["pm"], est["pe"], est["ps"], est["pq"], est["px"]) == ("one_row:pa", "1", "1", "1", "1", "1")
    assert (forced["kernel"], forced["rule"], forced["code"], forced["pq"], forced["px"]) == ("COVERAGE", "cover:force_general", "2", "0", "0")      # (a coverage answer keeps its rule's name)
    assert (nojit["kernel"], nojit["rule"]) == ("COVERAGE", "cover:pa")
    assert adaptive["refusal"] == "12" and adaptive["rule"] == "cover:pa"
    assert adaptive_comp["refusal"] == "9"                           # (an INSTALLED measurement-noise sequence is reported first, as before)
    assert alone["consistent"] == "0"                                # (the option without a delay is no fact: closed_loop_facts never sets it alone)
    assert all(q["consistent"] == "1" for q in (plain, comp, est, forced, nojit, adaptive, adaptive_comp))


# ---- the kernel header -----------------------------------------------------------------------------------------------------------------
def name_of(nx, nu, N, mode, soc=False):
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, 0, false, 4, false>" % (nx, nu, N, "true" if soc else "false", mode)


def compile_name(name, tmp_path):
    nx, nu = (int(v) for v in name.split("<")[1].split(",")[:2])
    src = tmp_path / "unit.hip"
    src.write_text('#define TINYMPC_FUSED_NX %d\n#define TINYMPC_FUSED_NU %d\n#include "%s"\ntemplate __global__ void %s(const tinympc_amd::SolveArgs);\n'
                   % (nx, nu, os.path.join(CSRC, "admm_kernel.hip.h"), name))
    return subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-c", str(src), "-o", str(tmp_path / "unit.o")], capture_output=True, text=True)


def test_the_launch_record_and_the_new_forms_compile_and_names_that_violate_the_asserts_are_refused(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    prog = tmp_path / "layout.cpp"
    prog.write_text('#include <hip/hip_runtime.h>\n#include <cstddef>\n#include "%s"\nusing namespace tinympc_amd;\n'
                    'static_assert(sizeof(ActuatorLaunch) == 40 && sizeof(DelayLaunch) == 48, "the record the PA forms read stays; the delay\'s lies behind it");\n'
                    'static_assert(offsetof(DelayLaunch, delay) == 0 && offsetof(DelayLaunch, queue) == 8 && offsetof(DelayLaunch, head) == 16 &&\n'
                    '              offsetof(DelayLaunch, model) == 24 && offsetof(DelayLaunch, xhat) == 32 && offsetof(DelayLaunch, d_max) == 40, "five pointers and two ints");\n'
                    'static_assert(sizeof(SolveArgs) == 472, "SolveArgs keeps its size");\nint main() { return 0; }\n' % os.path.join(CSRC, "admm_kernel.hip.h"))
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-fsyntax-only", str(prog)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    good = 2 + PP + PM + PA + PQ + PX
    p = compile_name(name_of(4, 2, 10, good), tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    p = compile_name(name_of(4, 2, 10, 2 + PP + PA + PQ), tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    for bad, why in ((2 + PP + PQ, "a transport delay: a form with an actuator model"), (2 + PP + PA + PQ + PX, "a delay predictor"), (2 + PP + PM + PA + PX, "a delay predictor"),
                     (2 + 16384, "MODE 0 | 1 | 2"), (2 + PP + PA + 2048, "2048 names no form")):
        p = compile_name(name_of(4, 2, 10, bad), tmp_path)
        assert p.returncode != 0 and why in p.stderr, (bad, p.stderr[-1500:])
