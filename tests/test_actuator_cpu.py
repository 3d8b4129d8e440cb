"""CPU: the actuator model between the command and the plant step (tiny_batch_set_actuator and its neighbours), as far as it can be
checked without a GPU -- the exported entry points, their ctypes mirror and their NULL returns; the reference's arithmetic; the visibility
conditions of every case the GPU tests use, from the reference and the oracle loops alone; actuator_entry against a dense restatement;
the path and variant rules (tests/dropin/actuator_path_driver.cpp) and the refusal's text and position; the argument block's fixed
layout; that the PA forms of the one-row kernel (run-time instantiated only) compile for gfx950 and that names with ADAPT, HALF, PF or
without the PP bit are refused by name; the host generator of the actuation noise against tests/noise_ref.py; and that the bit adds
nothing to the iteration loop."""
import ctypes as C
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import actuator_cases as ac
import noise_ref as nr
import plant_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

BATCH_SYMBOLS = ("tiny_batch_set_actuator", "tiny_batch_get_actuator", "tiny_batch_set_actuator_state", "tiny_batch_get_actuator_state", "tiny_batch_set_actuation_noise",
                 "tiny_batch_get_actuation_noise", "tiny_batch_generate_actuation_noise", "tiny_actuation_noise_generate", "tiny_batch_get_actuation_log")
GROUP_SYMBOLS = ("tiny_group_set_actuator", "tiny_group_set_actuator_state", "tiny_group_set_actuation_noise", "tiny_group_generate_actuation_noise")
PD, PP, PM, PE, PS, PA = 32, 64, 128, 256, 512, 1024         # bits 5 .. 10 of the kernel's MODE argument


def pa_name(nx, nu, N, soc=False, mode=2, lin=0, het=False, kmax=4, adapt=False, ub=False, half=False, pf=False):
    b = lambda v: "true" if v else "false"
    tail = ", %s, %s, %s" % (b(ub), b(half), b(pf)) if (half or pf) else (", true" if ub else "")
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, %d, %s, %d, %s%s>" % (nx, nu, N, b(soc), mode, lin, b(het), kmax, b(adapt), tail)


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in BATCH_SYMBOLS + GROUP_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
        assert name in (tm.BATCH_SYMBOLS if name in BATCH_SYMBOLS else tm.GROUP_SYMBOLS), name
    L = tm.lib()
    dp = np.zeros(4).ctypes.data_as(C.POINTER(C.c_double))
    assert L.tiny_batch_set_actuator(None, None, None, None, None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_actuator(None, 0, None, None, None, None, None) == tm.ERR_NULL
    assert L.tiny_batch_set_actuator_state(None, None, tm.HOST) == tm.ERR_NULL and L.tiny_batch_get_actuator_state(None, dp) == tm.ERR_NULL
    assert L.tiny_batch_set_actuation_noise(None, None, 0, tm.HOST) == tm.ERR_NULL and L.tiny_batch_get_actuation_noise(None, 0, 0, dp) == tm.ERR_NULL
    assert L.tiny_batch_generate_actuation_noise(None, None) == tm.ERR_NULL and L.tiny_batch_get_actuation_log(None, dp, 1) == tm.ERR_NULL
    assert L.tiny_group_set_actuator(None, None, None, None, None, None, tm.HOST) == tm.ERR_NULL and L.tiny_group_set_actuator_state(None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_group_set_actuation_noise(None, None, 0, tm.HOST) == tm.ERR_NULL and L.tiny_group_generate_actuation_noise(None, None) == tm.ERR_NULL
    # the host generator's argument errors: a null spec, a null output, no instances, no inputs, device arrays
    spec, keep = tm.noise_spec(3, 2, 5, 4, np.ones(2))
    out = np.zeros((4, 3, 2))
    op = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.tiny_actuation_noise_generate(None, 3, 2, op) == tm.ERR_ARG and L.tiny_actuation_noise_generate(C.byref(spec), 3, 2, None) == tm.ERR_ARG
    assert L.tiny_actuation_noise_generate(C.byref(spec), 0, 2, op) == tm.ERR_ARG and L.tiny_actuation_noise_generate(C.byref(spec), 3, 0, op) == tm.ERR_ARG
    assert L.tiny_actuation_noise_generate(C.byref(spec), 3, 2, op) == tm.OK and np.all(out != 0.0)
    spec.flags |= tm.DEVICE
    assert L.tiny_actuation_noise_generate(C.byref(spec), 3, 2, op) == tm.ERR_ARG
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        for name in ("set_actuator", "set_actuator_device", "set_actuator_state", "get_actuator_state", "set_actuation_noise", "generate_actuation_noise", "actuation_log"):
            assert callable(getattr(cls, name)), (cls, name)
    for name in ("get_actuator", "get_actuation_noise", "set_actuation_noise_device", "set_actuator_state_device"):
        assert callable(getattr(tm.TinyBatchSolver, name)), name
    assert callable(tm.actuation_noise_generate)
    for word in ("s = uc < lo[c] ? lo[c] : (uc > hi[c] ? hi[c] : uc)", "m = fma(alpha[c], d, a[c])", "g = fma(m, gain[c], offset[c])", "NULL offset means -0.0",
                 "no addition, not one of zero", "actuation_step", "last_actuator", "actuation_log", "actuator_lag", "actuation_noise_generated",
                 "a controller does not know what its actuator did", "Out of scope: pure transport delays", "adaptive rho does not combine with an actuator model"):
        assert word in header, word


def test_the_reference_rounds_once_per_stage_and_keeps_the_bits_of_an_absent_stage():
    one = lambda u, setup, a=None, row=None, **how: ac.actuate(np.array([u], dtype=float), tuple(None if s is None else np.array([s], dtype=float) for s in setup),
                                                             None if a is None else np.array([a], dtype=float), None if row is None else np.array([row], dtype=float), **how)
    # limits: two comparisons, two selects -- inside them the command's bits, the sign of a zero included; a NaN passes
    assert one(0.5, (0.0, 1.0, None, None, None))[0][0] == 0.5 and one(-3.0, (0.0, 1.0, None, None, None))[0][0] == 0.0 and one(3.0, (0.0, 1.0, None, None, None))[0][0] == 1.0
    z = one(-0.0, (-1.0, 1.0, None, None, None))[0][0]
    assert z == 0.0 and np.signbit(z)
    z = one(-0.0, (0.0, 1.0, None, None, None))[0][0]                   # (-0.0 < 0.0 is false: the command's own zero, not the limit's)
    assert z == 0.0 and np.signbit(z)
    assert np.isnan(one(np.nan, (0.0, 1.0, None, None, None))[0][0])
    # the lag: d is rounded, then ONE fma; a moves
    g = 1.0 + 2.0 ** -30
    ua, a = one(2.0 ** -30, (None, None, g, None, None), a=-1.0)         # (d = 1 + 2^-30 exactly; the product keeps its last bit under the fused addition)
    assert ua[0] == a[0] == 2.0 ** -29 + 2.0 ** -60 != g * g - 1.0
    ua, a = one(1.0, (None, None, 2.0 ** 54, None, None), a=2.0 ** -54)  # (d = fl(1 - 2^-54) = 1: the subtraction is rounded on its own; unrounded, 2^54 - 1 would come out)
    assert ua[0] == a[0] == 2.0 ** 54
    assert one(0.7, (None, None, 1.0, None, None), a=0.7)[0][0] == 0.7   # (alpha = 1 on a record that holds the command: the command)
    # gain and offset: ONE fma -- the product is not rounded first
    g = 1.0 + 2.0 ** -30
    assert one(g, (None, None, None, g, -1.0))[0][0] == 2.0 ** -29 + 2.0 ** -60 != g * g - 1.0
    # the neutral stage returns m's bits for every m: gain 1 and offset -0.0
    for m in (0.0, -0.0, 1.5, -2.0 ** -1074, np.inf):
        got = one(m, (None, None, None, 1.0, None))[0][0]
        assert got == m and np.signbit(got) == np.signbit(m), m
    other = one(-0.0, (None, None, None, 1.0, None), zero_offset=0.0)[0][0]
    assert other == 0.0 and not np.signbit(other)                       # (+0.0 as the default would lose the sign)
    # noise: one addition, and none without a row; alone (no setup) only it runs
    assert one(1.0, (None,) * 5, row=2.0 ** -53)[0][0] == 1.0 and one(1.0, (None,) * 5, row=2.0 ** -52)[0][0] == 1.0 + 2.0 ** -52
    z = one(-0.0, (None,) * 5)[0][0]
    assert np.signbit(z)
    z = one(-0.0, (None,) * 5, row=0.0)[0][0]                            # (an addition of zero is not no addition)
    assert z == 0.0 and not np.signbit(z)
    # the order: limits, lag, gain, noise
    setup = (0.0, 1.0, 0.5, 2.0, 0.25)
    ua, a = one(3.0, setup, a=0.5, row=0.125)
    assert a[0] == 0.75 and ua[0] == 0.75 * 2.0 + 0.25 + 0.125
    assert one(3.0, setup, a=0.5, row=0.125, variant="lag_before_limits")[0][0] == 1.0 * 2.0 + 0.25 + 0.125
    assert one(3.0, setup, a=0.5, row=0.125, variant="noise_before_gain")[0][0] == (0.75 + 0.125) * 2.0 + 0.25
    # an instance whose step ran no iteration: no stage runs, a stays
    uc, s5 = np.array([[3.0], [3.0]]), tuple(np.array([[v], [v]]) for v in setup)
    ua, a = ac.actuate_batch(uc, s5, np.array([[0.5], [0.5]]), None, ran=np.array([True, False]))
    assert ua.tolist() == [[1.75], [3.0]] and a.tolist() == [[0.75], [0.5]]


@pytest.mark.parametrize("name", ac.ALL_CASES)
def test_the_cases_of_the_gpu_tests_meet_their_conditions(name):
    ac.check_case(name)
    assert ac.T == 5 and ac.N_ROWS == 4
    assert [(pc.CASES[n]["shape"], pc.CASES[n]["B"]) for n in ac.ORACLE_CASES] == [((4, 2, 10), 13), ((5, 3, 7), 11), ((12, 4, 10), 2)]
    assert [pc.CASES[n]["shape"] for n in ac.EDGE_CASES] == [(15, 1, 3), (1, 15, 3)]
    assert pc.CASES[ac.COMPOSE_CASE]["shape"] == (6, 3, 10) and pc.CASES[ac.COVER_CASE]["shape"] == (20, 8, 10)


def test_predicting_the_estimate_with_the_applied_control_is_visible():
    ac.check_estimator_case()


# ---- actuator_entry ----------------------------------------------------------------------------------------------------------------------
def test_actuator_entry_against_a_dense_restatement(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    prog = ('#include <hip/hip_runtime.h>\n#include <cstdio>\n#include <vector>\n#include "%s"\nusing namespace tinympc_amd;\n'
            'int main() { if (actuator_block_doubles() != 80) return 1;\n'
            ' for (int nx : {1, 5, 12, 15}) for (int nu : {1, 3, 4, 15}) { if (nx + nu > 16) continue;\n'
            '  std::vector<double> a(5 * nu); for (int i = 0; i < 5 * nu; ++i) a[i] = 1000.0 * nx + 100.0 * nu + i + 0.5;\n'
            '  for (int given = 0; given < 32; ++given) for (int r = 0; r < 5; ++r) for (int lane = 0; lane < 16; ++lane)\n'
            '   printf("%%d %%d %%d %%d %%d %%.17g\\n", nx, nu, given, r, lane, actuator_entry((given & 1) ? a.data() : nullptr, (given & 2) ? a.data() + nu : nullptr,\n'
            '          (given & 4) ? a.data() + 2 * nu : nullptr, (given & 8) ? a.data() + 3 * nu : nullptr, (given & 16) ? a.data() + 4 * nu : nullptr, nx, nu, r, lane)); }\n'
            '  return 0; }\n' % os.path.join(CSRC, "lane_tables.hpp"))
    exe, cpp = str(tmp_path / "actuator"), tmp_path / "actuator.cpp"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, "-x", "hip", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    rows = [ln.split() for ln in subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()]
    shapes = [(nx, nu) for nx in (1, 5, 12, 15) for nu in (1, 3, 4, 15) if nx + nu <= 16]
    assert len(rows) == len(shapes) * 32 * 5 * 16 and (15, 1) in shapes and (1, 15) in shapes
    neutral = (-np.inf, np.inf, 1.0, 1.0, -0.0)
    for nx, nu, given, r, lane, val in rows:
        nx, nu, given, r, lane, val = int(nx), int(nu), int(given), int(r), int(lane), float(val)
        dense = (1000.0 * nx + 100.0 * nu + np.arange(5 * nu) + 0.5).reshape(5, nu)         # lo | hi | alpha | gain | offset over the inputs, as given
        inside = nx <= lane < nx + nu and (given >> r) & 1
        want = dense[r, lane - nx] if inside else neutral[r]
        assert val == want and np.signbit(val) == np.signbit(want), (nx, nu, given, r, lane, val)


# ---- the path and the variant choice ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("actuator_path") / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, os.path.join(ROOT, "tests", "dropin", "actuator_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _lines(exe, mode, stdin=None):
    out = subprocess.run([exe, mode], input=stdin, check=True, capture_output=True, text=True, timeout=1800).stdout.splitlines()
    return [dict(w.split("=", 1) for w in ln.split()) for ln in out]


BOX = dict(fits_box=1, fits=1, actuator=1)
CONE = dict(BOX, soc=1)
LIN = dict(BOX, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1)
FORM_KEYS = ("lin", "pl", "pb", "pc", "pd", "pp", "pm", "pe", "ps", "pa")


def test_path_rules_under_an_actuator(driver):
    # facts -> (kernel, rule, (lin, pl, pb, pc, pd, pp, pm, pe, ps, pa), path code, refusal)
    cases = [
        (BOX, ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),                                     # nothing else installed: the PP form, the model's block
        (dict(BOX, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),  # a compiled-in entry is not asked
        (CONE, ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (LIN, ("ONE_ROW", "one_row:pa", (1, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, hetero=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, state_log=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),               # (the PP form logs: no empty sequence)
        (dict(BOX, disturbance=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 1, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, plant=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, measurement=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 1, 0, 0, 1), 3, 0)),
        (dict(BOX, estimator=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 1, 1, 0, 1), 3, 0)),
        (dict(BOX, score=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 1, 1), 3, 0)),                    # (the score rides on the PP form the fact forces)
        (dict(BOX, estimator=1, measurement=1, plant=1, disturbance=1, state_log=1, score=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 1, 1, 1, 1, 1, 1), 3, 0)),
        # composition with the per-instance rules: their forms take the bits and keep their rule
        (dict(BOX, inst_bounds=1), ("ONE_ROW", "one_row:pb", (0, 0, 1, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(LIN, inst_lin=1), ("ONE_ROW", "one_row:pl", (1, 1, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(CONE, inst_cones=1), ("ONE_ROW", "one_row:pc", (0, 0, 0, 1, 0, 1, 0, 0, 0, 1), 3, 0)),
        # ... and a coverage answer stays coverage; where no PA form can be made: cover:pa
        (dict(CONE, cones_overlap=1), ("COVERAGE", "cones_overlap", (0,) * 10, 2, 0)),
        (dict(BOX, force_general=1), ("COVERAGE", "cover:force_general", (0,) * 10, 2, 0)),
        (dict(BOX, debug=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 0)),
        (dict(BOX, no_jit=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 0)),
        (dict(BOX, variant_jit_failed=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 0)),
        # never the tile kernel while the fact is on: its shapes run on the coverage kernel
        (dict(actuator=1, has_tile=1), ("COVERAGE", "cover:no_register_form", (0,) * 10, 2, 0)),
        (dict(BOX, has_tile=1, prefer_tile=1), ("ONE_ROW", "one_row:pa", (0, 0, 0, 0, 0, 1, 0, 0, 0, 1), 3, 0)),
        (dict(has_tile=1), ("TILE", "tile:no_register_form", (0,) * 10, 1, 0)),
        # adaptive rho: refused with the fact's own value, reported last; what was refused before keeps its value
        (dict(BOX, adaptive=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 12)),
        (dict(BOX, adaptive=1, score=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 11)),
        (dict(BOX, adaptive=1, estimator=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 10)),
        (dict(BOX, adaptive=1, measurement=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 9)),
        (dict(BOX, adaptive=1, state_log=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 8)),
        (dict(BOX, adaptive=1, plant=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 7)),
        (dict(BOX, adaptive=1, disturbance=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 6)),
        (dict(BOX, adaptive=1, inst_bounds=1), ("COVERAGE", "cover:pa", (0,) * 10, 2, 1)),
        # the fact off: the answers without the feature
        (dict(fits_box=1, fits=1), ("ONE_ROW", "one_row:plain", (0,) * 10, 3, 0)),
        (dict(fits_box=1, fits=1, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:plain", (0,) * 10, 0, 0)),
        (dict(fits_box=1, fits=1, adaptive=1), ("ONE_ROW", "one_row:adaptive", (0,) * 10, 3, 0)),
        (dict(fits_box=1, fits=1, score=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 1, 0, 0, 0, 1, 0), 3, 0)),
        (dict(fits_box=1, fits=1, plant=1, score=1), ("ONE_ROW", "one_row:ps", (0, 0, 0, 0, 0, 1, 0, 0, 1, 0), 3, 0)),
        (dict(fits_box=1, fits=1, estimator=1), ("ONE_ROW", "one_row:pe", (0, 0, 0, 0, 0, 1, 1, 1, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, state_log=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1, 0, 0, 0, 0, 0), 3, 0)),
        (dict(fits_box=1, fits=1, score=1, adaptive=1), ("COVERAGE", "cover:ps", (0,) * 10, 2, 11)),
    ]
    stdin = "".join(" ".join("%s=%d" % kv for kv in f.items()) + "\n" for f, _ in cases)
    got = _lines(driver, "path", stdin)
    assert len(got) == len(cases)
    for (f, (kernel, rule, forms, code, refusal)), g in zip(cases, got):
        assert (g["kernel"], g["rule"], int(g["code"]), int(g["refusal"]), g["consistent"]) == (kernel, rule, code, refusal, "1"), (f, g)
        assert tuple(int(g[k]) for k in FORM_KEYS) == forms, (f, g)
    p = subprocess.run([driver, "message"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.splitlines() == [
        "11 adaptive rho does not combine with a closed-loop score (tiny_batch_set_score)",
        "12 adaptive rho does not combine with an actuator model (tiny_batch_set_actuator)"], p.stdout
    # the value behind the score's, and reported last: with the score (or any earlier fact) on as well, the earlier refusal is answered;
    # with the actuator alone its own; with no such fact none
    order = _lines(driver, "path", "".join(" ".join("%s=%d" % kv for kv in dict(fits_box=1, fits=1, adaptive=1, **on).items()) + "\n"
                                           for on in (dict(actuator=1), dict(actuator=1, score=1), dict(actuator=1, score=1, estimator=1), dict(score=1), {})))
    assert [int(g["refusal"]) for g in order] == [12, 11, 10, 11, 0]


def test_path_and_variant_sweeps_follow_the_plants_rule(driver):
    tail = {k: int(v) for r in _lines(driver, "paths") if len(r) == 1 for k, v in r.items()}
    assert tail["violations"] == 0 and tail["tile_with_actuator"] == 0, tail
    assert min(tail["plain"], tail["with_actuator"], tail["one_row_pa"], tail["cover_pa"], tail["refused_12"]) > 1000, tail
    tail = {k: int(v) for r in _lines(driver, "variants") if len(r) == 1 for k, v in r.items()}
    assert tail["with_pa"] > 1000 and tail["violations"] == 0 and tail["key_order"] == 1, tail


def test_the_argument_block_keeps_its_size_and_the_new_fields_lie_in_the_padding_and_over_arho_max(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    fields = ("arho", "est_gain", "aC1", "est_model", "aC2", "score_tab", "atab", "score_rec", "arho_min", "score_step0", "act_step0", "arho_max", "act", "aclip", "ref_shared",
              "pf_mask", "meas", "pf_counter", "dist", "plant", "state_log")
    prog = ('#include <cstdio>\n#include "%s"\nusing tinympc_amd::SolveArgs;\nint main() { printf("%%zu %%zu %%zu", sizeof(SolveArgs), sizeof(tinympc_amd::ScoreRecord), sizeof(tinympc_amd::ActuatorLaunch));\n%s printf("\\n"); return 0; }\n'
            % (os.path.join(CSRC, "admm_kernel.hip.h"), "".join('printf(" %%zu", __builtin_offsetof(SolveArgs, %s));\n' % f for f in fields)))
    exe, cpp = str(tmp_path / "layout"), tmp_path / "layout.hip"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    words = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(w) for w in words] == [472, 24, 40, 304, 304, 328, 328, 336, 336, 344, 344, 352, 352, 356, 360, 360, 368, 372, 416, 416, 432, 440, 456, 464], words
    text = open(os.path.join(CSRC, "admm_kernel.hip.h")).read()
    # the three earlier static_assert lines, verbatim
    assert ('static_assert(sizeof(SolveArgs) == 472 && __builtin_offsetof(SolveArgs, het_tabs) == 208 && __builtin_offsetof(SolveArgs, pf_mask) == 416 &&\n'
            '              __builtin_offsetof(SolveArgs, pf_counter) == 432 && __builtin_offsetof(SolveArgs, pf_base) == 440, "SolveArgs: size and offsets are fixed");') in text
    assert ('static_assert(__builtin_offsetof(SolveArgs, arho) == 304 && __builtin_offsetof(SolveArgs, est_gain) == 304 && __builtin_offsetof(SolveArgs, est_xp) == 312 &&\n'
            '              __builtin_offsetof(SolveArgs, est_log) == 320 && __builtin_offsetof(SolveArgs, est_model) == 328 && __builtin_offsetof(SolveArgs, aC1) == 328 &&\n'
            '              __builtin_offsetof(SolveArgs, aC2) == 336 && __builtin_offsetof(SolveArgs, atab) == 344, "SolveArgs: the estimator\'s pointers share the adaptive-rho ones\' place");') in text
    assert ('static_assert(__builtin_offsetof(SolveArgs, aC2) == 336 && __builtin_offsetof(SolveArgs, score_tab) == 336 && __builtin_offsetof(SolveArgs, atab) == 344 &&\n'
            '              __builtin_offsetof(SolveArgs, score_rec) == 344 && __builtin_offsetof(SolveArgs, arho_min) == 352 && __builtin_offsetof(SolveArgs, score_step0) == 352 &&\n'
            '              __builtin_offsetof(SolveArgs, arho_max) == 360 && __builtin_offsetof(SolveArgs, aclip) == 368, "SolveArgs: the score\'s fields share the adaptive-rho tables\' place");') in text
    assert "__builtin_offsetof(SolveArgs, act_step0) == 356" in text and "__builtin_offsetof(SolveArgs, act) == 360" in text


# ---- the PA forms ------------------------------------------------------------------------------------------------------------------------
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

# the forms whose loops are counted below -- the (12,4,10) box (knot-invariant: UB) and the (6,3,10) cone, on the PP form and on the
# PE + PS form --, (5,3,7) with a disturbance, and a per-instance-data form
PLAIN, FULL = 2 | PP | PA, 2 | PP | PM | PE | PS | PA
PA_VARIANTS = [pa_name(12, 4, 10, mode=PLAIN, ub=True), pa_name(6, 3, 10, soc=True, mode=PLAIN), pa_name(12, 4, 10, mode=FULL, ub=True),
               pa_name(6, 3, 10, soc=True, mode=FULL | PD), pa_name(5, 3, 7, mode=PLAIN | PD, ub=True), pa_name(12, 4, 10, mode=PLAIN, het=True, ub=True)]


def test_pa_variants_compile_and_names_that_violate_the_asserts_are_refused():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    refused = [(pa_name(6, 3, 10, mode=2 | PA), "an actuator model: a form with a plant block (PP, bit 6)"),
               (pa_name(6, 3, 10, mode=2 | PD | PA), "an actuator model: a form with a plant block (PP, bit 6)"),
               (pa_name(6, 3, 10, mode=PLAIN, adapt=True), "not with adaptive rho"),
               (pa_name(4, 2, 10, mode=PLAIN, half=True), "not the half-row form"),
               (pa_name(12, 4, 10, mode=PLAIN, pf=True), "not the prefetch form"),
               (pa_name(6, 3, 10, mode=PLAIN | 2048), "+ 1024: an actuator model")]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PA_VARIANTS + [n for n, _ in refused], capture_output=True, text=True, timeout=3000, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    good, bad = res[:len(PA_VARIANTS)], res[len(PA_VARIANTS):]
    assert [r["name"] for r in good] == PA_VARIANTS
    assert not [r for r in good if "error" in r], [r for r in good if "error" in r]
    assert all(r["bytes"] > 1000 for r in good)
    for r, (_, text) in zip(bad, refused):
        assert "error" in r and text in r["error"], r


# ---- the host generator -----------------------------------------------------------------------------------------------------------------
def test_the_host_generator_of_the_actuation_noise_is_stream_2_of_the_reference_bit_for_bit():
    import tinympc_amd as tm
    rng = np.random.default_rng(77)
    for batch, nu, steps in ((5, 3, 4), (3, 4, 3), (2, 1, 6), (2, 15, 2)):
        scale, mean = rng.uniform(0.1, 2.0, (batch, nu)), rng.normal(0, 1, (batch, nu))
        got = tm.actuation_noise_generate(1234, steps, batch, nu, scale, mean, id_base=7, id_stride=3)
        assert got.shape == (steps, batch, nu)
        assert np.array_equal(got, nr.rows(1234, 2, steps, batch, nu, scale, mean, id_base=7, id_stride=3))
        assert not np.array_equal(got, nr.rows(1234, 0, steps, batch, nu, scale, mean, id_base=7, id_stride=3))      # (not the disturbance's deviates)
        one = tm.actuation_noise_generate(99, steps, batch, nu, scale[0])
        assert np.array_equal(one, nr.rows(99, 2, steps, batch, nu, scale[0]))
    S = rng.normal(0, 1, (4, 4))
    assert np.array_equal(tm.actuation_noise_generate(5, 3, 6, 4, S, factor=True), nr.rows(5, 2, 3, 6, 4, S, factor=True))
    # tiny_noise_generate keeps refusing the stream
    with pytest.raises(tm.TinyMPCError):
        tm.noise_generate(5, 2, 3, 6, 4, np.ones(4))


BOX_T = ("12", "4", "10", "false", "false", "MODE", "0", "false", "4", "false", "true")
CONE_T = ("6", "3", "10", "true", "false", "MODE")


@pytest.mark.parametrize("targs,base", [(BOX_T, 2 | PP), (CONE_T, 2 | PP), (BOX_T, 2 | PP | PM | PE | PS), (CONE_T, 2 | PP | PM | PE | PS)], ids=["box-pp", "cone-pp", "box-pe-ps", "cone-pe-ps"])
def test_the_bit_adds_nothing_to_the_iteration_loop(targs, base, tmp_path):
    """the assembly hipcc emits for the PA form and for the same form without the bit, through tools/isa_loop_stats.py (the fused column
    blocks, as the library is built): the iteration loop holds no FP64, LDS, VMEM or scratch instruction that the form without the bit
    lacks, and it is no longer.  Instruction-mix counts only.
    Seen when this was written (loop instructions; fp64 / lds / scratch among them): box PP 488 -> PP + PA 488 (419 / 0 / 0 both); box
    PE + PS 487 -> 487 (419 / 0 / 0 both); cone PP 730 -> 728, cone PE + PS 729 -> 729 (419 / 74 / 0 all four).  With the actuation log
    stored next to the other stages the cone PE + PS + PA loop had 730 instructions, 420 of them fp64 (a v_cvt_f64_f32 rematerialised
    inside the loop): the entry is stored behind the score instead (profiles/actuator.md, section 2)."""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    spec = importlib.util.spec_from_file_location("isa_loop_stats", os.path.join(ROOT, "tools", "isa_loop_stats.py"))
    ils = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ils)
    loops = {}
    for mode in (base | PA, base):
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
    pa, plain = loops[base | PA], loops[base]
    assert pa.get("scratch", 0) <= plain.get("scratch", 0), (pa, plain)
    for kind in ("fp64", "lds", "vmem"):
        assert pa.get(kind, 0) <= plain.get(kind, 0), (kind, pa, plain)
    assert sum(pa.values()) <= sum(plain.values()), (pa, plain)
