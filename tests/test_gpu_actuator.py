"""GPU tests of the actuator model between the command and the plant step (tiny_batch_set_actuator, tiny_batch_set_actuation_noise): the
one-row kernel's PA forms and the helper kernel behind the coverage kernel.  Cases, setups and the reference: tests/actuator_cases.py on
the problems of tests/plant_cases.py (batches of 13, 11 and 2: the last tile has 1, 3 or 2 rows; T = 5 MPC steps).  The yardstick is
never the code under test: the host-in-the-loop run of a handle WITHOUT an actuator -- single solves, the applied control by the Python
reference (actuator_cases.actuate_batch), the reference plant step under it (plant_cases.plant_step_batch), set_x0.
  1. every launch form gives that run bit for bit: records, step log, state log, actuation log, the final a and x0;
  2. every instance against its own ORACLE loop with the reference actuator: within the project's 1e-9, iteration counts equal;
  3. every absent stage leaves the bits alone: the neutral setup, and a lag with alpha = 1 on a record that holds the command;
  4. composition: a disturbance and a score, measurement noise and an estimator (which predicts with the command), per-instance problem
     data, PB, PL, PC;
  5. the coverage path;
  6. noise alone; generated noise; the counter moved; max_iter = 0; a launch without a plant step; setter, getters and their failures; the
     refusal; a sharded group; the example.
Every test asserts the kernel path and the read-backs, so that none passes on the wrong path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import actuator_cases as ac
import disturbance_cases as dc
import estimator_cases as ec
import measurement_cases as mc
import plant_cases as pc
import score_cases as scs
import tinympc_amd as tm
from test_gpu_plant import _hip_runtime, advance, assert_same_bits, fused, make, make_own, rel_err, snapshot

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                        # the project's parity contract (README.md)
T, KEYS = ac.T, pc.KEYS
NONE5 = (None,) * 5


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_run(got, want, what):
    """records and logs bit for bit -- the actuation log and the record a with the sign of their zeros"""
    assert_same_bits(got, want, what)
    for k in ("log_ua", "a"):
        if got.get(k) is not None:
            assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)


def assert_actuated(s, path, kind=2, lag=1, noise=ac.N_ROWS, counter=T):
    """the last solve's launches went through the actuator on the kernel `path` names, on full rows, not in the PREFETCH form"""
    have = tuple(s.get_option(n) for n in ("actuator", "actuator_lag", "actuation_noise", "last_actuator", "actuation_step"))
    assert have == (kind, lag, noise, 1, counter), have
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0
    assert s.get_option("last_plant") == (1 if s.get_option("plant") else 0)


# ---- the drives: every launch form with the actuation log next to the others ---------------------------------------------------------
def fused_a(s, steps=T):
    s.set_option("actuation_log", 1)
    out = dict(fused(s, steps))
    out["log_ua"] = s.actuation_log(steps)
    return out


def advance_a(s, steps=T):
    s.set_option("advance_x0", 1)
    s.set_option("state_log", 1)
    s.set_option("actuation_log", 1)
    its, u0s, xs, uas = [], [], [], []
    for _ in range(steps):
        s.solve()
        st = s.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0s.append(s.get("u")[:, :, 0].copy())
        xs.append(s.state_log(1)[0])
        uas.append(s.actuation_log(1)[0])
    return dict(log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs), log_ua=np.array(uas))


def _regroup(streams):
    def drive(s):
        s.set_option("step_regroup", 2)
        s.set_option("step_regroup_streams", streams)
        out = fused_a(s)
        assert s.get_option("step_regroup_stretches") > 1
        return out
    return drive


def _capped(s):
    s.set_option("grid_waves_per_cu", 1)
    return fused_a(s)


def _two_launches(s):
    a, b = fused_a(s, 2), fused_a(s, 3)
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def _mode0(s):
    s.set_option("dpp_mode", 0)
    return fused_a(s)


FORMS = {"fused": fused_a, "advance_x0": advance_a, "step_regroup": _regroup(1), "step_regroup_two_streams": _regroup(2), "grid_waves_per_cu": _capped,
         "two_plus_three": _two_launches, "dpp_mode_0": _mode0}


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
def host_loop(r, c, plant, setup=NONE5, noise=None, a0=None, w=None, v=None, est=None, steps=T, k0=0):
    """the host-in-the-loop form on handle r (no actuator, no plant, no noise, no estimator installed): `steps` single solves; the
    measurement and the estimator's correction, where there are any, the applied control, the model's prediction from the COMMAND and
    the plant step under the APPLIED control in Python (the references of the case files); set_x0.  setup: five (B, nu) arrays or None;
    noise (rows, B, nu) or None, row k0 + k applies at step k; a0: the record a where a lag is installed (default zeros)"""
    B, nu = c["B"], c["nu"]
    x = r.get("x0")
    a = None if setup[2] is None else (np.zeros((B, nu)) if a0 is None else np.array(a0, dtype=float))
    M, xp = est if est is not None else (None, None)
    model = mc.model_of(c)
    its, u0s, xs, uas, xhs = [], [], [], [], []
    for k in range(steps):
        xm = x + v[k] if (v is not None and k < len(v)) else x
        xs_ = ec.correct_batch(M, xp, xm) if est is not None else xm
        r.set_x0(xs_)
        r.solve()
        st = r.status()
        ran = st["iter"] > 0
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0 = r.get("u")[:, :, 0].copy()
        row = noise[k0 + k] if (noise is not None and 0 <= k0 + k < len(noise)) else None
        ua, a = ac.actuate_batch(u0, setup, a, row, ran)
        if est is not None:
            xp = np.where(ran[:, None], pc.plant_step_batch(model, xs_, u0), xp)
        xn = pc.plant_step_batch(plant, x, ua)
        if w is not None and k < len(w):
            xn = xn + w[k]
        x = np.where(ran[:, None], xn, x)
        u0s.append(u0), xs.append(x.copy()), uas.append(ua), xhs.append(np.array(xs_))
    r.set_x0(x)
    out = dict(log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs), log_ua=np.array(uas))
    extra = dict(a=a, xhat=np.array(xhs), estimate=xp)
    return out, extra


@functools.lru_cache(maxsize=None)
def host_reference(name, option=None, value=1):
    """the host-in-the-loop run of a case under its plant, its actuator and its noise, computed once and shared (never modified)"""
    c = pc.case(name)
    setup, noise = ac.setup(name)
    r = make(c)
    if option:
        r.set_option(option, value)
    run, extra = host_loop(r, c, c["plant"], setup, noise)
    want = dict(run, a=extra["a"])
    want.update(snapshot(r))
    assert (r.get_option("actuator"), r.get_option("last_actuator"), r.get_option("plant"), r.get_option("actuation_noise")) == (0, 0, 0, 0)
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0
    return want


def actuated(name, drive=fused_a, option=None, value=1, before=None):
    """the case on a handle with its plant, its actuator and its noise installed -> (records, logs and a, the handle)"""
    c = pc.case(name)
    setup, noise = ac.setup(name)
    s = make(c)
    if option:
        s.set_option(option, value)
    s.set_plant(*c["plant"])
    s.set_actuator(*setup)
    s.set_actuation_noise(noise)
    if before:
        before(s)
    run = drive(s)
    return dict(snapshot(s), a=s.get_actuator_state(), **run), s


# ---- 1. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [(n, f) for n in ac.ORACLE_CASES for f in FORMS if f != "dpp_mode_0" or n == "4_2_10"])
def test_every_launch_form_equals_the_host_in_the_loop_run_bit_for_bit(name, form):
    want = host_reference(name, "dpp_mode", 0) if form == "dpp_mode_0" else host_reference(name)
    got, s = actuated(name, FORMS[form])
    assert_actuated(s, "jit")
    s.close()
    assert_run(got, want, (name, form))
    assert not np.array_equal(got["log_ua"], got["log_u0"])


# ---- 2. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ac.ORACLE_CASES + ac.EDGE_CASES)
def test_every_instance_follows_its_own_oracle_loop_with_the_reference_actuator(name):
    ac.check_case(name)                                              # (the reference and the oracle alone: before anything runs on the GPU)
    c, want = pc.case(name), ac.oracle_case(name)
    got, s = actuated(name)
    assert_actuated(s, "jit")
    s.close()
    for i in range(c["B"]):
        assert np.array_equal(got["log_iter"][:, i], want[i]["iter"]), (i, got["log_iter"][:, i], want[i]["iter"])
        for k in KEYS:
            e = rel_err(got[k][i], want[i]["rec"][k])
            assert e < RTOL, (i, k, e)
        assert rel_err(got["log_u0"][:, i], want[i]["u0"]) < RTOL and rel_err(got["log_ua"][:, i], want[i]["ua"]) < RTOL, i
        assert rel_err(got["log_x0"][:, i], want[i]["states"]) < RTOL and rel_err(got["x0"][i], want[i]["x0"]) < RTOL and rel_err(got["a"][i], want[i]["a"]) < RTOL, i
    assert np.array_equal(got["log_x0"][-1], got["x0"])


# ---- 3. ------------------------------------------------------------------------------------------------------------------------------
def test_every_absent_stage_leaves_the_bits_alone():
    c = pc.case("12_4_10")
    B, nu = c["B"], c["nu"]
    r = make(c)
    want = dict(fused(r))
    want.update(snapshot(r))
    assert (r.get_option("actuator"), r.get_option("last_actuator"), r.get_option("plant")) == (0, 0, 0) and r.kernel_path() == "jit"      # (the state log alone: a PD form)
    r.close()
    # gain = ones and nothing else, on a handle whose plant is its model: the run with nothing installed
    for kind, gain in ((1, np.ones(nu)), (2, np.ones((B, nu)))):
        s = make(c)
        s.set_actuator(gain=gain)
        got = fused_a(s)
        ua = got.pop("log_ua")
        got.update(snapshot(s))
        assert_actuated(s, "jit", kind=kind, lag=0, noise=0)
        for out, none in zip(s.get_actuator(B - 1), (-np.inf, np.inf, 1.0, 1.0, -0.0)):
            assert np.array_equal(bits(out), bits(np.full(nu, none)))
        s.close()
        assert_same_bits(got, want, ("the neutral setup", kind))
        assert np.array_equal(bits(ua), bits(want["log_u0"]))                 # (the applied control is the command, bit for bit)
    # a lag alone with alpha = 1 on a record that holds the command: d = 0, m = a = the command
    s = make(c)
    s.set_actuator(alpha=np.ones((B, nu)))
    assert np.array_equal(s.get_actuator_state(), np.zeros((B, nu)))          # (installing a lag zeroes the record)
    s.set_actuator_state(want["log_u0"][0])
    got = advance_a(s, 1)
    assert_actuated(s, "jit", lag=1, noise=0, counter=1)
    assert np.array_equal(bits(got["log_ua"][0]), bits(want["log_u0"][0])) and np.array_equal(got["log_x0"][0], want["log_x0"][0])
    assert np.array_equal(bits(s.get_actuator_state()), bits(want["log_u0"][0]))
    s.close()
    # offset NULL is -0.0: an input held at lo = hi = -0.0 keeps its sign through the neutral gain stage
    z = ac.signed_zero_setup("12_4_10")
    s = make(c)
    s.set_actuator(*z)
    got = fused_a(s)
    assert_actuated(s, "jit", lag=0, noise=0)
    s.close()
    assert np.all(got["log_ua"][:, :, 0] == 0.0) and np.all(np.signbit(got["log_ua"][:, :, 0]))
    assert np.array_equal(bits(got["log_ua"][:, :, 1:]), bits(got["log_u0"][:, :, 1:]))


# ---- 4. ------------------------------------------------------------------------------------------------------------------------------
def _compose(build, c, plant, prepare=None, keys=KEYS, path="jit", w=None, v=None, est=None, name=ac.COMPOSE_CASE, hetero_model=False):
    """a handle with the case's actuator and noise (and whatever prepare installs) against the host-in-the-loop run of a bare handle"""
    B = c["B"]
    setup, noise = ac.setup_around(_commands_of(build, c, keys), 4711) if name is None else ac.setup(name)
    r = build()
    run, extra = host_loop(r, c, plant if plant is not None else mc.model_of(c), setup, noise, w=w, v=v, est=est)
    want = dict(run, a=extra["a"])
    want.update(snapshot(r, keys))
    assert r.get_option("actuator") == 0 and r.get_option("last_actuator") == 0
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0      # (something iterates, nothing diverges)
    s = build()
    if plant is not None:
        s.set_plant(*plant)
    if prepare:
        prepare(s)
    s.set_actuator(*setup)
    s.set_actuation_noise(noise)
    got = fused_a(s)
    got.update(snapshot(s, keys), a=s.get_actuator_state())
    assert_actuated(s, path)
    assert_run(got, want, "composition")
    assert np.any(got["log_ua"] != got["log_u0"])
    return s, got, extra, (setup, noise)


def _commands_of(build, c, keys):
    """u0 [B, T, nu] of a bare handle's fused run: what a setup for a case of another case file is drawn around"""
    r = build()
    u0 = fused(r)["log_u0"]
    r.close()
    return np.swapaxes(u0, 0, 1)


def test_pa_composes_with_a_disturbance_and_a_score_whose_u_entries_are_the_applied_control():
    c = pc.case(ac.COMPOSE_CASE)
    setup5, _ = ac.setup(ac.COMPOSE_CASE)
    score = scs.setup(ac.COMPOSE_CASE)

    def prepare(h):
        h.set_disturbance(c["w"])
        h.set_score(*score)
    s, got, _, _ = _compose(lambda: make(c), c, c["plant"], prepare, w=c["w"])
    assert (s.get_option("last_disturbance"), s.get_option("last_score"), s.get_option("score_step")) == (1, 1, T)
    rec = s.get_score()
    s.close()
    ref = scs.score_reference_batch(got["log_x0"], got["log_ua"], score)
    for g, wnt in zip(rec, ref):
        assert g.dtype == wnt.dtype and np.array_equal(g, wnt)
    assert not np.array_equal(scs.score_reference_batch(got["log_x0"], got["log_u0"], score)[0], ref[0])       # (the command would score otherwise)


def test_pa_under_measurement_noise_and_an_estimator_predicts_with_the_command():
    ac.check_estimator_case()
    name = ac.COMPOSE_CASE
    c, v = pc.case(name), mc.noise(name)
    M, xp0 = ec.gain(name), ec.estimate(name)

    def prepare(h):
        h.set_measurement_noise(v)
        h.set_estimator(M)
        h.set_estimate(xp0)
        h.set_option("estimate_log", 1)
    s, got, extra, _ = _compose(lambda: make(c), c, c["plant"], prepare, v=v, est=(M, xp0))
    assert (s.get_option("last_estimator"), s.get_option("last_measurement_noise")) == (1, 1)
    assert np.array_equal(s.estimate_log(T), extra["xhat"]) and np.array_equal(s.get_estimate(), extra["estimate"])
    s.close()


@pytest.mark.parametrize("what", ["hetero", "instance_box"])
def test_pa_composes_with_per_instance_problem_data_and_boxes(what):
    c = pc.case("12_4_10_hetero" if what == "hetero" else "6_3_10")
    build = lambda: make(c, own_box=what == "instance_box")
    s, _, _, _ = _compose(build, c, None, name=None)                 # (no plant installed: the launch forms the model's block, every instance's own)
    assert (s.get_option("plant"), s.get_option("last_instance_bounds")) == (0, int(what == "instance_box"))
    s.close()


@pytest.mark.parametrize("name,own", [("6_3_10_pl", "lin"), ("6_3_10_pc", "cones")])
def test_pa_composes_with_per_instance_halfspaces_and_cone_coefficients(name, own):
    c = dc.case(name)
    assert c["own"] == (own,) and c["path"] == "jit"
    s, _, _, _ = _compose(lambda: make_own(c), c, pc.plant_for(c), keys=dc.keys(c), name=None)
    assert (s.get_option("last_instance_linear"), s.get_option("last_instance_cones")) == (int(own == "lin"), int(own == "cones"))
    s.close()


# ---- 5. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,option", [(ac.COVER_CASE, None), ("5_3_7", "force_general")])
def test_the_coverage_path_actuates_the_same_way(name, option):
    ac.check_case(name)
    want = host_reference(name, option or "force_general")           # (the same kernel on both sides: a bare (20,8,10) handle would take the tile kernel)
    for drive in (fused_a, advance_a):
        got, s = actuated(name, drive, option)
        assert_actuated(s, "cover")
        s.close()
        assert_run(got, want, (name, drive.__name__))


# ---- 6. ------------------------------------------------------------------------------------------------------------------------------
def test_noise_alone_generated_noise_and_a_moved_counter():
    name = "5_3_7"
    c = pc.case(name)
    B, nu = c["B"], c["nu"]
    setup, noise = ac.setup(name)
    # noise alone, with no actuator and no plant: only stage 4 runs
    r = make(c)
    run, _ = host_loop(r, c, mc.model_of(c), NONE5, noise)
    want = dict(run, **snapshot(r))
    r.close()
    s = make(c)
    s.set_actuation_noise(noise)
    got = dict(fused_a(s), **snapshot(s))
    assert_actuated(s, "jit", kind=0, lag=0)
    assert_run(got, want, "noise alone")
    assert np.array_equal(got["log_ua"][:ac.N_ROWS], got["log_u0"][:ac.N_ROWS] + noise) and np.array_equal(bits(got["log_ua"][ac.N_ROWS:]), bits(got["log_u0"][ac.N_ROWS:]))
    for k, i in ((0, 0), (ac.N_ROWS - 1, B - 1)):
        assert np.array_equal(s.get_actuation_noise(k, i), noise[k, i])
    # one sequence for all
    s.set_actuation_noise(noise[:, 3])
    assert np.array_equal(s.get_actuation_noise(2, B - 1), noise[2, 3]) and s.get_option("actuation_step") == 0     # (the setter rewinds)
    s.close()
    # generated on the device: the host generator's rows, and the run under them
    scale = 0.03 * np.ptp(ac.commands(name), axis=1)
    rows = tm.actuation_noise_generate(2024, 6, B, nu, scale, id_base=5, id_stride=2)
    r = make(c)
    run, extra = host_loop(r, c, c["plant"], setup, rows, k0=2)
    want = dict(run, a=extra["a"], **snapshot(r))
    r.close()
    s = make(c)
    s.set_plant(*c["plant"])
    s.set_actuator(*setup)
    s.generate_actuation_noise(2024, 6, scale, id_base=5, id_stride=2)
    assert (s.get_option("actuation_noise"), s.get_option("actuation_noise_generated")) == (6, 1)
    for k, i in ((0, 0), (5, B - 1), (3, 4)):
        assert np.array_equal(s.get_actuation_noise(k, i), rows[k, i])
    s.set_option("actuation_step", 2)                                # the counter moved: rows 2 .. 5, then none
    got = dict(fused_a(s), **snapshot(s), a=s.get_actuator_state())
    assert_actuated(s, "jit", noise=6, counter=2 + T)
    assert_run(got, want, "generated noise from row 2")
    s.set_actuation_noise(noise)                                     # a caller's sequence in its place: no longer generated, rewound
    assert (s.get_option("actuation_noise"), s.get_option("actuation_noise_generated"), s.get_option("actuation_step")) == (ac.N_ROWS, 0, 0)
    s.close()


@pytest.mark.parametrize("option,drive,steps", [(None, fused_a, 3), (None, advance_a, 2), ("force_general", fused_a, 2)])
def test_a_step_without_an_iteration_runs_no_stage_and_the_counter_advances(option, drive, steps):
    name = "5_3_7"
    c = pc.case(name)
    setup, noise = ac.setup(name)
    a0 = 0.1 * setup[0]

    def no_iteration(h):
        h.set_actuator_state(a0)
        h.update_settings(max_iter=0, en_state_bound=1, en_input_bound=1)
    got, s = actuated(name, lambda h: drive(h, steps), option, before=no_iteration)
    path = "cover" if option else "jit"
    assert_actuated(s, path, counter=steps)
    assert np.array_equal(got["x0"], c["x0"]) and np.all(got["log_iter"] == 0) and np.array_equal(got["a"], a0)
    # ... and the steps after it run under the counter's value
    s.update_settings(max_iter=pc.MAX_ITER, en_state_bound=1, en_input_bound=1)
    run = drive(s, 2)
    got = dict(run, **snapshot(s), a=s.get_actuator_state())
    assert_actuated(s, path, counter=steps + 2)
    s.close()
    r = make(c)
    if option:
        r.set_option(option, 1)
    want, extra = host_loop(r, c, c["plant"], setup, noise, a0=a0, steps=2, k0=steps)
    want = dict(want, a=extra["a"], **snapshot(r))
    r.close()
    assert_run(got, want, "after the idle steps")


def test_a_launch_without_a_plant_step_reads_nothing():
    name = "4_2_10"
    c = pc.case(name)
    setup, noise = ac.setup(name)
    r = make(c)
    r.solve()
    want = snapshot(r)
    path = r.kernel_path()
    r.close()
    s = make(c)
    s.set_actuator(*setup)
    s.set_actuation_noise(noise)
    s.solve()
    have = tuple(s.get_option(n) for n in ("actuator", "actuator_lag", "actuation_noise", "last_actuator", "actuation_step"))
    assert have == (2, 1, ac.N_ROWS, 0, 0) and s.kernel_path() == path == "regs"
    assert tm.lib().tiny_batch_kernel_path(s._h) == 0                 # (a compiled-in shape keeps the compiled-in form)
    assert_same_bits(snapshot(s), want, "no plant step")
    assert np.array_equal(s.get_actuator_state(), np.zeros((c["B"], c["nu"])))
    s.close()


def test_setter_getters_broadcast_device_pointers_replacing_removal_failed_calls_and_reset():
    name = "4_2_10"
    c = pc.case(name)
    setup, noise = ac.setup(name)
    B, nu = c["B"], c["nu"]
    L = tm.lib()
    want = host_reference(name)
    dp = np.zeros(B * nu).ctypes.data_as(C.POINTER(C.c_double))
    s = make(c)
    s.set_plant(*c["plant"])
    # nothing installed
    assert L.tiny_batch_get_actuator(s._h, 0, dp, None, None, None, None) == tm.ERR_ARG and L.tiny_batch_get_actuator_state(s._h, dp) == tm.ERR_ARG
    assert L.tiny_batch_set_actuator_state(s._h, dp, tm.HOST) == tm.ERR_ARG and L.tiny_batch_get_actuation_noise(s._h, 0, 0, dp) == tm.ERR_ARG
    assert L.tiny_batch_get_actuation_log(s._h, dp, 1) == tm.ERR_ARG
    s.set_actuator(*setup)
    s.set_actuation_noise(noise)
    for i in (0, 4, B - 1):
        for got, given in zip(s.get_actuator(i), setup):
            assert np.array_equal(got, given[i])
    for i in (B, -1):
        assert L.tiny_batch_get_actuator(s._h, i, dp, None, None, None, None) == tm.ERR_ARG
    assert L.tiny_batch_get_actuator(s._h, 0, None, None, None, None, None) == tm.OK                              # (any output may be null)
    assert L.tiny_batch_get_actuation_noise(s._h, ac.N_ROWS, 0, dp) == tm.ERR_ARG and L.tiny_batch_get_actuation_noise(s._h, 0, B, dp) == tm.ERR_ARG
    got = dict(fused_a(s), **snapshot(s), a=s.get_actuator_state())
    assert_actuated(s, "jit")
    assert_run(got, want, "the episode")
    # failed calls leave what was installed: flags, lo > hi, a short array
    lo, hi = np.ascontiguousarray(setup[0]), np.ascontiguousarray(setup[1])
    assert L.tiny_batch_set_actuator(s._h, lo.ctypes.data_as(C.c_void_p), None, None, None, None, 64) == tm.ERR_ARG and "flags" in L.tiny_batch_last_error(s._h).decode()
    bad = hi.copy()
    bad[B - 1, nu - 1] = lo[B - 1, nu - 1] - 1.0
    assert L.tiny_batch_set_actuator(s._h, lo.ctypes.data_as(C.c_void_p), bad.ctypes.data_as(C.c_void_p), None, None, None, tm.HOST) == tm.ERR_ARG
    assert "lo > hi" in L.tiny_batch_last_error(s._h).decode()
    with pytest.raises(ValueError):
        s.set_actuator(lo=setup[0][:, :-1])
    with pytest.raises(ValueError):
        s.set_actuation_noise(noise[:, :, :-1])
    assert L.tiny_batch_set_actuator_state(s._h, None, tm.HOST) == tm.ERR_ARG
    assert tuple(s.get_option(n) for n in ("actuator", "actuator_lag", "actuation_noise", "actuation_step")) == (2, 1, ac.N_ROWS, T)
    assert np.array_equal(s.get_actuator(2)[1], setup[1][2]) and np.array_equal(bits(s.get_actuator_state()), bits(want["a"]))
    # tiny_batch_reset leaves the setup, the record, the sequence and the counter alone
    s.reset()
    assert tuple(s.get_option(n) for n in ("actuator", "actuator_lag", "actuation_noise", "actuation_step")) == (2, 1, ac.N_ROWS, T)
    assert np.array_equal(bits(s.get_actuator_state()), bits(want["a"])) and np.array_equal(s.get_actuation_noise(1, 2), noise[1, 2])
    # replacing the setup keeps a; the record can be set, for all or per instance; the noise setter rewinds the counter
    s.set_actuator(*[q[::-1].copy() for q in setup])
    assert np.array_equal(bits(s.get_actuator_state()), bits(want["a"])) and np.array_equal(s.get_actuator(0)[3], setup[3][B - 1]) and s.get_option("actuation_step") == T
    s.set_actuator_state(np.arange(nu) + 0.5)
    assert np.array_equal(s.get_actuator_state(), np.repeat((np.arange(nu) + 0.5)[None], B, axis=0))
    s.set_actuator(*setup)
    s.set_actuator_state(np.zeros((B, nu)))
    s.set_actuation_noise(noise)
    assert s.get_option("actuation_step") == 0
    s.set_x0(c["x0"])
    got = dict(fused_a(s), **snapshot(s), a=s.get_actuator_state())
    assert_run(got, want, "the episode again")
    # a setup without alpha drops the lag: no record; with alpha again: a zeroed one
    s.set_actuator(*[q if i != 2 else None for i, q in enumerate(setup)])
    assert (s.get_option("actuator"), s.get_option("actuator_lag")) == (2, 0) and L.tiny_batch_get_actuator_state(s._h, dp) == tm.ERR_ARG
    assert np.array_equal(s.get_actuator(1)[2], np.ones(nu))                                                      # (alpha reads 1.0 with no lag)
    s.set_actuator(*setup)
    assert np.array_equal(s.get_actuator_state(), np.zeros((B, nu)))
    # removal: the run is the one with the noise alone, then with nothing
    s.set_actuator()
    assert (s.get_option("actuator"), s.get_option("actuator_lag"), s.get_option("actuation_noise")) == (0, 0, ac.N_ROWS)
    s.set_actuation_noise(None)
    assert s.get_option("actuation_noise") == 0
    s.reset()
    s.set_x0(c["x0"])
    got = dict(fused(s), **snapshot(s))
    assert s.get_option("last_actuator") == 0 and s.kernel_path() == "jit" and L.tiny_batch_get_actuation_log(s._h, dp, 1) == tm.ERR_ARG
    s.close()
    r = make(c)
    r.set_plant(*c["plant"])
    plain = dict(fused(r), **snapshot(r))
    r.close()
    assert_same_bits(got, plain, "removed")
    # one setup for all against the same repeated, from host arrays and from device pointers: the same run
    one = tuple(q[5] for q in setup)
    full = ac.broadcast(one, B)
    r = make(c)
    run, extra = host_loop(r, c, c["plant"], full, noise)
    want1 = dict(run, a=extra["a"], **snapshot(r))
    r.close()
    hip = _hip_runtime()

    def on_device(a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return p
    for how in ("broadcast", "full", "device", "device_broadcast"):
        h = make(c)
        h.set_plant(*c["plant"])
        bc = how.endswith("broadcast")
        if how == "broadcast":
            h.set_actuator(*one)
            h.set_actuation_noise(noise)
        elif how == "full":
            h.set_actuator(*full)
            h.set_actuation_noise(noise)
        else:
            ps = [on_device(q) for q in (one if bc else full)] + [on_device(noise), on_device(np.zeros(nu if bc else B * nu))]
            h.set_actuator_device(*[p.value for p in ps[:5]], broadcast=bc)
            h.set_actuation_noise_device(ps[5].value, ac.N_ROWS)
            h.set_actuator_state_device(ps[6].value, broadcast=bc)
            for p in ps:
                assert hip.hipFree(p) == 0                             # (the arrays are copied)
        for got, given in zip(h.get_actuator(B - 1), one):
            assert np.array_equal(got, given)
        got = dict(fused_a(h), **snapshot(h), a=h.get_actuator_state())
        assert_actuated(h, "jit", kind=1 if bc else 2)
        assert_run(got, want1, how)
        h.close()


def test_adaptive_rho_is_refused_on_a_launch_with_a_plant_step_only():
    c = pc.case("6_3_10")
    setup, noise = ac.setup("6_3_10")
    L = tm.lib()
    q = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    q.update_settings(max_iter=pc.MAX_ITER, en_state_bound=0, en_input_bound=0)
    q.set_x0(c["x0"])
    q.set_actuator(*setup)
    q.set_adaptive_rho(1)
    q.solve()                                                        # no plant step: the actuator does not apply, adaptive rho runs
    assert q.get_option("last_actuator") == 0
    q.set_option("advance_x0", 1)
    assert L.tiny_batch_solve(q._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(q._h).decode()
    assert "adaptive rho does not combine with an actuator model (tiny_batch_set_actuator)" in msg, msg
    assert q.get_option("actuation_step") == 0 and np.array_equal(q.get_actuator_state(), np.zeros((c["B"], c["nu"])))
    q.set_adaptive_rho(0)
    q.solve()
    assert_actuated(q, "jit", noise=0, counter=1)
    q.close()


def test_group_with_interleaved_shards_equals_the_single_batch():
    name = "6_3_10"
    c = pc.case(name)                                                # 11 instances: shards of 6 and 5
    setup, noise = ac.setup(name)
    B, nu = c["B"], c["nu"]
    scale = 0.03 * np.ptp(ac.commands(name), axis=1)
    g, s = make(c, group=True), make(c)
    for h in (g, s):
        h.set_plant(*c["plant"])
        h.set_actuator(*setup)
        h.set_actuator_state(0.1 * setup[0])
        h.set_actuation_noise(noise)
        h.set_option("actuation_step", 1)                            # (forwarded to every shard)
        h.set_option("actuation_log", 1)
        h.set_option("steps_per_launch", 3)
        h.set_option("state_log", 1)
        h.set_option("step_log", 1)
        h.solve()
    for k in KEYS + ("x0",):
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(g.state_log(3), s.state_log(3)) and np.array_equal(bits(g.actuation_log(3)), bits(s.actuation_log(3)))
    assert np.array_equal(bits(g.get_actuator_state()), bits(s.get_actuator_state()))
    assert_actuated(s, "jit", counter=4)
    r = make(c)
    want, extra = host_loop(r, c, c["plant"], setup, noise, a0=0.1 * setup[0], steps=3, k0=1)
    r.close()
    assert np.array_equal(bits(s.actuation_log(3)), bits(want["log_ua"])) and np.array_equal(s.state_log(3), want["log_x0"])
    for k in range(g.shards):
        h = tm.lib().tiny_group_shard(g._h, k)
        opt = lambda n: int(tm.lib().tiny_batch_get_option(h, n))
        assert (opt(b"actuator"), opt(b"actuator_lag"), opt(b"last_actuator"), opt(b"actuation_step"), opt(b"last_half_rows"), opt(b"last_prefetch"),
                tm.lib().tiny_batch_kernel_path(h)) == (2, 1, 1, 4, 0, 0, 3)
    # generated noise does not depend on the sharding
    for h in (g, s):
        h.generate_actuation_noise(7, 3, scale)
        h.solve()
    assert np.array_equal(bits(g.actuation_log(3)), bits(s.actuation_log(3))) and np.array_equal(g.get("x0"), s.get("x0"))
    # one setup for all shards, and removal
    g.set_actuator(*[q[2] for q in setup])
    h = tm.lib().tiny_group_shard(g._h, 1)
    assert int(tm.lib().tiny_batch_get_option(h, b"actuator")) == 1
    g.set_actuator()
    g.set_actuation_noise(None)
    assert int(tm.lib().tiny_batch_get_option(h, b"actuator")) == 0 and int(tm.lib().tiny_batch_get_option(h, b"actuation_noise")) == 0
    g.close()
    s.close()


def test_the_example_runs_and_its_saturated_instances_score_worse():
    """examples/actuator_closed_loop.c (C99, built by __graft_entry__.build()): a fleet of point masses holding a hover point whose motors
    saturate, lag and lose effectiveness under seeded thrust noise, scored on the device; half of the fleet has limits the loop never
    reaches"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "actuator_closed_loop")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/actuator_closed_loop is missing: __graft_entry__.build() produces it")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "kernel path 3, actuator 2 (lag 1, applied 1, counter 60), score 2 (applied 1)" in p.stdout, p.stdout
    line = {ln.split()[1]: ln.split() for ln in p.stdout.splitlines() if ln.startswith("cost: ")}
    sat, free = float(line["saturated"][-1]), float(line["unsaturated"][-1])
    assert sat > free > 0.0, (sat, free)
    counts = [ln.split() for ln in p.stdout.splitlines() if ln.startswith("saturated steps: ")][0]
    assert int(counts[2]) > 0 and int(counts[-1]) == 0, counts
