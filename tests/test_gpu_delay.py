"""GPU tests of the transport delay in front of the actuator (tiny_batch_set_actuator_delay) and of the predictor that compensates it
(option "delay_compensation"): the one-row kernel's PQ and PX forms and the helper kernels around the coverage kernel.  Cases and the
reference: tests/delay_cases.py on the problems of tests/plant_cases.py (d[i] = i % 4: the four rows of a wave have four delays; batches
of 13, 11 and 2).  The yardstick is never the code under test: the host-in-the-loop run of a bare handle -- single solves; the predictor,
the queue, the actuator, the estimator and the plant step in Python (delay_cases, actuator_cases, plant_cases); set_x0.
  1. every launch form of test_gpu_actuator.FORMS gives that run bit for bit, with and without compensation;
  2. every instance against its own ORACLE loop: within the project's 1e-9, iteration counts equal;
  3. d = 0 everywhere is no delay, compensation without a delay is no compensation, one d for all equals the array;
  4. composition: measurement noise and an estimator (which predicts with what left the queue under compensation, with the command
     without), a disturbance and a score, the actuator's own stages, per-instance boxes, per-instance problem data, PL and PC; the
     coverage path;
  5. a step without an iteration leaves the queue alone; two launches equal one; a launch without a plant step reads nothing;
  6. setters, getters, device pointers, replacing, removal, failed calls, tiny_batch_reset; the refusal;
  7. a sharded group; the example.
Every test asserts the kernel path and the read-backs, so that none passes on the wrong path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import actuator_cases as ac
import delay_cases as dl
import disturbance_cases as dc
import estimator_cases as ec
import measurement_cases as mc
import plant_cases as pc
import score_cases as scs
import tinympc_amd as tm
from test_gpu_actuator import FORMS, advance_a, assert_run, bits, fused_a
from test_gpu_plant import _hip_runtime, assert_same_bits, make, make_own, rel_err, snapshot

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                        # the project's parity contract (README.md)
T, D_MAX, KEYS = dl.T, dl.D_MAX, pc.KEYS
STEPS = ac.T                                       # what the launch forms of test_gpu_actuator drive: 5 MPC steps (2 + 3)
NONE5 = dl.NONE5


def assert_delayed(s, path, counter, compensate, d_max=D_MAX):
    have = tuple(s.get_option(n) for n in ("actuator_delay", "delay_compensation", "last_actuator", "actuation_step"))
    assert have == (d_max, int(compensate), 1, counter), have
    assert s.kernel_path() == path, s.kernel_path()
    assert tm.lib().tiny_batch_kernel_path(s._h) == (3 if path == "jit" else 2)
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
def host_loop(r, c, d, compensate, plant, steps, setup=NONE5, noise=None, w=None, v=None, est=None, q0=None):
    """the host-in-the-loop form on the bare handle r: `steps` single solves from what the predictor makes of the measurement / the
    corrected estimate / x0; the queue, the actuator, the model's prediction and the plant step under the applied control in Python"""
    B, nu = c["B"], c["nu"]
    model = mc.model_of(c)
    x = r.get("x0")
    q = [[np.zeros(nu) for _ in range(d[i])] if q0 is None else [np.array(row) for row in q0[i][:d[i]]] for i in range(B)]
    a = None if setup[2] is None else np.zeros((B, nu))
    M, xp = est if est is not None else (None, None)
    its, u0s, xs, uas, xhs = [], [], [], [], []
    for k in range(steps):
        xm = x + v[k] if (v is not None and k < len(v)) else x
        xin = ec.correct_batch(M, xp, xm) if est is not None else xm
        xsolve = np.array([dl.predict(tuple(m[i] for m in model), xin[i], q[i], int(d[i])) for i in range(B)]) if compensate else xin
        r.set_x0(xsolve)
        r.solve()
        st = r.status()
        ran = st["iter"] > 0
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0 = r.get("u")[:, :, 0].copy()
        s0 = u0.copy()
        for i in range(B):
            if ran[i]:
                s0[i], q[i] = dl.fifo(q[i], int(d[i]), u0[i])
        ua, a = ac.actuate_batch(s0, setup, a, noise[k] if (noise is not None and k < len(noise)) else None, ran)
        if est is not None:
            xp = np.where(ran[:, None], pc.plant_step_batch(model, xin, s0 if compensate else u0), xp)
        xn = pc.plant_step_batch(plant, x, ua)
        if w is not None and k < len(w):
            xn = xn + w[k]
        x = np.where(ran[:, None], xn, x)
        u0s.append(u0), xs.append(x.copy()), uas.append(ua), xhs.append(np.array(xin))
    r.set_x0(x)
    queue = np.zeros((B, D_MAX, nu))
    for i in range(B):
        for t in range(d[i]):
            queue[i, t] = q[i][t]
    out = dict(log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs), log_ua=np.array(uas), queue=queue)
    return out, dict(a=a, xhat=np.array(xhs), estimate=xp)


_REFERENCES = {}


def host_reference(name, compensate, option=None, value=1, steps=STEPS):
    """the host-in-the-loop run of a case under its plant and its delays, computed once and shared (never modified)"""
    key = (name, compensate, option, value, steps)
    if key not in _REFERENCES:
        c = pc.case(name)
        r = make(c)
        if option:
            r.set_option(option, value)
        run, _ = host_loop(r, c, dl.delays(name), compensate, c["plant"], steps)
        want = dict(run, **snapshot(r))
        assert (r.get_option("actuator_delay"), r.get_option("last_actuator"), r.get_option("plant")) == (0, 0, 0)
        r.close()
        assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0
        _REFERENCES[key] = want
    return _REFERENCES[key]


def delayed(name, compensate, drive=fused_a, option=None, value=1, before=None, d=None, d_max=D_MAX):
    """the case on a handle with its plant and its delays installed -> (records, logs and the queue, the handle)"""
    c = pc.case(name)
    s = make(c)
    if option:
        s.set_option(option, value)
    s.set_plant(*c["plant"])
    s.set_actuator_delay(dl.delays(name) if d is None else d, d_max)
    s.set_option("delay_compensation", int(compensate))
    if before:
        before(s)
    run = drive(s)
    return dict(snapshot(s), queue=s.get_actuator_queue(), **run), s


def assert_delay_run(got, want, what):
    assert_run(got, want, what)
    assert np.array_equal(bits(got["queue"]), bits(want["queue"])), (what, "queue")


# ---- 1. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compensate", [False, True])
@pytest.mark.parametrize("name,form", [(n, f) for n in dl.ORACLE_CASES for f in FORMS if f != "dpp_mode_0" or n == "4_2_10"] + [(n, "fused") for n in dl.EDGE_CASES])
def test_every_launch_form_equals_the_host_in_the_loop_run_bit_for_bit(name, form, compensate):
    want = host_reference(name, compensate, "dpp_mode", 0) if form == "dpp_mode_0" else host_reference(name, compensate)
    got, s = delayed(name, compensate, FORMS[form])
    assert_delayed(s, "jit", STEPS, compensate)
    s.close()
    assert_delay_run(got, want, (name, form, compensate))
    assert not np.array_equal(got["log_ua"], got["log_u0"])


# ---- 2. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compensate", [False, True])
@pytest.mark.parametrize("name", dl.ORACLE_CASES + dl.EDGE_CASES)
def test_every_instance_follows_its_own_oracle_loop(name, compensate):
    dl.check_case(name)                                              # (the reference and the oracle alone: before anything runs on the GPU)
    c, want = pc.case(name), dl.oracle_case(name, compensate)
    got, s = delayed(name, compensate, lambda h: fused_a(h, T))
    assert_delayed(s, "jit", T, compensate)
    s.close()
    for i in range(c["B"]):
        assert np.array_equal(got["log_iter"][:, i], want[i]["iter"]), (i, got["log_iter"][:, i], want[i]["iter"])
        for k in KEYS:
            e = rel_err(got[k][i], want[i]["rec"][k])
            assert e < RTOL, (i, k, e)
        assert rel_err(got["log_u0"][:, i], want[i]["u0"]) < RTOL and rel_err(got["log_ua"][:, i], want[i]["ua"]) < RTOL, i
        assert rel_err(got["log_x0"][:, i], want[i]["states"]) < RTOL and rel_err(got["x0"][i], want[i]["x0"]) < RTOL, i
        assert np.max(np.abs(got["queue"][i] - want[i]["queue"])) <= RTOL * max(np.max(np.abs(want[i]["queue"])), 1e-300), i
    assert np.array_equal(got["log_x0"][-1], got["x0"])


# ---- 3. ------------------------------------------------------------------------------------------------------------------------------
def test_no_delay_no_compensation_and_one_delay_for_all():
    name = "4_2_10"
    c = pc.case(name)
    B = c["B"]
    # d = 0 everywhere, with and without compensation: the run with the plant alone plus the actuation log
    r = make(c)
    r.set_plant(*c["plant"])
    r.set_actuation_noise(np.zeros((1, c["nu"])))                    # (a PA launch without a delay: one row that applies at no step below)
    r.set_option("actuation_step", 1)
    want = dict(fused_a(r), **snapshot(r))
    assert r.get_option("actuator_delay") == 0 and r.kernel_path() == "jit"
    # ... and compensation switched on with no delay installed changes nothing
    r.set_x0(c["x0"])
    r.reset()
    r.set_option("delay_compensation", 1)
    again = dict(fused_a(r), **snapshot(r))
    assert r.get_option("delay_compensation") == 1 and r.get_option("actuator_delay") == 0
    r.close()
    assert_run(again, want, "compensation without a delay")
    for compensate in (False, True):
        got, s = delayed(name, compensate, d=np.zeros(B, dtype=np.int32))
        assert_delayed(s, "jit", STEPS, compensate)
        s.close()
        assert np.array_equal(bits(got.pop("queue")), bits(np.zeros((B, D_MAX, c["nu"]))))
        assert_run(got, want, ("d = 0", compensate))
        assert np.array_equal(bits(got["log_ua"]), bits(got["log_u0"]))
    # one d for all (TINY_BROADCAST) equals the array of equal entries
    for compensate in (False, True):
        one, s = delayed(name, compensate, d=2)
        assert_delayed(s, "jit", STEPS, compensate)
        assert [s.get_actuator_delay(i) for i in (0, B - 1)] == [2, 2]
        s.close()
        arr, s = delayed(name, compensate, d=np.full(B, 2, dtype=np.int32))
        s.close()
        assert_delay_run(one, arr, ("broadcast", compensate))
        assert np.all(one["log_ua"][:2] == 0.0) and np.array_equal(bits(one["log_ua"][2:]), bits(one["log_u0"][:-2]))


# ---- 4. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compensate", [False, True])
@pytest.mark.parametrize("option,path", [(None, "jit"), ("force_general", "cover")])
def test_under_measurement_noise_and_an_estimator_the_model_predicts_with_what_left_the_queue(option, path, compensate):
    dl.check_estimator_case()
    name = dl.COMPOSE_CASE
    c, d = pc.case(name), dl.delays(name)
    v, M, xp0 = dl.estimator_inputs(name)
    r = make(c)
    if option:
        r.set_option(option, 1)                                      # (the same kernel on both sides)
    want, extra = host_loop(r, c, d, compensate, c["plant"], STEPS, v=v, est=(M, xp0))
    want.update(snapshot(r))
    r.close()

    def prepare(h):
        h.set_measurement_noise(v)
        h.set_estimator(M)
        h.set_estimate(xp0)
        h.set_option("estimate_log", 1)
    got, s = delayed(name, compensate, option=option, before=prepare)
    assert_delayed(s, path, STEPS, compensate)
    assert (s.get_option("last_estimator"), s.get_option("last_measurement_noise")) == (1, 1)
    log, estimate = s.estimate_log(STEPS), s.get_estimate()
    s.close()
    assert_delay_run(got, want, ("estimator", compensate, path))
    assert np.array_equal(log, extra["xhat"]), "the estimate log keeps xhat"
    assert np.array_equal(estimate, extra["estimate"]), "the predicted estimate"


@pytest.mark.parametrize("compensate", [False, True])
def test_composes_with_the_actuator_a_disturbance_a_score_and_per_instance_boxes(compensate):
    name = dl.COMPOSE_CASE
    c, d = pc.case(name), dl.delays(name)
    setup, noise = ac.setup(name)
    score = scs.setup(name)
    r = make(c, own_box=True)
    want, extra = host_loop(r, c, d, compensate, c["plant"], STEPS, setup=setup, noise=noise, w=c["w"])
    want.update(snapshot(r), a=extra["a"])
    r.close()
    s = make(c, own_box=True)
    s.set_plant(*c["plant"])
    s.set_actuator(*setup)
    s.set_actuation_noise(noise)
    s.set_disturbance(c["w"])
    s.set_score(*score)
    s.set_actuator_delay(d, D_MAX)
    s.set_option("delay_compensation", int(compensate))
    got = dict(fused_a(s), **snapshot(s), a=s.get_actuator_state(), queue=s.get_actuator_queue())
    assert_delayed(s, "jit", STEPS, compensate)
    assert (s.get_option("last_disturbance"), s.get_option("last_score"), s.get_option("last_instance_bounds"), s.get_option("actuator_lag")) == (1, 1, 1, 1)
    rec = s.get_score()
    s.close()
    assert_delay_run(got, want, ("composition", compensate))
    for g, wnt in zip(rec, scs.score_reference_batch(got["log_x0"], got["log_ua"], score)):      # (z uses the applied control)
        assert g.dtype == wnt.dtype and np.array_equal(g, wnt)


def _compose(build, c, plant, compensate, keys=KEYS):
    """a handle of another case file with d = i % 4 (and whatever build installs) against the host-in-the-loop run of the same handle
    kind with no delay; plant None: none installed, the launch steps by the model's own block"""
    d = (np.arange(c["B"]) % 4).astype(np.int32)
    r = build()
    want, _ = host_loop(r, c, d, compensate, plant if plant is not None else mc.model_of(c), STEPS)
    want.update(snapshot(r, keys))
    assert r.get_option("actuator_delay") == 0 and r.get_option("last_actuator") == 0
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0       # (something iterates, nothing diverges)
    s = build()
    if plant is not None:
        s.set_plant(*plant)
    s.set_actuator_delay(d, D_MAX)
    s.set_option("delay_compensation", int(compensate))
    got = dict(fused_a(s), **snapshot(s, keys), queue=s.get_actuator_queue())
    assert_delayed(s, "jit", STEPS, compensate)
    assert_delay_run(got, want, "composition")
    assert np.any(got["log_ua"] != got["log_u0"])
    return s


@pytest.mark.parametrize("compensate", [False, True])
def test_composes_with_per_instance_problem_data(compensate):
    c = pc.case("12_4_10_hetero")
    s = _compose(lambda: make(c), c, None, compensate)               # (no plant installed: every instance's own model block steps and predicts)
    assert s.get_option("plant") == 0
    s.close()


@pytest.mark.parametrize("compensate", [False, True])
@pytest.mark.parametrize("name,own", [("6_3_10_pl", "lin"), ("6_3_10_pc", "cones")])
def test_composes_with_per_instance_halfspaces_and_cone_coefficients(name, own, compensate):
    c = dc.case(name)
    assert c["own"] == (own,) and c["path"] == "jit"
    s = _compose(lambda: make_own(c), c, pc.plant_for(c), compensate, keys=dc.keys(c))
    assert (s.get_option("last_instance_linear"), s.get_option("last_instance_cones")) == (int(own == "lin"), int(own == "cones"))
    s.close()


@pytest.mark.parametrize("compensate", [False, True])
@pytest.mark.parametrize("name,option", [(dl.COVER_CASE, None), ("5_3_7", "force_general")])
def test_the_coverage_path_gives_the_same_bits(name, option, compensate):
    dl.check_case(name)
    want = host_reference(name, compensate, option or "force_general")      # (the same kernel on both sides: a bare (20,8,10) handle would take the tile kernel)
    for drive in (fused_a, advance_a):
        got, s = delayed(name, compensate, drive, option)
        assert_delayed(s, "cover", STEPS, compensate)
        s.close()
        assert_delay_run(got, want, (name, drive.__name__, compensate))


# ---- 5. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option", [None, "force_general"])
def test_a_step_without_an_iteration_leaves_the_queue_alone_and_two_launches_equal_one(option):
    name = "5_3_7"
    c, d = pc.case(name), dl.delays(name)
    rng = np.random.default_rng(5)
    q0 = rng.uniform(-0.2, 0.2, (c["B"], D_MAX, c["nu"]))
    kept = np.where(np.arange(D_MAX)[None, :, None] < d[:, None, None], q0, 0.0)      # (+0.0 behind an instance's first d rows)

    def idle(h):
        h.set_actuator_queue(q0)
        h.update_settings(max_iter=0, en_state_bound=1, en_input_bound=1)
    got, s = delayed(name, True, lambda h: fused_a(h, 2), option, before=idle)
    assert_delayed(s, "cover" if option else "jit", 2, True)
    assert np.array_equal(got["x0"], c["x0"]) and np.all(got["log_iter"] == 0) and np.array_equal(bits(got["queue"]), bits(kept))
    # ... and the steps behind them start from that queue: 2 + 3 steps in two launches
    s.update_settings(max_iter=pc.MAX_ITER, en_state_bound=1, en_input_bound=1)
    a, b = fused_a(s, 2), fused_a(s, 3)
    got = {k: np.concatenate([a[k], b[k]]) for k in a}
    got.update(snapshot(s), queue=s.get_actuator_queue())
    s.close()
    r = make(c)
    if option:
        r.set_option(option, 1)
    want, _ = host_loop(r, c, d, True, c["plant"], 5, q0=q0)
    want.update(snapshot(r))
    r.close()
    assert_delay_run(got, want, "after the idle steps")


def test_a_launch_without_a_plant_step_reads_nothing():
    name = "4_2_10"
    c = pc.case(name)
    r = make(c)
    r.solve()
    want = snapshot(r)
    r.close()
    s = make(c)
    s.set_actuator_delay(dl.delays(name), D_MAX)
    s.set_option("delay_compensation", 1)
    q0 = np.full((c["B"], D_MAX, c["nu"]), 0.25)
    s.set_actuator_queue(q0[0])                                      # (one slice for all)
    s.solve()
    have = tuple(s.get_option(n) for n in ("actuator_delay", "last_actuator", "actuation_step"))
    assert have == (D_MAX, 0, 0) and s.kernel_path() == "regs" and tm.lib().tiny_batch_kernel_path(s._h) == 0
    assert_same_bits(snapshot(s), want, "no plant step")
    d = dl.delays(name)
    assert np.array_equal(s.get_actuator_queue(), np.where(np.arange(D_MAX)[None, :, None] < d[:, None, None], q0, 0.0))
    s.close()


# ---- 6. ------------------------------------------------------------------------------------------------------------------------------
def test_setters_getters_device_pointers_replacing_removal_failed_calls_and_reset():
    name = "5_3_7"
    c, d = pc.case(name), dl.delays(name)
    B, nu = c["B"], c["nu"]
    L = tm.lib()
    s = make(c)
    ip = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros((B, D_MAX, nu))
    one = C.c_int(-1)
    # nothing installed: the queue's setter and getter and the delay's getter refuse
    assert L.tiny_batch_set_actuator_queue(s._h, ip(out), tm.HOST) == tm.ERR_ARG and L.tiny_batch_get_actuator_queue(s._h, out.ctypes.data_as(C.POINTER(C.c_double))) == tm.ERR_ARG
    assert L.tiny_batch_get_actuator_delay(s._h, 0, C.byref(one)) == tm.ERR_ARG and s.get_option("actuator_delay") == 0
    assert L.tiny_batch_set_actuator_delay(None, None, 0, tm.HOST) == tm.ERR_NULL
    # refused arguments leave the handle as it was
    bad = d.copy()
    bad[B - 1] = D_MAX + 1
    for arr, dm, flags in ((bad, D_MAX, tm.HOST), (d, tm.MAX_DELAY + 1, tm.HOST), (-np.ones(B, dtype=np.int32), D_MAX, tm.HOST), (d, D_MAX, 4)):
        assert L.tiny_batch_set_actuator_delay(s._h, ip(arr), dm, flags) == tm.ERR_ARG
        assert s.get_option("actuator_delay") == 0
    s.set_actuator_delay(d, D_MAX)
    assert s.get_option("actuator_delay") == D_MAX and [s.get_actuator_delay(i) for i in range(B)] == d.tolist()
    assert np.array_equal(bits(s.get_actuator_queue()), bits(np.zeros((B, D_MAX, nu))))        # (+0.0)
    rng = np.random.default_rng(11)
    q0 = rng.uniform(-1, 1, (B, D_MAX, nu))
    mask = np.arange(D_MAX)[None, :, None] < d[:, None, None]
    s.set_actuator_queue(q0)
    assert np.array_equal(s.get_actuator_queue(), np.where(mask, q0, 0.0))
    assert L.tiny_batch_set_actuator_delay(s._h, ip(bad), D_MAX, tm.HOST) == tm.ERR_ARG          # (a failed call: delay and queue stay)
    assert L.tiny_batch_set_actuator_queue(s._h, None, tm.HOST) == tm.ERR_ARG and L.tiny_batch_get_actuator_delay(s._h, B, C.byref(one)) == tm.ERR_ARG
    assert np.array_equal(s.get_actuator_queue(), np.where(mask, q0, 0.0)) and s.get_actuator_delay(B - 1) == int(d[B - 1])
    # the actuator's own life cycle and tiny_batch_reset leave delay and queue alone
    s.set_actuator(alpha=np.full(nu, 0.5))
    s.set_actuator()
    s.reset()
    assert np.array_equal(s.get_actuator_queue(), np.where(mask, q0, 0.0)) and s.get_option("actuator_delay") == D_MAX
    # device pointers
    hip = _hip_runtime()
    dev_d, dev_q = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dev_d), C.c_size_t(B * 4)) == 0 and hip.hipMalloc(C.byref(dev_q), C.c_size_t(q0.nbytes)) == 0
    d2 = ((d + 1) % 3).astype(np.int32)
    q2 = np.ascontiguousarray(-q0)
    assert hip.hipMemcpy(dev_d, ip(d2), C.c_size_t(B * 4), 1) == 0 and hip.hipMemcpy(dev_q, ip(q2), C.c_size_t(q2.nbytes), 1) == 0
    s.set_actuator_delay_device(dev_d.value, 2)
    assert s.get_option("actuator_delay") == 2 and [s.get_actuator_delay(i) for i in range(B)] == d2.tolist()
    assert np.array_equal(bits(s.get_actuator_queue()), bits(np.zeros((B, 2, nu))))              # (replacing zeroes the queue)
    s.set_actuator_queue_device(dev_q.value, broadcast=True)                                      # (the first [2][nu] doubles, for all)
    first = q2.reshape(-1)[:2 * nu].reshape(2, nu)
    assert np.array_equal(s.get_actuator_queue(), np.where(np.arange(2)[None, :, None] < d2[:, None, None], first[None], 0.0))
    assert hip.hipFree(dev_d) == 0 and hip.hipFree(dev_q) == 0
    # removal
    s.set_actuator_delay(None)
    assert s.get_option("actuator_delay") == 0 and L.tiny_batch_get_actuator_queue(s._h, out.ctypes.data_as(C.POINTER(C.c_double))) == tm.ERR_ARG
    s.close()


def test_adaptive_rho_is_refused_with_the_actuators_text_on_a_launch_with_a_plant_step_only():
    c = pc.case("6_3_10")
    L = tm.lib()
    q = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    q.update_settings(max_iter=pc.MAX_ITER, en_state_bound=0, en_input_bound=0)
    q.set_x0(c["x0"])
    q.set_actuator_delay(dl.delays("6_3_10"), D_MAX)
    q.set_option("delay_compensation", 1)
    q.set_adaptive_rho(1)
    q.solve()                                                        # no plant step: the delay does not apply, adaptive rho runs
    assert q.get_option("last_actuator") == 0
    q.set_option("advance_x0", 1)
    assert L.tiny_batch_solve(q._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(q._h).decode()
    assert "adaptive rho does not combine with an actuator model (tiny_batch_set_actuator)" in msg, msg
    assert q.get_option("actuation_step") == 0 and not np.any(q.get_actuator_queue())
    q.set_adaptive_rho(0)
    q.solve()
    assert_delayed(q, "jit", 1, True)
    q.close()


# ---- 7. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compensate", [False, True])
def test_group_with_interleaved_shards_equals_the_single_batch(compensate):
    name = "6_3_10"
    c, d = pc.case(name), dl.delays(name)                            # 11 instances: shards of 6 and 5
    rng = np.random.default_rng(3)
    q0 = rng.uniform(-0.1, 0.1, (c["B"], D_MAX, c["nu"]))
    g, s = make(c, group=True), make(c)
    for h in (g, s):
        h.set_plant(*c["plant"])
        h.set_actuator_delay(d, D_MAX)
        h.set_actuator_queue(q0)
        h.set_option("delay_compensation", int(compensate))          # (forwarded to every shard)
        h.set_option("actuation_log", 1)
        h.set_option("steps_per_launch", 3)
        h.set_option("state_log", 1)
        h.solve()
    for k in KEYS + ("x0",):
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(g.state_log(3), s.state_log(3)) and np.array_equal(bits(g.actuation_log(3)), bits(s.actuation_log(3)))
    assert np.array_equal(bits(g.get_actuator_queue()), bits(s.get_actuator_queue()))
    assert_delayed(s, "jit", 3, compensate)
    r = make(c)
    want, _ = host_loop(r, c, d, compensate, c["plant"], 3, q0=q0)
    r.close()
    assert np.array_equal(bits(s.actuation_log(3)), bits(want["log_ua"])) and np.array_equal(s.state_log(3), want["log_x0"])
    assert np.array_equal(bits(s.get_actuator_queue()), bits(want["queue"]))
    for k in range(g.shards):
        h = tm.lib().tiny_group_shard(g._h, k)
        opt = lambda n: int(tm.lib().tiny_batch_get_option(h, n))
        assert (opt(b"actuator_delay"), opt(b"delay_compensation"), opt(b"last_actuator"), tm.lib().tiny_batch_kernel_path(h)) == (D_MAX, int(compensate), 1, 3)
    # a value out of range in the LAST shard's part: the whole call is refused before any shard is touched
    bad = d.copy()
    bad[c["B"] - 1] = D_MAX + 1
    before = g.get_actuator_queue()
    assert tm.lib().tiny_group_set_actuator_delay(g._h, bad.ctypes.data_as(C.POINTER(C.c_int)), D_MAX, tm.HOST) == tm.ERR_ARG
    assert tm.lib().tiny_group_set_actuator_delay(g._h, d.ctypes.data_as(C.POINTER(C.c_int)), tm.MAX_DELAY + 1, tm.HOST) == tm.ERR_ARG
    assert np.array_equal(bits(g.get_actuator_queue()), bits(before)) and np.any(before != 0.0)
    g.set_actuator_delay(1)                                          # (one for all shards, and removal)
    h = tm.lib().tiny_group_shard(g._h, 1)
    assert int(tm.lib().tiny_batch_get_option(h, b"actuator_delay")) == 1
    g.set_actuator_delay(None)
    assert int(tm.lib().tiny_batch_get_option(h, b"actuator_delay")) == 0
    g.close()
    s.close()


def test_the_example_runs_and_its_compensated_fleet_scores_no_worse_on_every_delayed_instance():
    """examples/delayed_closed_loop.c (C99, built by __graft_entry__.build()): one fleet of point masses under a stiff controller, delays
    0 .. 3, flown with and without the predictor and scored on the device"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "delayed_closed_loop")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/delayed_closed_loop is missing: __graft_entry__.build() produces it")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    for flight in (0, 1):
        assert "flight %d: 4096 instances x 60 MPC steps in one launch, kernel path 3, delay 3, compensation %d, applied 1" % (flight, flight) in p.stdout, p.stdout
    assert "delayed instances that score worse with the predictor: 0; undelayed instances it moves: 0" in p.stdout, p.stdout
    cost = {int(ln.split()[2]): (float(ln.split()[5]), float(ln.split()[-1])) for ln in p.stdout.splitlines() if ln.startswith("cost: delay ")}
    assert sorted(cost) == [0, 1, 2, 3] and cost[0][0] == cost[0][1] > 0.0
    assert all(cost[k][1] < cost[k][0] for k in (1, 2, 3)), cost      # (every instance of a delay flies the same flight: the means are theirs)
    assert cost[1][0] < cost[2][0] < cost[3][0], cost                 # (the longer the delay, the more it costs)
