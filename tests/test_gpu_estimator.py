"""GPU tests of the fixed-gain state estimator at the plant step of a closed loop (tiny_batch_set_estimator): the one-row kernel's PE forms
and the helper kernels around the coverage kernel.  Cases, gains, initial estimates and oracle loops: tests/estimator_cases.py on the
problems of tests/plant_cases.py under the noise of tests/measurement_cases.py (batches of 13, 11 and 2: the last tile has 1, 3 or 2
rows; T = 5 MPC steps).
  a. every launch form, bit for bit, against the host-in-the-loop form: the same library with nothing installed, per MPC step the Python
     reference correction, set_x0(xhat), one single-step solve, u[:,0] read back, the reference prediction and plant step -- every record,
     the step log, the state log, the estimate log, the final x0 and the final estimate;
  b. every instance against its own oracle loop within the project's 1e-9, iteration counts equal, the edge shapes included;
  c. M = 0, and a perfect start without noise, give the bits of a handle with nothing installed;
  d. composition with a plant and a disturbance, without a noise sequence, per-instance problem data, PB, PL and PC, the coverage path;
  e. two launches of 2 + 3 steps equal one of 5; x[:,0] holds xhat, the state log true states; max_iter = 0; a launch without a plant step;
  f. setters, getters, broadcast, device pointers, replacing the gain, removal, a failed call, reset, the lifecycle; the refusal;
  g. a sharded group;  h. the example.
Every test asserts the kernel path and the read-backs, so that none passes on the wrong path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import disturbance_cases as dc
import estimator_cases as ec
import measurement_cases as mc
import plant_cases as pc
import tinympc_amd as tm
from test_gpu_plant import _hip_runtime, assert_same_bits, make, make_own, rel_err, snapshot

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                        # the project's parity contract (README.md)
T, KEYS = ec.T, ec.KEYS


def assert_applied(s, path, kind=2, noise=T, plant=0):
    """the last solve's launches went through the estimator on the kernel `path` names, on full rows, not in the PREFETCH form"""
    assert (s.get_option("estimator"), s.get_option("last_estimator"), s.get_option("estimate_log")) == (kind, 1, 1)
    assert (s.get_option("measurement_noise"), s.get_option("last_measurement_noise")) == (noise, int(noise != 0))
    assert (s.get_option("plant"), s.get_option("last_plant")) == (plant, int(plant != 0))
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


def install(s, M, xp0, v=None, plant=None, w=None):
    if v is not None:
        s.set_measurement_noise(v)
    if plant is not None:
        s.set_plant(*plant)
    if w is not None:
        s.set_disturbance(w)
    s.set_estimator(M)
    if xp0 is not None:
        s.set_estimate(xp0)
    s.set_option("estimate_log", 1)


def fused(s, steps=T):
    s.set_option("steps_per_launch", steps)
    s.set_option("step_log", 1)
    s.set_option("state_log", 1)
    s.solve()
    it, u0 = s.step_log(steps)
    return dict(log_iter=it.copy(), log_u0=u0.copy(), log_x0=s.state_log(steps), log_xhat=s.estimate_log(steps), estimate=s.get_estimate())


def advance(s, steps=T):
    s.set_option("advance_x0", 1)
    s.set_option("state_log", 1)
    its, u0s, xs, xhs = [], [], [], []
    for _ in range(steps):
        s.solve()
        st = s.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0s.append(s.get("u")[:, :, 0].copy())
        xs.append(s.state_log(1)[0])
        xhs.append(s.estimate_log(1)[0])
    return dict(log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs), log_xhat=np.array(xhs), estimate=s.get_estimate())


def _regroup(streams):
    def drive(s):
        s.set_option("step_regroup", 2)
        s.set_option("step_regroup_streams", streams)
        out = fused(s)
        assert s.get_option("step_regroup_stretches") > 1
        return out
    return drive


def _mode0(s):
    s.set_option("dpp_mode", 0)
    return fused(s)


FORMS = {"fused": fused, "advance_x0": advance, "step_regroup": _regroup(1), "step_regroup_two_streams": _regroup(2), "dpp_mode_0": _mode0}


def host_loop(r, c, M, xp0, v=None, plant=None, w=None, steps=T, keys=KEYS):
    """the host-in-the-loop form on handle r (nothing installed): per MPC step xm = fl(x + v[k]) where the row exists, the reference
    correction, set_x0(xhat), one single-step solve, u[:,0] read back, xp = the reference step of the model from xhat, x = the reference
    plant step of the true x plus the disturbance row, in Python.  Returns the logs, the records after the last solve, the final TRUE
    state as x0 and the final estimate"""
    model = mc.model_of(c)
    plant = plant or model
    x, xp = c["x0"].copy(), np.array(xp0, dtype=float)
    its, u0s, xs, xhs = [], [], [], []
    for k in range(steps):
        xm = x + v[k] if (v is not None and k < len(v)) else x
        xhat = ec.correct_batch(M, xp, xm)
        r.set_x0(xhat)
        r.solve()
        st = r.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0 = r.get("u")[:, :, 0].copy()
        u0s.append(u0)
        xhs.append(xhat)
        xp = pc.plant_step_batch(model, xhat, u0)
        x = pc.plant_step_batch(plant, x, u0)
        if w is not None and k < len(w):
            x = x + w[k]
        xs.append(x)
    out = dict(snapshot(r, keys), log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs), log_xhat=np.array(xhs), estimate=xp)
    out["x0"] = x
    assert (r.get_option("estimator"), r.get_option("last_estimator"), r.get_option("measurement_noise"), r.get_option("plant"), r.get_option("disturbance")) == (0, 0, 0, 0, 0)
    return out


def assert_logs_follow_the_reference(c, run, M, xp0, v, plant=None):
    """every logged estimate is the reference correction of the measurement of the TRUE state under the reference prediction, every logged
    state the reference plant step of the true state before it, from the logged u0, bit for bit (whatever kernel solved)"""
    model = mc.model_of(c)
    x, xp = c["x0"], np.array(xp0, dtype=float)
    for k in range(len(run["log_x0"])):
        xhat = ec.correct_batch(M, xp, x + v[k])
        assert np.array_equal(run["log_xhat"][k], xhat), (k, float(np.max(np.abs(run["log_xhat"][k] - xhat))))
        xp = pc.plant_step_batch(model, xhat, run["log_u0"][k])
        x = pc.plant_step_batch(plant or model, x, run["log_u0"][k])
        assert np.array_equal(run["log_x0"][k], x), (k, float(np.max(np.abs(run["log_x0"][k] - x))))
    assert np.array_equal(run["estimate"], xp)


@functools.lru_cache(maxsize=None)
def host_reference(name, option=None, value=1):
    """the host-in-the-loop run of a case under its gain, noise and perturbed plant, computed once and shared (never modified)"""
    c = pc.case(name)
    r = make(c)
    if option:
        r.set_option(option, value)
    want = host_loop(r, c, ec.gain(name), ec.estimate(name), mc.noise(name), c["plant"])
    r.close()
    return want


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [(n, f) for n in ec.ORACLE_CASES for f in FORMS])
def test_launch_forms_equal_the_host_in_the_loop_form_bit_for_bit(name, form):
    c = pc.case(name)
    s = make(c)
    install(s, ec.gain(name), ec.estimate(name), mc.noise(name), c["plant"])
    run = FORMS[form](s)
    got = dict(snapshot(s), **run)
    assert_applied(s, "jit", plant=2)
    assert s.get_option("measurement_step") == T
    s.close()
    assert_same_bits(got, host_reference(name, "dpp_mode", 0) if form == "dpp_mode_0" else host_reference(name), (name, form))


# ---- b. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.ORACLE_CASES + ec.EDGE_CASES)
def test_every_instance_follows_its_own_oracle_loop(name):
    c, want = pc.case(name), ec.oracle_case(name)
    s = make(c)
    install(s, ec.gain(name), ec.estimate(name), mc.noise(name), c["plant"])
    run = fused(s)
    got = snapshot(s)
    assert_applied(s, "jit", plant=2)
    for i in range(c["B"]):
        assert np.array_equal(run["log_iter"][:, i], want[i]["iter"]), (i, run["log_iter"][:, i], want[i]["iter"])
        for k in KEYS:
            e = rel_err(got[k][i], want[i]["rec"][k])
            assert e < RTOL, (i, k, e)
        assert rel_err(run["log_u0"][:, i], want[i]["u0"]) < RTOL and rel_err(got["x0"][i], want[i]["x0"]) < RTOL, i
        assert rel_err(run["log_x0"][:, i], want[i]["states"]) < RTOL and rel_err(run["log_xhat"][:, i], want[i]["xhat"]) < RTOL, i
        assert rel_err(run["estimate"][i], want[i]["estimate"]) < RTOL, i
    assert np.array_equal(run["log_x0"][-1], got["x0"])
    s.close()


# ---- c. ------------------------------------------------------------------------------------------------------------------------------
def _plain_run(h, steps=T):
    h.set_option("steps_per_launch", steps)
    h.set_option("step_log", 1)
    h.set_option("state_log", 1)
    h.solve()
    out = snapshot(h)
    out["log_iter"], out["log_u0"] = (a.copy() for a in h.step_log(steps))
    out["log_x0"] = h.state_log(steps)
    return out


@pytest.mark.parametrize("name", ["12_4_10", "5_3_7"])
def test_a_zero_gain_and_a_perfect_start_give_the_bits_of_a_handle_with_nothing_installed(name):
    c, v, M = pc.case(name), mc.noise(name), ec.gain(name)
    r = make(c)
    want = _plain_run(r)
    assert (r.get_option("estimator"), r.get_option("last_estimator"), r.get_option("measurement_noise"), r.get_option("plant")) == (0, 0, 0, 0)
    r.close()
    # M = 0 closes the sensor off, whatever noise is installed: xhat and the true state go through the same chain with the same inputs
    for plant in (None, mc.model_of(c)):
        s = make(c)
        install(s, np.zeros_like(M), None, v, plant)                 # (xp = the x0 record as it stands)
        got = _plain_run(s)
        assert_applied(s, "jit", plant=2 if plant else 0)
        assert np.array_equal(s.estimate_log(T)[1:], got["log_x0"][:-1]) and np.array_equal(s.get_estimate(), got["x0"])
        s.close()
        assert_same_bits(got, want, ("M = 0", plant is not None))
    # a perfect start stays perfect: no noise, e = 0 at every step, any finite M
    for gain in (M, 1e6 * M, M[0]):
        s = make(c)
        install(s, gain, c["x0"])
        got = _plain_run(s)
        assert_applied(s, "jit", kind=1 if gain.ndim == 2 else 2, noise=0)
        assert np.array_equal(s.get_estimate(), got["x0"])
        s.close()
        assert_same_bits(got, want, "a perfect start")


# ---- d. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["plant_and_disturbance", "no_noise", "hetero", "instance_box"])
def test_pe_composes(what):
    name = "12_4_10_hetero" if what == "hetero" else "6_3_10"
    c = pc.case(name)
    M, xp0 = ec.gain_for(c["B"], c["nx"], 321), ec.estimate_for(c["x0"], 123)
    v = None if what == "no_noise" else mc.noise(name)
    plant = c["plant"] if "plant" in what else None
    w = c["w"] if "disturbance" in what else None
    s = make(c, own_box=what == "instance_box")
    install(s, M, xp0, v, plant, w)
    run = fused(s)
    got = dict(snapshot(s), **run)
    assert_applied(s, "jit", noise=0 if v is None else T, plant=2 if plant else 0)
    assert s.get_option("last_disturbance") == int(w is not None) and s.get_option("last_instance_bounds") == int(what == "instance_box")
    s.close()
    r = make(c, own_box=what == "instance_box")
    want = host_loop(r, c, M, xp0, v, plant, w)
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0
    assert_same_bits(got, want, what)


@pytest.mark.parametrize("name,own", [("6_3_10_pl", "lin"), ("6_3_10_pc", "cones")])
def test_pe_composes_with_per_instance_halfspaces_and_cone_coefficients(name, own):
    c = dc.case(name)
    assert c["own"] == (own,) and c["path"] == "jit"
    keys = dc.keys(c)
    v = mc.noise_for(c["B"], c["nx"], 4711)
    M, xp0 = ec.gain_for(c["B"], c["nx"], 322), ec.estimate_for(c["x0"], 124)
    s = make_own(c)
    install(s, M, xp0, v)
    run = fused(s)
    got = dict(snapshot(s, keys), **run)
    assert_applied(s, "jit")
    assert (s.get_option("last_instance_linear"), s.get_option("last_instance_cones")) == (int(own == "lin"), int(own == "cones"))
    s.close()
    r = make_own(c)
    want = host_loop(r, c, M, xp0, v, keys=keys)
    assert r.kernel_path() == "jit"
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0      # (something iterates, nothing diverges)
    assert_same_bits(got, want, name)


@pytest.mark.parametrize("name,option", [("5_3_7", "force_general"), ("20_8_10", None)])
def test_the_coverage_path_corrects_and_predicts_the_same_way(name, option):
    c, v = pc.case(name), mc.noise(name)
    M, xp0 = ec.gain(name), ec.estimate(name)
    r = make(c)
    r.set_option("force_general", 1)
    want = host_loop(r, c, M, xp0, v, c["plant"])
    r.close()
    for drive in (fused, advance):
        s = make(c)
        if option:
            s.set_option(option, 1)
        install(s, M, xp0, v, c["plant"])
        run = drive(s)
        got = dict(snapshot(s), **run)
        assert_applied(s, "cover", plant=2)
        s.close()
        assert_same_bits(got, want, (name, drive.__name__))
        assert_logs_follow_the_reference(c, run, M, xp0, v, c["plant"])
    if option:                                                       # where both exist: the PE form's estimates and states obey the same reference, bit for bit
        s = make(c)
        install(s, M, xp0, v, c["plant"])
        run = fused(s)
        assert_applied(s, "jit", plant=2)
        s.close()
        assert_logs_follow_the_reference(c, run, M, xp0, v, c["plant"])


# ---- e. ------------------------------------------------------------------------------------------------------------------------------
def test_two_launches_carry_the_estimate_and_the_logs_hold_what_they_say():
    name = "5_3_7"
    c, v, M, xp0 = pc.case(name), mc.noise(name), ec.gain(name), ec.estimate(name)
    want = host_reference(name)
    s = make(c)
    install(s, M, xp0, v, c["plant"])
    first = fused(s, 2)
    assert_applied(s, "jit", plant=2)
    assert np.array_equal(first["estimate"], pc.plant_step_batch(mc.model_of(c), first["log_xhat"][1], first["log_u0"][1]))
    second = fused(s, 3)
    got = dict(snapshot(s), estimate=second["estimate"], **{k: np.concatenate([first[k], second[k]]) for k in ("log_iter", "log_u0", "log_x0", "log_xhat")})
    assert_same_bits(got, want, "2 + 3 steps")
    # x[:,0] of the last solve is its xhat, not its measurement and not the true state; the state log holds true states
    assert np.array_equal(s.get("x")[:, :, 0], got["log_xhat"][T - 1])
    assert not np.array_equal(got["log_xhat"][T - 1], got["log_x0"][T - 2] + v[T - 1]) and not np.array_equal(got["log_xhat"][T - 1], got["log_x0"][T - 2])
    x = c["x0"]
    for k in range(T):
        x = pc.plant_step_batch(c["plant"], x, got["log_u0"][k])
        assert np.array_equal(got["log_x0"][k], x), k
    assert np.array_equal(s.get("x0"), x)
    # a launch without a plant step reads nothing, leaves the estimate alone and runs the form it runs without an estimator
    s.set_option("steps_per_launch", 1)
    s.set_option("state_log", 0)
    before = s.get_estimate()
    s.solve()
    assert (s.get_option("estimator"), s.get_option("last_estimator"), s.get_option("last_measurement_noise"), s.get_option("measurement_step")) == (2, 0, 0, T)
    assert np.array_equal(s.get_estimate(), before) and np.array_equal(s.get("x0"), x) and np.array_equal(s.get("x")[:, :, 0], x)
    s.close()


def test_a_step_without_an_iteration_shows_xhat_and_keeps_state_and_estimate():
    name = "5_3_7"
    c, v, M, xp0 = pc.case(name), mc.noise(name), ec.gain(name), ec.estimate(name)
    for option, drive, steps in ((None, advance, 2), ("force_general", advance, 2), (None, fused, 3)):
        s = make(c)
        if option:
            s.set_option(option, 1)
        install(s, M, xp0, v)
        s.update_settings(max_iter=0, en_state_bound=1, en_input_bound=1)
        run = drive(s, steps)
        assert_applied(s, "cover" if option else "jit")
        xhat = np.array([ec.correct_batch(M, xp0, c["x0"] + v[k]) for k in range(steps)])
        assert np.array_equal(run["log_xhat"], xhat) and np.array_equal(s.get("x")[:, :, 0], xhat[-1])
        assert np.array_equal(run["log_x0"], np.broadcast_to(c["x0"], run["log_x0"].shape)) and np.array_equal(s.get("x0"), c["x0"])
        assert np.array_equal(run["estimate"], xp0) and s.get_option("measurement_step") == steps
        s.close()


# ---- f. ------------------------------------------------------------------------------------------------------------------------------
def _run(s):
    run = fused(s)
    return dict(snapshot(s), **run)


def test_setters_getters_broadcast_device_pointers_replacing_removal_failed_call_and_reset():
    name = "4_2_10"
    c, v, M, xp0 = pc.case(name), mc.noise(name), ec.gain(name), ec.estimate(name)
    B, nx = c["B"], c["nx"]
    L = tm.lib()
    out = np.zeros(nx * nx)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    s = make(c)
    flat = np.ascontiguousarray(xp0).ravel()
    assert L.tiny_batch_get_estimator(s._h, 0, dp) == tm.ERR_ARG and L.tiny_batch_get_estimate(s._h, dp) == tm.ERR_ARG           # none installed
    assert L.tiny_batch_set_estimate(s._h, flat.ctypes.data_as(C.c_void_p), tm.HOST) == tm.ERR_ARG
    assert L.tiny_batch_get_estimate_log(s._h, dp, 1) == tm.ERR_ARG
    s.set_measurement_noise(v)
    s.set_estimator(M)
    assert s.get_option("estimator") == 2 and np.array_equal(s.get_estimate(), c["x0"])          # installing starts the estimate at the x0 record
    s.set_estimate(xp0)
    s.set_estimator(M[::-1].copy())                                   # replacing the gain keeps xp
    assert np.array_equal(s.get_estimate(), xp0) and np.array_equal(s.get_estimator(2), M[B - 3])
    s.set_estimator(M)
    s.set_option("estimate_log", 1)
    for i in (0, 4, B - 1):
        assert np.array_equal(s.get_estimator(i), M[i])
    for i, p in ((B, dp), (-1, dp), (0, None)):
        assert L.tiny_batch_get_estimator(s._h, i, p) == tm.ERR_ARG
    own = _run(s)
    assert_applied(s, "jit")
    assert L.tiny_batch_get_estimate_log(s._h, dp, T + 1) == tm.ERR_ARG
    # one gain and one estimate for all against the same repeated, from host arrays and from device pointers: the same bits
    one_M, one_xp = M[3], xp0[3]
    hip = _hip_runtime()

    def on_device(a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return p
    runs = []
    for how in ("broadcast", "full", "device", "device_broadcast"):
        h = make(c)
        h.set_measurement_noise(v)
        bc = how.endswith("broadcast")
        if how == "broadcast":
            h.set_estimator(one_M)
            h.set_estimate(one_xp)
        elif how == "full":
            h.set_estimator(np.repeat(one_M[None], B, axis=0))
            h.set_estimate(np.repeat(one_xp[None], B, axis=0))
        else:
            G = one_M.T[None] if bc else np.repeat(one_M.T[None], B, axis=0)                   # (column-major)
            p, q = on_device(G), on_device(one_xp if bc else np.repeat(one_xp[None], B, axis=0))
            h.set_estimator_device(p.value, broadcast=bc)
            assert L.tiny_batch_set_estimate(h._h, q, tm.DEVICE | (tm.BROADCAST if bc else 0)) == tm.OK
            assert hip.hipFree(p) == 0 and hip.hipFree(q) == 0          # (the arrays are copied)
        h.set_option("estimate_log", 1)
        assert np.array_equal(h.get_estimator(B - 1), one_M) and np.array_equal(h.get_estimate()[B - 1], one_xp)
        runs.append(_run(h))
        assert_applied(h, "jit", kind=1 if bc else 2)
        h.close()
    for other in runs[1:]:
        assert_same_bits(other, runs[0], "one gain for all, four ways")
    assert not np.array_equal(runs[0]["x0"], own["x0"])
    # a failed call leaves what was installed
    kept = s.get_estimate()
    s2 = make(c)
    s2.set_estimator(M)
    assert L.tiny_batch_set_estimate(s2._h, None, tm.HOST) == tm.ERR_ARG and np.array_equal(s2.get_estimate(), c["x0"]) and s2.get_option("estimator") == 2
    s2.close()
    # reset keeps gain and estimate: the estimate and the counter put back by hand, the same episode again
    s.set_estimator(M)
    s.reset()
    assert s.get_option("estimator") == 2 and np.array_equal(s.get_estimate(), kept) and np.array_equal(s.get_estimator(1), M[1])
    s.set_estimate(xp0)
    s.set_option("measurement_step", 0)
    s.set_x0(c["x0"])
    assert_same_bits(_run(s), own, "after reset")
    # removal: the estimate record goes with it, the run is the one under measurement noise alone
    s.set_estimator(None)
    assert s.get_option("estimator") == 0 and L.tiny_batch_get_estimate(s._h, dp) == tm.ERR_ARG and L.tiny_batch_get_estimator(s._h, 0, dp) == tm.ERR_ARG
    s.reset()
    s.set_x0(c["x0"])
    s.set_option("measurement_step", 0)
    s.set_option("steps_per_launch", T)
    s.solve()
    assert (s.get_option("last_estimator"), s.get_option("last_measurement_noise")) == (0, 1) and s.kernel_path() == "jit"
    assert not np.array_equal(s.get("x0"), own["x0"])
    s.close()


def test_install_replace_remove_reinstall_equals_a_fresh_handle():
    name = "5_3_7"
    c, v, M, xp0 = pc.case(name), mc.noise(name), ec.gain(name), ec.estimate(name)
    fresh = make(c)
    install(fresh, M, xp0, v)
    want = _run(fresh)
    assert_applied(fresh, "jit")
    fresh.close()
    s = make(c)
    s.set_measurement_noise(v)
    s.set_option("estimate_log", 1)
    for gain in (M[0], M[::-1].copy(), None, M):
        s.reset()
        s.set_x0(c["x0"])
        s.set_option("measurement_step", 0)
        s.set_estimator(gain)
        if gain is not None:
            s.set_estimate(xp0)
        got = _run(s) if gain is not None else None
    assert_applied(s, "jit")
    s.close()
    assert_same_bits(got, want, "install, replace, remove, reinstall")


def test_adaptive_rho_is_refused_on_a_launch_with_a_plant_step_only():
    c = pc.case("6_3_10")
    L = tm.lib()
    q = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    q.update_settings(max_iter=pc.MAX_ITER, en_state_bound=0, en_input_bound=0)
    q.set_x0(c["x0"])
    q.set_estimator(ec.gain_for(c["B"], c["nx"], 321))
    q.set_option("estimate_log", 1)
    q.set_adaptive_rho(1)
    q.solve()                                                        # no plant step: the estimator does not apply, adaptive rho runs
    assert q.get_option("last_estimator") == 0
    q.set_option("advance_x0", 1)
    assert L.tiny_batch_solve(q._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(q._h).decode()
    assert "adaptive rho does not combine with a state estimator (tiny_batch_set_estimator)" in msg, msg
    assert np.array_equal(q.get_estimate(), c["x0"])
    q.set_adaptive_rho(0)
    q.solve()
    assert_applied(q, "jit", noise=0)
    q.close()


# ---- g. ------------------------------------------------------------------------------------------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    c, v = pc.case("6_3_10"), mc.noise("6_3_10")                     # 11 instances: shards of 6 and 5
    M, xp0 = ec.gain_for(c["B"], c["nx"], 321), ec.estimate_for(c["x0"], 123)
    g, s = make(c, group=True), make(c)
    for h in (g, s):
        h.set_measurement_noise(v)
        h.set_estimator(M)
        h.set_estimate(xp0)
        h.set_option("estimate_log", 1)                              # (forwarded to every shard)
        h.set_option("steps_per_launch", 3)
        h.set_option("state_log", 1)
        h.solve()
    st, gst = s.status(), g.status()
    for k in KEYS + ("x0",):
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(gst["iter"], st["iter"]) and np.array_equal(gst["solved"], st["solved"])
    assert np.array_equal(g.state_log(3), s.state_log(3)) and np.array_equal(g.estimate_log(3), s.estimate_log(3))
    assert np.array_equal(g.get_estimate(), s.get_estimate()) and not np.array_equal(s.get_estimate(), xp0)
    assert np.array_equal(g.get_estimator(7), M[7])
    assert_applied(s, "jit", noise=T)
    for k in range(g.shards):
        h = tm.lib().tiny_group_shard(g._h, k)
        opt = lambda n: int(tm.lib().tiny_batch_get_option(h, n))
        assert (opt(b"estimator"), opt(b"last_estimator"), opt(b"estimate_log"), opt(b"last_half_rows"), opt(b"last_prefetch"),
                tm.lib().tiny_batch_kernel_path(h)) == (2, 1, 1, 0, 0, 3)
    # one gain and one estimate for all shards
    g.set_estimator(M[2])
    g.set_estimate(xp0[2])
    assert np.array_equal(g.get_estimator(9), M[2]) and np.array_equal(g.get_estimate(), np.broadcast_to(xp0[2], xp0.shape))
    g.close()
    s.close()


# ---- h. ------------------------------------------------------------------------------------------------------------------------------
def test_output_feedback_example_estimates_better_than_the_raw_readings():
    """examples/output_feedback_closed_loop.c (C99, built by __graft_entry__.build()): double integrators that measure position only,
    every instance its own steady-state Kalman gain, 60 fused steps on a PE form; its estimator line reports a smaller estimation error
    than the raw noise"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "output_feedback_closed_loop")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/output_feedback_closed_loop is missing: __graft_entry__.build() produces it")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "kernel path 3, estimator 2 (applied 1)" in p.stdout and "kernel path 3, estimator 0 (applied 0)" in p.stdout, p.stdout
    err = {ln.split(":")[0]: float(ln.split("RMS estimation error")[1].split(",")[0]) for ln in p.stdout.splitlines() if "RMS estimation error" in ln}
    assert 0.0 < err["estimator"] < err["raw"], err
