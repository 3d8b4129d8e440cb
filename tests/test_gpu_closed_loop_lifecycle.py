"""GPU tests of what the stages at the fused closed-loop plant step share on ONE handle (csrc/batch_closed_loop.hip, csrc/closed_loop.hpp):
install, remove and reinstall of the disturbance, the plant with the state log, measurement noise, the estimator with the estimate log,
the score and the actuator with its lag, its noise and the actuation log; the model's plant block, which three stages step through; the
counters and log pointers a launch in stretches re-bases.  The per-stage tests (test_gpu_plant.py ... test_gpu_actuator.py) take a fresh
handle per case; here a handle that has been through every stage's install -> remove -> reinstall must be indistinguishable, bit for bit,
from a fresh one given the final data at once.  Shape (6, 3, 10), nine instances (two full waves of four and a tail of one), the problem
of plant_cases' "6_3_10"; the setups are drawn by the case files' own rules around a bare handle's run.  The library is compared with
itself: no tolerance is involved."""
import functools

import numpy as np
import pytest

import actuator_cases as ac
import estimator_cases as ec
import measurement_cases as mc
import plant_cases as pc
import score_cases as scs
import tinympc_amd as tm
from test_gpu_plant import assert_same_bits, snapshot

pytestmark = pytest.mark.gpu
NX, NU, N, B = 6, 3, 10, 9
STEPS = 3
KEYS = pc.KEYS
LAST = ("last_disturbance", "last_plant", "last_measurement_noise", "last_estimator", "last_score", "last_actuator")
COUNTERS = ("disturbance_step", "measurement_step", "score_step", "actuation_step")
INSTALLED = ("disturbance", "plant", "measurement_noise", "estimator", "score", "actuator", "actuator_lag", "actuation_noise")
LOGS = ("state_log", "estimate_log", "actuation_log")


@functools.lru_cache(maxsize=None)
def problem():
    """the first nine instances of plant_cases' 6_3_10"""
    c = pc.case("6_3_10")
    assert (c["nx"], c["nu"], c["N"]) == (NX, NU, N) and c["B"] >= B and not c["hetero"]
    return dict(c, B=B, x0=c["x0"][:B], Xref=c["Xref"][:B], Uref=c["Uref"][:B])


def handle(force_general=False):
    c = problem()
    s = tm.TinyBatchSolver.from_problem(c["fams"][0], B)
    s.set_bound_constraints(*[a[0] for a in c["box"]])
    s.update_settings(max_iter=pc.MAX_ITER, en_state_bound=1, en_input_bound=1)
    s.set_option("force_general", int(force_general))
    start(s)
    return s


def start(s):
    c = problem()
    s.set_x0(c["x0"])
    s.set_x_ref(c["Xref"])
    s.set_u_ref(c["Uref"])


@functools.lru_cache(maxsize=None)
def bare_run():
    """z [B, STEPS, nx + nu] = [state handed on | u0] of a handle with nothing installed: what the score's limits and the actuator's
    setup are drawn around"""
    s = handle()
    out = run(s, STEPS, logs=("state_log",))
    assert [s.get_option(k) for k in LAST] == [0] * 6
    s.close()
    return np.concatenate([np.swapaxes(out["state_log"], 0, 1), np.swapaxes(out["log_u0"], 0, 1)], axis=2)


def stage_data(seed):
    """one draw of every stage's data, by the rules of the case files"""
    c, z, rng = problem(), bare_run(), np.random.default_rng(seed)
    act, n = ac.setup_around(z[:, :, NX:], seed + 5)
    return dict(w=0.1 * rng.uniform(0.5, 1.0, (STEPS, B, NX)) * rng.choice([-1.0, 1.0], (STEPS, B, NX)), plant=pc.plant_for(c, seed),
                v=mc.noise_for(B, NX, seed + 1, STEPS), M=ec.gain_for(B, NX, seed + 2), xp0=ec.estimate_for(c["x0"], seed + 3),
                score=(rng.uniform(0.5, 2.0, (B, NX + NU)), rng.uniform(-0.3, 0.3, (B, NX + NU))) + tuple(scs.limits_around(z, NX, NU, seed + 4)),
                act=act, n=n)


def install(s, d):
    s.set_disturbance(d["w"])
    s.set_plant(*d["plant"])
    s.set_measurement_noise(d["v"])
    s.set_estimator(d["M"])
    s.set_estimate(d["xp0"])
    s.set_score(*d["score"])
    s.set_actuator(*d["act"])
    s.set_actuation_noise(d["n"])
    for k in LOGS:
        s.set_option(k, 1)


def remove(s):
    s.set_disturbance(None)
    s.set_plant(None)
    s.set_measurement_noise(None)
    s.set_estimator(None)
    s.set_score(None)
    s.set_actuator()
    s.set_actuation_noise(None)
    for k in LOGS:
        s.set_option(k, 0)


def run(s, steps, logs=LOGS):
    """one fused launch of `steps` MPC steps -> the step log and the logs asked for"""
    s.set_option("steps_per_launch", steps)
    s.set_option("step_log", 1)
    for k in logs:
        s.set_option(k, 1)
    s.solve()
    it, u0 = s.step_log(steps)
    out = dict(log_iter=it.copy(), log_u0=u0.copy())
    for k in logs:
        out[k] = getattr(s, k)(steps)
    return out


def rewind(s, d):
    """the records, the stages' own state and every counter back to where a fresh handle with the data d starts"""
    s.reset()
    start(s)
    s.set_estimate(d["xp0"])
    s.set_actuator_state(np.zeros((B, NU)))
    s.reset_score()
    for k in ("disturbance_step", "measurement_step", "actuation_step"):
        s.set_option(k, 0)


def state(s):
    """everything a solve call leaves on the handle: x0 and every record, the score record, the estimate, the lag's record, the
    counters and the `last` read-backs"""
    out = snapshot(s, KEYS)
    out.update(zip(("cost", "worst", "violated_steps", "first_violation"), s.get_score()))
    out.update(estimate=s.get_estimate(), lag=s.get_actuator_state(), counters=np.array([s.get_option(k) for k in COUNTERS]),
               last=np.array([s.get_option(k) for k in LAST]))
    return out


def assert_getters(s, d):
    for i in (0, B - 1):
        for got, want in zip(s.get_plant(i), d["plant"]):
            assert np.array_equal(got, want[i]), i
        assert np.array_equal(s.get_estimator(i), d["M"][i]), i
        for got, want in zip(s.get_score_setup(i), d["score"]):
            assert np.array_equal(got, want[i]), i
        for got, want in zip(s.get_actuator(i), d["act"]):
            assert np.array_equal(got, want[i]), i
        for k in range(STEPS):
            assert np.array_equal(s.get_disturbance(k, i), d["w"][k, i]) and np.array_equal(s.get_measurement_noise(k, i), d["v"][k, i]), (k, i)
        for k in range(ac.N_ROWS):
            assert np.array_equal(s.get_actuation_noise(k, i), d["n"][k, i]), (k, i)


def lifecycle(force_general):
    path = "cover" if force_general else "jit"
    first, final = stage_data(1), stage_data(2)
    a = handle(force_general)
    install(a, first)
    run(a, STEPS)                                                    # (discarded: every block has been built and read once)
    assert [a.get_option(k) for k in LAST] == [1] * 6 and a.kernel_path() == path, a.kernel_path()
    # the measurement sequence goes while the estimator and the actuator, which step through the model's block as well, stay
    # -- the model's block they predict and step by is kept: the launch equals a fresh handle's that never had a sequence, bit for bit
    a.set_measurement_noise(None)
    rewind(a, first)
    logs_a = run(a, STEPS)
    got_a = state(a)
    assert [a.get_option(k) for k in LAST] == [1, 1, 0, 1, 1, 1] and a.get_option("measurement_noise") == 0 and a.kernel_path() == path
    c = handle(force_general)
    install(c, dict(first, v=None))
    logs_c = run(c, STEPS)
    assert_same_bits(got_a, state(c), "the measurement sequence removed, estimator and actuator staying, against a handle that never had one")
    assert_same_bits(logs_a, logs_c, "... and their logs")
    assert c.kernel_path() == path and np.any(np.abs(logs_a["log_iter"]) > 1)
    c.close()
    # ... and the plant: the actuator's plant step goes through the model's block itself
    a.set_plant(None)
    run(a, STEPS)
    assert [a.get_option(k) for k in LAST] == [1, 0, 0, 1, 1, 1] and a.kernel_path() == path
    # every stage removed: a launch reads none of them, the logs are gone with their switches
    remove(a)
    assert [a.get_option(k) for k in INSTALLED] == [0] * 8
    run(a, STEPS, logs=())
    assert [a.get_option(k) for k in LAST] == [0] * 6 and a.kernel_path() == ("cover" if force_general else "regs")
    for name in LOGS:
        with pytest.raises(tm.TinyMPCError):
            getattr(a, name)(1)
    for getter in (a.get_score, a.get_estimate, a.get_actuator_state):
        with pytest.raises(tm.TinyMPCError):
            getter()
    # the final data, from the records a fresh handle starts from
    a.reset()
    start(a)
    install(a, final)
    logs_a = run(a, STEPS)
    got_a = state(a)

    b = handle(force_general)
    install(b, final)
    logs_b = run(b, STEPS)
    got_b = state(b)

    assert_same_bits(got_a, got_b, "a handle that went through install -> remove -> reinstall against a fresh one")
    assert_same_bits(logs_a, logs_b, "... and their logs")
    assert np.any(np.abs(logs_a["log_iter"]) > 1), "nothing iterates"
    assert np.max(np.abs(got_a["x"])) < 100.0, "the loop diverges"
    assert list(got_a["last"]) == [1] * 6 and list(got_a["counters"]) == [STEPS] * 4, (got_a["last"], got_a["counters"])
    assert a.kernel_path() == b.kernel_path() == path, (a.kernel_path(), b.kernel_path())
    assert np.any(logs_a["actuation_log"] != logs_a["log_u0"]) and np.any(logs_a["estimate_log"][0] != final["xp0"])
    for s in (a, b):
        assert [s.get_option(k) for k in INSTALLED] == [STEPS, 2, STEPS, 2, 2, 2, 1, ac.N_ROWS]
        assert_getters(s, final)
    a.close()
    b.close()


def test_every_stage_removed_and_reinstalled_leaves_no_trace_on_the_one_row_kernel():
    lifecycle(force_general=False)


def test_every_stage_removed_and_reinstalled_leaves_no_trace_on_the_coverage_kernel():
    lifecycle(force_general=True)


def test_a_launch_in_stretches_takes_every_stage_through_the_rows_of_its_own_steps():
    """steps_per_launch = 5 cut into stretches of two MPC steps (the halves: 8 and 1 instances) against the same launch uncut, every
    stage on: the four counters and the two log pointers a stretch re-bases, the actuation log through the counter.  The sequences are
    shorter than the launch (3 and 4 rows): the last steps take none"""
    steps, final = 5, stage_data(2)
    got = []
    for regroup in (2, 0):
        s = handle()
        install(s, final)
        s.set_option("step_regroup", regroup)
        logs = run(s, steps)
        assert (s.get_option("step_regroup_stretches") > 1) == (regroup > 0) and s.kernel_path() == "jit", (s.get_option("step_regroup_stretches"), s.kernel_path())
        got.append((state(s), logs))
        s.close()
    assert_same_bits(got[0][0], got[1][0], "stretches of two MPC steps against one launch")
    assert_same_bits(got[0][1], got[1][1], "... and their logs")
    assert list(got[0][0]["counters"]) == [steps] * 4 and list(got[0][0]["last"]) == [1] * 6
    assert np.any(np.abs(got[0][1]["log_iter"]) > 1), "nothing iterates"
