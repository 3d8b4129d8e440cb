"""The reference and the oracle-side conditions of tests/test_gpu_delay.py and tests/test_delay_cpu.py (CPU only; computed once per case
and shared): the transport delay in front of the actuator (tiny_batch_set_actuator_delay) and the predictor that compensates it (option
"delay_compensation"), restated in plain Python on the references of actuator_cases and plant_cases.  For one instance with delay d and
queue q (a list of its last d commands, oldest first), command uc:

    0. delay:   d == 0: s0 = uc (its own bits).  d > 0: s0 = q[0]; q = q[1:] + [uc]
    1. - 4.     actuator_cases.actuate over s0
    predictor:  xs = xin;  for t = 0 .. d-1: xs = plant_cases.plant_step(MODEL, xs, q[t])     -- q as it stands BEFORE this step's push

Cases: those of actuator_cases.ALL_CASES under the case's perturbed plant, T = 8 MPC steps, d[i] = i % 4, d_max = 3, a zero queue, no
other stage installed.  check_case asserts, from the reference and the oracle loops alone, the conditions the users of this module rely
on: every loop stays bounded, everything iterates, the delay and the compensation are visible, and so is every misreading."""
import functools

import numpy as np

import actuator_cases as ac
import estimator_cases as ec
import instance_cone_cases as icc
import measurement_cases as mc
import plant_cases as pc
import scenarios as sc
from cpu_solvers import OracleSolver

T = 8
D_MAX = 3
ALL_CASES = ac.ALL_CASES
ORACLE_CASES, EDGE_CASES, COMPOSE_CASE, COVER_CASE = ac.ORACLE_CASES, ac.EDGE_CASES, ac.COMPOSE_CASE, ac.COVER_CASE
NONE5 = (None,) * 5
# push before pop: the command enters first, so the delay is d - 1; the predictor reads the queue newest first; it steps with the
# installed plant instead of the model; it reads the queue as a push would leave it (the oldest entry gone, the newest standing in for
# the command not yet computed)
MISREADINGS = ("push_before_pop", "newest_first", "predict_with_plant", "queue_after_push")
ESTIMATOR_MISREADING = "estimator_predicts_with_uc"


def delays(name):
    """d [B]: i % 4"""
    return (np.arange(pc.case(name)["B"]) % 4).astype(np.int32)


def fifo(q, d, uc, variant=None):
    """stage 0 of ONE instance: q the list of its last d commands, oldest first -> (s0, the new q)"""
    uc = np.array(uc, dtype=float)
    if d == 0:
        return uc, []
    after = list(q[1:]) + [uc]
    if variant == "push_before_pop":
        return (after[0] if d > 1 else uc).copy(), after
    return np.array(q[0], dtype=float), after


def predict(model_i, xin, q, d, variant=None, plant_i=None):
    """the predictor of ONE instance: xin stepped d times by the model over the queue, oldest first"""
    A, Bm, f = plant_i if variant == "predict_with_plant" else model_i
    rows = list(q[:d])
    if variant == "newest_first":
        rows = rows[::-1]
    if variant == "queue_after_push" and d > 0:
        rows = rows[1:] + [rows[-1]]
    xs = np.array(xin, dtype=float)
    for t in range(d):
        xs = pc.plant_step(A, Bm, f, xs, rows[t])
    return xs


def zero_queue(name):
    c = pc.case(name)
    return np.zeros((c["B"], D_MAX, c["nu"]))


def delay_loop(c, i, d, compensate=False, setup_i=NONE5, noise_i=None, est=None, variant=None, steps=T, q0=None):
    """instance i's oracle loop under its plant with the delay (and, compensate, the predictor) in front of the reference actuator.
    est: None or (v [steps', nx], M, xp0): measurement noise and an estimator in front (estimator_cases' chain); under compensation the
    model predicts the next xp from xhat with s0, without it with the command.  -> records, iter, u0, states (true), ua, s0, a, queue
    (oldest first, [D_MAX, nu], zeros behind d), xhat, xs (what every step solved from), estimate"""
    mA, mB, mf = (m[i] for m in mc.model_of(c))
    plant = tuple(m[i] for m in c["plant"])
    o = sc.make_solver(OracleSolver, c["fams"][i if c["hetero"] else 0], icc.config(c, i, max_iter=pc.MAX_ITER))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    nu = c["nu"]
    x = c["x0"][i].copy()
    q = [np.zeros(nu) for _ in range(d)] if q0 is None else [np.array(r, dtype=float) for r in q0[:d]]
    a = np.zeros(nu)
    v, M, xp = est if est is not None else (None, None, None)
    xp = None if xp is None else np.array(xp, dtype=float)
    out = dict(iter=[], u0=[], states=[], ua=[], s0=[], xhat=[], xs=[])
    for k in range(steps):
        xin = x + v[k] if (v is not None and k < len(v)) else x.copy()
        if est is not None:
            xin = ec.correct(M, xp, xin)
        xs = predict((mA, mB, mf), xin, q, d, variant, plant) if compensate else xin
        o["x"][:, 0] = xs
        o.solve()
        it = int(o.get("sol_iter"))
        out["iter"].append(it if int(o.get("sol_solved")) else -it)
        u0 = np.array(o["u"])[:, 0].copy()
        s0, q = fifo(q, d, u0, variant)
        ua, a = ac.actuate(s0, setup_i, a, noise_i[k] if (noise_i is not None and k < len(noise_i)) else None)
        if est is not None:
            xp = pc.plant_step(mA, mB, mf, xin, s0 if (compensate and variant != ESTIMATOR_MISREADING) else u0)
        x = pc.plant_step(*plant, x, ua)
        for key, val in (("u0", u0), ("states", x.copy()), ("ua", ua), ("s0", s0), ("xhat", xin), ("xs", xs)):
            out[key].append(val)
    rec = {k: np.array(o[k]) for k in pc.KEYS}
    o.close()
    queue = np.zeros((D_MAX, nu))
    for t in range(d):
        queue[t] = q[t]
    out = {k: np.array(val) for k, val in out.items()}
    out.update(rec=rec, x0=x, a=a, queue=queue, estimate=xp)
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(name, compensate=False):
    """every instance's own oracle loop under the case's delays"""
    c = pc.case(name)
    d = delays(name)
    return [delay_loop(c, i, int(d[i]), compensate) for i in range(c["B"])]


@functools.lru_cache(maxsize=None)
def undelayed_case(name):
    c = pc.case(name)
    return [delay_loop(c, i, 0) for i in range(c["B"])]


def estimator_inputs(name=COMPOSE_CASE):
    """(v [T, B, nx], M, xp0) of the composition case: estimator_cases' own, the noise rows repeated to T steps"""
    v = mc.noise(name)
    v = np.concatenate([v, v])[:T] if len(v) < T else v[:T]
    return v, ec.gain(name), ec.estimate(name)


def moved(other, own):
    return ac.moved(other, own)


def check_case(name):
    """the reference conditions, from the reference and the oracle loops alone"""
    c = pc.case(name)
    d = delays(name)
    assert T == 8 and D_MAX == 3 and d.max() <= D_MAX and (c["B"] < 4 or d.max() == D_MAX)
    plain, own, comp = undelayed_case(name), oracle_case(name), oracle_case(name, True)
    for i in range(c["B"]):
        for run in (plain[i], own[i], comp[i]):
            assert max(np.max(np.abs(run["rec"]["x"])), np.max(np.abs(run["states"]))) < 100.0, (name, "instance %d: the loop diverges" % i)
            assert np.max(np.abs(run["iter"])) > 1, (name, "instance %d: nothing iterates" % i)
        if d[i] == 0:
            for k in ("u0", "states", "iter"):
                assert np.array_equal(own[i][k], plain[i][k]) and np.array_equal(comp[i][k], plain[i][k])
            continue
        assert moved(own[i], plain[i]) >= 0.29, (name, i, "the delay", moved(own[i], plain[i]))
        assert moved(comp[i], own[i]) >= 0.32, (name, i, "the compensation", moved(comp[i], own[i]))
        for what in MISREADINGS:
            base = own[i] if what == "push_before_pop" else comp[i]
            if what in ("newest_first", "queue_after_push") and d[i] < 2:
                continue                                   # (one entry reads the same from either end)
            other = delay_loop(c, i, int(d[i]), what != "push_before_pop", variant=what)
            assert moved(other, base) > 1e-6, (name, "instance %d under %s" % (i, what), moved(other, base))


def check_estimator_case(name=COMPOSE_CASE):
    """under compensation, an estimator that predicts with the command instead of what left the queue moves a later u0"""
    c = pc.case(name)
    d = delays(name)
    v, M, xp0 = estimator_inputs(name)
    for i in range(c["B"]):
        if d[i] == 0:
            continue
        est = (v[:, i], M[i], xp0[i])
        own = delay_loop(c, i, int(d[i]), True, est=est)
        other = delay_loop(c, i, int(d[i]), True, est=est, variant=ESTIMATOR_MISREADING)
        assert np.max(np.abs(own["states"])) < 100.0 and moved(other, own) > 1e-6, (name, i, moved(other, own))
