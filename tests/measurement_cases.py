"""The noise sequences of tests/test_gpu_measurement.py and the oracle closed loops under measurement noise (CPU only; computed once per
case and shared).  The meaning of tiny_batch_set_measurement_noise, restated: the state x is the plant's true one; MPC step k solves from
xm = fl(x + v[k][i]) -- one double addition --, applies u0, and the plant steps the TRUE x by the reference chain of tests/plant_cases.py
(plant_step), by the installed plant or, with none, by the model.

Cases: those of plant_cases (4_2_10 with 13 instances, 5_3_7 with 11, 12_4_10 with 2 and the edge shapes), T = 5 MPC steps; every entry of v
is 0.05 * U(0.5, 1) * +-1.  check_case asserts, from the ORACLE alone, that each of these misreadings moves the u0 of a later step by more
than 1e-6 relative: the plant stepped from the MEASURED state, instance i + 1's noise for instance i, row k + 1 for row k, and the noise
added after the solve (to the state handed on) instead of before it -- the 1e-9 comparison of the GPU tests tells every one of them apart --
and that no loop exceeds 100 in magnitude."""
import functools

import numpy as np

import instance_cone_cases as icc
import plant_cases as pc
import scenarios as sc
from cpu_solvers import OracleSolver

MAX_ITER = pc.MAX_ITER
T = pc.T
KEYS = pc.KEYS
AMPLITUDE = 0.05
ORACLE_CASES = pc.ORACLE_CASES
EDGE_CASES = pc.EDGE_CASES


def noise_for(B, nx, seed, steps=T):
    """v [steps, B, nx]: every entry AMPLITUDE * U(0.5, 1) * +-1"""
    rng = np.random.default_rng(seed)
    return AMPLITUDE * rng.uniform(0.5, 1.0, (steps, B, nx)) * rng.choice([-1.0, 1.0], (steps, B, nx))


@functools.lru_cache(maxsize=None)
def noise(name, steps=T):
    """the sequence of a plant_cases case"""
    c = pc.case(name)
    return noise_for(c["B"], c["nx"], 977 + 13 * sum(map(ord, name)), steps)


def model_of(c):
    """(A [B, nx, nx], B [B, nx, nu], f [B, nx]) of a case of plant_cases or disturbance_cases: every instance's own model"""
    if "model" in c:
        return c["model"]
    return tuple(np.stack([c["fams"][i if c["hetero"] else 0][k] for i in range(c["B"])]) for k in ("A", "B", "f"))


def oracle_loop(c, i, v, plant=None, steps=T, variant=None):
    """instance i's closed loop on the oracle under the noise rows v [steps, nx] (a row of None: outside the sequence), stepped by
    `plant` (default: its model).  variant: None, or one of the misreadings of the docstring ("from_measured", "after_solve")"""
    A, Bm, f = (m[i] for m in (plant or model_of(c)))
    o = sc.make_solver(OracleSolver, c["fams"][i if c["hetero"] else 0], icc.config(c, i, max_iter=MAX_ITER))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    x = c["x0"][i].copy()
    its, u0s, xs, xms = [], [], [], []
    for k in range(steps):
        row = v[k] if k < len(v) else None
        xm = x.copy() if (row is None or variant == "after_solve") else x + row
        o["x"][:, 0] = xm
        o.solve()
        it = int(o.get("sol_iter"))
        its.append(it if int(o.get("sol_solved")) else -it)
        u0 = np.array(o["u"])[:, 0].copy()
        u0s.append(u0)
        xms.append(xm)
        x = pc.plant_step(A, Bm, f, xm if variant == "from_measured" else x, u0)
        if variant == "after_solve" and row is not None:
            x = x + row
        xs.append(x.copy())
    rec = {key: np.array(o[key]) for key in KEYS}
    o.close()
    return dict(rec=rec, iter=np.array(its), u0=np.array(u0s), x0=x, states=np.array(xs), measured=np.array(xms))


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    c, v = pc.case(name), noise(name)
    return [oracle_loop(c, i, v[:, i]) for i in range(c["B"])]


def check_case(name):
    """the visibility conditions, from the oracle alone"""
    c, v = pc.case(name), noise(name)
    own = oracle_case(name)
    B = c["B"]
    for i in range(B):
        r = own[i]
        assert np.max(np.abs(r["rec"]["x"])) < 100.0 and np.max(np.abs(r["states"])) < 100.0, ("instance %d: the loop diverges" % i)
        assert np.max(np.abs(r["iter"])) > 1, ("instance %d: nothing iterates" % i)
        n = (i + 1) % B
        others = (("the plant stepped from the measured state", dict(v=v[:, i], variant="from_measured")),
                  ("the noise of instance %d" % n, dict(v=v[:, n])),
                  ("row k + 1 for row k", dict(v=v[1:, i])),
                  ("the noise added after the solve", dict(v=v[:, i], variant="after_solve")))
        for what, kw in others:
            other = oracle_loop(c, i, steps=3, **kw)
            moved = max(float(np.max(np.abs(other["u0"][k] - r["u0"][k])) / max(np.max(np.abs(r["u0"][k])), 1e-300)) for k in (1, 2))
            assert moved > 1e-6, ("instance %d under %s" % (i, what), moved)
