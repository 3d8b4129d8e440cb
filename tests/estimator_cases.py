"""The gains, initial estimates and oracle closed loops of tests/test_gpu_estimator.py (CPU only; computed once per case and shared).
The meaning of tiny_batch_set_estimator, restated: x is the plant's true state, xp the predicted estimate.  MPC step k measures
xm = fl(x + v[k][i]) (no row: xm = x), corrects

    e[c] = fl(xm[c] - xp[c]);  acc = xp[j];  acc = fma(e[c], M[j][c], acc), c = 0 .. nx-1;  xhat[j] = acc

solves from xhat, applies u0, predicts xp = plant_step(model, xhat, u0) and steps the TRUE x by plant_step(plant, x, u0) -- the
reference chain of tests/plant_cases.py, in the rational-arithmetic fma of that file.

Cases: those of plant_cases (4_2_10 with 13 instances, 5_3_7 with 11, 12_4_10 with 2 and the edge shapes 15_1_3 and 1_15_3), T = 5 MPC
steps, the noise of measurement_cases.noise, the case's perturbed plant.  Gains per instance: diagonal U(0.4, 0.8), off-diagonal
+-U(0.05, 0.15) * 2 / nx; initial estimate x0 +- U(0.05, 0.1) per entry.  check_case asserts, from the ORACLE alone, that each of these
misreadings moves the u0 of step 1 or 2 by more than 1e-6 relative: no correction (xhat = xp), M transposed (not at nx = 1), the
correction from the true state instead of the measurement, the raw measurement handed on, the prediction from xm instead of xhat, the
prediction by the plant instead of the model, the plant stepped from xhat, and instance i + 1's gain -- the 1e-9 comparison of the GPU
tests tells every one of them apart -- and that no loop exceeds 100 in magnitude and every instance iterates."""
import functools

import numpy as np

import instance_cone_cases as icc
import measurement_cases as mc
import plant_cases as pc
import scenarios as sc
from cpu_solvers import OracleSolver

MAX_ITER = pc.MAX_ITER
T = pc.T
KEYS = pc.KEYS
ORACLE_CASES = pc.ORACLE_CASES
EDGE_CASES = pc.EDGE_CASES
MISREADINGS = ("no_correction", "transposed", "from_true", "raw_measurement", "predict_from_measured", "predict_by_plant", "plant_from_estimate", "neighbour_gain")
fma = pc.fma


def correct(M, xp, xm):
    """the reference correction of ONE instance: M (nx, nx), xp (nx,), xm (nx,) -> xhat (nx,)"""
    nx = len(xp)
    e = np.asarray(xm, dtype=float) - np.asarray(xp, dtype=float)          # (one IEEE subtraction per state)
    out = np.zeros(nx)
    for j in range(nx):
        acc = float(xp[j])
        for c in range(nx):
            acc = fma(e[c], M[j, c], acc)
        out[j] = acc
    return out


def correct_batch(M, xp, xm):
    return np.array([correct(M[i], xp[i], xm[i]) for i in range(len(xp))])


def gain_for(B, nx, seed):
    """M [B, nx, nx]: diagonal U(0.4, 0.8), off-diagonal +-U(0.05, 0.15) * 2 / nx"""
    rng = np.random.default_rng(seed)
    M = rng.uniform(0.05, 0.15, (B, nx, nx)) * rng.choice([-1.0, 1.0], (B, nx, nx)) / max(nx, 1) * 2
    for i in range(B):
        M[i][np.diag_indices(nx)] = rng.uniform(0.4, 0.8, nx)
    return M


def estimate_for(x0, seed):
    """xp [B, nx]: x0 +- U(0.05, 0.1) per entry"""
    rng = np.random.default_rng(seed)
    return x0 + 0.1 * rng.uniform(0.5, 1.0, x0.shape) * rng.choice([-1.0, 1.0], x0.shape)


@functools.lru_cache(maxsize=None)
def gain(name):
    c = pc.case(name)
    return gain_for(c["B"], c["nx"], 555 + c["nx"])


@functools.lru_cache(maxsize=None)
def estimate(name):
    c = pc.case(name)
    return estimate_for(c["x0"], 99 + c["nx"])


def oracle_loop(c, i, v, M, xp0, plant=None, steps=T, variant=None):
    """instance i's closed loop on the oracle: noise rows v [steps, nx] (a row of None, or v None: no noise), gain M (nx, nx), initial
    estimate xp0 (nx,), stepped by `plant` (default: its model), predicted by its model.  variant: None, or one of MISREADINGS but the
    last (a neighbour's gain is the caller's M)"""
    mA, mB, mf = (m[i] for m in mc.model_of(c))
    A, Bm, f = (m[i] for m in plant) if plant is not None else (mA, mB, mf)
    o = sc.make_solver(OracleSolver, c["fams"][i if c["hetero"] else 0], icc.config(c, i, max_iter=MAX_ITER))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    x, xp = c["x0"][i].copy(), np.array(xp0, dtype=float)
    its, u0s, xs, xhs = [], [], [], []
    for k in range(steps):
        row = v[k] if (v is not None and k < len(v)) else None
        xm = x.copy() if row is None else x + row
        if variant == "no_correction":
            xhat = xp.copy()
        elif variant == "transposed":
            xhat = correct(M.T, xp, xm)
        elif variant == "from_true":
            xhat = correct(M, xp, x)
        elif variant == "raw_measurement":
            xhat = xm.copy()
        else:
            xhat = correct(M, xp, xm)
        o["x"][:, 0] = xhat
        o.solve()
        it = int(o.get("sol_iter"))
        its.append(it if int(o.get("sol_solved")) else -it)
        u0 = np.array(o["u"])[:, 0].copy()
        u0s.append(u0)
        xhs.append(xhat)
        xp = pc.plant_step(mA, mB, mf, xm if variant == "predict_from_measured" else xhat, u0)
        if variant == "predict_by_plant":
            xp = pc.plant_step(A, Bm, f, xhat, u0)
        x = pc.plant_step(A, Bm, f, xhat if variant == "plant_from_estimate" else x, u0)
        xs.append(x.copy())
    rec = {key: np.array(o[key]) for key in KEYS}
    o.close()
    return dict(rec=rec, iter=np.array(its), u0=np.array(u0s), x0=x, states=np.array(xs), xhat=np.array(xhs), estimate=xp)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    c, v, M, xp0 = pc.case(name), mc.noise(name), gain(name), estimate(name)
    return [oracle_loop(c, i, v[:, i], M[i], xp0[i], plant=c["plant"]) for i in range(c["B"])]


def check_case(name):
    """the visibility conditions, from the oracle alone"""
    c, v, M, xp0 = pc.case(name), mc.noise(name), gain(name), estimate(name)
    own = oracle_case(name)
    B = c["B"]
    for i in range(B):
        r = own[i]
        assert max(np.max(np.abs(r["rec"]["x"])), np.max(np.abs(r["states"])), np.max(np.abs(r["xhat"]))) < 100.0, ("instance %d: the loop diverges" % i)
        assert np.max(np.abs(r["iter"])) > 1, ("instance %d: nothing iterates" % i)
        n = (i + 1) % B
        for what in MISREADINGS:
            if what == "transposed" and c["nx"] == 1:
                continue                                       # (the same matrix)
            kw = dict(M=M[n]) if what == "neighbour_gain" else dict(M=M[i], variant=what)
            other = oracle_loop(c, i, v[:, i], xp0=xp0[i], plant=c["plant"], steps=3, **kw)
            moved = max(float(np.max(np.abs(other["u0"][k] - r["u0"][k])) / max(np.max(np.abs(r["u0"][k])), 1e-300)) for k in (1, 2))
            assert moved > 1e-6, ("instance %d under %s" % (i, what), moved)
