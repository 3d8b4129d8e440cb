"""The setups, the reference and the oracle-side conditions of tests/test_gpu_actuator.py and tests/test_actuator_cpu.py (CPU only;
computed once per case and shared).  The meaning of tiny_batch_set_actuator, restated in plain Python floats with the rational-arithmetic
fma of plant_cases: for input c of an instance, command uc, actuator state a, noise row n,

    1. limits:  s = lo[c] if uc < lo[c] else (hi[c] if uc > hi[c] else uc)          (None: no limit; inside them uc's own bits)
    2. lag:     d = s - a[c];  m = fma(alpha[c], d, a[c]);  a[c] = m               (alpha None: m = s, no record)
    3. gain:    g = fma(m, gain[c], offset[c])                                     (gain None: 1.0, offset None: -0.0)
    4. noise:   ua[c] = g + n[c]                                                   (no row: ua[c] = g, no addition)

Cases: those of plant_cases -- 4_2_10 with 13 instances, 5_3_7 with 11, 12_4_10 with 2, the edge shapes 15_1_3 and 1_15_3, 6_3_10 and the
tile-kernel shape 20_8_10 -- each under its perturbed plant, T = 5 MPC steps.  Setups are per instance and per input, drawn from the u0
the case's oracle loop WITHOUT an actuator produces: with v the sorted commands of (instance, input) over the steps and r their range,
lo lies in the gap above the smallest and hi in the gap below the largest (RULES: two cases differ); alpha U(0.3, 0.9); gain U(0.7, 1.1); offset +-U(1, 5) % of r;
a noise sequence of 4 rows, +-U(1, 5) % of r.  check_case asserts the visibility conditions of the module's users from the reference and
plant_cases.oracle_loop(c, i, step=...) alone: the step closure carries a and k."""
import functools

import numpy as np

import estimator_cases as ec
import instance_cone_cases as icc
import measurement_cases as mc
import plant_cases as pc
import scenarios as sc
from cpu_solvers import OracleSolver

T = pc.T
N_ROWS = 4                                         # rows of the actuation-noise sequence
ORACLE_CASES = pc.ORACLE_CASES
EDGE_CASES = pc.EDGE_CASES
COMPOSE_CASE = "6_3_10"
COVER_CASE = "20_8_10"
ALL_CASES = ORACLE_CASES + EDGE_CASES + (COMPOSE_CASE, COVER_CASE)
STAGES = ("limits", "lag", "gain", "noise")
MISREADINGS = tuple("no_" + s for s in STAGES) + ("lag_before_limits", "noise_before_gain")


def fma(a, b, c):
    """plant_cases.fma with the sign of a zero result: the rational sum has none.  A zero product on a zero addend keeps the sign both
    share (else +0.0); an exact cancellation is +0.0"""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return float(a) * float(b) + float(c)      # (an infinity or a NaN: no rounding to tell apart)
    r = pc.fma(a, b, c)
    if r == 0.0 and (float(a) == 0.0 or float(b) == 0.0) and float(c) == 0.0:
        return -0.0 if ((np.signbit(a) != np.signbit(b)) and np.signbit(c)) else 0.0
    return r


def limits(u, lo, hi):
    """two comparisons, two selects: inside the limits the command's own bits"""
    if lo is not None and u < lo:
        return float(lo)
    if hi is not None and u > hi:
        return float(hi)
    return float(u)


def actuate(uc, setup, a, row, variant=None, zero_offset=-0.0):
    """the applied control of ONE instance at one MPC step: uc (nu,), setup = (lo, hi, alpha, gain, offset), each (nu,) or None, a (nu,)
    the actuator state (read only with alpha), row (nu,) the noise row or None -> (ua (nu,), the new a).  variant: None or one of
    MISREADINGS; zero_offset: what a None offset stands for (the misreading +0.0)"""
    lo, hi, alpha, gain, offset = setup
    nu = len(uc)
    ua, an = np.zeros(nu), (None if a is None else np.array(a, dtype=float))
    bare = all(p is None for p in setup)          # (no actuator installed, the noise alone: only stage 4 runs)
    for c in range(nu):
        v = float(uc[c])

        def lim(v):
            return v if variant == "no_limits" else limits(v, None if lo is None else lo[c], None if hi is None else hi[c])

        def lag(v):
            if alpha is None or variant == "no_lag":
                return v
            m = fma(alpha[c], v - float(an[c]), an[c])
            an[c] = m
            return m

        def scale(v):
            if variant == "no_gain":
                return v
            return fma(v, 1.0 if gain is None else gain[c], zero_offset if offset is None else offset[c])

        def noise(v):
            return v if (row is None or variant == "no_noise") else v + float(row[c])
        if bare:
            v = noise(v)
        elif variant == "lag_before_limits":
            v = noise(scale(lim(lag(v))))
        elif variant == "noise_before_gain":
            v = scale(noise(lag(lim(v))))
        else:
            v = noise(scale(lag(lim(v))))
        ua[c] = v
    return ua, an


def actuate_batch(uc, setups, a, row, ran=None):
    """every instance by its own setup: uc (B, nu), setups = five (B, nu) arrays (or None), a (B, nu) or None, row (B, nu) or None;
    ran (B,) bool: whether the instance's step ran an iteration (one that did not takes no plant step: no stage runs, a stays) ->
    (ua (B, nu), a)"""
    B = len(uc)
    ua = np.array(uc, dtype=float)
    an = None if a is None else np.array(a, dtype=float)
    for i in range(B):
        if ran is not None and not ran[i]:
            continue
        ua[i], ai = actuate(uc[i], tuple(None if s is None else s[i] for s in setups), None if a is None else a[i], None if row is None else row[i])
        if an is not None:
            an[i] = ai
    return ua, an


def broadcast(setup, B):
    """one setup for all, as five (B, nu) arrays"""
    return tuple(None if s is None else np.repeat(np.asarray(s, dtype=float)[None], B, axis=0) for s in setup)


def commands(name):
    """u0 [B, T, nu] of the case's oracle loops WITHOUT an actuator"""
    return np.array([r["u0"] for r in pc.oracle_case(name)])


def setup_around(u, seed, rule=(0, 0, 0.3, 0.7)):
    """(lo, hi, alpha, gain, offset) [B, nu] and noise [N_ROWS, B, nu] drawn from the commands u [B, T, nu] by the rule of the docstring;
    rule = (g, h, f0, f1): lo in the gap above the g-th smallest command, hi in the gap below the h-th largest, U(f0, f1) of the gap in"""
    rng = np.random.default_rng(seed)
    B, steps, nu = u.shape
    g, h, f0, f1 = rule
    v = np.sort(u, axis=1)
    r = v[:, -1] - v[:, 0]
    assert np.all(r > 0.0) and g + h + 2 < steps
    lo = v[:, g] + rng.uniform(f0, f1, (B, nu)) * (v[:, g + 1] - v[:, g])
    hi = v[:, -1 - h] - rng.uniform(f0, f1, (B, nu)) * (v[:, -1 - h] - v[:, -2 - h])
    alpha = rng.uniform(0.3, 0.9, (B, nu))
    gain = rng.uniform(0.7, 1.1, (B, nu))
    offset = rng.uniform(0.01, 0.05, (B, nu)) * rng.choice([-1.0, 1.0], (B, nu)) * r
    noise = rng.uniform(0.01, 0.05, (N_ROWS, B, nu)) * rng.choice([-1.0, 1.0], (N_ROWS, B, nu)) * r[None]
    return (lo, hi, alpha, gain, offset), noise


# the seed of every case's draws: the first from 0 on at which check_case holds
SEEDS = {"4_2_10": 0, "5_3_7": 0, "12_4_10": 0, "15_1_3": 1, "1_15_3": 0, "6_3_10": 0, "20_8_10": 0}


# where the limits lie among the sorted commands (setup_around's rule): by default in the outermost gaps.  Under the actuator the loop's
# commands move: on 4_2_10 fewer than a third of them would then saturate, on 1_15_3 (15 inputs on one state) more than two thirds
RULES = {"4_2_10": (1, 0, 0.3, 0.7), "1_15_3": (0, 0, 0.05, 0.3)}


@functools.lru_cache(maxsize=None)
def setup(name):
    """((lo, hi, alpha, gain, offset) [B, nu], noise [N_ROWS, B, nu]) of the case"""
    c = pc.case(name)
    return setup_around(commands(name), 8000 + 31 * c["nx"] + c["nu"] + 100000 * SEEDS[name], RULES.get(name, (0, 0, 0.3, 0.7)))


def initial_state(name):
    """a [B, nu]: zeros, what installing a lag leaves"""
    c = pc.case(name)
    return np.zeros((c["B"], c["nu"]))


def actuated_loop(c, i, setup_i, noise_i, variant=None, steps=T, a0=None):
    """instance i's oracle loop under its plant with the reference actuator between the command and the plant step:
    plant_cases.oracle_loop with a step closure that carries a and k.  -> its result, plus ua [steps, nu], a (the final record) and
    saturated [steps, nu] (the limits moved the command)"""
    A, Bm, f = (m[i] for m in c["plant"])
    st = dict(a=np.zeros(c["nu"]) if a0 is None else np.array(a0, dtype=float), k=0, ua=[], sat=[])

    def step(x0, u0):
        row = noise_i[st["k"]] if (noise_i is not None and st["k"] < len(noise_i)) else None
        ua, st["a"] = actuate(u0, setup_i, st["a"], row, variant)
        st["ua"].append(ua)
        lo, hi = setup_i[0], setup_i[1]
        st["sat"].append(np.array([limits(u0[q], None if lo is None else lo[q], None if hi is None else hi[q]) != u0[q] for q in range(len(u0))]))
        st["k"] += 1
        return pc.plant_step(A, Bm, f, x0, ua)
    out = pc.oracle_loop(c, i, step, steps=steps)
    out.update(ua=np.array(st["ua"]), a=st["a"], saturated=np.array(st["sat"]))
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """every instance's own oracle loop with the reference actuator of the case's setup"""
    c = pc.case(name)
    s, n = setup(name)
    return [actuated_loop(c, i, tuple(q[i] for q in s), n[:, i]) for i in range(c["B"])]


def moved(other, own):
    """the largest relative change of a LATER u0 (steps 1 on)"""
    return max(float(np.max(np.abs(other["u0"][k] - own["u0"][k])) / max(np.max(np.abs(own["u0"][k])), 1e-300)) for k in range(1, len(own["u0"])))


def estimator_loop(c, i, v, M, xp0, setup_i, noise_i, predict_with_applied=False, steps=T):
    """instance i's loop behind measurement noise and an estimator (estimator_cases.oracle_loop's chain) with the actuator in front of
    the plant: the estimate is predicted from the COMMAND; predict_with_applied: the misreading that predicts it from ua"""
    mA, mB, mf = (m[i] for m in mc.model_of(c))
    A, Bm, f = (m[i] for m in c["plant"])
    o = sc.make_solver(OracleSolver, c["fams"][i if c["hetero"] else 0], icc.config(c, i, max_iter=pc.MAX_ITER))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    x, xp, a = c["x0"][i].copy(), np.array(xp0, dtype=float), np.zeros(c["nu"])
    its, u0s, xs, xhs, uas = [], [], [], [], []
    for k in range(steps):
        xm = x + v[k] if k < len(v) else x.copy()
        xhat = ec.correct(M, xp, xm)
        o["x"][:, 0] = xhat
        o.solve()
        it = int(o.get("sol_iter"))
        its.append(it if int(o.get("sol_solved")) else -it)
        u0 = np.array(o["u"])[:, 0].copy()
        ua, a = actuate(u0, setup_i, a, noise_i[k] if k < len(noise_i) else None)
        xp = pc.plant_step(mA, mB, mf, xhat, ua if predict_with_applied else u0)
        x = pc.plant_step(A, Bm, f, x, ua)
        u0s.append(u0), xs.append(x.copy()), xhs.append(xhat), uas.append(ua)
    o.close()
    return dict(iter=np.array(its), u0=np.array(u0s), states=np.array(xs), xhat=np.array(xhs), ua=np.array(uas), a=a, estimate=xp)


def signed_zero_setup(name):
    """a setup whose offset is None and whose m hits -0.0: input 0 of every instance is held at lo = hi = -0.0, gain ones, no lag"""
    c = pc.case(name)
    B, nu = c["B"], c["nu"]
    lo, hi = np.full((B, nu), -np.inf), np.full((B, nu), np.inf)
    lo[:, 0] = hi[:, 0] = -0.0
    return (lo, hi, None, np.ones((B, nu)), None)


def check_case(name):
    """the visibility conditions, from the reference and the oracle loops alone"""
    c = pc.case(name)
    B, nu = c["B"], c["nu"]
    s, n = setup(name)
    u = commands(name)
    v = np.sort(u, axis=1)
    r = v[:, -1] - v[:, 0]
    lo, hi, alpha, gain, offset = s
    assert all(q.shape == (B, nu) for q in s) and n.shape == (N_ROWS, B, nu) and N_ROWS < T
    # the draws: limits inside the range of the commands without an actuator, alpha, gain, offsets and noise as stated
    assert np.all(lo > v[:, 0]) and np.all(hi < v[:, -1]) and np.all(lo < hi)
    assert np.all((alpha >= 0.3) & (alpha <= 0.9)) and np.all((gain >= 0.7) & (gain <= 1.1))
    assert np.all((np.abs(offset) >= 0.01 * r) & (np.abs(offset) <= 0.05 * r)) and np.all((np.abs(n) >= 0.01 * r[None]) & (np.abs(n) <= 0.05 * r[None]))
    own = oracle_case(name)
    sat = np.array([q["saturated"] for q in own])
    assert sat.shape == (B, T, nu)
    assert 3 * int(np.sum(sat)) >= sat.size and 3 * int(np.sum(~sat)) >= sat.size, (name, int(np.sum(sat)), sat.size)
    for i in range(B):
        q = own[i]
        assert max(np.max(np.abs(q["rec"]["x"])), np.max(np.abs(q["states"]))) < 100.0, ("instance %d: the loop diverges" % i)
        assert np.max(np.abs(q["iter"])) > 1, ("instance %d: nothing iterates" % i)
        for what in MISREADINGS:
            other = actuated_loop(c, i, tuple(p[i] for p in s), n[:, i], variant=what)
            assert moved(other, q) > 1e-6, (name, "instance %d under %s" % (i, what), moved(other, q))
    # a None offset is -0.0: where m hits -0.0 the applied control keeps the sign, and under +0.0 it would not
    z = signed_zero_setup(name)
    for i in (0, B - 1):
        zi = tuple(None if p is None else p[i] for p in z)
        for uc in u[i, :2]:
            if uc[0] == 0.0:
                continue
            got, _ = actuate(uc, zi, None, None)
            other, _ = actuate(uc, zi, None, None, zero_offset=0.0)
            assert got[0] == 0.0 and np.signbit(got[0]) and other[0] == 0.0 and not np.signbit(other[0])
            assert np.array_equal(got[1:], uc[1:]) and np.array_equal(np.signbit(got[1:]), np.signbit(uc[1:]))


def check_estimator_case(name=COMPOSE_CASE):
    """predicting the estimate with ua instead of the command moves a later u0 of every instance"""
    c = pc.case(name)
    s, n = setup(name)
    v, M, xp0 = mc.noise(name), ec.gain(name), ec.estimate(name)
    for i in range(c["B"]):
        si = tuple(p[i] for p in s)
        own = estimator_loop(c, i, v[:, i], M[i], xp0[i], si, n[:, i])
        other = estimator_loop(c, i, v[:, i], M[i], xp0[i], si, n[:, i], predict_with_applied=True)
        assert np.max(np.abs(own["states"])) < 100.0 and moved(other, own) > 1e-6, (name, i, moved(other, own))
