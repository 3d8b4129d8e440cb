"""The problems of tests/test_gpu_instance_cones.py and their oracle solutions (CPU only; computed once per case and shared): small
batches on random stable families (instance_bounds_cases.random_family), every instance its own coefficient for every cone, every
drawn coefficient distinct and in [0.2, 1.5].  Where the cones sit is the batch's.  x0 lies outside every state cone on the side
whose projection depends on the coefficient (the cone's last row positive and small against the norm of the other two).  The
conditions that make a misread coefficient visible are asserted here from the ORACLE's results alone (check_case): in every enabled
cone family every instance has an item whose cone dual is non-zero after the solve (its projection took the exact path), and solving
instance i under instance i + 1's coefficients moves vcnew | zcnew by more than 1e-6 -- a coefficient read from the wrong instance,
cone or lane cannot pass."""
import functools

import numpy as np

import instance_bounds_cases as ibc
import instance_halfspace_cases as ihc
import scenarios as sc
from cpu_solvers import OracleSolver

MAX_ITER = 60
KEYS = ibc.KEYS + ("vcnew", "zcnew", "gc", "yc")
LIN_KEYS = ("vlnew", "gl", "zlnew", "yl")
RHO_SCALE = 0.1                                   # (every slack family that is on adds its own rho term: instance_halfspace_cases.family)

# name: shape, batch, per-instance problem data, first rows of the state / input cones, which families are on, what else is set
# ("pl": per-instance static half-spaces, "box": a per-instance box, "force_general": the option), how the coefficients are drawn,
# the kernel path the GPU test expects
CASES = {
    "6_3_10_both": dict(shape=(6, 3, 10), B=13, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra=None, coef="random", path="jit"),
    "6_3_10_input": dict(shape=(6, 3, 10), B=13, hetero=False, Acx=[1], Acu=[0], on=(0, 1), extra=None, coef="random", path="jit"),
    "6_3_10_state": dict(shape=(6, 3, 10), B=13, hetero=False, Acx=[1], Acu=[0], on=(1, 0), extra=None, coef="random", path="jit"),
    "6_3_10_pow2_mix": dict(shape=(6, 3, 10), B=8, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra=None, coef="pow2_mix", path="jit"),
    "12_4_10_hetero": dict(shape=(12, 4, 10), B=11, hetero=True, Acx=[1, 6], Acu=[0], on=(1, 1), extra=None, coef="random", path="jit"),
    "5_3_7": dict(shape=(5, 3, 7), B=11, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra=None, coef="random", path="jit"),
    "6_3_10_b2": dict(shape=(6, 3, 10), B=2, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra=None, coef="random", path="jit"),
    "12_4_10_overlap": dict(shape=(12, 4, 10), B=11, hetero=False, Acx=[0, 2, 1], Acu=[0, 1], on=(1, 1), extra=None, coef="random", path="cover"),
    "20_4_10": dict(shape=(20, 4, 10), B=11, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra=None, coef="random", path="cover"),
    "6_3_10_with_pl": dict(shape=(6, 3, 10), B=11, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra="pl", coef="random", path="cover"),
    "6_3_10_with_box": dict(shape=(6, 3, 10), B=11, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra="box", coef="random", path="cover"),
    "6_3_10_force_general": dict(shape=(6, 3, 10), B=13, hetero=False, Acx=[1], Acu=[0], on=(1, 1), extra="force_general", coef="random", path="cover"),
    # the cones on the last rows of a full DPP row: state rows 10..12, inputs 0..2 = lanes 13..15
    "13_3_4": dict(shape=(13, 3, 4), B=11, hetero=False, Acx=[10], Acu=[0], on=(1, 1), extra=None, coef="random", path="jit"),
}
# cases whose first draw fails check_case (6_3_10_input: an instance whose input cone never projects) or solves every instance in two or
# three iterations: name -> seed offset.  The draws kept spread the cold iteration counts between a handful and the cap
RESEED = {"6_3_10_both": 7, "6_3_10_input": 8, "6_3_10_state": 11, "13_3_4": 1}      # (13_3_4: an input cone that never projects)


def keys(c):
    return KEYS + (LIN_KEYS if c["extra"] == "pl" else ())


def family(nx, nu, N, seed):
    fam = ibc.random_family(nx, nu, N, seed)
    fam["rho"] *= RHO_SCALE
    return fam


def coefficients(spec, rng):
    """cx [B, n_state_cones], cu [B, n_input_cones]"""
    B, ns, ni = spec["B"], len(spec["Acx"]), len(spec["Acu"])
    if spec["coef"] == "pow2_mix":
        # the first wave's four rows alternate a power of two and 0.7 in both families; the second wave holds powers of two only
        assert B == 8 and ns == 1 and ni == 1
        cx = np.array([0.5, 0.7, 0.5, 0.7, 0.25, 0.5, 0.25, 0.5])
        cu = np.array([0.7, 0.5, 0.7, 0.5, 0.5, 0.25, 0.5, 0.25])
        return cx[:, None], cu[:, None]
    drawn = rng.uniform(0.2, 1.5, (B, ns + ni))
    assert np.unique(drawn).size == drawn.size
    return np.ascontiguousarray(drawn[:, :ns]), np.ascontiguousarray(drawn[:, ns:])


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of one batch: families (one, or one per instance), x0, references, every instance's cone coefficients (and what else
    the case sets)"""
    spec = CASES[name]
    nx, nu, N = spec["shape"]
    B = spec["B"]
    seed = 1000 * nx + 100 * nu + N + sum(map(ord, name)) + 7919 * RESEED.get(name, 0)
    rng = np.random.default_rng(seed)
    fams = [family(nx, nu, N, seed + 17 * i) for i in range(B if spec["hetero"] else 1)]
    x0 = rng.uniform(0.5, 1.0, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))
    for first in spec["Acx"]:                      # outside the cone, its last row positive: the projection depends on the coefficient
        x0[:, first + 2] = rng.uniform(0.2, 0.45, B)
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    for first in spec["Acu"]:                      # the input cone's last row is pulled to the positive side, the other two away from zero
        Uref[:, first + 2, :] += 0.3
        Uref[:, first:first + 2, :] += rng.choice([-0.4, 0.4], (B, 2, 1))
    cx, cu = coefficients(spec, rng)
    c = dict(spec, name=name, nx=nx, nu=nu, N=N, fams=fams, x0=x0, Xref=Xref, Uref=Uref, cx=cx, cu=cu, box=None, linear=None)
    if spec["extra"] == "box":
        c["box"] = ibc.boxes(B, nx, nu, N, seed + 9, True)
    if spec["extra"] == "pl":                      # two static state half-spaces around x0 (instance_halfspace_cases.state_sets), one loose input half-space
        Ax, bx, _, _ = ihc.state_sets(x0, nx, N, rng)
        c["linear"] = (Ax, bx, rng.normal(0, 1, (B, 1, nu)), rng.uniform(0.3, 0.6, (B, 1)))
    return c


def config(c, i, coef_of=None, max_iter=MAX_ITER):
    """oracle/scenarios.py's configuration of instance i of case c under the cone coefficients of instance coef_of (default: its own)"""
    j = i if coef_of is None else coef_of
    three = lambda first: [3] * len(first)
    kw = dict(max_iter=max_iter, en_state_soc=c["on"][0], en_input_soc=c["on"][1], state_cone=(c["Acx"], three(c["Acx"]), list(c["cx"][j])),
              input_cone=(c["Acu"], three(c["Acu"]), list(c["cu"][j])), en_state_bound=int(c["box"] is not None), en_input_bound=int(c["box"] is not None))
    if c["box"] is not None:
        kw.update(x_min=c["box"][0][i], x_max=c["box"][1][i], u_min=c["box"][2][i], u_max=c["box"][3][i])
    if c["linear"] is not None:
        kw.update(en_state_linear=1, en_input_linear=1, linear=tuple(a[i] for a in c["linear"]))
    return sc.default_config(c["fams"][i if c["hetero"] else 0], **kw)


def oracle_solve(c, i, coef_of=None, max_iter=MAX_ITER, x0_scale=(1.0,)):
    """instance i of case c: [(records, iter, solved)] of successive solves from x0 * x0_scale[k] (the later ones warm-started)"""
    fam = c["fams"][i if c["hetero"] else 0]
    o = sc.make_solver(OracleSolver, fam, config(c, i, coef_of, max_iter))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    out = []
    for scale in x0_scale:
        o["x"][:, 0] = c["x0"][i] * scale
        o.solve()
        out.append(({k: np.array(o[k]) for k in keys(c)}, int(o.get("sol_iter")), int(o.get("sol_solved"))))
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    """every instance's cold solve and warm second solve from 0.9 x0 under its own coefficients"""
    c = case(name)
    return [oracle_solve(c, i, x0_scale=(1.0, 0.9)) for i in range(c["B"])]


def check_case(name):
    """the conditions on the inputs, from the oracle alone"""
    c = case(name)
    own = oracle_case(name)
    for i in range(c["B"]):
        r = own[i][0][0]
        assert max(np.max(np.abs(r["x"])), np.max(np.abs(r["u"]))) < 100.0, ("instance %d: the iteration diverges" % i)
        for on, dual in zip(c["on"], ("gc", "yc")):
            assert not on or np.any(r[dual] != 0.0), ("instance %d: no item of %s ever projected" % (i, dual))
        other = oracle_solve(c, i, coef_of=(i + 1) % c["B"])[0][0]
        moved = max(np.max(np.abs(other["vcnew"] - r["vcnew"])), np.max(np.abs(other["zcnew"] - r["zcnew"])))
        assert moved > 1e-6, ("instance %d under the coefficients of instance %d" % (i, (i + 1) % c["B"]), moved)


def launch_case():
    """6_3_10_both: its cold iteration counts run from 4 to the cap and straddle 10 (what a split solve at K = 10 needs)"""
    return case("6_3_10_both")
