"""The problems of tests/test_gpu_disturbance.py and their oracle closed loops (CPU only; computed once per case and shared): small
batches on random stable families (instance_bounds_cases.random_family), T = 5 MPC steps under a disturbance sequence of
N_STEPS = 4 rows -- the last step is undisturbed --, every w[k][i] distinct and of the size of x0.  The oracle's closed loop of
instance i is `solve; x0 = x[:,1] + w[k][i]` on one warm-started solver.  The condition that makes a misread row visible is asserted
here from the ORACLE alone (check_case): giving instance i the sequence of instance i + 1, or its own shifted by one step, moves the
NEXT step's u0 (step 1: both changes alter the row step 0 adds) by more than 1e-6, for every instance -- a row read from the wrong
instance, grid slot or step cannot pass."""
import functools

import numpy as np

import instance_bounds_cases as ibc
import instance_cone_cases as icc
import instance_halfspace_cases as ihc
import scenarios as sc
from cpu_solvers import OracleSolver

MAX_ITER = 60
T = 5                                             # MPC steps of an episode
N_STEPS = 4                                       # rows of the sequence: the last step takes the undisturbed plant step
LIN_KEYS = icc.LIN_KEYS

# name: shape, batch, per-instance problem data, what is on ("box": a box, "cones": both cone families, "lin": static half-spaces),
# what of it every instance has its OWN of (the PB / PL / PC forms), an option set on the handle, the kernel path the GPU test expects
CASES = {
    "6_3_10_box": dict(shape=(6, 3, 10), B=13, hetero=False, on=("box",), own=(), option=None, path="jit"),
    "6_3_10_cones": dict(shape=(6, 3, 10), B=13, hetero=False, on=("cones",), own=(), option=None, path="jit"),
    "12_4_10_hetero": dict(shape=(12, 4, 10), B=11, hetero=True, on=("box",), own=(), option=None, path="jit"),
    "5_3_7": dict(shape=(5, 3, 7), B=11, hetero=False, on=("box",), own=(), option=None, path="jit"),
    "4_2_10": dict(shape=(4, 2, 10), B=13, hetero=False, on=("box",), own=(), option=None, path="jit"),       # a half-row shape: full rows
    "6_3_10_b2": dict(shape=(6, 3, 10), B=2, hetero=False, on=("box",), own=(), option=None, path="jit"),
    "20_4_10": dict(shape=(20, 4, 10), B=11, hetero=False, on=("box",), own=(), option=None, path="cover"),
    "6_3_10_force_general": dict(shape=(6, 3, 10), B=13, hetero=False, on=("box",), own=(), option="force_general", path="cover"),
    # composition: PD with PB, with PL, with PC; PL + PC + disturbance on the coverage kernel
    "6_3_10_pb": dict(shape=(6, 3, 10), B=11, hetero=False, on=("box",), own=("box",), option=None, path="jit"),
    "6_3_10_pl": dict(shape=(6, 3, 10), B=11, hetero=False, on=("lin",), own=("lin",), option=None, path="jit"),
    "6_3_10_pc": dict(shape=(6, 3, 10), B=11, hetero=False, on=("cones",), own=("cones",), option=None, path="jit"),
    "6_3_10_pl_pc": dict(shape=(6, 3, 10), B=11, hetero=False, on=("cones", "lin"), own=("cones", "lin"), option=None, path="cover"),
    # the extreme splits of a full row (instance_bounds_cases.EDGE_SHAPES): the row w[k][i] ends at lane 14 / is lane 0 alone, N - 1 = 2
    "15_1_3": dict(shape=ibc.EDGE_SHAPES[0], B=11, hetero=False, on=("box",), own=(), option=None, path="jit"),
    "1_15_3": dict(shape=ibc.EDGE_SHAPES[1], B=11, hetero=False, on=("box",), own=(), option=None, path="jit"),
}
COMPOSITION = ("6_3_10_pb", "6_3_10_pl", "6_3_10_pc", "6_3_10_pl_pc")
# cases whose first draw fails check_case (6_3_10_cones: an instance whose loop diverges): name -> seed offset.  The draw kept
# converges at most steps, with iteration counts spread between 3 and the cap
RESEED = {"6_3_10_cones": 5}
ACX, ACU = [1], [0]                               # first rows of the state / input cone


def keys(c):
    return ibc.KEYS + (("vcnew", "zcnew", "gc", "yc") if "cones" in c["on"] else ()) + (LIN_KEYS if "lin" in c["on"] else ())


def wide_boxes(B, nx, nu, N, seed):
    """x_min, x_max [B, nx, N], u_min, u_max [B, nu, N-1], knot-invariant, every number distinct: wide enough that u0 is not held on a
    bound at every step (an input on its bound does not answer to the disturbance), narrow enough that some entries are"""
    rng = np.random.default_rng(seed)
    xw, uw = rng.uniform(1.5, 2.5, (2, B, nx, 1)), rng.uniform(0.8, 1.6, (2, B, nu, 1))
    out = [np.broadcast_to(-xw[0], (B, nx, N)), np.broadcast_to(xw[1], (B, nx, N)), np.broadcast_to(-uw[0], (B, nu, N - 1)), np.broadcast_to(uw[1], (B, nu, N - 1))]
    return [np.ascontiguousarray(a) for a in out]


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of one batch in the layout instance_cone_cases.config reads, and the sequence w [N_STEPS, B, nx]"""
    spec = CASES[name]
    nx, nu, N = spec["shape"]
    B = spec["B"]
    seed = 1000 * nx + 100 * nu + N + sum(map(ord, name)) + 7919 * RESEED.get(name, 0)
    rng = np.random.default_rng(seed)
    soft = "cones" in spec["on"] or "lin" in spec["on"]          # (every slack family that is on adds its own rho term: instance_halfspace_cases.family)
    fams = [(icc.family if soft else ibc.random_family)(nx, nu, N, seed + 17 * i) for i in range(B if spec["hetero"] else 1)]
    x0 = rng.uniform(0.5, 1.0, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    w = rng.uniform(0.5, 1.0, (N_STEPS, B, nx)) * rng.choice([-1.0, 1.0], (N_STEPS, B, nx))
    assert np.unique(w).size == w.size
    c = dict(spec, name=name, nx=nx, nu=nu, N=N, fams=fams, x0=x0, Xref=Xref, Uref=Uref, w=w, box=None, linear=None, extra=None,
             Acx=[], Acu=[], cx=np.zeros((B, 0)), cu=np.zeros((B, 0)))
    c["on"] = (int("cones" in spec["on"]),) * 2                    # (instance_cone_cases.config: the cone switches)
    c["has"] = spec["on"]
    if "box" in spec["on"]:
        box = wide_boxes(B, nx, nu, N, seed + 9)
        c["box"] = box if "box" in spec["own"] else [np.ascontiguousarray(np.broadcast_to(a[:1], a.shape)) for a in box]
    if "cones" in spec["on"]:
        cf = rng.uniform(0.2, 1.5, (B, 2))
        if "cones" not in spec["own"]:
            cf = np.broadcast_to(cf[:1], cf.shape)
        c.update(Acx=ACX, Acu=ACU, cx=np.ascontiguousarray(cf[:, :1]), cu=np.ascontiguousarray(cf[:, 1:]))
    if "lin" in spec["on"]:                                       # two static state half-spaces around x0, one loose input half-space
        Ax, bx, _, _ = ihc.state_sets(x0, nx, N, rng)
        c["linear"] = (Ax, bx, rng.normal(0, 1, (B, 1, nu)), rng.uniform(0.3, 0.6, (B, 1)))
    return c


def oracle_loop(c, i, w=None, steps=T):
    """instance i's closed loop under the rows w [n, nx] (default: its own; None rows: none): the records after the last step, the
    iteration count (negative: not converged) and u0 of every step, x0 after the last plant step"""
    fam = c["fams"][i if c["hetero"] else 0]
    rows = c["w"][:, i] if w is None else w
    o = sc.make_solver(OracleSolver, fam, icc.config(c, i, max_iter=MAX_ITER))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    x0 = c["x0"][i].copy()
    its, u0s = [], []
    for k in range(steps):
        o["x"][:, 0] = x0
        o.solve()
        it = int(o.get("sol_iter"))
        its.append(it if int(o.get("sol_solved")) else -it)
        u0s.append(np.array(o["u"])[:, 0].copy())
        x1 = np.array(o["x"])[:, 1]
        x0 = x1 + rows[k] if k < len(rows) else x1.copy()
    rec = {k: np.array(o[k]) for k in keys(c)}
    o.close()
    return dict(rec=rec, iter=np.array(its), u0=np.array(u0s), x0=x0)


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    c = case(name)
    return [oracle_loop(c, i) for i in range(c["B"])]


def check_case(name):
    """the visibility condition, from the oracle alone"""
    c = case(name)
    own = oracle_case(name)
    B = c["B"]
    for i in range(B):
        r = own[i]
        assert np.max(np.abs(r["rec"]["x"])) < 100.0, ("instance %d: the loop diverges" % i)
        assert np.max(np.abs(r["iter"])) > 1, ("instance %d: nothing iterates" % i)
        for what, rows in (("the sequence of instance %d" % ((i + 1) % B), c["w"][:, (i + 1) % B]), ("its sequence shifted by one step", c["w"][1:, i])):
            other = oracle_loop(c, i, rows, steps=2)
            moved = float(np.max(np.abs(other["u0"][1] - r["u0"][1])))
            assert moved > 1e-6, ("instance %d under %s" % (i, what), moved)
