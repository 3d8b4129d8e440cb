"""The problems of tests/test_gpu_plant.py, the reference plant step and the oracle closed loops stepped by it (CPU only; computed once
per case and shared).  The plant step of tiny_batch_set_plant, restated: state row j of an instance becomes

    acc = f_p[j];  acc = fma(x0[k], A_p[j][k], acc), k = 0 .. nx-1;  acc = fma(u0[k], B_p[j][k], acc), k = 0 .. nu-1

one chain, one rounding per term.  Python 3.10 has no math.fma: float(Fraction(a) * Fraction(b) + Fraction(c)) is the exact sum, rounded
once (Fraction -> float rounds correctly).

Cases: (4,2,10), a half-row shape, 13 instances; (5,3,7), not compiled in, nx no multiple of 4, 11 instances; (12,4,10), the shape whose
chain is cut into blocks, 2 instances -- the last tile has 1, 3 or 2 rows; T = 5 MPC steps.  Every instance's plant is the model perturbed
entry by entry: a factor 1 +- (1 .. 5) % and an offset of +- (0.002 .. 0.01), so that A_p differs from A in every entry of every row.
check_case asserts, from the ORACLE alone, that stepping instance i by the plant of instance i + 1, by the model, or by its own plant with
the A_p and B_p columns read in swapped order (the B_p columns against the leading entries of [x0 | u0], the A_p columns against the
rest: a lane or column misread) moves the u0 of a later step by more than 1e-6 relative -- the 1e-9 comparison of the GPU tests tells
every such misread apart."""
import functools
from fractions import Fraction

import numpy as np

import disturbance_cases as dc
import instance_bounds_cases as ibc
import instance_cone_cases as icc
import scenarios as sc
from cpu_solvers import OracleSolver

MAX_ITER = dc.MAX_ITER
T = 5
N_STEPS = 4                                       # rows of the disturbance sequence of the composition tests
KEYS = ibc.KEYS

CASES = {
    "4_2_10": dict(shape=(4, 2, 10), B=13, hetero=False),
    "5_3_7": dict(shape=(5, 3, 7), B=11, hetero=False),
    "12_4_10": dict(shape=(12, 4, 10), B=2, hetero=False),
    "12_4_10_hetero": dict(shape=(12, 4, 10), B=11, hetero=True),      # per-instance problem data (composition; plant equal to the model)
    "6_3_10": dict(shape=(6, 3, 10), B=11, hetero=False),              # composition with PB / PD; the sharded group
    "20_8_10": dict(shape=(20, 8, 10), B=11, hetero=False),            # a tile-kernel shape: the coverage path
    # the extreme splits of a full row (instance_bounds_cases.EDGE_SHAPES): a chain of 15 A_p terms and one B_p term, and the reverse
    "15_1_3": dict(shape=ibc.EDGE_SHAPES[0], B=11, hetero=False),
    "1_15_3": dict(shape=ibc.EDGE_SHAPES[1], B=11, hetero=False),
}
ORACLE_CASES = ("4_2_10", "5_3_7", "12_4_10")
EDGE_CASES = ("15_1_3", "1_15_3")                 # every instance against its own oracle loop, as ORACLE_CASES (test a. of tests/test_gpu_plant.py)


def fma(a, b, c):
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def plant_step(A_p, B_p, f_p, x0, u0):
    """the reference plant step of ONE instance: A_p (nx, nx), B_p (nx, nu), f_p (nx,) or None, x0 (nx,), u0 (nu,) -> (nx,)"""
    nx, nu = B_p.shape
    out = np.zeros(nx)
    for j in range(nx):
        acc = 0.0 if f_p is None else float(f_p[j])
        for k in range(nx):
            acc = fma(x0[k], A_p[j, k], acc)
        for k in range(nu):
            acc = fma(u0[k], B_p[j, k], acc)
        out[j] = acc
    return out


def plant_step_batch(plant, x0, u0):
    """every instance by its own plant: plant = (A_p [B, nx, nx], B_p [B, nx, nu], f_p [B, nx] or None)"""
    A, Bm, f = plant
    return np.array([plant_step(A[i], Bm[i], None if f is None else f[i], x0[i], u0[i]) for i in range(len(x0))])


def swapped_columns_step(A_p, B_p, f_p, x0, u0):
    """the misread of the docstring: the row [B_p[j] | A_p[j]] against [x0 | u0]"""
    z = np.concatenate([x0, u0])
    rows = np.concatenate([B_p, A_p], axis=1)
    return f_p + rows @ z


@functools.lru_cache(maxsize=None)
def case(name):
    """the inputs of one batch in the layout instance_cone_cases.config reads (a shared, knot-invariant box), the plants and a
    disturbance sequence w [N_STEPS, B, nx] for the composition tests"""
    spec = CASES[name]
    nx, nu, N = spec["shape"]
    B = spec["B"]
    seed = 31 * (1000 * nx + 100 * nu + N) + sum(map(ord, name))
    rng = np.random.default_rng(seed)
    fams = [ibc.random_family(nx, nu, N, seed + 17 * i) for i in range(B if spec["hetero"] else 1)]
    x0 = rng.uniform(0.5, 1.0, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    w = 0.1 * rng.uniform(0.5, 1.0, (N_STEPS, B, nx)) * rng.choice([-1.0, 1.0], (N_STEPS, B, nx))
    box = dc.wide_boxes(B, nx, nu, N, seed + 9)
    own_box = box
    box = [np.ascontiguousarray(np.broadcast_to(a[:1], a.shape)) for a in box]
    model = tuple(np.stack([fams[i if spec["hetero"] else 0][k] for i in range(B)]) for k in ("A", "B", "f"))

    def perturbed(m):
        factor = 1.0 + rng.uniform(0.01, 0.05, m.shape) * rng.choice([-1.0, 1.0], m.shape)
        offset = rng.uniform(0.002, 0.01, m.shape) * rng.choice([-1.0, 1.0], m.shape)
        return m * factor + offset
    plant = tuple(perturbed(m) for m in model)
    assert all(np.all(p != m) for p, m in zip(plant, model))
    return dict(spec, name=name, nx=nx, nu=nu, N=N, fams=fams, x0=x0, Xref=Xref, Uref=Uref, w=w, box=box, own_box=own_box, linear=None, extra=None,
                Acx=[], Acu=[], cx=np.zeros((B, 0)), cu=np.zeros((B, 0)), on=(0, 0), has=("box",), own=(), model=model, plant=plant)


def plant_for(c, seed=4242):
    """plants for a case of another case file (disturbance_cases: the PL and PC compositions): its model perturbed as above"""
    rng = np.random.default_rng(seed)
    B = c["B"]
    model = tuple(np.stack([c["fams"][i if c["hetero"] else 0][k] for i in range(B)]) for k in ("A", "B", "f"))
    plant = tuple(m * (1.0 + rng.uniform(0.01, 0.05, m.shape) * rng.choice([-1.0, 1.0], m.shape)) + rng.uniform(0.002, 0.01, m.shape) * rng.choice([-1.0, 1.0], m.shape)
                  for m in model)
    assert all(np.all(p != m) for p, m in zip(plant, model))
    return plant


def oracle_loop(c, i, step=None, steps=T):
    """instance i's closed loop on the oracle, handed on by step(x0, u0) (default: the reference plant step under its own plant): the
    records after the last step, the iteration count (negative: not converged), u0 and the state handed on of every step"""
    A, Bm, f = (m[i] for m in c["plant"])
    step = step or (lambda x0, u0: plant_step(A, Bm, f, x0, u0))
    o = sc.make_solver(OracleSolver, c["fams"][i if c["hetero"] else 0], icc.config(c, i, max_iter=MAX_ITER))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    x0 = c["x0"][i].copy()
    its, u0s, xs = [], [], []
    for _ in range(steps):
        o["x"][:, 0] = x0
        o.solve()
        it = int(o.get("sol_iter"))
        its.append(it if int(o.get("sol_solved")) else -it)
        u0 = np.array(o["u"])[:, 0].copy()
        u0s.append(u0)
        x0 = np.asarray(step(x0, u0), dtype=float)
        xs.append(x0.copy())
    rec = {k: np.array(o[k]) for k in KEYS}
    o.close()
    return dict(rec=rec, iter=np.array(its), u0=np.array(u0s), x0=x0, states=np.array(xs))


@functools.lru_cache(maxsize=None)
def oracle_case(name):
    c = case(name)
    return [oracle_loop(c, i) for i in range(c["B"])]


def check_case(name):
    """the visibility condition, from the oracle alone"""
    c = case(name)
    own = oracle_case(name)
    B = c["B"]
    A, Bm, f = c["plant"]
    mA, mB, mf = c["model"]
    for i in range(B):
        r = own[i]
        assert np.max(np.abs(r["rec"]["x"])) < 100.0, ("instance %d: the loop diverges" % i)
        assert np.max(np.abs(r["iter"])) > 1, ("instance %d: nothing iterates" % i)
        n = (i + 1) % B
        others = (("the plant of instance %d" % n, lambda x0, u0: plant_step(A[n], Bm[n], f[n], x0, u0)),
                  ("the model", lambda x0, u0: plant_step(mA[i], mB[i], mf[i], x0, u0)),
                  ("its plant with the A_p and B_p columns swapped", lambda x0, u0: swapped_columns_step(A[i], Bm[i], f[i], x0, u0)))
        for what, step in others:
            other = oracle_loop(c, i, step, steps=3)
            moved = max(float(np.max(np.abs(other["u0"][k] - r["u0"][k])) / max(np.max(np.abs(r["u0"][k])), 1e-300)) for k in (1, 2))
            assert moved > 1e-6, ("instance %d under %s" % (i, what), moved)
