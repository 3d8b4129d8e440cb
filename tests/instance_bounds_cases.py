"""The problems of tests/test_gpu_instance_bounds.py and their oracle solutions (CPU only; computed once per case and shared): batches
of 11 or 13 instances, every instance its own box -- knot-invariant, or every (instance, row, knot) bound pair distinct.  The
conditions that make a misread bound visible are asserted here from the ORACLE's results alone (check_case): every instance has a
state entry of vnew and an input entry of znew on a bound, and solving instance i under instance i + 1's box moves vnew | znew by more
than 1e-6 -- a bound read from the wrong instance, slot or lane cannot pass."""
import functools

import numpy as np

import scenarios as sc
from cpu_solvers import OracleSolver

KEYS = ("x", "u", "vnew", "znew", "g", "y", "v", "z")
MAX_ITER = 60
# nx + nu = 16 split as one input / one state: the lane tables are [batch][16] blocks, and here the field boundary sits at lane 15 / lane 1
# (the per-instance box, disturbance and plant cases all take these two shapes)
EDGE_SHAPES = [(15, 1, 3), (1, 15, 3)]


def random_family(nx, nu, N, seed):
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((nx, nx))
    A = M * rng.uniform(0.7, 0.99) / np.max(np.abs(np.linalg.eigvals(M)))
    return dict(nx=nx, nu=nu, N=N, rho=float(rng.uniform(0.5, 5.0)), A=A, B=rng.standard_normal((nx, nu)) / np.sqrt(nx),
                f=rng.normal(0, 0.01, nx), Q=rng.uniform(1, 10, nx), R=rng.uniform(0.1, 1, nu))


def boxes(B, nx, nu, N, seed, varying):
    """x_min, x_max [B, nx, N], u_min, u_max [B, nu, N-1]: finite, non-zero, every drawn number distinct.  Narrow enough that the
    trajectories from the cases' x0 (0.5 <= |x0_j| <= 1) meet them."""
    rng = np.random.default_rng(seed)
    kx, ku = (N, N - 1) if varying else (1, 1)
    xw, uw = rng.uniform(0.15, 0.45, (2, B, nx, kx)), rng.uniform(0.02, 0.2, (2, B, nu, ku))
    out = [np.broadcast_to(-xw[0], (B, nx, N)), np.broadcast_to(xw[1], (B, nx, N)), np.broadcast_to(-uw[0], (B, nu, N - 1)), np.broadcast_to(uw[1], (B, nu, N - 1))]
    drawn = np.concatenate([xw.ravel(), uw.ravel()])
    assert np.unique(drawn).size == drawn.size
    return [np.ascontiguousarray(a) for a in out]


@functools.lru_cache(maxsize=None)
def case(nx, nu, N, hetero, varying, B):
    """the inputs of one batch: families (one, or one per instance), x0, references, boxes"""
    seed = 1000 * nx + 100 * nu + N + (7 if hetero else 0) + (3 if varying else 0)
    rng = np.random.default_rng(seed)
    fams = [random_family(nx, nu, N, seed + 17 * i) for i in range(B if hetero else 1)]
    x0 = rng.uniform(0.5, 1.0, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))      # (beyond every state bound: knot 0 is clamped)
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    return dict(nx=nx, nu=nu, N=N, B=B, hetero=hetero, fams=fams, x0=x0, Xref=Xref, Uref=Uref, box=boxes(B, nx, nu, N, seed + 5, varying))


def oracle_solve(c, i, box_of=None, max_iter=MAX_ITER, x0_scale=(1.0,)):
    """instance i of case c under the box of instance box_of (default: its own): [(records, iter, solved)] of successive solves from
    x0 * x0_scale[k] (the second and later ones warm-started)"""
    fam = c["fams"][i if c["hetero"] else 0]
    j = i if box_of is None else box_of
    cfg = sc.default_config(fam, max_iter=max_iter, x_min=c["box"][0][j], x_max=c["box"][1][j], u_min=c["box"][2][j], u_max=c["box"][3][j])
    o = sc.make_solver(OracleSolver, fam, cfg)
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    out = []
    for scale in x0_scale:
        o["x"][:, 0] = c["x0"][i] * scale
        o.solve()
        out.append(({k: np.array(o[k]) for k in KEYS}, int(o.get("sol_iter")), int(o.get("sol_solved"))))
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(nx, nu, N, hetero, varying, B):
    """every instance's cold solve and warm second solve from 0.9 x0 under its own box"""
    c = case(nx, nu, N, hetero, varying, B)
    return [oracle_solve(c, i, x0_scale=(1.0, 0.9)) for i in range(B)]


def check_case(nx, nu, N, hetero, varying, B):
    """the conditions on the inputs, from the oracle alone"""
    c = case(nx, nu, N, hetero, varying, B)
    own = oracle_case(nx, nu, N, hetero, varying, B)
    for i in range(B):
        r = own[i][0][0]
        on_x = (r["vnew"] == c["box"][0][i]) | (r["vnew"] == c["box"][1][i])
        on_u = (r["znew"] == c["box"][2][i]) | (r["znew"] == c["box"][3][i])
        assert on_x.any() and on_u.any(), ("instance %d: no active state / input bound" % i, int(on_x.sum()), int(on_u.sum()))
        other = oracle_solve(c, i, box_of=(i + 1) % B)[0][0]
        moved = max(np.max(np.abs(other["vnew"] - r["vnew"])), np.max(np.abs(other["znew"] - r["znew"])))
        assert moved > 1e-6, ("instance %d under the box of instance %d" % (i, (i + 1) % B), moved)


@functools.lru_cache(maxsize=None)
def launch_case():
    """(12,4,10), 13 instances, every bound pair distinct, x0 and the references scaled instance by instance from 1e-3 to 1: the cold
    iteration counts run from a handful to the cap (straddling 10: what a split solve at K = 10 needs)"""
    c = dict(case(12, 4, 10, False, True, 13))
    scale = np.logspace(-3, 0, 13)
    c["x0"] = c["x0"] * scale[:, None]
    c["Xref"] = c["Xref"] * scale[:, None, None]
    c["Uref"] = c["Uref"] * scale[:, None, None]
    return c
