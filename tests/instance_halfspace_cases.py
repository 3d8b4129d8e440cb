"""The problems of tests/test_gpu_instance_halfspaces.py and their oracle solutions (CPU only; computed once per case and shared):
batches of 11 or 13 instances on random stable families (instance_bounds_cases.random_family), every instance its own static and
time-varying half-spaces, every drawn number distinct.  The sets are drawn so that the trajectories from the case's x0 meet them: a
state normal lies around the direction of x0 with its offset inside |a'x0| (knot 0, where x = x0, is outside for good), an input
normal around the direction of the input the problem applies at that knot while only its state half-spaces act (one oracle solve per
instance) with its offset inside |a'u|.  The conditions that make a misread block visible are
asserted here from the ORACLE's results alone (check_case): in every enabled family every instance has a knot whose dual is non-zero
after the solve (its last iterations projected), and solving instance i under instance i + 1's sets moves vnew | znew by more than
1e-6 -- a block read from the wrong instance, knot, slot or lane cannot pass."""
import functools

import numpy as np

import instance_bounds_cases as ibc
import scenarios as sc
from cpu_solvers import OracleSolver

BOX_KEYS = ibc.KEYS
MAX_ITER = 60
NS, NI, NTS, NTI = 2, 1, 1, 1                      # half-spaces per family (per knot for the time-varying set)
STATE_CONE = ([1], [3], [0.7])                   # the (6,3,10) case's cone: rows 1..3 of the state
FAMILY_FIELDS = {"sx": ("vlnew", "gl"), "su": ("zlnew", "yl"), "tx": ("vlnew_tv", "gl_tv"), "tu": ("zlnew_tv", "yl_tv")}


def families(lin):
    """the families a LIN value switches on: bit 0 the static set, bit 1 the time-varying one"""
    return (("sx", "su") if lin & 1 else ()) + (("tx", "tu") if lin & 2 else ())


def keys(lin, cone=False):
    """the records a solve with these families leaves"""
    return BOX_KEYS + tuple(k for f in families(lin) for k in FAMILY_FIELDS[f]) + (("vcnew", "gc") if cone else ())


RHO_SCALE = 0.1
RESEED = {(5, 3, 7, False, 11, 3, False, False): 1, (13, 3, 4, False, 11, 3, False, False): 2}      # cases whose first draw left an instance with a family that never projects (check_case)


def family(nx, nu, N, seed):
    """instance_bounds_cases.random_family with a tenth of its rho.  Every slack family that is on -- the box's always is -- adds its own
    rho-weighted term to the linear cost, while the cache is built for ONE such term (admm.cpp:262-304): with both half-space sets on
    the iteration sees three times the penalty its gains were computed for, and at the family's own rho (0.5 .. 5 against R = 0.1 .. 1)
    it does not contract -- the oracle itself diverges.  check_case asserts that it does not here."""
    fam = ibc.random_family(nx, nu, N, seed)
    fam["rho"] *= RHO_SCALE
    return fam


def state_sets(x0, nx, N, rng, ns=NS, nts=NTS):
    """Alin_x [B, ns, nx], blin_x [B, ns], tv_Alin_x [B, nts * N, nx] (row nts * i + k = constraint k at knot i), tv_blin_x [B, nts, N]"""
    B = x0.shape[0]
    d = x0 / np.linalg.norm(x0, axis=1, keepdims=True)

    def draw(rows):
        a = d[:, None, :] + rng.normal(0.0, 0.3, (B, rows, nx))
        return a, rng.uniform(0.6, 0.95, (B, rows)) * np.abs(np.einsum("brn,bn->br", a, x0))

    Ax, bx = draw(ns)
    tAx, tbx = draw(nts * N)
    return Ax, bx, tAx, np.ascontiguousarray(tbx.reshape(B, N, nts).transpose(0, 2, 1))      # (row nts * i + k is entry (k, i) of tv_blin_x)


def input_sets(u, nu, N, rng, ni=NI, nti=NTI):
    """u [B, nu, N - 1]: the inputs the normals are drawn around -> Alin_u [B, ni, nu], blin_u [B, ni], tv_Alin_u [B, nti * (N - 1), nu],
    tv_blin_u [B, nti, N - 1].  The static half-spaces are the tighter ones at knot 0, whose input both sets are drawn around: neither
    set shadows the other there, and the later knots belong to the time-varying one"""
    B = u.shape[0]

    def draw(at, lo, hi):                            # at [B, rows, nu]
        a = at / np.linalg.norm(at, axis=2, keepdims=True) + rng.normal(0.0, 0.3, at.shape)
        return a, rng.uniform(lo, hi, at.shape[:2]) * np.abs(np.einsum("brn,brn->br", a, at))

    Au, bu = draw(np.repeat(u[:, None, :, 0], ni, axis=1), 0.3, 0.55)
    tAu, tbu = draw(np.repeat(u.transpose(0, 2, 1), nti, axis=1), 0.6, 0.95)
    return Au, bu, tAu, np.ascontiguousarray(tbu.reshape(B, N - 1, nti).transpose(0, 2, 1))


def inputs_under_state_sets(c):
    """u [B, nu, N - 1] of every instance's problem under its state half-spaces alone (and its cone and box), inputs free: 200
    iterations of the oracle"""
    none = (np.zeros((0, c["nu"])), np.zeros(0))
    free = dict(c, linear=c["linear"][:2] + (np.zeros((c["B"], 0, c["nu"])), np.zeros((c["B"], 0))),
                tv_linear=c["tv_linear"][:2] + (np.zeros((c["B"], 0, c["nu"])), np.zeros((c["B"], 0, c["N"] - 1))))
    out = []
    for i in range(c["B"]):
        fam = c["fams"][i if c["hetero"] else 0]
        o = sc.make_solver(OracleSolver, fam, config(free, i, max_iter=200))
        o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
        o["x"][:, 0] = c["x0"][i]
        o.solve()
        out.append(np.array(o["u"]))
        o.close()
    return np.stack(out)


def draw_halfspaces(c, seed):
    """fills c["linear"] and c["tv_linear"] for the x0, references (cone, box) c holds"""
    rng = np.random.default_rng(seed)
    nx, nu, N = c["nx"], c["nu"], c["N"]
    Ax, bx, tAx, tbx = state_sets(c["x0"], nx, N, rng)
    c["linear"], c["tv_linear"] = (Ax, bx), (tAx, tbx)
    Au, bu, tAu, tbu = input_sets(inputs_under_state_sets(c), nu, N, rng)
    c["linear"], c["tv_linear"] = (Ax, bx, Au, bu), (tAx, tbx, tAu, tbu)
    drawn = np.concatenate([v.ravel() for v in c["linear"] + c["tv_linear"]])
    assert np.unique(drawn).size == drawn.size
    return c


@functools.lru_cache(maxsize=None)
def case(nx, nu, N, hetero, B, lin=3, cone=False, box=False):
    """the inputs of one batch: families (one, or one per instance), x0, references, every instance's half-spaces (and box)"""
    seed = 1000 * nx + 100 * nu + N + (7 if hetero else 0) + 31 * lin
    rng = np.random.default_rng(seed)
    fams = [family(nx, nu, N, seed + 17 * i) for i in range(B if hetero else 1)]
    x0 = rng.uniform(0.5, 1.0, (B, nx)) * rng.choice([-1.0, 1.0], (B, nx))
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    c = dict(nx=nx, nu=nu, N=N, B=B, hetero=hetero, lin=lin, cone=cone, fams=fams, x0=x0, Xref=Xref, Uref=Uref,
             box=ibc.boxes(B, nx, nu, N, seed + 9, True) if box else None)
    return draw_halfspaces(c, seed + 5 + RESEED.get((nx, nu, N, hetero, B, lin, cone, box), 0))


def config(c, i, sets_of=None, max_iter=MAX_ITER):
    """oracle/scenarios.py's configuration of instance i of case c under the sets of instance sets_of (default: its own)"""
    j = i if sets_of is None else sets_of
    lin = c["lin"]
    kw = dict(max_iter=max_iter, en_state_linear=lin & 1, en_input_linear=lin & 1, en_tv_state_linear=(lin >> 1) & 1, en_tv_input_linear=(lin >> 1) & 1,
              linear=tuple(a[j] for a in c["linear"]), tv_linear=tuple(a[j] for a in c["tv_linear"]))
    if c["cone"]:
        kw.update(en_state_soc=1, state_cone=STATE_CONE)
    # (the box is off unless the case has one, as in the reference's half-space examples: every slack family that is on adds its own
    # rho-weighted term to the linear cost while the cache is built for one, and with three of them the iteration need not contract)
    kw.update(en_state_bound=int(c["box"] is not None), en_input_bound=int(c["box"] is not None))
    if c["box"] is not None:
        kw.update(x_min=c["box"][0][j], x_max=c["box"][1][j], u_min=c["box"][2][j], u_max=c["box"][3][j])
    return sc.default_config(c["fams"][i if c["hetero"] else 0], **kw)


def oracle_solve(c, i, sets_of=None, max_iter=MAX_ITER, x0_scale=(1.0,)):
    """instance i of case c: [(records, iter, solved)] of successive solves from x0 * x0_scale[k] (the later ones warm-started)"""
    fam = c["fams"][i if c["hetero"] else 0]
    o = sc.make_solver(OracleSolver, fam, config(c, i, sets_of, max_iter))
    o["Xref"], o["Uref"] = c["Xref"][i], c["Uref"][i]
    out = []
    for scale in x0_scale:
        o["x"][:, 0] = c["x0"][i] * scale
        o.solve()
        out.append(({k: np.array(o[k]) for k in keys(c["lin"], c["cone"])}, int(o.get("sol_iter")), int(o.get("sol_solved"))))
    o.close()
    return out


@functools.lru_cache(maxsize=None)
def oracle_case(nx, nu, N, hetero, B, lin=3, cone=False, box=False):
    """every instance's cold solve and warm second solve from 0.9 x0 under its own sets"""
    c = case(nx, nu, N, hetero, B, lin, cone, box)
    return [oracle_solve(c, i, x0_scale=(1.0, 0.9)) for i in range(B)]


def check_case(nx, nu, N, hetero, B, lin=3, cone=False, box=False):
    """the conditions on the inputs, from the oracle alone"""
    c = case(nx, nu, N, hetero, B, lin, cone, box)
    own = oracle_case(nx, nu, N, hetero, B, lin, cone, box)
    for i in range(B):
        r = own[i][0][0]
        assert max(np.max(np.abs(r["x"])), np.max(np.abs(r["u"]))) < 100.0, ("instance %d: the iteration diverges" % i)
        for f in families(lin):
            dual = r[FAMILY_FIELDS[f][1]]
            assert np.any(dual != 0.0), ("instance %d: family %s never projected" % (i, f))
        other = oracle_solve(c, i, sets_of=(i + 1) % B)[0][0]
        moved = max(np.max(np.abs(other["vnew"] - r["vnew"])), np.max(np.abs(other["znew"] - r["znew"])))
        assert moved > 1e-6, ("instance %d under the sets of instance %d" % (i, (i + 1) % B), moved)


# every case the GPU tests use: (nx, nu, N, hetero, B, lin, cone, box)
GPU_CASES = [(12, 4, 10, False, 13, 1, False, False), (12, 4, 10, False, 13, 2, False, False), (12, 4, 10, False, 13, 3, False, False),
             (12, 4, 10, True, 11, 3, False, False), (6, 3, 10, False, 13, 3, True, False), (5, 3, 7, False, 11, 3, False, False),
             (4, 2, 30, False, 11, 2, False, False), (20, 4, 10, False, 11, 3, False, False), (12, 4, 10, False, 11, 2, False, True),
             (13, 3, 4, False, 11, 3, False, False)]                # all 16 lanes in use, the inputs in lanes 13..15, N - 1 = 3


@functools.lru_cache(maxsize=None)
def launch_case():
    """(12,4,10), 13 instances, both sets, x0 and the references scaled instance by instance from 1e-3 to 1, the half-spaces drawn
    around the scaled problem: the cold iteration counts run from a handful to the cap (straddling 10: what a split solve at K = 10
    needs)"""
    c = dict(case(12, 4, 10, False, 13, 3))
    scale = np.logspace(-3, 0, 13)
    c["x0"] = c["x0"] * scale[:, None]
    c["Xref"] = c["Xref"] * scale[:, None, None]
    c["Uref"] = c["Uref"] * scale[:, None, None]
    return draw_halfspaces(c, 4242)
