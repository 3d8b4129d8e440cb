"""TEST INFRASTRUCTURE -- batches on which ONE entry of ONE residual decides whether a solve stops (admm.cpp:310-328).

termination_condition stops a solve when all four maxima -- max|x - vnew|, rho max|v - vnew| and the two input ones -- are below their
tolerances.  On random problems dozens of entries are above tolerance at every check, so a test that drops a row, a knot or a whole
residual kind is never seen.  Here every (row j, knot k, kind) in turn is the only entry that keeps a solve open:

* no bounds, cones or half-spaces, so vnew = x + g and znew = u + y: the primal residual at an entry is |x - (x + g_warm)|, exactly 0
  where the warm dual is 0; work->v | z on entry reach nothing but the dual residual of iteration 1; q, r, p, d are no inputs at all
  (the loop opens with update_linear_cost);
* the base case of a shape: a random x0, every warm field zero.  Its iteration-1 slacks vnew1 | znew1 as warm v | z make the dual
  residual of iteration 1 zero: the CONTROL, which stops at iteration 1 with all four residuals 0;
* "pri" at (j, k): g[j,k] = DELTA (y for an input row) and v | z = that instance's own iteration-1 slacks;
* "dua" at (j, k): v | z = vnew1 | znew1 of the base case with DELTA added at (j, k);
* tolerances DELTA / 4 and rho DELTA / 4: the offending kind sits at 4x its tolerance, the other three at 0, and every offender stops
  at a later iteration.  After every 4 offenders comes a control (period 5, coprime to the 4 | 8 instances of a wave), so controls and
  offenders meet in every row and half-row position of a wave.

A kernel that misses the offender reports iter = 1, solved = 1; one that hears a neighbour's offender, a dummy slot or a pad lane
leaves a control open.  tests/test_termination_ref_cpu.py asserts these preconditions on the oracle for every shape used on the GPU.

strict_suite() is the equality case: x0 = 0, references 0, f = 0, so x = u = 0 exactly on any implementation and a residual is
exactly DELTA (primal, knot 0 of a state row: x[:,0] = x0 is never rewritten and q_0 does not reach the backward pass) or
fl(DELTA rho) (dual, any position).  With the tolerance EQUAL to the residual the strict `<` keeps the solve open for one more
iteration; with the next double above it, it stops at iteration 1.
"""
import copy
import functools

import numpy as np

import scenarios as sc
from cpu_solvers import OracleSolver

DELTA = 2.0 ** -7
CTL, PRI, DUA = 0, 1, 2
KIND = ("ctl", "pri", "dua")
RESIDUALS = ("primal_residual_state", "dual_residual_state", "primal_residual_input", "dual_residual_input")
SCALARS = ("iter", "sol_solved", "status") + RESIDUALS
PERIOD = 5                      # offenders 4 : control 1


def problem(nx, nu, N):
    prob, _ = sc.random_problem(nx, nu, N)
    return prob


def config(prob, max_iter, check_termination=1, pri=None, dua=None):
    return sc.default_config(prob, max_iter=max_iter, check_termination=check_termination, en_state_bound=0, en_input_bound=0,
                             abs_pri_tol=DELTA / 4 if pri is None else pri, abs_dua_tol=prob["rho"] * DELTA / 4 if dua is None else dua)


def with_config(suite, **kw):
    """the same problem and cases under other settings (max_iter, check_termination, abs_pri_tol, abs_dua_tol)"""
    return dict(suite, config=dict(suite["config"], **kw))


def positions(nx, nu, N):
    """every (row, knot): state rows j < nx at k < N, input rows nx <= j < nx + nu at k < N - 1"""
    return [(j, k) for j in range(nx) for k in range(N)] + [(nx + j, k) for j in range(nu) for k in range(N - 1)]


def residual_index(kind, j, nx):
    """which of RESIDUALS an offender of this kind at row j raises"""
    return (0 if kind == PRI else 1) + (2 if j >= nx else 0)


def _first_slacks(cls, prob, cases):
    """vnew | znew of iteration 1 (max_iter = 1, tolerances 0: no solve stops)"""
    out = sc.run_cases(cls, dict(problem=prob, config=config(prob, 1, pri=0.0, dua=0.0), cases=cases), fields=("vnew", "znew"))
    assert not out["sol_solved"].any()
    return out["vnew"], out["znew"]


def _interleave(offenders):
    """a control after every 4 offenders (and one at the end): -> list of offender indices, -1 = control"""
    order = []
    for n in range(len(offenders)):
        order.append(n)
        if n % (PERIOD - 1) == PERIOD - 2:
            order.append(-1)
    if order[-1] != -1:
        order.append(-1)
    return order


def _add(field_x, field_u, b, j, k, nx, value):
    if j < nx:
        field_x[b, j, k] += value
    else:
        field_u[b, j - nx, k] += value


@functools.lru_cache(maxsize=None)
def _position_suite(nx, nu, N, cls):
    prob = problem(nx, nu, N)
    rng = np.random.default_rng([nx, nu, N, 20261019])
    x0 = rng.uniform(-0.3, 0.3, nx)
    pos = positions(nx, nu, N)
    offenders = [(kind, j, k) for j, k in pos for kind in (PRI, DUA)]
    order = _interleave(offenders)
    B = len(order)
    cases = sc.zero_cases(prob, B)
    cases["x0"][:] = x0
    table = np.zeros((B, 3), dtype=np.int32)                      # kind, j, k
    for b, n in enumerate(order):
        table[b] = (CTL, -1, -1) if n < 0 else offenders[n]
        if n >= 0 and offenders[n][0] == PRI:
            _add(cases["g"], cases["y"], b, offenders[n][1], offenders[n][2], nx, DELTA)
    # warm v | z: every instance's own iteration-1 slacks (the base case's for controls and dua: their warm duals are zero) ...
    cases["v"], cases["z"] = _first_slacks(cls, prob, cases)
    # ... plus DELTA at the dua position
    for b in np.flatnonzero(table[:, 0] == DUA):
        _add(cases["v"], cases["z"], b, table[b, 1], table[b, 2], nx, DELTA)
    return dict(problem=prob, config=config(prob, 40), cases=cases), table


def position_suite(nx, nu, N, cls=OracleSolver, **cfg):
    """-> (suite for run_cases / run_cases_hip, table[B, 3] of (kind, j, k)); max_iter = 40, check_termination = 1 unless given"""
    suite, table = _position_suite(nx, nu, N, cls)
    return with_config(copy.deepcopy(suite), **cfg), table.copy()


@functools.lru_cache(maxsize=None)
def _strict_suite(nx, nu, N, kind):
    prob = dict(problem(nx, nu, N))
    prob["f"] = np.zeros(nx)                                      # (random_problem has f = 0 already)
    pos = positions(nx, nu, N) if kind == DUA else [(j, 0) for j in range(nx)]
    offenders = [(kind, j, k) for j, k in pos]
    order = _interleave(offenders)
    B = len(order)
    cases = sc.zero_cases(prob, B)
    table = np.zeros((B, 3), dtype=np.int32)
    for b, n in enumerate(order):
        table[b] = (CTL, -1, -1) if n < 0 else offenders[n]
        if n >= 0:
            j, k = offenders[n][1:]
            if kind == DUA:
                _add(cases["v"], cases["z"], b, j, k, nx, DELTA)
            else:                                                 # vnew1[j,0] = x0 + g = DELTA: v takes it, so the dual residual is 0
                cases["g"][b, j, 0] = DELTA
                cases["v"][b, j, 0] = DELTA
    return dict(problem=prob, config=config(prob, 40), cases=cases), table


def strict_residual(prob, kind):
    """the one residual of a strict_suite offender, exact on any implementation"""
    return np.float64(DELTA) if kind == PRI else np.float64(DELTA) * np.float64(prob["rho"])


def strict_suite(nx, nu, N, kind, above, **cfg):
    """kind PRI: g[j,0] = DELTA on every state row; kind DUA: v | z = DELTA at every position.  above = False: the tolerance of that
    kind EQUALS the residual (oracle: iter = 2); True: the next double above it (oracle: iter = 1).  The other tolerance: for DUA the
    usual DELTA / 4 (the primal residuals are 0); for PRI 2 rho DELTA, because iteration 2 sees v = vnew1 = DELTA against vnew = 0."""
    suite, table = _strict_suite(nx, nu, N, kind)
    prob = suite["problem"]
    r = strict_residual(prob, kind)
    tol = np.nextafter(r, np.inf) if above else r
    tols = dict(abs_pri_tol=float(tol), abs_dua_tol=2 * prob["rho"] * DELTA) if kind == PRI else dict(abs_pri_tol=DELTA / 4, abs_dua_tol=float(tol))
    return with_config(copy.deepcopy(suite), **dict(tols, **cfg)), table.copy()


def residual_fields(prob, cases, out):
    """the per-element terms of the four residuals of ITERATION 1 of a solve: the solve's x, vnew, u, znew after max_iter = 1 and the
    v | z it was GIVEN (a solve that does not stop overwrites v with vnew, admm.cpp:445) -> dict name -> [B, rows, knots]"""
    rho = prob["rho"]
    return {"primal_residual_state": np.abs(out["x"] - out["vnew"]), "dual_residual_state": np.abs(cases["v"] - out["vnew"]) * rho,
            "primal_residual_input": np.abs(out["u"] - out["znew"]), "dual_residual_input": np.abs(cases["z"] - out["znew"]) * rho}


def residuals(prob, cases, out):
    """the four scalars of iteration 1 (admm.cpp:314-317), [B] each"""
    return {k: f.reshape(f.shape[0], -1).max(axis=1) for k, f in residual_fields(prob, cases, out).items()}


def noise_floor(prob, out, rtol):
    """what a residual that is 0 on the oracle may be on another implementation whose slacks agree with the oracle's to rtol of their
    largest entry: the warm v | z are the ORACLE's vnew1 | znew1, so rho |v - vnew| is rho times that disagreement"""
    return rtol * prob["rho"] * max(float(np.max(np.abs(out["vnew"]))), float(np.max(np.abs(out["znew"]))))


def wave_position(b):
    return "instance %d (row %d of 4, half row %d of 8)" % (b, b % 4, b % 8)


def describe(table, b):
    kind, j, k = (int(v) for v in table[b])
    return "%s at (j=%d, k=%d), %s" % (KIND[kind], j, k, wave_position(b)) if kind != CTL else "control, " + wave_position(b)
