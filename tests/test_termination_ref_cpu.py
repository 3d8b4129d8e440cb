"""CPU: the preconditions of tests/termination_ref.py, asserted on the oracle for every shape tests/test_gpu_termination_edges.py runs.
They are conditions, not measurements: the GPU test concludes "the kernel missed position (j, k)" from iter = 1 where the oracle has
3, which only follows if on the oracle that position alone keeps the solve open, with room on both sides of the decision."""
import numpy as np
import pytest

import scenarios as sc
import termination_ref as tr
from cpu_solvers import OracleSolver

SHAPES = [(4, 2, 10), (12, 4, 10), (4, 2, 30), (20, 4, 10), (4, 2, 50), (12, 8, 30), (12, 4, 50), (5, 3, 7)]


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "%d_%d_%d" % d)
def test_one_position_alone_keeps_each_solve_open(dims):
    nx, nu, N = dims
    suite, table = tr.position_suite(*dims, max_iter=1)
    prob, cases = suite["problem"], suite["cases"]
    B = len(table)
    kind = table[:, 0]
    n_pos = nx * N + nu * (N - 1)
    assert (kind == tr.PRI).sum() == n_pos and (kind == tr.DUA).sum() == n_pos                    # no position left out
    assert sorted(map(tuple, table[kind == tr.PRI][:, 1:])) == sorted(tr.positions(*dims)) == sorted(map(tuple, table[kind == tr.DUA][:, 1:]))
    # controls and offenders of both kinds in every row position of a wave (4) and of a HALF wave (8)
    for m in (4, 8):
        for r in range(m):
            assert {tr.CTL, tr.PRI, tr.DUA} <= set(kind[np.arange(B) % m == r]), (m, r)
    one = sc.run_cases(OracleSolver, suite)
    tol = np.array([suite["config"]["abs_pri_tol"], suite["config"]["abs_dua_tol"]] * 2)
    got = np.stack([one[k] for k in tr.RESIDUALS], axis=1)
    mine = tr.residuals(prob, cases, one)
    fields = tr.residual_fields(prob, cases, one)
    for i, k in enumerate(tr.RESIDUALS):
        assert np.array_equal(mine[k], one[k]), k                                                 # the numpy residuals ARE the oracle's
    ctl = kind == tr.CTL
    assert np.all(one["iter"][ctl] == 1) and np.all(one["sol_solved"][ctl] == 1) and np.all(one["status"][ctl] == 1)
    assert np.all(got[ctl] == 0.0)
    assert np.all(one["iter"][~ctl] == 1) and not one["sol_solved"][~ctl].any()
    margins = []
    for b in np.flatnonzero(~ctl):
        c = tr.residual_index(kind[b], table[b, 1], nx)
        assert got[b, c] >= 2 * tol[c], (tr.describe(table, b), got[b], tol)
        others = np.delete(got[b] / tol, c)
        assert np.all(others <= 0.5), (tr.describe(table, b), got[b], tol)
        f = np.sort(fields[tr.RESIDUALS[c]][b].ravel())
        j, k = table[b, 1] - (nx if table[b, 1] >= nx else 0), table[b, 2]
        assert fields[tr.RESIDUALS[c]][b, j, k] == f[-1] and f[-2] <= 0.5 * tol[c], tr.describe(table, b)    # the maximum IS the position, alone
        margins.append((got[b, c] / tol[c], others.max(), f[-2] / tol[c]))
    margins = np.array(margins)
    full = sc.run_cases(OracleSolver, tr.with_config(suite, max_iter=40))
    assert np.all(full["sol_solved"] == 1) and np.all(full["iter"][ctl] == 1) and np.all(full["iter"][~ctl] >= 2)
    assert np.all(full["iter"] < 40)
    print("termination positions %s: B %d, offender / tol %.3f..%.3f, other kinds / tol <= %.3g, second entry / tol <= %.3g, iters %s"
          % (dims, B, margins[:, 0].min(), margins[:, 0].max(), margins[:, 1].max(), margins[:, 2].max(),
             dict(zip(*[a.tolist() for a in np.unique(full["iter"][~ctl].astype(int), return_counts=True)]))))


@pytest.mark.parametrize("dims", SHAPES, ids=lambda d: "%d_%d_%d" % d)
@pytest.mark.parametrize("kind", [tr.PRI, tr.DUA], ids=["pri", "dua"])
def test_a_residual_equal_to_its_tolerance_does_not_stop_the_solve(dims, kind):
    nx, nu, N = dims
    for above in (False, True):
        suite, table = tr.strict_suite(*dims, kind, above)
        prob = suite["problem"]
        assert not prob["f"].any()
        off = table[:, 0] != tr.CTL
        assert off.sum() == (nx if kind == tr.PRI else nx * N + nu * (N - 1))
        one = sc.run_cases(OracleSolver, tr.with_config(suite, max_iter=1))
        assert not one["x"].any() and not one["u"].any()                                          # the trajectory stays zero
        r = tr.strict_residual(prob, kind)
        for b in np.flatnonzero(off):
            c = tr.residual_index(kind, table[b, 1], nx)
            got = [one[k][b] for k in tr.RESIDUALS]
            assert got[c] == r and not np.delete(got, c).any(), (tr.describe(table, b), got)       # exactly DELTA | fl(DELTA rho), the rest 0
        assert not np.stack([one[k][~off] for k in tr.RESIDUALS]).any()
        out = sc.run_cases(OracleSolver, suite)
        assert np.all(out["sol_solved"] == 1)
        assert np.all(out["iter"][~off] == 1)
        assert np.all(out["iter"][off] == (1 if above else 2)), (above, out["iter"][off])
        assert np.all(one["sol_solved"][off] == (1 if above else 0))
