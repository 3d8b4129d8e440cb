"""CPU: pins tests/riccati_ref.py -- the extended-precision reference of the cache precompute -- against the real reference's stored
caches and the oracle, and asserts on the reference alone that every instance set of riccati_ref.py -- the inputs of
tests/test_gpu_riccati.py -- reaches the code it is meant to reach: row exchanges in the pivot sets, step counts decided well away from
the 1e-5 threshold, the cap, the single step, a refused inversion, and solves the oracle itself does not amplify."""
import os

import numpy as np
import pytest

import riccati_ref as rr
import scenarios as sc
from cpu_solvers import OracleSolver

if np.finfo(np.longdouble).eps >= 1e-18:
    pytest.skip("np.longdouble is no wider than float64 on this platform (eps %.3g): there is no extended-precision reference here"
                % np.finfo(np.longdouble).eps, allow_module_level=True)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def random_family(nx, nu, N, seed):      # as tests/test_gpu_hetero.py
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((nx, nx))
    A = M * rng.uniform(0.7, 0.99) / np.max(np.abs(np.linalg.eigvals(M)))
    return dict(nx=nx, nu=nu, N=N, rho=float(rng.uniform(0.5, 5.0)), A=A, B=rng.standard_normal((nx, nu)) / np.sqrt(nx),
                f=rng.normal(0, 0.01, nx), Q=rng.uniform(1, 10, nx), R=rng.uniform(0.1, 1, nu))


# ---- the reference itself
def test_inverse_counts_exchanges_and_refuses_a_zero_pivot():
    G = np.array([[1.0, 2.0, 0.0], [4.0, 1.0, 1.0], [2.0, 7.0, 1.0]], dtype=rr.LD)     # column 0 takes row 1, column 1 then row 2
    Gi, swaps = rr.inverse(G)
    assert swaps == 2 and rr.rel_dev(Gi @ G, np.eye(3, dtype=rr.LD)) < 1e-18
    Gi, swaps = rr.inverse(np.diag(np.array([3.0, 2.0, 5.0], dtype=rr.LD)))
    assert swaps == 0 and np.array_equal(np.diag(Gi), np.array([1.0, 1.0, 1.0], dtype=rr.LD) / np.array([3.0, 2.0, 5.0], dtype=rr.LD))
    assert rr.inverse(np.array([[1.0, 0.0], [0.0, 0.0]], dtype=rr.LD))[0] is None
    Gi, swaps = rr.inverse(np.array([[1.0, 5.0], [-1.0, 2.0]]))                        # equal magnitudes: no exchange (strict >)
    assert swaps == 0 and Gi.dtype == np.float64


@pytest.mark.parametrize("name,steps", [("cartpole", 454), ("quadrotor_20hz", 55), ("rocket_landing_20hz", 218), ("codegen_random", None)])
def test_reference_reproduces_the_real_reference_s_stored_caches(name, steps):
    """tests/golden/cache_kat.npz holds what the real reference computed, in float64: its step counts exactly,
    its matrices to what float64 can know of them -- max(32 d, 1e-14), d = the float64 replay's own distance from longdouble."""
    kat = np.load(os.path.join(GOLDEN, "cache_kat.npz"))
    prob, _ = sc.load_problem(name)
    ref, f64 = rr.reference(prob)
    assert ref["ok"] and f64["ok"]
    if steps:
        assert ref["riccati_iters"] == steps and f64["riccati_iters"] == steps
    tol = rr.tolerances(ref, f64)
    for k in rr.MEMBERS:
        e = rr.rel_dev(kat[f"{name}.{k}"], ref[k])
        print(name, k, "stored cache against longdouble", e, "tolerance", tol[k])
        assert e <= tol[k], (name, k, e, tol[k])


@pytest.mark.parametrize("nx,nu,seed", [(12, 4, 912), (6, 3, 906), (20, 8, 920)])
def test_reference_agrees_with_the_oracle_s_cache(nx, nu, seed):
    fam = random_family(nx, nu, 10, seed)
    ref, f64 = rr.reference(fam)
    tol = rr.tolerances(ref, f64)
    o = sc.make_solver(OracleSolver, fam, sc.default_config(fam))
    assert int(o.get("riccati_iters")) == ref["riccati_iters"] == f64["riccati_iters"]
    for k in rr.MEMBERS:
        e = rr.rel_dev(o[k], ref[k])
        assert e <= tol[k], (k, e, tol[k])
    o.close()


def test_float64_replay_follows_the_format_argument():
    fam = rr.tame_family(6, 3, 4, 1)
    ref, f64 = rr.reference(fam)
    assert all(ref[k].dtype == rr.LD and f64[k].dtype == np.float64 for k in rr.MEMBERS)
    assert all(0.0 < rr.rel_dev(f64[k], ref[k]) < 1e-13 for k in ("Kinf", "Pinf"))       # (they differ, by rounding)


# ---- input conditions of the instance sets, on the reference alone
def every_set():
    out = [("edge", s, rr.edge_set(*s)) for s in rr.EDGE_SHAPES] + [("pivot", s, rr.pivot_set(*s)) for s in rr.PIVOT_SHAPES]
    for s in rr.STEP_SHAPES:
        out += [("step", s, rr.step_set(*s)), ("step, ordinary", s, rr.step_set(*s, edges=False))]
    return out + [("refusal", rr.REFUSAL_SHAPE, rr.refusal_set())]


def test_generators_are_pure_functions_of_their_seeds():
    for (_, _, a), (_, _, b) in zip(every_set(), every_set()):
        assert len(a) == len(b) <= 24
        for fa, fb in zip(a, b):
            assert all(np.array_equal(fa[k], fb[k]) for k in ("A", "B", "f", "Q", "R", "rho"))


@pytest.mark.parametrize("kind,shape,fams", every_set(), ids=[f"{k} {s}" for k, s, _ in every_set()])
def test_every_instance_decides_its_step_count_away_from_the_threshold(kind, shape, fams):
    """float64 and longdouble take the same number of steps, and the longdouble max|K - Kprev| at the deciding step and at the one
    before lie at least 1 % away from 1e-5: float64's error in Kinf, the member the exit test reads (at most 1.1e-12 relative to its
    largest entry over these sets; AmBKt and APf, which the exit test does not read, are known less well where B Kinf cancels A), is
    nine orders below that margin, so riccati_iters of the device has to EQUAL the reference's, whatever its summation order."""
    assert len(fams) == {"edge": 9, "pivot": 8}.get(kind, 7)
    worst, steps = 1.0, []
    for i, fam in enumerate(fams):
        assert fam["A"].shape == (shape[0], shape[0]) and fam["B"].shape == (shape[0], shape[1])
        ref, f64 = rr.reference(fam)
        assert ref["ok"] and f64["ok"], i
        assert ref["riccati_iters"] == f64["riccati_iters"], (i, ref["riccati_iters"], f64["riccati_iters"])
        assert all(np.all(np.isfinite(ref[k])) for k in rr.MEMBERS), i
        m = rr.margin(ref["deltas"])
        assert m >= 0.01, (i, ref["deltas"][-2:])
        worst = min(worst, m)
        steps.append(ref["riccati_iters"])
    print(kind, shape, "steps", steps, "smallest margin", worst)


@pytest.mark.parametrize("shape", rr.EDGE_SHAPES)
def test_edge_sets_carry_a_load(shape):
    """|f| in 0.5..1.5 where random_family draws N(0, 0.01): APf and BPf are values to compare, not rounding noise around zero"""
    for fam in rr.edge_set(*shape):
        ref, _ = rr.reference(fam)
        assert np.min(np.abs(fam["f"])) >= 0.5 and np.all(ref["APf"] != 0) and np.all(ref["BPf"] != 0)


@pytest.mark.parametrize("shape", rr.PIVOT_SHAPES)
def test_pivot_sets_exchange_rows(shape):
    """every instance at least once; at nu = 16 -- the size perm[16] and x[16] are dimensioned for -- at least half of them in the
    FIRST step's inversion and at least three times overall"""
    refs = [rr.reference(fam)[0] for fam in rr.pivot_set(*shape)]
    print(shape, "row exchanges", [r["swaps"] for r in refs], "in the first step", [r["swaps_first"] for r in refs])
    assert all(r["swaps"] >= 1 for r in refs)
    if shape[1] == 16:
        assert 2 * sum(r["swaps_first"] >= 1 and r["swaps"] >= 3 for r in refs) >= len(refs)


def test_tame_draws_never_exchange_rows_where_nu_is_at_most_nx():
    """why the pivot sets exist: the ordinary families leave the exchange untouched"""
    for shape in ((15, 1), (31, 1), (16, 16)):
        assert all(rr.reference(fam)[0]["swaps"] == 0 for fam in rr.edge_set(*shape))


@pytest.mark.parametrize("shape", rr.STEP_SHAPES)
def test_step_count_edges(shape):
    nx, nu, N = shape
    fams, plain = rr.step_set(*shape), rr.step_set(*shape, edges=False)
    assert 0 < rr.ZERO_AT < len(fams) - 1 and 0 < rr.CAP_AT < len(fams) - 1
    for i, (a, b) in enumerate(zip(fams, plain)):                      # the other five are the same instances in both batches
        same = all(np.array_equal(a[k], b[k]) for k in ("A", "B", "f", "Q", "R", "rho"))
        assert same == (i not in (rr.ZERO_AT, rr.CAP_AT)), i
    assert all(3 < rr.reference(f)[0]["riccati_iters"] < 1000 for f in plain)
    for dtype in (rr.LD, np.float64):
        zero = rr.precompute(fams[rr.ZERO_AT], dtype)
        assert zero["riccati_iters"] == 1 and np.all(zero["Kinf"] == 0) and zero["deltas"] == [0.0]
        q = fams[rr.ZERO_AT]["Q"].astype(dtype) + dtype(fams[rr.ZERO_AT]["rho"]) + dtype(fams[rr.ZERO_AT]["rho"])
        assert np.array_equal(zero["Pinf"], np.diag(q))
        cap = rr.precompute(fams[rr.CAP_AT], dtype)
        assert cap["riccati_iters"] == 1000 and len(cap["deltas"]) == 1000 and cap["deltas"][-1] >= 1.01e-5
        assert all(np.all(np.isfinite(cap[k])) for k in rr.MEMBERS) and np.max(np.abs(cap["Pinf"])) < 1e4
    print(shape, "cap instance: last max|K - Kprev|", cap["deltas"][-1], "max|Pinf|", float(np.max(np.abs(cap["Pinf"]))))


def test_singular_instance_is_refused_by_the_reference_too():
    fams = rr.refusal_set()
    for at in (rr.BAD_AT, 0):
        bad = rr.singular_family(fams[at])
        assert (bad["R"][0] + bad["rho"]) + bad["rho"] == 0.0 and not np.any(bad["B"][:, 0])
        for dtype in (rr.LD, np.float64):
            out = rr.precompute(bad, dtype)
            assert not out["ok"] and out["deltas"] == []               # refused in the first step's inversion
        assert rr.reference(fams[at])[0]["ok"]


def solved_sets():
    return [("edge", s, rr.edge_set(*s)) for s in rr.SOLVED_SHAPES] + [("step", s, rr.step_set(*s)) for s in rr.STEP_SHAPES]


@pytest.mark.parametrize("kind,shape,fams", solved_sets(), ids=[f"{k} {s}" for k, s, _ in solved_sets()])
def test_solved_batches_are_well_conditioned_for_the_oracle(kind, shape, fams):
    """the oracle alone: finite fields, its own termination or max_iter, and a 1 + 1e-15 scaling of A and B moves no field by more than
    1e-11 relative -- two orders inside the 1e-9 the device is held to"""
    x0, Xref, Uref = rr.solve_data(fams)
    worst = 0.0
    for i, fam in enumerate(fams):
        for rec in rr.oracle_solves(fam, x0[i], Xref[i], Uref[i]):
            assert all(np.all(np.isfinite(rec[k])) for k in rec if k not in ("iter", "solved")), i
            assert rec["solved"] == 1 or rec["iter"] == rr.MAX_ITER, (i, rec["iter"], rec["solved"])
        amp = rr.oracle_amplification(fam, x0[i], Xref[i], Uref[i])
        assert amp < 1e-11, (i, amp)
        worst = max(worst, amp)
    print(kind, shape, "worst oracle amplification", worst)
