"""GPU tests of riccati_kernel (csrc/riccati_kernel.hip.h), the batched cache precompute of tiny_batch_setup_hetero, at its shape, pivot
and step-count edges.  The arbiter is tests/riccati_ref.py in x86 longdouble; every cache member of every instance is held to
max(32 d, 1e-14) relative to the member's largest entry, d = the deviation of the SAME numpy recursion in float64 from the longdouble one on
that instance (riccati_ref.tolerances), and riccati_iters to the longdouble count.  The instance sets are riccati_ref.py's, whose input
conditions (row exchanges, margins of the step counts, the cap, the single step, conditioning of the solved batches)
tests/test_riccati_ref_cpu.py asserts on the reference alone.  The lane tables the kernel's epilogue writes cannot be read back: they
are checked through solves against each instance's own oracle."""
import time

import numpy as np
import pytest

import riccati_ref as rr
import tinympc_amd as tm

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                   # fields of a solve against the instance's own oracle, as tests/test_gpu_hetero.py

if np.finfo(np.longdouble).eps >= 1e-18:
    pytest.skip("np.longdouble is no wider than float64 on this platform (eps %.3g): there is no extended-precision reference here"
                % np.finfo(np.longdouble).eps, allow_module_level=True)


def make(fams):
    t = time.perf_counter()
    s = tm.TinyBatchSolver.hetero(*[np.stack([f[k] for f in fams]) for k in ("A", "B", "f", "Q", "R")],
                                  np.array([f["rho"] for f in fams]), fams[0]["N"])
    print("    hetero() of %d instances (%d,%d,%d): %.1f ms" % (len(fams), fams[0]["nx"], fams[0]["nu"], fams[0]["N"], 1e3 * (time.perf_counter() - t)))
    return s


def check_caches(label, fams, s, host=True):
    """all six members and riccati_iters of every instance against the longdouble reference; instance 0 also against the host recursion
    of a shared-family handle (two float64 evaluations, each within its tolerance of the reference: within twice that of each other).
    Prints every figure, then asserts."""
    bad = []
    worst = dict(d=0.0, dev=0.0, ratio=0.0, where=None)
    for i, fam in enumerate(fams):
        ref, f64 = rr.reference(fam)
        tol = rr.tolerances(ref, f64)
        its = int(s.cache_instance(i, "riccati_iters")[0, 0])
        if its != ref["riccati_iters"]:
            bad.append((i, "riccati_iters", its, ref["riccati_iters"]))
        for k in rr.MEMBERS:
            d, dev = rr.rel_dev(f64[k], ref[k]), rr.rel_dev(s.cache_instance(i, k), ref[k])
            ratio = dev / max(d, 1e-14 / 32.0)
            worst["d"], worst["dev"] = max(worst["d"], d), max(worst["dev"], dev)
            if ratio > worst["ratio"]:
                worst["ratio"], worst["where"] = ratio, (i, k)
            if not dev <= tol[k]:
                bad.append((i, k, dev, tol[k]))
    print("    %s: worst d %.2e, worst device deviation %.2e, worst ratio %.1f at %s (bound 32)" % (label, worst["d"], worst["dev"], worst["ratio"], worst["where"]))
    if host:
        ref, f64 = rr.reference(fams[0])
        tol = rr.tolerances(ref, f64)
        hom = tm.TinyBatchSolver.from_problem(fams[0], 2)
        for k in ("Kinf", "Pinf"):
            dev, hst = s.cache_instance(0, k), hom.cache(k)
            e = rr.rel_dev(dev, hst)
            print("    %s: instance 0 %s device against host %.2e%s" % (label, k, e, " (bit-identical)" if np.array_equal(dev, hst) else ""))
            if not e <= 2.0 * tol[k]:
                bad.append((0, k, "host", e, 2.0 * tol[k]))
        hom.close()
    assert not bad, (label, bad)


def check_solves(label, fams, s, paths):
    """one cold and one warm box-constrained solve of the whole batch against each instance's own oracle: equal iteration counts, fields
    within RTOL"""
    nx, nu = fams[0]["nx"], fams[0]["nu"]
    x0, Xref, Uref = rr.solve_data(fams)
    s.set_bound_constraints(np.full((nx, 1), rr.BOX["x_min"]), np.full((nx, 1), rr.BOX["x_max"]), np.full((nu, 1), rr.BOX["u_min"]), np.full((nu, 1), rr.BOX["u_max"]))
    s.update_settings(max_iter=rr.MAX_ITER)
    s.set_x0(x0)
    s.set_x_ref(Xref)
    s.set_u_ref(Uref)
    assert s.kernel_path() in paths, s.kernel_path()
    t = time.perf_counter()
    s.solve()
    t_cold = time.perf_counter() - t
    st = s.status()
    cold = {k: s.get(k) for k in rr.FIELDS}
    s.set_x0(0.9 * x0)
    t = time.perf_counter()
    s.solve()
    t_warm = time.perf_counter() - t
    st2 = s.status()
    warm = {k: s.get(k) for k in rr.WARM_FIELDS}
    assert s.kernel_path() in paths, s.kernel_path()
    print("    %s: kernel path %s, first solve() %.1f ms (with whatever it had to instantiate), second %.1f ms" % (label, s.kernel_path(), 1e3 * t_cold, 1e3 * t_warm))
    worst = 0.0
    for i, fam in enumerate(fams):
        oc, ow = rr.oracle_solves(fam, x0[i], Xref[i], Uref[i])
        assert (oc["iter"], oc["solved"]) == (st["iter"][i], st["solved"][i]), (label, i, oc["iter"], st["iter"][i])
        assert ow["iter"] == st2["iter"][i], (label, i, "warm", ow["iter"], st2["iter"][i])
        for got, want, fields, tag in ((cold, oc, rr.FIELDS, "cold"), (warm, ow, rr.WARM_FIELDS, "warm")):
            for k in fields:
                e = rr.rel_dev(got[k][i], want[k])
                worst = max(worst, e)
                assert e < RTOL, (label, i, k, tag, e)
    print("    %s: iterations cold %s warm %s, worst field deviation %.2e" % (label, st["iter"].tolist(), st2["iter"].tolist(), worst))


def assert_same_bits(a, i, b, j, what):
    for k in rr.MEMBERS + ("riccati_iters", "Q", "R"):
        assert np.array_equal(a.cache_instance(i, k), b.cache_instance(j, k)), (what, i, k)


# ---- (a) shape edges, well-conditioned
@pytest.mark.parametrize("nx,nu", rr.EDGE_SHAPES)
def test_shape_edges(nx, nu):
    """(1,1) the smallest, (15,1) / (1,15) the one-row limit, (2,14) nu > nx, (31,1) the largest LDS request (56 080 bytes), (16,16) nx + nu
    = 32, (8,16) / (1,16) nu = 16"""
    fams = rr.edge_set(nx, nu)
    s = make(fams)
    check_caches("edge (%d,%d)" % (nx, nu), fams, s)
    s.close()


@pytest.mark.parametrize("nx,nu", [(4, 17), (16, 17)])
def test_shapes_past_the_kernel_s_arrays_are_refused(nx, nu):
    """nu > 16 (perm[16], x[16]) and nx + nu > 32: TINY_ERR_UNSUPPORTED, and a valid setup works right after"""
    fams = [rr.tame_family(nx, nu, 4, 3000 + i) for i in range(3)]
    with pytest.raises(tm.TinyMPCError, match=r"\(%d\)" % tm.ERR_UNSUPPORTED):
        make(fams)
    fams = rr.edge_set(1, 1)
    s = make(fams)
    check_caches("after the refusal of (%d,%d)" % (nx, nu), fams, s, host=False)
    s.close()


# ---- (b) pivoting
@pytest.mark.parametrize("nx,nu", rr.PIVOT_SHAPES)
def test_row_exchanges(nx, nu):
    """strong inputs under a light weight: every instance exchanges rows in w_invert, at nu = 16 in the first step's inversion"""
    fams = rr.pivot_set(nx, nu)
    s = make(fams)
    check_caches("pivot (%d,%d)" % (nx, nu), fams, s)
    s.close()


# ---- (c) step-count edges among ordinary neighbours
@pytest.mark.parametrize("nx,nu,N", rr.STEP_SHAPES)
def test_single_step_and_cap_among_ordinary_neighbours(nx, nu, N):
    fams, plain = rr.step_set(nx, nu, N), rr.step_set(nx, nu, N, edges=False)
    s, p = make(fams), make(plain)
    zero = fams[rr.ZERO_AT]
    assert int(s.cache_instance(rr.ZERO_AT, "riccati_iters")[0, 0]) == 1
    assert np.all(s.cache_instance(rr.ZERO_AT, "Kinf") == 0.0)
    assert np.array_equal(s.cache_instance(rr.ZERO_AT, "Pinf"), np.diag((zero["Q"] + zero["rho"]) + zero["rho"]))
    assert int(s.cache_instance(rr.CAP_AT, "riccati_iters")[0, 0]) == 1000
    check_caches("step (%d,%d,%d)" % (nx, nu, N), fams, s)
    for i in range(len(fams)):                                # the kernel's LDS is reused from instance to instance
        if i not in (rr.ZERO_AT, rr.CAP_AT):
            assert_same_bits(s, i, p, i, "neighbour of the edge instances")
    p.close()
    check_solves("step (%d,%d,%d)" % (nx, nu, N), fams, s, ("regs", "jit"))
    s.close()


# ---- (d) solves on the table-layout edges
@pytest.mark.parametrize("nx,nu", rr.SOLVED_SHAPES)
def test_lane_tables_of_the_layout_edges_solve(nx, nu):
    """the lane tables of the epilogue, through the kernels that read them: (2,14,4) one-row layout with nu > nx, (16,16,4) tile layout with
    tab_lw = 32 and a 16-wide Quu_inv block, (31,1,4).  All three run on run-time instantiated kernels, none on the coverage kernel."""
    fams = rr.edge_set(nx, nu)
    s = make(fams)
    check_solves("edge (%d,%d,4)" % (nx, nu), fams, s, ("regs", "jit") if nx + nu <= 16 else ("tile", "tile-jit"))
    s.close()


HALF = 4096        # 8 x 512: the first half of the batch below fills the first pass of every device of at most 512 CUs


def test_single_step_as_a_block_s_second_instance():
    """Kp is re-zeroed per instance: riccati_kernel launches min(batch, 8 CUs) blocks, so a block reaches a second instance only in a batch
    past 8 CUs, and an ordinary instance's first step does not notice a stale Kp (max|K - Kp| is far above 1e-5 either way).  HALF
    copies of one ordinary instance, then the seven of step_set(2,1,4) over and over: with 8 CUs <= HALF every A = 0 instance of the first
    8 CUs of the second half follows an ordinary instance through the same LDS -- with that instance's gain left in Kp it would miss the
    exit of its first step and report 2 -- and the later ones follow whatever the stride brings.  Every instance of the second half is
    what it is in a batch of seven (held to the reference above), bit for bit."""
    fams = rr.step_set(2, 1, 4)
    first = rr.step_set(2, 1, 4, edges=False)[0]
    ref = rr.reference(first)[0]
    assert ref["riccati_iters"] > 1 and np.max(np.abs(ref["Kinf"])) > 1e-3          # (what the first pass leaves in Kp is no zero)
    small, big = make(fams), make([first] * HALF + [fams[i % 7] for i in range(HALF)])
    want = [{k: small.cache_instance(i, k) for k in rr.MEMBERS + ("riccati_iters",)} for i in range(7)]
    assert want[rr.ZERO_AT]["riccati_iters"][0, 0] == 1 and want[rr.CAP_AT]["riccati_iters"][0, 0] == 1000
    for i in range(HALF):
        for k in rr.MEMBERS + ("riccati_iters",) if i < 14 or i >= HALF - 14 else ("riccati_iters", "Kinf", "Pinf"):
            assert np.array_equal(big.cache_instance(HALF + i, k), want[i % 7][k]), (i, k)
    for i in (0, HALF - 1):
        assert_same_bits(big, i, small, 0, "first half")
    small.close()
    big.close()


# ---- (e) refusals and poison
def test_singular_instance_is_refused_wherever_it_sits():
    """a zero column of B under (R_j + rho) + rho == 0.0: instance 3 is refused by the kernel, instance 0 by the host recursion"""
    fams = rr.refusal_set()
    bad = list(fams)
    bad[rr.BAD_AT] = rr.singular_family(fams[rr.BAD_AT])
    with pytest.raises(tm.TinyMPCError):
        make(bad)
    s = make(fams)
    check_caches("refusal set, healthy", fams, s)
    s.close()
    bad = list(fams)
    bad[0] = rr.singular_family(fams[0])
    with pytest.raises(tm.TinyMPCError):
        make(bad)


def test_nan_instance_leaves_its_neighbours_alone():
    """a NaN in A of instance 3: what setup makes of that instance is not asserted (today: accepted, non-finite caches, as the reference
    would) beyond its step count being readable; the other six are what they are next to a healthy instance 3, bit for bit"""
    fams = rr.refusal_set()
    bad = [dict(f) for f in fams]
    bad[rr.BAD_AT]["A"] = fams[rr.BAD_AT]["A"].copy()
    bad[rr.BAD_AT]["A"][1, 2] = np.nan
    s, p = make(fams), make(bad)
    print("    NaN instance: riccati_iters", int(p.cache_instance(rr.BAD_AT, "riccati_iters")[0, 0]))
    for i in range(len(fams)):
        if i != rr.BAD_AT:
            assert_same_bits(p, i, s, i, "neighbour of the NaN instance")
    p.close()
    s.close()
