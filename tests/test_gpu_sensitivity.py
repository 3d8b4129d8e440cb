"""GPU: the adaptive-rho sensitivity tables computed on the device (csrc/sensitivity_kernel.hip.h; tiny_batch_compute_sensitivity,
tiny_compute_sensitivity) and adaptive rho on per-instance batches (the HET && ADAPT form of the one-row kernel), every instance
against its own oracle solver.  The formulas themselves are pinned on the CPU (tests/test_sensitivity_ref_cpu.py)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pod  # noqa: E402
import scenarios as sc  # noqa: E402
import sens_ref  # noqa: E402
import tinympc_amd as tm  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402
from hip_runner import make_batch  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-9                       # the project's parity tolerance (two summation orders of the Lyapunov series differ by 3e-13)
NAMES = sens_ref.NAMES
rel_err = sens_ref.rel_max


def random_family(nx, nu, N, seed):      # as tests/test_gpu_hetero.py
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((nx, nx))
    A = M * rng.uniform(0.7, 0.99) / np.max(np.abs(np.linalg.eigvals(M)))
    return dict(nx=nx, nu=nu, N=N, rho=float(rng.uniform(0.5, 5.0)), A=A, B=rng.standard_normal((nx, nu)) / np.sqrt(nx),
                f=rng.normal(0, 0.01, nx), Q=rng.uniform(1, 10, nx), R=rng.uniform(0.1, 1, nu))


def hetero_batch(fams, N):
    return tm.TinyBatchSolver.hetero(np.stack([f["A"] for f in fams]), np.stack([f["B"] for f in fams]), np.stack([f["f"] for f in fams]),
                                     np.stack([f["Q"] for f in fams]), np.stack([f["R"] for f in fams]), np.array([f["rho"] for f in fams]), N)


# ---- 1. the device's tables equal the formulas at the device's own cache
def shared_problems():
    quad, _ = sc.load_problem("quadrotor_20hz")
    cart, _ = sc.load_problem("cartpole")
    return [("quadrotor", quad), ("cartpole", cart), ("random_20_8", random_family(20, 8, 10, 424242))]


@pytest.mark.parametrize("name,prob", shared_problems(), ids=[n for n, _ in shared_problems()])
def test_shared_family_tables_equal_the_formulas_at_the_cache(name, prob):
    s = tm.TinyBatchSolver.from_problem(prob, 4)
    s.compute_sensitivity()
    ref = sens_ref.tables(prob["A"], prob["B"], s.cache("Kinf"), s.cache("Quu_inv"))
    for k in NAMES:
        e = rel_err(s.sensitivity(k), ref[k])
        print(name, k, "device against the formulas", e)
        assert e < RTOL, (name, k, e)
    assert 1 <= s.sensitivity_instance(0, "steps") <= 64
    s.close()


@pytest.mark.parametrize("nx,nu", [(2, 2), (4, 1), (7, 7), (12, 4), (24, 8), (31, 1)])
def test_per_instance_tables_equal_the_formulas_at_every_cache(nx, nu):
    B, N = 203, 10
    fams = [random_family(nx, nu, N, 7000 + 13 * i + nx) for i in range(B)]
    s = hetero_batch(fams, N)
    s.compute_sensitivity()
    worst = dict.fromkeys(NAMES, 0.0)
    for i, fam in enumerate(fams):
        ref = sens_ref.tables(fam["A"], fam["B"], s.cache_instance(i, "Kinf"), s.cache_instance(i, "Quu_inv"))
        assert np.all(np.isfinite(s.cache_instance(i, "Pinf")))
        for k in NAMES:
            e = rel_err(s.sensitivity_instance(i, k), ref[k])
            worst[k] = max(worst[k], e)
            assert e < RTOL, (i, k, e)
        steps = s.sensitivity_instance(i, "steps")
        assert 1 <= steps <= 64, (i, steps)
    print((nx, nu), "worst device-against-formula deviation", worst)
    s.close()


# ---- 2. it is the derivative of setup
def derivative_systems():
    quad, _ = sc.load_problem("quadrotor_20hz")
    out = [("quadrotor", (quad["A"], quad["B"], quad["Q"], quad["R"], quad["rho"]))]
    rng = np.random.default_rng(7)
    for nx, nu in ((4, 2), (6, 3), (12, 4), (10, 6)):
        for k in range(3):
            out.append((f"r{nx}_{nu}_{k}", sens_ref.random_system(rng, nx, nu)))
    return out


@pytest.mark.parametrize("name,system", derivative_systems(), ids=[n for n, _ in derivative_systems()])
def test_first_order_step_predicts_the_cache_of_a_fresh_setup_at_a_moved_rho(name, system):
    """max |K(rho) + 0.1 rho dK - K(1.1 rho)| <= 0.15 max |K(1.1 rho) - K(rho)| (the reference recursion alone gives at most 0.094 on
    the CPU: the second-order term scales with the relative step), and the same for Pinf with 0.01 (0.0039)."""
    A, B, Qd, Rd, rho = system
    nx, nu = B.shape
    at = {}
    for r in (rho, 1.1 * rho):
        s = tm.TinyBatchSolver(A, B, np.zeros(nx), Qd, Rd, r, nx, nu, 10, 2)
        at[r] = (s.cache("Kinf"), s.cache("Pinf"))
        if r == rho:
            s.compute_sensitivity()
            dK, dP = s.sensitivity("dKinf_drho"), s.sensitivity("dPinf_drho")
        s.close()
    (K0, P0), (K1, P1) = at[rho], at[1.1 * rho]
    rk = np.max(np.abs(K0 + 0.1 * rho * dK - K1)) / np.max(np.abs(K1 - K0))
    rp = np.max(np.abs(P0 + 0.1 * rho * dP - P1)) / np.max(np.abs(P1 - P0))
    print(name, "first-order residual / change: Kinf", rk, "Pinf", rp)
    assert rk <= 0.15, (name, rk)
    assert rp <= 0.01, (name, rp)


# ---- 3. plumbing
def test_compute_get_and_set_round_trip():
    prob, _ = sc.load_problem("cartpole")
    s = tm.TinyBatchSolver.from_problem(prob, 3)
    with pytest.raises(tm.TinyMPCError):
        s.sensitivity("dKinf_drho")                       # nothing installed yet
    s.compute_sensitivity()
    first = {k: s.sensitivity(k) for k in NAMES}
    ref = sens_ref.tables(prob["A"], prob["B"], s.cache("Kinf"), s.cache("Quu_inv"))
    assert all(rel_err(first[k], ref[k]) < RTOL for k in NAMES)
    s.compute_sensitivity()
    assert all(np.array_equal(first[k], s.sensitivity(k)) for k in NAMES)      # (deterministic)
    rng = np.random.default_rng(3)
    mine = {k: rng.normal(size=first[k].shape) for k in NAMES}
    s.set_sensitivity(*[mine[k] for k in NAMES])
    assert all(np.array_equal(mine[k], s.sensitivity(k)) for k in NAMES)       # set overrides what was computed
    s.close()


def _tiny_setup(name):                                     # as tests/test_abi.py _setup
    L = tm.lib()
    prob, _ = sc.load_problem(name)
    keep = []
    mats = []
    for a in (prob["A"], prob["B"], prob["f"], np.diag(prob["Q"]), np.diag(prob["R"])):
        m, k = pod.mat(a)
        mats.append(m); keep.append(k)
    sp = C.POINTER(pod.TinySolver)()
    L.tiny_setup.argtypes = [C.POINTER(C.POINTER(pod.TinySolver))] + [C.POINTER(pod.Mat)] * 5 + [C.c_double] + [C.c_int] * 4
    rc = L.tiny_setup(C.byref(sp), *[C.byref(m) for m in mats], prob["rho"], prob["nx"], prob["nu"], prob["N"], 0)
    assert rc == 0
    L.tiny_compute_sensitivity.argtypes = [C.POINTER(pod.TinySolver)]
    L.tiny_initialize_sensitivity_matrices.argtypes = [C.POINTER(pod.TinySolver)]
    L.tiny_initialize_sensitivity_matrices.restype = None
    L.tiny_destroy.argtypes = [C.POINTER(pod.TinySolver)]
    return L, sp, prob, keep


def test_drop_in_entry_point_fills_the_cache_of_a_cartpole_solver():
    L, sp, prob, keep = _tiny_setup("cartpole")
    assert L.tiny_compute_sensitivity(sp) == 0
    c = sp.contents.cache.contents
    ref = sens_ref.tables(prob["A"], prob["B"], pod.to_np(c.Kinf), pod.to_np(c.Quu_inv))
    for k in NAMES:
        got = pod.to_np(getattr(c, k))
        assert got.shape == ref[k].shape, (k, got.shape)
        assert rel_err(got, ref[k]) < RTOL, k
    L.tiny_destroy(sp)


def test_quadrotor_literals_come_back_bit_for_bit_after_a_computed_set():
    L, sp, prob, keep = _tiny_setup("quadrotor_20hz")
    c = sp.contents.cache.contents
    L.tiny_initialize_sensitivity_matrices(sp)
    lit = {k: pod.to_np(getattr(c, k)).copy() for k in NAMES}
    assert all(np.array_equal(lit[k], sc.quadrotor_sensitivity()[k]) for k in NAMES)
    assert L.tiny_compute_sensitivity(sp) == 0
    ref = sens_ref.tables(prob["A"], prob["B"], pod.to_np(c.Kinf), pod.to_np(c.Quu_inv))
    assert all(rel_err(pod.to_np(getattr(c, k)), ref[k]) < RTOL for k in NAMES)
    assert rel_err(pod.to_np(c.dPinf_drho), lit["dPinf_drho"]) > 1.0          # a different set
    L.tiny_initialize_sensitivity_matrices(sp)
    assert all(np.array_equal(pod.to_np(getattr(c, k)), lit[k]) for k in NAMES)
    L.tiny_destroy(sp)


def test_computed_tables_survive_the_codegen_round_trip(tmp_path):
    """tiny_codegen with adaptive_rho on writes whatever the cache holds: the computed tables come out as %.17g literals, bit for bit"""
    import re
    L, sp, prob, keep = _tiny_setup("cartpole")
    sp.contents.settings.contents.adaptive_rho = 1
    assert L.tiny_compute_sensitivity(sp) == 0
    L.tiny_codegen.argtypes = [C.POINTER(pod.TinySolver), C.c_char_p, C.c_int]
    assert L.tiny_codegen(sp, str(tmp_path / "gen").encode(), 0) == 0
    src = open(tmp_path / "gen" / "src" / "tiny_data.c").read()
    c = sp.contents.cache.contents
    for k in NAMES:
        m = re.search(r"static const double %s_data\[(\d+)\] = \{(.*?)\};" % k, src, re.S)
        assert m, k
        v = np.array([float(t) for t in m.group(2).replace("\n", " ").split(",")])
        assert np.array_equal(v, pod.to_np(getattr(c, k)).T.ravel()), k
    L.tiny_destroy(sp)


# ---- adaptive solves against the oracle.  The tolerance: the re-estimated rho feeds back through the Taylor steps of the cache, so one
# rounding in the tables is amplified over the adaptations of a solve.  The oracle measures its own amplification: it runs once with
# the tables and once with them scaled by 1 + 1e-15; the tolerance is 100 x the worst relative field difference, and never below the
# 1e-7 tools/fuzz_parity.py adaptive_trial uses for random tables.
FIELDS = ("x", "u", "vnew", "znew", "g", "y", "v", "z")
STATE = ("Kinf", "Pinf", "C1", "C2")
BOX = dict(x_min=-2.0, x_max=2.0, u_min=-0.4, u_max=0.4)


def oracle_runs(fam, tables, x0, Xref, Uref, clip, scale=1.0, max_iter=80, **settings):
    """one cold solve, then a warm one from 0.9 x0 (the cache state persists) -> [record, record]; settings: further entries of the
    oracle's config (abs_pri_tol, abs_dua_tol, ...)"""
    nx, nu = fam["nx"], fam["nu"]
    cfg = sc.adaptive_cfg(sc.default_config(fam, max_iter=max_iter, **settings, x_min=np.full((nx, 1), BOX["x_min"]), x_max=np.full((nx, 1), BOX["x_max"]),
                                            u_min=np.full((nu, 1), BOX["u_min"]), u_max=np.full((nu, 1), BOX["u_max"])),
                          rho_min=0.7, rho_max=6.0, clip=clip, sensitivity={k: np.asarray(tables[k]) * scale for k in NAMES})
    o = sc.make_solver(OracleSolver, fam, cfg)
    o["Xref"], o["Uref"] = Xref, Uref
    recs = []
    for x in (x0, 0.9 * x0):
        o["x"][:, 0] = x
        o.solve()
        rec = {k: o[k].copy() for k in FIELDS + STATE}
        rec.update(rho=np.array([o.get("rho")]), iter=int(o.get("sol_iter")), solved=int(o.get("sol_solved")), status=int(o.get("status")))
        recs.append(rec)
    o.close()
    return recs


def amplification(a, b):
    """worst relative difference of two oracle runs over every field of both solves"""
    return max(rel_err(ra[k], rb[k]) for ra, rb in zip(a, b) for k in FIELDS + STATE + ("rho",))


def device_runs(s, x0):
    recs = []
    for x in (x0, 0.9 * x0):
        s.set_x0(x)
        s.solve()
        st = s.status()
        rec = {k: s.get(k) for k in FIELDS}
        rec.update({k: s.get_cache_state(k) for k in STATE + ("rho",)})
        rec.update(iter=st["iter"].copy(), solved=st["solved"].copy(), status=st["status"].copy())
        recs.append(rec)
    return recs


def compare(dev, ora, i, tol):
    for d, o in zip(dev, ora):
        assert (d["iter"][i], d["solved"][i], d["status"][i]) == (o["iter"], o["solved"], o["status"]), (i, d["iter"][i], o["iter"])
        for k in FIELDS + STATE:
            assert rel_err(d[k][i], o[k]) < tol, (i, k, rel_err(d[k][i], o[k]), tol)
        assert rel_err(d["rho"][i], o["rho"][0]) < tol, (i, "rho")


def test_shared_family_adaptive_solve_with_computed_tables_matches_the_oracle():
    suite = sc.tracking_adaptive_suite(B=16, seed=606, rho_min=0.7, rho_max=30.0, clip=1, max_iter=60)
    s = make_batch(suite)
    s.compute_sensitivity()
    tables = {k: s.sensitivity(k) for k in NAMES}
    cases, cfg = suite["cases"], suite["config"]
    s.set_x0(cases["x0"]); s.set_x_ref(cases["Xref"]); s.set_u_ref(cases["Uref"])
    s.solve()
    st = s.status()
    out = {k: s.get(k) for k in FIELDS}
    out.update({k: s.get_cache_state(k) for k in STATE + ("rho",)})
    s.close()
    runs = []
    for scale in (1.0, 1.0 + 1e-15):
        su = dict(suite, config=sc.adaptive_cfg(cfg, rho_min=0.7, rho_max=30.0, clip=1, sensitivity={k: tables[k] * scale for k in NAMES}))
        runs.append(sc.run_cases(OracleSolver, su))
    ref, pert = runs
    assert all(np.all(np.isfinite(ref[k])) for k in FIELDS + STATE + ("rho",))
    floor = max(rel_err(pert[k], ref[k]) for k in FIELDS + STATE + ("rho",))
    tol = max(1e-7, 100.0 * floor)
    print("oracle amplification of one rounding in the tables", floor, "tolerance", tol)
    assert np.array_equal(st["iter"], ref["iter"].astype(int)) and np.array_equal(st["solved"], ref["sol_solved"].astype(int))
    for k in FIELDS + STATE + ("rho",):
        for b in range(out[k].shape[0]):
            assert rel_err(out[k][b], ref[k][b]) < tol, (k, b, rel_err(out[k][b], ref[k][b]))


# ---- 4. per-instance adaptive solves, every instance against its own oracle
HET_SEED = 1300


def het_data(nx, nu, N, B=11, seed=HET_SEED):
    """the families, x0 and references of het_setup (numpy only)"""
    fams = [random_family(nx, nu, N, seed + 17 * i + nx) for i in range(B)]
    rng = np.random.default_rng(seed + nx + N)
    for f in fams:
        f["rho"] = float(rng.uniform(1.0, 3.0))
    x0 = rng.uniform(-1, 1, (B, nx))
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    return fams, x0, Xref, Uref


def het_setup(nx, nu, N, B=11, seed=HET_SEED):
    fams, x0, Xref, Uref = het_data(nx, nu, N, B, seed)
    s = hetero_batch(fams, N)
    s.set_bound_constraints(np.full((nx, 1), BOX["x_min"]), np.full((nx, 1), BOX["x_max"]), np.full((nu, 1), BOX["u_min"]), np.full((nu, 1), BOX["u_max"]))
    s.update_settings(max_iter=80)
    s.set_x_ref(Xref)
    s.set_u_ref(Uref)
    return fams, x0, Xref, Uref, s


@pytest.mark.parametrize("clip", [1, 0])
@pytest.mark.parametrize("nx,nu,N", [(12, 4, 10), (6, 3, 10), (5, 3, 7)])
def test_per_instance_adaptive_solve_matches_each_instances_own_oracle(nx, nu, N, clip):
    """B = 11: a partial last tile, four different systems in every wave.  Each instance's oracle gets the tables read back for that
    instance.  Tolerance: 100 x the oracle's own amplification of a 1e-15 relative change of the tables, at least 1e-7.  Measured
    on the CPU for these inputs (oracle alone, tables from tests/sens_ref.py): the floor lies between 2.3e-15 and 4.0e-14 in the six
    cases (every field finite, rho moves in 11 of 11 instances), so the tolerance is 1e-7 in all of them."""
    B = 11
    fams, x0, Xref, Uref, s = het_setup(nx, nu, N, B)
    s.compute_sensitivity()
    s.set_adaptive_rho(1, 0.7, 6.0, clip)
    assert s.kernel_path() in ("regs", "jit")             # the one-row kernel: compiled in, or (5,3,7) instantiated at run time
    tables = [{k: s.sensitivity_instance(i, k) for k in NAMES} for i in range(B)]
    for i, fam in enumerate(fams):                         # the lane tables are built from these: they must be the instance's own
        ref = sens_ref.tables(fam["A"], fam["B"], s.cache_instance(i, "Kinf"), s.cache_instance(i, "Quu_inv"))
        assert all(rel_err(tables[i][k], ref[k]) < RTOL for k in NAMES), i
    ora = [oracle_runs(fams[i], tables[i], x0[i], Xref[i], Uref[i], clip) for i in range(B)]
    pert = [oracle_runs(fams[i], tables[i], x0[i], Xref[i], Uref[i], clip, scale=1.0 + 1e-15) for i in range(B)]
    # conditions on the inputs (oracle alone): finite fields, and rho moves in at least 80 % of the instances
    assert all(np.all(np.isfinite(r[k])) for runs in ora for r in runs for k in FIELDS + STATE + ("rho",))
    moved = sum(any(r["rho"][0] != fams[i]["rho"] for r in ora[i]) for i in range(B))
    assert moved >= 0.8 * B, moved
    floor = max(amplification(ora[i], pert[i]) for i in range(B))
    tol = max(1e-7, 100.0 * floor)
    print((nx, nu, N), "clip", clip, "oracle amplification floor", floor, "tolerance", tol, "instances whose rho moved", moved)
    dev = device_runs(s, x0)
    for i in range(B):
        compare(dev, ora[i], i, tol)
    # reset, then the first solve again: exactly the same
    s.reset()
    s.set_x0(x0)
    s.solve()
    st = s.status()
    assert np.array_equal(st["iter"], dev[0]["iter"])
    for k in FIELDS:
        assert np.array_equal(s.get(k), dev[0][k]), k
    for k in STATE + ("rho",):
        assert np.array_equal(s.get_cache_state(k), dev[0][k]), k
    s.close()


def test_one_set_of_zero_tables_on_a_per_instance_batch_moves_rho_alone():
    """set_sensitivity on a per-instance batch = the same tables for every instance; all zero: only rho and each instance's own
    ATAB_AT (A' g, B' g of the dual residual) are in play"""
    nx, nu, N, B = 12, 4, 10, 11
    fams, x0, Xref, Uref, s = het_setup(nx, nu, N, B)
    zero = {"dKinf_drho": np.zeros((nu, nx)), "dPinf_drho": np.zeros((nx, nx)), "dC1_drho": np.zeros((nu, nu)), "dC2_drho": np.zeros((nx, nx))}
    s.compute_sensitivity()                                # (then replaced: set overrides computed, on every instance)
    s.set_sensitivity(*[zero[k] for k in NAMES])
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    dev = device_runs(s, x0)
    moved = 0
    for i in range(B):
        ora = oracle_runs(fams[i], zero, x0[i], Xref[i], Uref[i], 1)
        moved += any(r["rho"][0] != fams[i]["rho"] for r in ora)
        compare(dev, ora, i, 1e-7)
    assert moved >= 0.8 * B, moved
    s.close()


# ---- 5. what stays refused
def test_wide_per_instance_shapes_still_refuse_adaptive_rho():
    fams = [random_family(20, 8, 10, 5100 + i) for i in range(5)]
    s = hetero_batch(fams, 10)
    s.compute_sensitivity()                                # the tables exist for any nx + nu <= 32 ...
    assert np.all(np.isfinite(s.sensitivity_instance(4, "dPinf_drho")))
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    s.set_x0(np.zeros((5, 20)))
    with pytest.raises(tm.TinyMPCError, match="register-resident kernel"):   # ... the adaptive solve lives on the one-row kernel
        s.solve()
    s.close()


@pytest.mark.parametrize("per_instance", [False, True])
def test_adaptive_rho_without_tables_fails_and_names_both_entry_points(per_instance):
    if per_instance:
        s = hetero_batch([random_family(6, 3, 10, 5200 + i) for i in range(5)], 10)
    else:
        prob, _ = sc.load_problem("cartpole")
        s = tm.TinyBatchSolver.from_problem(prob, 5)
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    L = tm.lib()
    assert L.tiny_batch_solve(s._h) == tm.ERR_DIM
    msg = L.tiny_batch_last_error(s._h).decode()
    assert "tiny_batch_set_sensitivity" in msg and "tiny_batch_compute_sensitivity" in msg, msg
    s.close()
