"""GPU: adaptive rho on per-instance batches (the HET && ADAPT form of the one-row kernel, sensitivity_kernel, tiny_batch_compute_sensitivity)
where tests/test_gpu_sensitivity.py does not reach: a wave that runs several tiles, the grid-stride loop of the two setup kernels, the
flush of the C1 / C2 log inside the iteration loop, fused closed-loop steps, and a Lyapunov series that does not converge."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import scenarios as sc  # noqa: E402
import sens_ref  # noqa: E402
import tinympc_amd as tm  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402
from test_gpu_sensitivity import (BOX, FIELDS, RTOL, STATE, amplification, compare, device_runs, het_data, het_setup, hetero_batch,  # noqa: E402
                                  oracle_runs, random_family)

pytestmark = pytest.mark.gpu
NAMES = sens_ref.NAMES
rel_err = sens_ref.rel_max
CACHE = ("Kinf", "Pinf", "Quu_inv", "AmBKt", "APf", "BPf", "riccati_iters")


def boxed(s, nx, nu, max_iter=80, **settings):
    s.set_bound_constraints(np.full((nx, 1), BOX["x_min"]), np.full((nx, 1), BOX["x_max"]), np.full((nu, 1), BOX["u_min"]), np.full((nu, 1), BOX["u_max"]))
    s.update_settings(max_iter=max_iter, **settings)
    return s


# ---- 1. many tiles per wave, second passes of the setup kernels
@pytest.mark.parametrize("nx,nu,N", [(12, 4, 10), (6, 3, 10)])
def test_every_replica_of_a_many_tile_batch_equals_the_verified_eleven(nx, nu, N):
    """The B = 11 batch of het_setup (pinned against eleven oracles by tests/test_gpu_sensitivity.py) against the same eleven families
    tiled R times, instance r * 11 + i = family i, launched with grid_waves_per_cu = 1: at most one wave per CU, four instances per
    wave.  R = the smallest odd number with 11 R >= 12 CUs + 1 (256 CUs: 3073 / 11 = 279.4 -> 280 -> 281, B = 3091): the batch has
    more than 3 CUs tiles of four, so every wave of the launch runs at least three tiles; 11 is coprime with 4, so every family
    meets every row position; B is odd, so the last tile is partial.  B > 8 CUs (2048 at 256 CUs): riccati_kernel and
    sensitivity_kernel launch 8 CUs blocks and reach the rest by grid stride, about a third of the instances in a second pass.
    Neither setup kernel contracts an FMA and both run one instance per wavefront; the solve is the same code on the same data in
    another row: everything is compared bit for bit."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    R = -(-(12 * cus + 1) // 11)
    R += 1 - R % 2
    B = 11 * R
    assert B > 12 * cus and B > 8 * cus and R % 2 == 1 and B % 4 != 0, (cus, R, B)
    fams, x0, Xref, Uref, base = het_setup(nx, nu, N)
    big = boxed(hetero_batch(fams * R, N), nx, nu)
    big.set_x_ref(np.tile(Xref, (R, 1, 1)))
    big.set_u_ref(np.tile(Uref, (R, 1, 1)))
    big.set_option("grid_waves_per_cu", 1)
    for s in (base, big):
        s.compute_sensitivity()
        s.set_adaptive_rho(1, 0.7, 6.0, 1)
    for i in range(11):
        want = {k: base.cache_instance(i, k) for k in CACHE}
        want.update({k: base.sensitivity_instance(i, k) for k in NAMES + ("steps",)})
        assert 1 <= want["steps"] <= 64
        for r in range(R):
            b = r * 11 + i
            for k in CACHE:
                assert np.array_equal(big.cache_instance(b, k), want[k]), (b, i, k)
            for k in NAMES + ("steps",):
                assert np.array_equal(big.sensitivity_instance(b, k), want[k]), (b, i, k)
    one, many = device_runs(base, x0), device_runs(big, np.tile(x0, (R, 1)))
    assert base.kernel_path() == big.kernel_path() and base.kernel_path() in ("regs", "jit")
    for solve, (a, m) in enumerate(zip(one, many)):
        assert np.any(a["rho"] != np.array([f["rho"] for f in fams]))                     # (the solves do adapt)
        for k in ("iter", "solved", "status") + FIELDS + STATE + ("rho",):
            got = m[k].reshape((R, 11) + m[k].shape[1:])
            differ = np.argwhere(np.any((got != a[k][None]).reshape(R, 11, -1), axis=2))
            assert differ.size == 0, (solve, k, "first (replica, family) that differ", differ[:8].tolist())
    base.close()
    big.close()


# ---- 2. the flush of the C1 / C2 log inside the iteration loop
FLUSH_SEED = 1300         # (HET_SEED itself meets the conditions below)


def test_per_instance_long_solves_flush_the_c1_c2_log_inside_the_loop():
    """(6,3,10), B = 11, max_iter = 300 with both tolerances 0: every solve runs its 300 iterations and takes 59 adaptations -- the
    32-entry log of rho steps that C1 / C2 still owe fills once inside the loop (flush_c reading ATAB_DC1 / ATAB_DC2 at the instance's
    own tables) and is flushed once more at the end.  Each instance against its own oracle with the tables read back for it.
    Tolerance max(1e-7, 100 x floor), floor = the oracle's own amplification of a 1e-15 relative change of the tables.  Measured on
    the CPU (oracle alone, tables from tests/sens_ref.py at the oracle's cache): every field finite, 22 of 22 solves at 300
    iterations, rho moves in 11 of 11 instances, floor 5.1e-14 -- the tolerance is 1e-7."""
    nx, nu, N, B = 6, 3, 10, 11
    kw = dict(max_iter=300, abs_pri_tol=0.0, abs_dua_tol=0.0)
    fams, x0, Xref, Uref, s = het_setup(nx, nu, N, B, seed=FLUSH_SEED)
    s.update_settings(**kw)
    s.compute_sensitivity()
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    tables = [{k: s.sensitivity_instance(i, k) for k in NAMES} for i in range(B)]
    ora = [oracle_runs(fams[i], tables[i], x0[i], Xref[i], Uref[i], 1, **kw) for i in range(B)]
    pert = [oracle_runs(fams[i], tables[i], x0[i], Xref[i], Uref[i], 1, scale=1.0 + 1e-15, **kw) for i in range(B)]
    assert all(np.all(np.isfinite(r[k])) for runs in ora for r in runs for k in FIELDS + STATE + ("rho",))
    assert all(r["iter"] == 300 for runs in ora for r in runs)
    moved = sum(any(r["rho"][0] != fams[i]["rho"] for r in ora[i]) for i in range(B))
    assert moved >= 9, moved
    floor = max(amplification(ora[i], pert[i]) for i in range(B))
    assert floor < 1e-9, floor
    tol = max(1e-7, 100.0 * floor)
    dev = device_runs(s, x0)
    worst = max(rel_err(d[k][i], o[k]) for i in range(B) for d, o in zip(dev, ora[i]) for k in FIELDS + STATE)
    print("in-loop flush: oracle amplification floor", floor, "tolerance", tol, "instances whose rho moved", moved, "worst device deviation", worst)
    for i in range(B):
        compare(dev, ora[i], i, tol)
    s.close()


# ---- 3. fused closed-loop steps
T = 7


def oracle_episode(fam, tables, x0, Xref, Uref, steps, scale=1.0):
    """the instance's own oracle in closed loop, stepped with its own A, B, f (tests/test_gpu_fused_variants.py, tools/fuzz_closed_loop.py)
    -> per step: iter, x0 after the plant step, rho and the cache state"""
    nx, nu = fam["nx"], fam["nu"]
    cfg = sc.adaptive_cfg(sc.default_config(fam, max_iter=80, x_min=np.full((nx, 1), BOX["x_min"]), x_max=np.full((nx, 1), BOX["x_max"]),
                                            u_min=np.full((nu, 1), BOX["u_min"]), u_max=np.full((nu, 1), BOX["u_max"])),
                          rho_min=0.7, rho_max=6.0, clip=1, sensitivity={k: np.asarray(tables[k]) * scale for k in NAMES})
    o = sc.make_solver(OracleSolver, fam, cfg)
    o["Xref"], o["Uref"] = Xref, Uref
    x, out = np.array(x0, dtype=np.float64), []
    for _ in range(steps):
        o["x"][:, 0] = x
        o.solve()
        x = fam["A"] @ x + fam["B"] @ o["u"][:, 0] + fam["f"]
        rec = {k: o[k].copy() for k in STATE}
        rec.update(iter=int(o.get("sol_iter")), x0=x.copy(), rho=np.array([o.get("rho")]))
        out.append(rec)
    o.close()
    return out


def episode_amplification(a, b):
    return max(rel_err(rb[k], ra[k]) for ra, rb in zip(a, b) for k in STATE + ("x0", "rho"))


@pytest.mark.parametrize("nx,nu,N", [(12, 4, 10), (5, 3, 7)])
def test_fused_closed_loop_steps_on_a_per_instance_adaptive_batch(nx, nu, N):
    """advance_x0 = 1, T = 7 MPC steps, max_iter = 80, B = 11 of het_setup: rho, Kinf, Pinf and the C1 / C2 log carry over from step to
    step.  (a) seven single-step launches; (b) reset, the same x0, one launch of seven fused steps: bit for bit what (a) left;
    (c) the chain of (a) against each instance's own oracle in closed loop: identical iteration counts per step, rho / x0 / cache
    after every step within max(1e-7, 100 x floor), floor = the amplification of a 1e-15 relative change of the tables over the whole
    episode.  Measured on the CPU (oracle alone, tables from tests/sens_ref.py): rho moves in 11 of 11 instances in both shapes, floor
    1.4e-15 at (12,4,10) and 9.6e-16 at (5,3,7): T stays 7 and the tolerance 1e-7."""
    B = 11
    fams, x0, Xref, Uref, s = het_setup(nx, nu, N, B)
    s.compute_sensitivity()
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    s.set_option("advance_x0", 1)
    tables = [{k: s.sensitivity_instance(i, k) for k in NAMES} for i in range(B)]
    # (a)
    s.set_x0(x0)
    chain = []
    for _ in range(T):
        s.solve()
        rec = {k: s.get_cache_state(k) for k in STATE + ("rho",)}
        rec.update(iter=s.status()["iter"].copy(), x0=s.get("x0"))
        chain.append(rec)
    last = {k: s.get(k) for k in FIELDS}
    total = s.reduce_stats()[7]
    assert total == sum(int(np.sum(r["iter"])) for r in chain)
    assert s.kernel_path() in ("regs", "jit")
    # (b)
    s.reset()
    s.set_x0(x0)
    s.set_option("steps_per_launch", T)
    s.solve()
    assert s.reduce_stats()[7] == total
    assert np.array_equal(s.get("x0"), chain[-1]["x0"])
    for k in FIELDS:
        assert np.array_equal(s.get(k), last[k]), k
    for k in STATE + ("rho",):
        assert np.array_equal(s.get_cache_state(k), chain[-1][k]), k
    s.close()
    # (c)
    ora = [oracle_episode(fams[i], tables[i], x0[i], Xref[i], Uref[i], T) for i in range(B)]
    pert = [oracle_episode(fams[i], tables[i], x0[i], Xref[i], Uref[i], T, scale=1.0 + 1e-15) for i in range(B)]
    assert all(np.all(np.isfinite(r[k])) for ep in ora for r in ep for k in STATE + ("x0", "rho"))
    moved = sum(any(r["rho"][0] != fams[i]["rho"] for r in ora[i]) for i in range(B))
    assert moved >= 9, moved
    floor = max(episode_amplification(ora[i], pert[i]) for i in range(B))
    assert 100.0 * floor <= 1e-7, floor
    tol = max(1e-7, 100.0 * floor)
    worst = 0.0
    for i in range(B):
        assert [int(r["iter"][i]) for r in chain] == [r["iter"] for r in ora[i]], (i, [int(r["iter"][i]) for r in chain], [r["iter"] for r in ora[i]])
        for t, (d, o) in enumerate(zip(chain, ora[i])):
            for k in STATE + ("x0",):
                e = rel_err(d[k][i], o[k])
                worst = max(worst, e)
                assert e < tol, (i, t, k, e)
            e = rel_err(d["rho"][i], o["rho"][0])
            worst = max(worst, e)
            assert e < tol, (i, t, "rho", e)
    print((nx, nu, N), "closed loop: oracle amplification floor", floor, "tolerance", tol, "instances whose rho moved", moved, "worst device deviation", worst)


# ---- 4. a Lyapunov series that does not converge
def unstabilisable(nx, nu, N, lam):
    """random_family seed 77 with its last state decoupled (A[-1,-1] = lam, the rest of that row and column 0) and not actuated
    (B[-1,:] = 0): the Riccati recursion stops (Kinf's last column is exactly 0), A - B Kinf keeps the eigenvalue lam"""
    fam = random_family(nx, nu, N, 77)
    fam["A"][-1, :] = 0.0
    fam["A"][:, -1] = 0.0
    fam["A"][-1, -1] = lam
    fam["B"][-1, :] = 0.0
    return fam


def failing_batch(lam, nx=6, nu=3, N=10, B=11, bad=4):
    fams = [unstabilisable(nx, nu, N, lam) if i == bad else random_family(nx, nu, N, 5300 + 19 * i) for i in range(B)]
    rng = np.random.default_rng(5300)
    for f in fams:
        f["rho"] = float(rng.uniform(1.0, 3.0))
    x0 = rng.uniform(-1, 1, (B, nx))
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    return fams, x0, Xref, Uref


def plain_oracle(fam, x0, Xref, Uref):
    nx, nu = fam["nx"], fam["nu"]
    cfg = sc.default_config(fam, max_iter=80, x_min=np.full((nx, 1), BOX["x_min"]), x_max=np.full((nx, 1), BOX["x_max"]),
                            u_min=np.full((nu, 1), BOX["u_min"]), u_max=np.full((nu, 1), BOX["u_max"]))
    o = sc.make_solver(OracleSolver, fam, cfg)
    o["Xref"], o["Uref"] = Xref, Uref
    o["x"][:, 0] = x0
    o.solve()
    rec = {k: o[k].copy() for k in FIELDS}
    rec.update(iter=int(o.get("sol_iter")), solved=int(o.get("sol_solved")))
    o.close()
    return rec


@pytest.mark.parametrize("lam", [1.05, 1.0], ids=["overflow", "exhausted"])
def test_a_failed_per_instance_computation_installs_nothing(lam):
    """Instance 4 of 11 has an unactuated mode lam: 1.05 makes the Lyapunov series overflow (the kernel's any_bad exit), 1.0 runs all
    64 squarings with inc / top = 0.5 (every value finite).  compute_sensitivity names the instance, the read-back still works
    (steps = -1 for it, the other ten untouched and within RTOL of the formulas), the adaptive solve is refused and leaves the
    records alone, set_sensitivity makes the handle solvable again, the plain solve never cared.  Measured on the CPU: sens_ref.tables
    raises for instance 4 at both lam (its Pinf stays below 260), the ten healthy oracles with instance 0's tables amplify a 1e-15
    relative change of them to 6.5e-14: 1e-7 holds for them."""
    nx, nu, N, B, bad = 6, 3, 10, 11, 4
    fams, x0, Xref, Uref = failing_batch(lam)
    s = boxed(hetero_batch(fams, N), nx, nu)
    s.set_x_ref(Xref)
    s.set_u_ref(Uref)
    assert 1 <= s.cache_instance(bad, "riccati_iters")[0, 0] <= 999
    # the plain solve, before anything else: every instance against its plain oracle
    s.set_x0(x0)
    s.solve()
    plain = {k: s.get(k) for k in FIELDS}
    plain_iter = s.status()["iter"].copy()
    for i in range(B):
        o = plain_oracle(fams[i], x0[i], Xref[i], Uref[i])
        assert plain_iter[i] == o["iter"], (i, plain_iter[i], o["iter"])
        for k in FIELDS:
            assert rel_err(plain[k][i], o[k]) < RTOL, (i, k)
    # the computation fails and says where
    with pytest.raises(tm.TinyMPCError, match=r"instance 4\b"):
        s.compute_sensitivity()
    assert s.sensitivity_instance(bad, "steps") == -1
    with np.errstate(all="ignore"), pytest.raises(RuntimeError):                    # the reference agrees: there is no derivative
        sens_ref.tables(fams[bad]["A"], fams[bad]["B"], s.cache_instance(bad, "Kinf"), s.cache_instance(bad, "Quu_inv"))
    for i in range(B):
        if i != bad:
            assert 1 <= s.sensitivity_instance(i, "steps") <= 64, i
            ref = sens_ref.tables(fams[i]["A"], fams[i]["B"], s.cache_instance(i, "Kinf"), s.cache_instance(i, "Quu_inv"))
            for k in NAMES:
                assert rel_err(s.sensitivity_instance(i, k), ref[k]) < RTOL, (i, k)
    # the adaptive solve is refused, nothing was launched
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    s.set_x0(0.5 * x0)
    L = tm.lib()
    rc = L.tiny_batch_solve(s._h)
    msg = L.tiny_batch_last_error(s._h).decode()
    assert rc != tm.OK and rc == tm.ERR_DIM, (rc, msg)                              # (as without any tables: TINY_ERR_DIM)
    assert "tiny_batch_compute_sensitivity" in msg, msg
    for k in FIELDS:
        assert np.array_equal(s.get(k), plain[k]), k
    with pytest.raises(tm.TinyMPCError, match="no sensitivity tables"):            # (the one-set read-back: nothing is installed)
        s.sensitivity("dKinf_drho")
    # one finite set for all: solvable again, the healthy ten as their oracles with those tables
    tab0 = {k: s.sensitivity_instance(0, k) for k in NAMES}
    s.set_sensitivity(*[tab0[k] for k in NAMES])
    assert s.sensitivity_instance(bad, "steps") == 0                                 # (tables set by the caller)
    s.reset()
    dev = device_runs(s, x0)
    worst = 0.0
    for i in range(B):
        if i != bad:
            ora = oracle_runs(fams[i], tab0, x0[i], Xref[i], Uref[i], 1)
            worst = max([worst] + [rel_err(d[k][i], o[k]) for d, o in zip(dev, ora) for k in FIELDS + STATE])
            compare(dev, ora, i, 1e-7)
    print("lambda", lam, "adaptive solve with instance 0's tables on all: worst deviation of the healthy ten", worst)
    # a second failed computation takes them away again; a plain solve works on all eleven, exactly as at the start
    with pytest.raises(tm.TinyMPCError, match=r"instance 4\b"):
        s.compute_sensitivity()
    s.set_x0(x0)
    assert L.tiny_batch_solve(s._h) == tm.ERR_DIM
    s.set_adaptive_rho(0)
    s.reset()
    s.set_x0(x0)
    s.solve()
    assert np.array_equal(s.status()["iter"], plain_iter)
    for k in FIELDS:
        assert np.array_equal(s.get(k), plain[k]), k
    s.close()


@pytest.mark.parametrize("lam", [1.05, 1.0], ids=["overflow", "exhausted"])
def test_a_failed_shared_family_computation_installs_nothing(lam):
    fam = unstabilisable(6, 3, 10, lam)
    s = tm.TinyBatchSolver(fam["A"], fam["B"], fam["f"], fam["Q"], fam["R"], fam["rho"], 6, 3, 10, 5)
    with pytest.raises(tm.TinyMPCError, match="did not converge"):
        s.compute_sensitivity()
    with pytest.raises(tm.TinyMPCError, match="no sensitivity tables"):
        s.sensitivity("dKinf_drho")
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    s.set_x0(np.zeros((5, 6)))
    L = tm.lib()
    assert L.tiny_batch_solve(s._h) == tm.ERR_DIM
    msg = L.tiny_batch_last_error(s._h).decode()
    assert "tiny_batch_set_sensitivity" in msg and "tiny_batch_compute_sensitivity" in msg, msg
    s.close()
