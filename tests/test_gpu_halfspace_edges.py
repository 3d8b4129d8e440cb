"""GPU: the half-space step of update_slack on every kernel form, bit for bit against tests/halfspace_ref.py (the numpy model that
tests/test_halfspace_ref_cpu.py pins to the oracle bit for bit and to the real reference on tests/golden/halfspace_edges.npz).

The project restates the step (admm.cpp:137-211, project_hyperplane :70-73) five times: project_halfspace_columns (the one-row
kernel's slack planes), the per-knot register form of the one-row kernel (shapes whose planes do not fit the LDS), project_columns
(the tile kernel), halfspace_inplace (the coverage kernel) and project_hyperplane_kernel (the exported symbol).  The state families
are driven through whole solves of the pure-map family (A = B = 0: x is x0 at knot 0 and +0 afterwards, so vlnew / gl are the map
iterated) on directed batches -- columns on a decision boundary, one ulp to either side, chains of sequential projections, repeated,
null, sparse, scaled half-spaces, time-varying tables that differ at every knot; all four families through the own-output identity on
real dynamics (at max_iter = 1 a kernel's own x, u and the warm duals give its slacks and duals through the model).  Any difference
is a difference of the projection: a fused z - dist a, a sum in another order, a non-strict test, a table read at the wrong knot or
slot.  Every test asserts which kernel ran."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import halfspace_ref as hr  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")


def make(prob, cfg, B, options=None):
    from hip_runner import make_batch
    s = make_batch(dict(problem=prob, config=cfg, cases=dict(x0=np.zeros((B, prob["nx"])))), batch=B)
    for k, v in (options or {}).items():
        s.set_option(k, v)
    return s


def assert_kernel(s, path, used=None):
    import tinympc_amd as tm
    got = s.kernel_path()
    assert got in ((path,) if isinstance(path, str) else path), (got, path)
    if got in ("regs", "jit"):
        assert s.get_option("last_half_rows") == 0
    if used:
        assert any(n.replace(" ", "").startswith(used) for n in tm.jit_used()), (used, tm.jit_used())


def differing(got, want, labels=None):
    same = np.all(hr.same_bits(got, want), axis=1)
    if same.all():
        return None
    first = tuple(np.argwhere(~same)[0])
    return dict(columns=int((~same).sum()), of=int(same.size), classes=sorted({hr.CLASSES[c] for c in labels[~same]}) if labels is not None else None,
                first=first, got=got[first[0], :, first[1]].tolist(), want=want[first[0], :, first[1]].tolist())


def on_families(sets):
    return [(v, g, src, fam) for v, g, src, fam in hr.FAMILIES if sets[hr.FLAG[fam]]]


# ---- (a) + (c): the pure map on every form, family combination and count
@pytest.mark.parametrize("name", list(hr.CASES))
def test_state_columns_of_a_solve_are_the_models_map(name):
    """the directed batch of the case after 1 and after 3 iterations: vlnew, gl, vlnew_tv, gl_tv bit for bit at every knot (knot 0 is
    P(x0 + gl) with x0 != 0), x itself x0 | +0; after 1 iteration the input families through the kernel's own u.  The cases cover LIN
    = 1, 2, 3 with the compiled-in tables, KMAX = 8 and 16, a cone next to the half-spaces, only the input or only the state family,
    a count of 0 with the switch on, nsl != nil, and the same on the coverage kernel."""
    c = hr.CASES[name]
    nx, nu, N = c["dims"]
    t0 = time.time()
    for iters in (1, 3):
        prob, cfg, sets, x0, duals, labels = hr.case_setup(name, iters)
        want = hr.pure_map_want(sets, nx, nu, N, x0, duals, iters)
        s = make(prob, cfg, x0.shape[0], c.get("options"))
        s.set_x0(x0)
        for v, g, _, _ in on_families(sets):
            s.set(g, duals[g])
        s.solve()
        assert_kernel(s, c["path"], c.get("used"))
        got = {k: s.get(k) for k in ("x", "u") + tuple(f for v, g, _, _ in on_families(sets) for f in (v, g))}
        it = s.status()["iter"]
        s.close()
        assert np.all(it == iters), it
        assert np.array_equal(got["x"][:, :, 0], x0) and not np.any(got["x"][:, :, 1:]) and not np.any(np.signbit(got["x"][:, :, 1:]))
        for k in want:
            lab = labels[{"vlnew": "gl", "vlnew_tv": "gl_tv"}.get(k, k)]
            assert differing(got[k], want[k], lab) is None, (name, k, iters, differing(got[k], want[k], lab))
        if iters == 1:
            own = hr.step(sets, got["x"], got["u"], duals)
            for v, g, src, fam in on_families(sets):
                if src == "u":
                    assert differing(got[v], own[v]) is None and differing(got[g], own[g]) is None, (name, v, differing(got[v], own[v]))
                    assert sets[hr.FLAG[fam]] and (own["viol_" + fam].size == 0 or own["viol_" + fam].any())
    print("halfspace edges:", name, "classes", {g: hr.class_counts(l) for g, l in labels.items()}, "seconds %.2f" % (time.time() - t0))


# ---- (b) the own-output identity on real dynamics, all four families, every form
IDENTITY_CASES = [(n, {}, p) for n, (_, p) in hr.IDENTITY_SUITES.items() if p is not None and n != "sweep_4_2_30_tv"] + \
                 [("quad_all", {"force_general": 1}, "cover"), ("sweep_20_4_10", {"force_general": 1}, "cover"),
                  ("sweep_4_2_30_tv", {"no_tile": 1}, "regs"), ("sweep_4_2_30_tv", {"debug": 1}, "regs")]


@pytest.mark.parametrize("name,options,path", IDENTITY_CASES, ids=["-".join([n] + sorted(o)) for n, o, _ in IDENTITY_CASES])
def test_own_outputs_reproduce_the_slacks_and_duals_on_real_dynamics(name, options, path):
    """max_iter = 1, warm gl, yl, gl_tv, yl_tv pushed over their half-spaces: the kernel's own x, u and the input duals give its vlnew,
    zlnew, gl, yl and the time-varying fields through the model, bit for bit -- the input lanes' slot shift (knot i in slot i + 1) and
    the last knots (state N - 1, input N - 2) included.  On the model at least half of the state and of the input columns project."""
    from hip_runner import run_cases_hip
    suite = hr.identity_suite(name)
    s = make(suite["problem"], suite["config"], suite["cases"]["x0"].shape[0], options)
    assert_kernel(s, path)
    s.close()
    out = run_cases_hip(suite, options=options)
    assert np.all(out["iter"] == 1)
    own = hr.step(hr.sets_of(suite["config"]), out["x"], out["u"], suite["cases"])
    moved = {"x": [], "u": []}
    for v, g, src, fam in on_families(suite["config"]):
        assert differing(out[v], own[v]) is None, (name, v, differing(out[v], own[v]))
        assert differing(out[g], own[g]) is None, (name, g, differing(out[g], own[g]))
        moved[src].append(own["viol_" + fam].any(axis=-1).ravel())
    for src in ("x", "u"):
        assert moved[src] and np.concatenate(moved[src]).mean() >= 0.5, (src, np.concatenate(moved[src]).mean())


# ---- (d) the exported symbol, and update_slack alone
def test_project_hyperplane_symbol_on_the_directed_set():
    """project_hyperplane(z, a, b) with the reference's calling convention on columns of every class, the non-finite ones included
    (a'a = inf, 0; a = 0; NaN / inf in z): the model's z - round(dist a) bit for bit, NaN where it has NaN.  (No batch handle, no
    dispatcher: the symbol always launches project_hyperplane_kernel.)"""
    import pod
    import tinympc_amd as tm
    L = tm.lib()
    L.project_hyperplane.argtypes = [C.POINTER(pod.Vec), C.POINTER(pod.Vec), C.POINTER(pod.Vec), C.c_double]
    L.project_hyperplane.restype = C.POINTER(pod.Vec)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    calls, seen, bad = 0, set(), []
    for name, nx, nu, N in hr.NONFINITE_SETS:
        sets, duals, labels = hr.nonfinite_batch(name, nx, nu, N)
        for v, g, src, fam in hr.FAMILIES:
            A, b = hr.tables(sets, fam, N, nx, nu)
            knots = duals[g].shape[2]
            A, b = np.broadcast_to(A, (knots,) + A.shape[-2:]), np.broadcast_to(b, (knots,) + b.shape[-1:])
            for bi in range(2):
                for i in range(knots):
                    k = (bi + i) % A.shape[1]
                    z = duals[g][bi, :, i]
                    vz, k1 = pod.vec(z)
                    va, k2 = pod.vec(A[i, k])
                    out = pod.Vec()
                    L.project_hyperplane(C.byref(out), C.byref(vz), C.byref(va), float(b[i, k]))
                    got = pod.to_np(out).copy()
                    libc.free(C.cast(out.data, C.c_void_p))
                    want = hr.hyperplane(z, A[i, k], b[i, k])
                    calls += 1
                    seen.add(hr.CLASSES[labels[g][bi, i]])
                    if not np.all(hr.same_bits(got, want)):
                        bad.append((name, fam, hr.CLASSES[labels[g][bi, i]], got.tolist(), want.tolist()))
    assert not bad, (len(bad), calls, bad[:3])
    assert set(hr.NONFINITE) <= seen and {"on_plane", "ulp_above", "ulp_below", "chain_on"} <= seen and calls >= 300


@pytest.mark.parametrize("name,nx,nu,N", hr.NONFINITE_SETS)
def test_coverage_kernel_update_slack_on_every_class(name, nx, nu, N):
    """phase("update_slack") with x = u = 0 on all four families, the non-finite classes between finite ones of the same instance: the
    model bit for bit (NaN equal to NaN), and the duals untouched.  tiny_batch_phase launches the coverage kernel's single-phase form
    whatever the shape; kernel_path() describes solves only -- nothing to assert."""
    sets, duals, labels = hr.nonfinite_batch(name, nx, nu, N)
    B = duals["gl"].shape[0]
    s = make(hr.family(nx, nu, N), hr.config(sets, nx, nu, N, 1), B)
    for g, d in duals.items():
        s.set(g, d)
    s.phase("update_slack")
    want = hr.step(sets, np.zeros((B, nx, N)), np.zeros((B, nu, N - 1)), duals)
    for v, g, _, _ in hr.FAMILIES:
        assert differing(s.get(v), want[v], labels[g]) is None, (name, v, differing(s.get(v), want[v], labels[g]))
        assert np.all(hr.same_bits(s.get(g), duals[g]))
    s.close()


# ---- (e) a non-finite dual stays in its instance
@pytest.mark.parametrize("name", ["planes_12_4_10_lin3", "perknot_4_2_30_no_tile", "tile_20_4_10"])
def test_a_non_finite_dual_does_not_reach_its_wave_neighbours(name):
    """3 iterations, B = 16: instance 4 m + 1 carries ONE NaN or inf in a warm half-space dual (varying family, knot and row), the others
    the directed batch.  The poisoned instance is NaN all over in the reference too (0 * NaN in the backward pass); every clean instance
    must have the bits of the same launch without the poison -- the model's.  NaN arithmetic, not a fault; each launch runs once."""
    c = hr.CASES[name]
    nx, nu, N = c["dims"]
    prob, cfg, sets, x0, duals, labels = hr.case_setup(name, 3)
    B = 16
    x0, duals = x0[:B], {g: d[:B].copy() for g, d in duals.items()}
    poisoned = np.arange(B) % 4 == 1
    fams = [g for _, g, src, _ in on_families(sets) if src == "x"]
    for n, b in enumerate(np.flatnonzero(poisoned)):
        duals[fams[n % len(fams)]][b, (5 * n) % nx, (3 * n + 1) % N] = (np.nan, np.inf, -np.inf, np.nan)[n % 4]
    want = hr.pure_map_want(sets, nx, nu, N, x0, duals, 3)
    s = make(prob, cfg, B, c.get("options"))
    s.set_x0(x0)
    for v, g, _, _ in on_families(sets):
        s.set(g, duals[g])
    s.solve()
    assert_kernel(s, c["path"], c.get("used"))
    got = {k: s.get(k) for k in want}
    it = s.status()["iter"]
    s.close()
    assert np.all(it[~poisoned] == 3), it
    for k in want:
        assert differing(got[k][~poisoned], want[k][~poisoned]) is None, (name, k, differing(got[k][~poisoned], want[k][~poisoned]))
        assert np.all(np.isfinite(got[k][~poisoned]))


# ---- (f) launch modes
@pytest.mark.parametrize("name,path", [("quad_all", "regs"), ("sweep_20_4_10", "tile")])
def test_fused_steps_and_split_solves_leave_the_same_bits(name, path):
    """half-spaces on, one planes form and one tile form: T fused closed-loop steps = T launches, and a split solve (repack_after = 8;
    some instance runs past iteration 8, so a second launch resumes it from the saved slacks and duals) = the plain one, bit for bit
    in every half-space field.  (Which buffers the resumed launch of these two forms reads is not asserted here.)"""
    from hip_runner import make_batch, run_cases_hip
    suite = hr.identity_suite(name)
    suite["config"].update(max_iter=20, abs_pri_tol=1e-3, abs_dua_tol=1e-3)
    fields = ("x", "u") + tuple(f for v, g, _, _ in on_families(suite["config"]) for f in (v, g))
    plain = run_cases_hip(suite, options={"repack_after": 0})
    split = run_cases_hip(suite, options={"repack_after": 8})
    assert np.array_equal(plain["iter"], split["iter"]) and np.any(plain["iter"] > 8), plain["iter"]
    for k in fields:
        assert np.all(hr.same_bits(plain[k], split[k])), (name, "split", k)
    T, cases = 3, suite["cases"]

    def closed_loop(fused):
        s = make_batch(suite)
        s.set_x0(cases["x0"]); s.set("Xref", cases["Xref"]); s.set("Uref", cases["Uref"])
        for v, g, _, _ in on_families(suite["config"]):
            s.set(g, cases[g])
        s.set_option("advance_x0", 1)
        if fused:
            s.set_option("steps_per_launch", T)
        for _ in range(1 if fused else T):
            s.solve_async()
        out = {k: s.get(k) for k in fields}
        got = s.kernel_path()
        s.close()
        return out, got
    a, pa = closed_loop(False)
    b, pb = closed_loop(True)
    assert pa == path, pa
    assert pb in ((path, "cover") if path == "tile" else (path,)), pb
    for k in fields:
        assert np.all(hr.same_bits(a[k], b[k])), (name, "fused", k)
