"""CPU: the numpy model of the half-space step of update_slack (tests/halfspace_ref.py) against the C restatement, bit for bit, and
against the real reference's recorded answers (tests/golden/halfspace_edges.npz) -- bit for bit where a family has at most 3 rows,
within the standard summation bound beyond (the reference's Eigen reductions pair the terms of a'z and a'a differently from the
oracle's row-order loops once a row has more than 3 entries) -- on the directed classes: columns on a decision boundary, chains of
sequential projections, repeated, null, sparse and scaled half-spaces, time-varying tables that differ at every knot.  Also the two
constructions the GPU tests rest on: the pure-map family (A = B = 0: the state columns of a solve are the map iterated) and the
per-iteration identity on real dynamics (at max_iter = 1 a solver's own x, u and the warm duals reproduce its slacks and duals)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import halfspace_ref as hr  # noqa: E402
import scenarios as sc  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
HIPCC = "/opt/rocm/bin/hipcc"


def oracle_update_slack(sets, nx, nu, N, duals, x=None, u=None):
    """update_slack alone in the oracle, per instance -> the four slack fields"""
    o = sc.make_solver(OracleSolver, hr.family(nx, nu, N), hr.config(sets, nx, nu, N, 1))
    B = next(iter(duals.values())).shape[0]
    out = {}
    for b in range(B):
        o["x"] = np.zeros((nx, N)) if x is None else x[b]
        o["u"] = np.zeros((nu, N - 1)) if u is None else u[b]
        for _, g, _, _ in hr.FAMILIES:
            if g in duals:
                o[g] = duals[g][b]
        o.phase("update_slack")
        for v, g, _, _ in hr.FAMILIES:
            if g in duals:
                out.setdefault(v, np.zeros_like(duals[g]))[b] = o[v]
    o.close()
    return out


def test_scalar_and_vector_model_agree_and_every_draw_is_a_member():
    """the generators decide membership on a plain-Python restatement; the numpy model the tests compare with must be the same map"""
    for name, nx, nu, N, sets, duals, labels in hr.fixture_items()[:4]:
        for v, g, src, fam in hr.FAMILIES:
            A, b = hr.tables(sets, fam, N, nx, nu)
            cols = duals[g].transpose(0, 2, 1)
            out, f = hr.project(0.0 + cols, A, b)
            knots = cols.shape[1]
            A, b = np.broadcast_to(A, (knots,) + A.shape[-2:]), np.broadcast_to(b, (knots,) + b.shape[-1:])
            for bi in range(cols.shape[0]):
                for i in range(knots):
                    z1, viol, _, _ = hr._facts1(0.0 + cols[bi, i], A[i], b[i])
                    assert np.all(hr.same_bits(out[bi, i], z1)) and list(f["viol"][bi, i]) == viol
                    cls = hr.CLASSES[labels[g][bi, i]]
                    assert cls == "negzero" or hr.member(cls, 0.0 + cols[bi, i], A[i], b[i]), (name, fam, cls)


def test_the_time_varying_lookup_is_the_references():
    """half-space k of knot i: row nt * i + k of tv_Alin, tv_blin(k, i) (admm.cpp:186-211); the sets differ at every knot"""
    sets = hr.make_sets("plain", 6, 3, 10)
    tA, tb = sets["tv_linear"][0], sets["tv_linear"][1]
    A, b = hr.tables(sets, "tx", 10, 6, 3)
    assert A.shape == (10, 2, 6) and b.shape == (10, 2)
    for i in range(10):
        for k in range(2):
            assert np.array_equal(A[i, k], tA[2 * i + k]) and b[i, k] == tb[k, i]
    assert len({A[i].tobytes() for i in range(10)}) == 10 and len({b[i].tobytes() for i in range(10)}) == 10


@pytest.mark.parametrize("name,nx,nu,N", hr.NONFINITE_SETS)
def test_model_equals_the_oracle_through_update_slack_on_every_class(name, nx, nu, N):
    """update_slack alone, x = u = 0, all four families, the non-finite classes included (NaN equal to NaN)"""
    sets, duals, labels = hr.nonfinite_batch(name, nx, nu, N)
    got = oracle_update_slack(sets, nx, nu, N, duals)
    zero_x, zero_u = np.zeros((duals["gl"].shape[0], nx, N)), np.zeros((duals["gl"].shape[0], nu, N - 1))
    want = hr.step(sets, zero_x, zero_u, duals)
    seen = set()
    for v, g, _, _ in hr.FAMILIES:
        same = np.all(hr.same_bits(got[v], want[v]), axis=1)
        assert same.all(), (v, sorted({hr.CLASSES[c] for c in labels[g][~same]}))
        seen |= set(hr.class_counts(labels[g]))
    if name != "plain":
        assert seen & set(hr.NONFINITE)
    else:
        assert {"nan_in", "inf_in", "chain_on", "chain_off", "on_plane", "ulp_above", "ulp_below"} <= seen


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("name", list(hr.CASES))
def test_pure_map_family_iterates_the_model_in_the_oracle(name, iters):
    """every directed batch the GPU tests use: the oracle stays finite, runs its iterations, and its vlnew / gl / vlnew_tv / gl_tv are
    the model's map iterated, bit for bit, at every knot -- knot 0 with x0 != 0 included; the input families satisfy the own-output
    identity after one iteration"""
    c = hr.CASES[name]
    nx, nu, N = c["dims"]
    prob, cfg, sets, x0, duals, labels = hr.case_setup(name, iters)
    assert np.any(x0) or c["set"] == "scaled"
    want = hr.pure_map_want(sets, nx, nu, N, x0, duals, iters)
    fields = ("x", "u") + tuple(f for v, g, _, fam in hr.FAMILIES if sets[hr.FLAG[fam]] for f in (v, g))
    got, it = hr.oracle_solve(prob, cfg, x0, duals, fields)
    assert np.all(it == iters) and all(np.all(np.isfinite(a)) for a in got.values())
    assert np.array_equal(got["x"][:, :, 0], x0) and not np.any(got["x"][:, :, 1:]) and not np.any(np.signbit(got["x"][:, :, 1:]))
    for k in want:
        same = np.all(hr.same_bits(got[k], want[k]), axis=1)
        lab = labels[k if k in labels else {"vlnew": "gl", "vlnew_tv": "gl_tv"}[k]]
        assert same.all(), (k, sorted({hr.CLASSES[c_] for c_ in lab[~same]}))
    for v, g, src, fam in hr.FAMILIES:           # every class a family can hold at a knot has members there, whatever handed over
        if g not in labels:
            continue
        A, b = hr.tables(sets, fam, N, nx, nu)
        A, b = np.broadcast_to(A, (N,) + A.shape[-2:]), np.broadcast_to(b, (N,) + b.shape[-1:])
        can = set().union(*[hr.classes_for(A[i], b[i]) for i in range(N)])
        counts = hr.class_counts(labels[g])
        assert set(counts) == can and min(counts.values()) >= 4, (g, counts, can)
        if "one_violated" in can and iters == 1:   # the violated half-space runs over every slot, the last before the padding included
            cols = (x0[:, None, :] * (np.arange(N) == 0)[None, :, None] + duals[g].transpose(0, 2, 1))[labels[g] == hr.CLASSES.index("one_violated")]
            knot = np.broadcast_to(np.arange(N), labels[g].shape)[labels[g] == hr.CLASSES.index("one_violated")]
            hit = {int(np.flatnonzero(hr.project(z, A[i], b[i])[1]["viol"])[0]) for z, i in zip(cols, knot)}
            alone = set().union(*[set(hr._rows(A[i])) - {k for pair in hr._dups(A[i], b[i]) for k in pair} for i in range(N)])
            assert hit >= alone, (g, hit, alone)          # (a repeated half-space cannot be the only one violated)
    if iters == 1:
        own = hr.step(sets, got["x"], got["u"], duals)
        for v, g, src, fam in hr.FAMILIES:
            if src == "u" and sets[hr.FLAG[fam]]:
                assert np.all(hr.same_bits(got[v], own[v])) and np.all(hr.same_bits(got[g], own[g])), v


@pytest.mark.parametrize("name", list(hr.IDENTITY_SUITES))
def test_per_iteration_identity_on_real_dynamics_in_the_oracle(name):
    """admm.cpp:378-392: the linear cost and the passes come first, then update_slack and update_dual -- so at max_iter = 1 the
    oracle's own x, u outputs and the warm duals give its slacks and duals through the model, bit for bit, in all four families"""
    suite = hr.identity_suite(name)
    suite["config"]["max_iter"] = 1
    out = sc.run_cases(OracleSolver, suite)
    own = hr.step(hr.sets_of(suite["config"]), out["x"], out["u"], suite["cases"])
    moved = {"x": [], "u": []}
    for v, g, src, fam in hr.FAMILIES:
        if suite["config"][hr.FLAG[fam]]:
            assert np.all(hr.same_bits(out[v], own[v])) and np.all(hr.same_bits(out[g], own[g])), v
            moved[src].append(own["viol_" + fam].any(axis=-1).ravel())
    for src in ("x", "u"):                       # the test must not pass on identities: at least half of the columns project
        assert moved[src] and np.concatenate(moved[src]).mean() >= 0.5, (src, np.concatenate(moved[src]).mean())


@pytest.fixture(scope="module")
def edges():
    z = np.load(os.path.join(GOLDEN, "halfspace_edges.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_items_are_members_of_their_classes(edges):
    """the committed inputs, read back (the generators' last bits depend on the machine's BLAS, so they are not drawn again): every
    column is a member of the class its label names, on the model's own facts; every class a family can hold is there; about 2 000"""
    columns = 0
    for name, nx, nu, N, sets, duals, labels in hr.fixture_from(edges):
        for v, g, src, fam in hr.FAMILIES:
            A, b = hr.tables(sets, fam, N, nx, nu)
            knots = duals[g].shape[2]
            A, b = np.broadcast_to(A, (knots,) + A.shape[-2:]), np.broadcast_to(b, (knots,) + b.shape[-1:])
            for bi in range(duals[g].shape[0]):
                for i in range(knots):
                    cls, gl = hr.CLASSES[labels[g][bi, i]], duals[g][bi, :, i]
                    assert cls in hr.classes_for(A[i], b[i]), (name, fam, cls)
                    assert hr.member(cls, 0.0 + gl, A[i], b[i]) and (cls != "negzero" or np.any((gl == 0) & np.signbit(gl))), (name, fam, cls)
            assert set(hr.class_counts(labels[g])) == set().union(*[hr.classes_for(A[i], b[i]) for i in range(knots)]), (name, fam)
            columns += labels[g].size
    assert 1800 <= columns <= 2600, columns


def test_model_against_the_reference_fixture(edges):
    """bit for bit where a family has at most 3 rows; beyond, the reference's Eigen reductions pair the terms of the two sums
    differently: within hr.summation_bound of each other wherever both took the same branches; a column on which they did not must
    flip only decisions whose a'z lies within the bound on |d cv| of the offset, and match within the bound along the flipped pattern.  The largest observed ratio to the bound is printed
    (profiles/halfspace_edge_tests.md records it)."""
    worst, bitwise, bounded, differ, flipped, exact_checked = 0.0, 0, 0, 0, 0, 0
    for n_, (name, nx, nu, N, sets, duals, labels) in enumerate(hr.fixture_from(edges)):
        for v, g, src, fam in hr.FAMILIES:
            A, b = hr.tables(sets, fam, N, nx, nu)
            cols = 0.0 + duals[g].transpose(0, 2, 1)
            want, f = hr.project(cols, A, b)
            ref = edges["%d.%s" % (n_, v)].transpose(0, 2, 1)
            n = cols.shape[-1]
            same = np.all(hr.same_bits(want, ref), axis=-1)
            if n <= 3:
                assert same.all(), (name, fam, sorted({hr.CLASSES[c] for c in labels[g][~same]}))
                bitwise += same.size
                continue
            knots = cols.shape[1]
            A, b = np.broadcast_to(A, (knots,) + A.shape[-2:]), np.broadcast_to(b, (knots,) + b.shape[-1:])
            for bi, i in np.argwhere(~same):
                differ += 1
                viol = list(f["viol"][bi, i])
                bound = hr.summation_bound(cols[bi, i], A[i], b[i], viol)
                err = np.abs(ref[bi, i] - want[bi, i])
                if np.all(err <= bound):
                    worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
                    continue
                # another branch pattern: the reference decided cv > b differently at some half-spaces.  Every pattern is tried; one must
                # (1) flip only decisions whose cv lies within the bound on |d cv| of b and (2) reproduce the reference within the
                # summation bound taken along THAT pattern
                K, ok = len(viol), False
                for code in range(2 ** K):
                    pat = [bool(code >> k & 1) for k in range(K)]
                    zp, cvp = hr.project_forced(cols[bi, i], A[i], b[i], pat)
                    flips = [k for k in range(K) if pat[k] != bool(cvp[k] > b[i][k])]
                    if not flips or not np.all(np.isfinite(zp)):
                        continue
                    bound_p, dcv = hr.summation_bound(cols[bi, i], A[i], b[i], pat, with_dcv=True)
                    if all(abs(cvp[k] - b[i][k]) <= dcv[k] for k in flips) and np.all(np.abs(ref[bi, i] - zp) <= bound_p):
                        worst = max(worst, float(np.max(np.abs(ref[bi, i] - zp) / np.maximum(bound_p, 1e-300))))
                        ok = True
                        break
                assert ok, (name, fam, hr.CLASSES[labels[g][bi, i]], err.tolist(), bound.tolist())
                flipped += 1
            bounded += same.size
            # the exact evaluation agrees with the model within the same bound (the bound is a bound on the MODEL's error too)
            for bi in range(cols.shape[0]):
                for i in range(bi % 3, knots, 3):
                    pat = list(f["viol"][bi, i])
                    exact = np.array([float(q) for q in hr.exact_column(cols[bi, i], A[i], b[i], pat)])
                    assert np.all(np.abs(exact - want[bi, i]) <= hr.summation_bound(cols[bi, i], A[i], b[i], pat)), (name, fam, bi, i)
                    exact_checked += 1
    print("halfspace fixture: bitwise columns", bitwise, "bounded columns", bounded, "of which differ", differ, "flipped branch", flipped,
          "largest ratio to the summation bound", worst, "columns checked against exact arithmetic", exact_checked)
    assert bitwise >= 400 and bounded >= 400 and exact_checked >= 400


@pytest.fixture(scope="module")
def lin_forms(tmp_path_factory):
    assert os.path.exists(HIPCC), "hipcc is what builds the library: the per-knot expectation of the GPU tests rests on this pin"
    exe = str(tmp_path_factory.mktemp("lin_forms") / "dump")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "tinympc_amd", "csrc"), "-x", "hip",
                    os.path.join(ROOT, "tests", "dropin", "lin_forms_dump.cpp"), "-o", exe], check=True, capture_output=True, timeout=600)

    def run(*rows):
        out = subprocess.run([exe] + [",".join(str(v) for v in r) for r in rows], check=True, capture_output=True, text=True, timeout=60).stdout
        return [tuple(int(v) for v in ln.split()) for ln in out.splitlines()]
    return run


def test_which_shapes_take_the_slack_planes_and_which_the_per_knot_form(lin_forms):
    """the rows tests/test_gpu_halfspace_edges.py depends on (nx, nu, N, soc, lin, kmax, ub) -> planes, waves, LDS bytes.  The dispatcher
    asks with ub = 0 (the one-row half-space variants are instantiated without UB): (4,2,30) with time-varying tables is the per-knot
    register form (67 712 B > 64 KiB - 512); every planes case of the GPU tests fits"""
    rows = lin_forms((4, 2, 30, 0, 2, 4, 0), (12, 4, 10, 0, 3, 4, 0), (12, 4, 10, 0, 1, 4, 0), (12, 4, 10, 0, 2, 4, 0), (12, 4, 10, 0, 3, 8, 0),
                     (12, 4, 10, 0, 1, 8, 0), (12, 4, 10, 0, 1, 16, 0), (6, 3, 10, 1, 3, 4, 0), (6, 3, 10, 0, 3, 4, 0), (5, 3, 7, 0, 3, 4, 0))
    assert rows[0][7:] == (0, 1, 67712) and 8 * (64 + 960 + 5760 + 1680) == 67712
    assert all(r[7] == 1 and r[9] <= 64 * 1024 - 512 for r in rows[1:]), rows
