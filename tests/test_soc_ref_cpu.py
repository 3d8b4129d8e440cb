"""CPU: the numpy model of project_soc (tests/soc_ref.py) against the real reference's recorded outputs and against the C restatement,
on the directed set of tests/golden/project_soc_edges.npz -- inputs within a float rounding of a branch boundary, at the all-inside
fast path's margin, at both ends of the float and double ranges, non-finite -- and the construction that drives such inputs through
whole solves: on the A = 0 family the cone rows of a solve are the pure map vcnew = P(gc), gc = gc - vcnew, bit for bit."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import scenarios as sc  # noqa: E402
import soc_ref as sr  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


@pytest.fixture(scope="module")
def edges():
    z = np.load(os.path.join(GOLDEN, "project_soc_edges.npz"))
    return {k: z[k] for k in z.files}


def test_fixture_is_the_generators_directed_set(edges):
    """the committed inputs are what tests/soc_ref.py draws today (a changed generator must regenerate the fixture), about 2 000 items"""
    s, mu, lab, names = sr.fixture_items()
    assert np.all(sr.same_bits(edges["s"], s)) and np.array_equal(edges["mu"], mu) and np.array_equal(edges["label"], lab)
    assert tuple(edges["names"]) == names
    assert 1800 <= len(s) <= 2200


def test_model_equals_the_reference_bit_for_bit(edges):
    out, _ = sr.project(edges["s"], edges["mu"])
    same = np.all(sr.same_bits(out, edges["out"]), axis=1)
    assert np.array_equal(np.isnan(out), np.isnan(edges["out"]))
    assert same.all(), [(str(edges["names"][edges["label"][i]]), edges["mu"][i], edges["s"][i].tolist()) for i in np.flatnonzero(~same)[:5]]


def test_oracle_equals_the_reference_bit_for_bit(edges):
    prob, _ = sc.load_problem("codegen_random")
    o = sc.make_solver(OracleSolver, prob, sc.default_config(prob))
    got = np.stack([o.project_soc(edges["s"][i], edges["mu"][i]) for i in range(len(edges["s"]))])
    o.close()
    same = np.all(sr.same_bits(got, edges["out"]), axis=1)
    assert same.all(), [(str(edges["names"][edges["label"][i]]), edges["mu"][i], edges["s"][i].tolist()) for i in np.flatnonzero(~same)[:5]]


def test_every_class_is_populated_on_the_reference_alone(edges):
    """membership decided from the recorded inputs and the REFERENCE's outputs where the output tells (the branch taken), else from the
    class's defining property on the inputs: at least 32 of each (exact: sqrt(q) == u0 in double, the float rounding goes either way)"""
    names = [str(n) for n in edges["names"]]
    s, mu, out, lab = edges["s"], edges["mu"], edges["out"], edges["label"]
    zeros = np.all(out == 0, axis=1)
    kept = np.all(sr.same_bits(out, s), axis=1)
    for k, name in enumerate(names):
        at = lab == k
        assert at.sum() >= sr.MIN_PER_CLASS, (name, int(at.sum()))
        if name in sr.CLASSES:
            assert np.all(sr.member(name, s[at], mu[at])), name
    want = {"rounded_in": kept, "neg_rounded_in": zeros, "margin_below": kept, "margin_above": kept,
            "below": zeros, "inside": kept, "zero": zeros, "u0_small": kept, "u0_big": kept, "nan_head": zeros, "nan_last": zeros,
            "rounded_out": ~kept & ~zeros, "neg_rounded_out": ~kept & ~zeros, "outside": ~kept & ~zeros, "quot_tiny": ~kept}
    for name, prop in want.items():
        at = lab == names.index(name)
        assert np.all(prop[at]), name
    fast = sr.fast_path_takes(s, mu)
    assert np.all(fast[lab == names.index("margin_below")]) and not np.any(fast[lab == names.index("margin_above")])
    assert not np.any(fast[np.isin(lab, [names.index(c) for c in ("u0_small", "u0_big", "q_big", "rounded_in", "exact", "nan_head", "nan_last", "inf_last")])])
    assert np.all(kept[fast])                                        # what the fast path would copy through, the reference keeps


CASES = sr.CASES
oracle_cone_rows = sr.oracle_cone_rows


@pytest.mark.parametrize("iters", [1, 3])
@pytest.mark.parametrize("form,mu_set", CASES)
def test_zero_dynamics_family_iterates_the_pure_map_in_the_oracle(form, mu_set, iters):
    """every directed batch the GPU tests use: each class has its 32 members, and the oracle's vcnew / gc on the cone rows after 1 and 3
    iterations are the model's, bit for bit, at every knot (the rows of no cone: vcnew = x, gc = +0)"""
    items, labels, mus = sr.directed_batch(form, mu_set, iters)
    counts = sr.class_counts(labels)
    for mu in mus:
        for c in sr.classes_for(mu, iters > 1, True):
            assert counts.get(c, 0) >= sr.MIN_PER_CLASS, (c, counts)
    L, B, K, N = labels.shape
    mu_arr = np.asarray(mus)[None, :, None]
    rng = np.random.default_rng(3)
    for l in range(L):
        x0 = np.zeros((B, sr.FORMS[form]["nx"]))
        x0[:, sr.noncone_rows(form)] = rng.normal(0.0, 1.0, (B, len(sr.noncone_rows(form))))
        v, g, it = oracle_cone_rows(form, mu_set, iters, sr.pack(form, items[l]), x0)
        want_v, want_g = sr.iterate(items[l], mu_arr, iters)
        assert np.all(it == iters)
        for name, got, want in (("vcnew", v, want_v), ("gc", g, want_g)):
            same = np.all(sr.same_bits(sr.unpack(form, got), want), axis=-1)
            assert same.all(), (name, [sr.CLASSES[c] for c in labels[l][~same][:6]], np.argwhere(~same)[:6].tolist())
        assert not np.any(g[:, sr.noncone_rows(form), :]) and not np.any(np.signbit(g[:, sr.noncone_rows(form), :]))


@pytest.mark.parametrize("form", ["one_cone_6_3_10", "wide_20_4_10"])
def test_early_and_late_instances_iterate_the_map_as_often_as_they_run(form):
    """the batch of tests/test_gpu_soc_edges.py's stopping-rows test in the oracle: default tolerances, max_iter = 4, dynamics on the rows
    of no cone; a zero x0 converges at iteration 1, 1e3 in a row of no cone runs to the cap; the cone rows are the map iterated that often"""
    f = sr.FORMS[form]
    B, N = 8, f["N"]
    rng = np.random.default_rng(44)
    mus = np.array(sr.cone_setup(form, "mixed")[2])
    x0 = np.zeros((B, f["nx"]))
    x0[1::2, sr.noncone_rows(form)[0]] = 1e3
    items = np.stack([sr.draw(rng, "margin_below", mu, B * N).reshape(B, N, 3) for mu in mus], axis=1)
    v, g, it = oracle_cone_rows(form, "mixed", 4, sr.pack(form, items), x0, tol=1e-3, dynamics=True)
    assert np.all(it[0::2] == 1) and np.all(it[1::2] == 4), it
    for n in (1, 4):
        want_v, want_g = sr.iterate(items[it == n], mus[None, :, None], n)
        assert np.all(sr.same_bits(sr.unpack(form, v[it == n]), want_v)) and np.all(sr.same_bits(sr.unpack(form, g[it == n]), want_g))
