"""CPU: the closed-loop fuzzer's helper logic that needs no GPU -- a trial is a pure function of its seed, and the sensitivity
check classifies the one loop of round 1 that ended 5.8e-6 away from the oracle (seed 600878) as ill-conditioned: the oracle
itself moves further than that when its initial state is perturbed by 1e-14."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(HERE, ".."), os.path.join(HERE, "..", "oracle"), os.path.join(HERE, "..", "tools"), HERE):
    sys.path.insert(0, p)

from cpu_solvers import build_oracle  # noqa: E402


def test_trials_are_functions_of_the_seed_and_the_chaotic_loop_is_recognised():
    assert build_oracle()
    import fuzz_closed_loop as f
    a, b = f.draw(600878), f.draw(600878)
    assert (a["nx"], a["nu"], a["N"], a["T"], a["launches"]) == (8, 4, 30, 8, 2)
    assert np.array_equal(a["x0"], b["x0"]) and np.array_equal(a["fams"][0]["A"], b["fams"][0]["A"])
    ep = f.oracle_episode(a, 0)
    assert len(ep) == 16 and all(it == 29 for _, _, it in ep)              # every solve of that loop stops at max_iter
    amp = f.sensitivity(a, 0)
    assert amp > 1e-6, amp                                                 # 1e-14 in, more than the fuzzer's tolerance out
    calm = f.draw(700001)
    assert f.sensitivity(calm, 0) < 1e-9


def test_a_loop_that_has_gone_chaotic_is_recognised_whatever_size_the_probe_has():
    """Round 6, seed 67620 instance 1: 21 closed-loop steps that all run out of iterations with cones and half-spaces active.  The
    oracle's own final state moves by order one for perturbations of 1e-15 and 1e-13 and by 1e-2 for 1e-14 -- with identical
    iteration counts in every case: sensitivity() takes the largest response of three probe sizes, so that a deviation of that size
    on the GPU is reported as a note, not as a mismatch."""
    assert build_oracle()
    import fuzz_closed_loop as f
    d = f.draw(67620)
    assert (d["nx"], d["nu"], d["N"]) == (4, 8, 10)
    one = f.sensitivity(d, 1, eps=1e-14)
    three = f.sensitivity(d, 1)
    assert three >= one and three > 0.1, (one, three)
    base, pert = f.oracle_episode(d, 1, 0.0), f.oracle_episode(d, 1, 1e-15)
    assert [it for _, _, it in base] == [it for _, _, it in pert]          # the iteration counts do not move: only the fields do


def test_hetero_adaptive_draws_are_functions_of_the_seed():
    """tools/fuzz_parity.py hetero_adaptive_draw: two draws of one seed are identical, down to every array, and the oracle half of a
    trial (hetero_adaptive_oracle, hetero_adaptive_floor) runs from a draw alone"""
    assert build_oracle()
    import fuzz_parity as f
    import sens_ref

    def same(a, b):
        if isinstance(a, dict):
            return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
        if isinstance(a, (list, tuple)):
            return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
        return np.array_equal(a, b)
    seen = set()
    for seed in range(1, 41):
        a, b = f.hetero_adaptive_draw(seed), f.hetero_adaptive_draw(seed)
        assert same(a, b), seed
        assert (a["nx"], a["nu"], a["N"]) in f.HET_ADAPT_SHAPES and 1 <= a["B"] <= 9 and 0 <= a["kw"]["max_iter"] <= 59
        assert len({fam["rho"] for fam in a["fams"]}) == a["B"]                    # every instance its own rho
        seen.add(((a["nx"], a["nu"], a["N"]), a["tables"] is None, a["cache"] is None, "state_cone" in a["kw"]))
        if "state_cone" in a["kw"]:
            assert (a["nx"], a["nu"], a["N"]) == (6, 3, 10)
    assert {k[0] for k in seen} == set(f.HET_ADAPT_SHAPES) and {k[1] for k in seen} == {k[2] for k in seen} == {k[3] for k in seen} == {True, False}
    d = f.hetero_adaptive_draw(8)                                                  # (6, 3, 10), B = 4, computed tables
    assert (d["nx"], d["B"], d["tables"]) == (6, 4, None)
    fam = d["fams"][1]
    K, _, C1, _ = sens_ref.dare_cache(fam["A"], fam["B"], fam["Q"], fam["R"], fam["rho"])
    tab = sens_ref.tables(fam["A"], fam["B"], K, C1)
    r1, r2 = f.hetero_adaptive_oracle(d, 1, tab), f.hetero_adaptive_oracle(d, 1, tab)
    assert r1["counts"] == r2["counts"] and all(np.array_equal(r1[k], r2[k]) for k in r1 if k != "counts")
    assert f.hetero_adaptive_floor(d, 1, tab) < 1e-9
