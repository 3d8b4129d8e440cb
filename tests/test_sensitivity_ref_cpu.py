"""CPU: the closed form of tests/sens_ref.py IS the derivative of tiny_setup's cache with respect to rho -- pinned against central
differences of a Riccati recursion iterated to 1e-14 (h = 1e-5 rho).  The finite-difference floor measured for these systems is
1.0e-8; the bound 1e-6 leaves two orders of margin and is four orders below what any wrong formula gives."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import scenarios as sc  # noqa: E402
import sens_ref  # noqa: E402


def systems():
    prob, _ = sc.load_problem("quadrotor_20hz")
    out = [("quadrotor", (prob["A"], prob["B"], prob["Q"], prob["R"], prob["rho"]))]
    rng = np.random.default_rng(20261017)
    for nx, nu in ((4, 2), (12, 4), (20, 8)):
        out.append((f"random_{nx}_{nu}", sens_ref.random_system(rng, nx, nu)))
    return out


@pytest.mark.parametrize("name,system", systems(), ids=[n for n, _ in systems()])
def test_closed_form_equals_central_differences_of_the_converged_cache(name, system):
    A, B, Qd, Rd, rho = system
    K, P, C1, C2 = sens_ref.dare_cache(A, B, Qd, Rd, rho)
    t = sens_ref.tables(A, B, K, C1)
    assert 1 <= t["steps"] <= 64
    h = 1e-5 * rho
    plus, minus = sens_ref.dare_cache(A, B, Qd, Rd, rho + h), sens_ref.dare_cache(A, B, Qd, Rd, rho - h)
    for k, (p, m) in zip(("dKinf_drho", "dPinf_drho", "dC1_drho", "dC2_drho"), zip(plus, minus)):
        fd = (p - m) / (2.0 * h)
        err = sens_ref.rel_max(t[k], fd)
        print(name, k, "relative max-norm error against central differences", err)
        assert err < 1e-6, (name, k, err)


def test_the_quadrotor_literals_of_the_reference_are_a_different_set():
    """what tiny_initialize_sensitivity_matrices installs is kept for parity and is NOT this derivative"""
    prob, _ = sc.load_problem("quadrotor_20hz")
    K, P, C1, C2 = sens_ref.dare_cache(prob["A"], prob["B"], prob["Q"], prob["R"], prob["rho"])
    t = sens_ref.tables(prob["A"], prob["B"], K, C1)
    lit = sc.quadrotor_sensitivity()
    assert np.max(np.abs(lit["dPinf_drho"])) < 0.1 * np.max(np.abs(t["dPinf_drho"]))
    assert not np.any(lit["dC1_drho"]) and np.all(np.diag(t["dC1_drho"]) < 0.0)
