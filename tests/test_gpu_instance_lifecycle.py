"""GPU tests of what the four per-instance families share on ONE handle: the drop of a family when its shared setter comes back, the
reinstall after it, and the dirty marks in between (csrc/batch_instance.hip).  The per-family tests (test_gpu_instance_bounds.py,
..._halfspaces.py, ..._cones.py, test_gpu_disturbance.py) take a fresh handle per case; here a handle that has been through every
family's install -> replace -> reinstall must be indistinguishable, bit for bit, from a fresh one given the final data at once.  The
rocket's shape (6, 3, 10: cones, a one-row instantiation), nine instances (two full waves of four and a tail of one), default
tolerances.  The library is compared with itself: no tolerance is involved."""
import numpy as np
import pytest

import disturbance_cases as dc
import instance_cone_cases as icc
import instance_halfspace_cases as ihc
import tinympc_amd as tm
from test_gpu_disturbance import assert_same_bits, fused, snapshot

pytestmark = pytest.mark.gpu
NX, NU, N, B = 6, 3, 10, 9
STEPS = 3
MAX_ITER = icc.MAX_ITER
LAST = ("last_instance_bounds", "last_instance_linear", "last_instance_cones", "last_disturbance")
KEYS = icc.KEYS + icc.LIN_KEYS


def problem():
    """the family and the records every handle starts from: x0 outside the state cone on the side whose projection reads the
    coefficient, as instance_cone_cases.case draws it"""
    rng = np.random.default_rng(6310)
    fam = icc.family(NX, NU, N, 6310)
    x0 = rng.uniform(0.5, 1.0, (B, NX)) * rng.choice([-1.0, 1.0], (B, NX))
    x0[:, dc.ACX[0] + 2] = rng.uniform(0.2, 0.45, B)
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, NX, 1)), N, axis=2) + rng.normal(0, 0.02, (B, NX, N))
    Uref = rng.normal(0, 0.05, (B, NU, N - 1))
    return fam, x0, Xref, Uref


def instance_data(x0, seed, n_state):
    """one draw of all four families: a box per instance, n_state static state half-spaces around x0 and one loose input half-space
    (the sets of instance_cone_cases' "pl" case), a coefficient per cone and instance, a 3-step disturbance"""
    rng = np.random.default_rng(seed)
    Ax, bx, _, _ = ihc.state_sets(x0, NX, N, rng, ns=n_state)
    return dict(box=dc.wide_boxes(B, NX, NU, N, seed + 1), linear=(Ax, bx, rng.normal(0, 1, (B, 1, NU)), rng.uniform(0.3, 0.6, (B, 1))),
                cones=(rng.uniform(0.2, 1.5, (B, 1)), rng.uniform(0.2, 1.5, (B, 1))),
                w=rng.uniform(0.1, 0.3, (STEPS, B, NX)) * rng.choice([-1.0, 1.0], (STEPS, B, NX)))


def handle(fam, cone_shared, **switches):
    s = tm.TinyBatchSolver.from_problem(fam, B)
    if cone_shared is not None:
        s.set_cone_constraints(dc.ACX, [3], cone_shared[0], dc.ACU, [3], cone_shared[1])
    s.update_settings(max_iter=MAX_ITER, **switches)
    return s


def start(s, x0, Xref, Uref):
    s.set_x0(x0)
    s.set_x_ref(Xref)
    s.set_u_ref(Uref)


def install(s, d):
    s.set_instance_bounds(*d["box"])
    s.set_instance_linear_constraints(*d["linear"])
    s.set_instance_cone_coefficients(*d["cones"])
    s.set_disturbance(d["w"])


def assert_getters(s, box, linear, cones, w):
    """every getter, every instance: box / linear / cones [B, ...] per-instance arrays; w None: no sequence installed"""
    for i in range(B):
        for got, want in zip(s.instance_bounds(i), box):
            assert np.array_equal(got, want[i]), i
        for got, want in zip(s.instance_linear_constraints(i), linear):
            assert np.array_equal(got, want[i]), i
        for got, want in zip(s.get_instance_cone_coefficients(i), cones):
            assert np.array_equal(got, want[i]), i
        if w is not None:
            for k in range(len(w)):
                assert np.array_equal(s.get_disturbance(k, i), w[k, i]), (k, i)
    if w is None:
        assert s.get_option("disturbance") == 0
        with pytest.raises(tm.TinyMPCError):
            s.get_disturbance(0, 0)


def test_all_four_families_replaced_and_reinstalled_leave_no_trace():
    fam, x0, Xref, Uref = problem()
    on = dict(en_state_bound=1, en_input_bound=1, en_state_soc=1, en_input_soc=1, en_state_linear=1, en_input_linear=1)
    first, final = instance_data(x0, 1, n_state=1), instance_data(x0, 2, n_state=3)
    shared_cones = (np.array([0.6]), np.array([0.9]))
    a = handle(fam, (np.array([1.0]), np.array([1.0])), **on)
    start(a, x0, Xref, Uref)
    install(a, first)
    fused(a, STEPS)                                                  # (discarded: every block has been built and read once)
    assert [a.get_option(k) for k in LAST] == [1, 1, 1, 1] and a.get_option("instance_linear") == 1
    # every family back on its shared or removed form: the shared data is instance 0's of the first draw
    shared_box = [v[0] for v in first["box"]]
    shared_lin = [v[0] for v in first["linear"]]
    a.set_bound_constraints(*shared_box)
    a.set_linear_constraints(*shared_lin)
    a.set_cone_constraints(dc.ACX, [3], shared_cones[0], dc.ACU, [3], shared_cones[1])
    a.set_disturbance(None)
    assert [a.get_option(k) for k in ("instance_bounds", "instance_linear", "instance_cones", "disturbance")] == [0, 0, 0, 0]
    assert_getters(a, [np.broadcast_to(v, (B,) + v.shape) for v in shared_box], [np.broadcast_to(v, (B,) + v.shape) for v in shared_lin],
                   [np.broadcast_to(v, (B, 1)) for v in shared_cones], None)
    # the final data: three state half-spaces where there was one (block stride 1 -> 4)
    install(a, final)
    a.reset()
    start(a, x0, Xref, Uref)
    log_a = fused(a, STEPS)
    got_a = snapshot(a, KEYS)

    b = handle(fam, shared_cones, **on)
    start(b, x0, Xref, Uref)
    install(b, final)
    log_b = fused(b, STEPS)
    got_b = snapshot(b, KEYS)

    assert_same_bits(got_a, got_b, "a handle that went through install -> replace -> reinstall against a fresh one")
    assert np.array_equal(log_a[0], log_b[0]) and np.array_equal(log_a[1], log_b[1])
    assert np.any(np.abs(log_a[0]) > 1), "nothing iterates"
    assert a.kernel_path() == b.kernel_path(), (a.kernel_path(), b.kernel_path())
    assert [a.get_option(k) for k in LAST] == [b.get_option(k) for k in LAST] == [1, 1, 1, 1]
    assert a.get_option("disturbance_step") == b.get_option("disturbance_step") == STEPS
    for s in (a, b):
        assert_getters(s, final["box"], final["linear"], final["cones"], final["w"])
    a.close()
    b.close()


def test_half_spaces_alone_on_the_one_row_form_dropped_reinstalled_and_their_offsets_moved():
    fam, x0, Xref, Uref = problem()
    on = dict(en_state_bound=0, en_input_bound=0, en_state_linear=1, en_input_linear=1)
    first, final = instance_data(x0, 3, n_state=1)["linear"], instance_data(x0, 4, n_state=3)["linear"]
    moved = (final[1] * 0.9, final[3] * 1.1)                         # the offsets-only update: every offset moves, no coefficient does
    keys = ihc.BOX_KEYS + icc.LIN_KEYS

    def solve(s):
        s.solve()
        assert s.kernel_path() == "jit" and s.get_option("last_instance_linear") == 1, (s.kernel_path(), s.get_option("last_instance_linear"))
        return snapshot(s, keys)

    a = handle(fam, None, **on)
    start(a, x0, Xref, Uref)
    a.set_instance_linear_constraints(*first)
    solve(a)
    a.set_linear_constraints(*[v[0] for v in first])                 # dropped to the shared set ...
    assert a.get_option("instance_linear") == 0
    a.set_instance_linear_constraints(*final)                        # ... three where there was one ...
    solve(a)                                                         # (the blocks are built at stride 4: the update below rewrites offsets in them)
    a.set_instance_linear_constraints(None, moved[0], None, moved[1])
    a.reset()
    start(a, x0, Xref, Uref)
    got_a = solve(a)

    b = handle(fam, None, **on)
    start(b, x0, Xref, Uref)
    b.set_instance_linear_constraints(final[0], moved[0], final[2], moved[1])
    got_b = solve(b)

    assert_same_bits(got_a, got_b, "dropped, reinstalled and offsets-only updated against a fresh handle")
    assert np.any(got_a["iter"] > 1), "nothing iterates"
    for i in range(B):
        for got, want in zip(a.instance_linear_constraints(i), (final[0], moved[0], final[2], moved[1])):
            assert np.array_equal(got, want[i]), i
    a.close()
    b.close()
