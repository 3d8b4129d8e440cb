"""GPU: which instantiation of the one-row kernel a solve runs (csrc/one_row_variant.hpp choose_one_row_variant), end to end through
what a caller can read: kernel_path(), the options last_uniform_bounds / last_half_rows / last_prefetch and the names jit_used() gained
during the solve.  One solve of 64 instances per case, repack_after = 0 (no probe intervenes), no_tile = 1.  The expected read-backs are
written from the rules (profiles/one_row_variant.md), nothing is recorded from a library:
  - a shape of kernel_dims.txt without `lean` holds every slot (FULL), one with it only <box, no debug, mode 2> and its UB form (LEAN);
  - the HALF slots exist where nx + nu <= 8, the PREFETCH slots where pf_shape (kernel_entry.hpp, restated below) holds;
  - kernel_path() says "regs" for every form of a compiled-in shape but the per-instance box / half-space forms ("jit"), also where
    the variant itself had to be instantiated at run time;
  - a run-time instantiated variant is named admm_solve_kernel<nx, nu, N, soc, dbg, mode | 4 pb | 8 pl, lin, het, kmax, adapt[, true: ub]>.
Shapes: (2,2,3) and (4,1,10) FULL with HALF, (12,4,10) FULL with full rows, (4,2,10) LEAN with HALF, (8,8,10) LEAN with full rows; (4,2,30),
LEAN with HALF, is the one shape here WITHOUT a PREFETCH form (one wave per SIMD)."""
import numpy as np
import pytest

import tinympc_amd as tm

pytestmark = pytest.mark.gpu
B = 64
FULL = {(2, 2, 3), (4, 1, 10), (12, 4, 10)}
LEAN = {(4, 2, 10), (8, 8, 10), (4, 2, 30)}


def has_half(shape):
    return shape[0] + shape[1] <= 8


def has_prefetch(shape, half):
    """pf_shape of kernel_entry.hpp: eight waves per CU, 16-byte pieces that stay inside a record, the tile buffer within a wave's LDS share"""
    nx, nu, n = shape
    nz, ipw = nx + nu, 8 if half else 4
    waves = 4 * (2 if (n <= 10 or 2 * (6 * n + 2 * nz + 8) + 40 <= 256) else 1)
    arr = (ipw * n * nz * 8 + 1023) // 1024 * 1024
    return waves >= 8 and (n * nz) % 2 == 0 and 1024 + 3 * arr + 8 * (nx * 16 + 2 * n * 16) <= 160 * 1024 // waves


def test_the_shapes_are_what_the_cases_below_take_them_for():
    dims = {tuple(d) for d in tm.supported_dims()}
    assert FULL | LEAN <= dims
    assert [has_half(s) for s in ((2, 2, 3), (4, 1, 10), (12, 4, 10), (4, 2, 10), (8, 8, 10), (4, 2, 30))] == [True, True, False, True, False, True]
    assert has_prefetch((12, 4, 10), False) and has_prefetch((4, 2, 10), True) and not has_prefetch((4, 2, 30), True) and not has_prefetch((4, 2, 30), False)


def name(shape, soc=0, dbg=0, mode=2, lin=0, het=0, kmax=4, adapt=0, ub=0, pb=0, pl=0):
    tf = lambda v: "true" if v else "false"
    return "tinympc_amd::admm_solve_kernel<%d,%d,%d,%s,%s,%d,%d,%s,%d,%s%s>" % (shape + (tf(soc), tf(dbg), mode | (4 if pb else 0) | (8 if pl else 0), lin, tf(het), kmax, tf(adapt),
                                                                                        ",true" if ub else ""))


def solver(shape, hetero=False):
    nx, nu, N = shape
    prob, rng = tm.random_problem(nx, nu, N)
    if hetero:
        scale = 1.0 + 0.01 * np.arange(B)
        s = tm.TinyBatchSolver.hetero(prob["A"][None] * np.ones((B, 1, 1)), prob["B"][None] * scale[:, None, None], None, np.tile(prob["Q"], (B, 1)), np.tile(prob["R"], (B, 1)),
                                      np.full(B, prob["rho"]), N)
    else:
        s = tm.TinyBatchSolver.from_problem(prob, B)
    s.update_settings(max_iter=20)
    s.set_x0(rng.uniform(-0.5, 0.5, (B, nx)))
    s.set_option("repack_after", 0)
    s.set_option("no_tile", 1)
    return s, rng


def box(shape, varying):
    nx, nu, N = shape
    x_max = np.full((nx, N), 0.6) + (0.01 * np.arange(N)[None, :] if varying else 0.0)
    return -x_max, x_max, np.full((nu, N - 1), -0.3), np.full((nu, N - 1), 0.3)


def halfspaces(rng, n, width, lead=()):
    A = rng.normal(size=lead + (n, width))
    return A / np.linalg.norm(A, axis=-1, keepdims=True), rng.uniform(0.4, 0.8, lead + (n,))


def solve_and_read(s):
    before = set(n.replace(" ", "") for n in tm.jit_used())
    s.solve()
    gained = set(n.replace(" ", "") for n in tm.jit_used()) - before
    got = dict(path=s.kernel_path(), ub=s.get_option("last_uniform_bounds"), half=s.get_option("last_half_rows"), prefetch=s.get_option("last_prefetch"))
    assert np.all(np.isfinite(s.get("x")))
    s.close()
    return got, gained


def check(s, want, instantiated=None, what=None):
    """instantiated: the one variant the solve may have made at run time (it is in jit_used() afterwards, and nothing else was gained);
    None: the solve ran a compiled-in slot and gained nothing"""
    got, gained = solve_and_read(s)
    assert got == want, (what, got, want)
    if instantiated is None:
        assert not gained, (what, gained)
    else:
        assert gained <= {instantiated} and instantiated in {n.replace(" ", "") for n in tm.jit_used()}, (what, gained, instantiated)


PLAIN = [(shape, varying, use_ub, half_rows) for shape in ((2, 2, 3), (4, 1, 10), (12, 4, 10), (4, 2, 10), (8, 8, 10))
         for varying in (False, True) for use_ub in (1, 0) for half_rows in (1, 0)]


@pytest.mark.parametrize("shape,varying,use_ub,half_rows", PLAIN, ids=lambda v: "_".join(map(str, v)) if isinstance(v, tuple) else str(int(v)))
def test_plain_box_launch_kub_or_k002_and_the_half_upgrade(shape, varying, use_ub, half_rows):
    """The plain rung: kub where the box is knot-invariant and uniform_bounds is on, else k[0][0][2]; both are in the FULL and the LEAN
    set.  HALF from either where the slot exists and half_rows is on; khalf[1] counts as a UB form.  prefetch = -1 (by rule) leaves a
    batch of 8 or 16 tiles on the plain form: it wants three tiles per resident wave."""
    s, _ = solver(shape)
    s.set_bound_constraints(*box(shape, varying))
    s.set_option("uniform_bounds", use_ub)
    s.set_option("half_rows", half_rows)
    check(s, dict(path="regs", ub=int(use_ub and not varying), half=int(bool(half_rows) and has_half(shape)), prefetch=0), what=(shape, varying, use_ub, half_rows))


@pytest.mark.parametrize("shape,half_rows", [((12, 4, 10), 1), ((4, 2, 10), 1), ((4, 2, 10), 0), ((4, 2, 30), 1)], ids=str)
def test_prefetch_slot_of_the_chosen_variant(shape, half_rows):
    """prefetch = 1: wherever the form exists -- kpf[1] of kub, khalfpf[1] of khalf[1]; (4,2,30) has neither"""
    s, _ = solver(shape)
    s.set_bound_constraints(*box(shape, False))
    s.set_option("prefetch", 1)
    s.set_option("half_rows", half_rows)
    half = bool(half_rows) and has_half(shape)
    check(s, dict(path="regs", ub=1, half=int(half), prefetch=int(has_prefetch(shape, half))), what=(shape, half_rows))


@pytest.mark.parametrize("option,value", [("debug", 1), ("dpp_mode", 0), ("dpp_mode", 1)])
def test_debug_and_dpp_mode_take_k_soc_dbg_mode_without_ub_half_or_prefetch(option, value):
    """k[0][dbg][mode] of a FULL shape: the UB rung needs no debug and mode 2, HALF and PREFETCH start from kub / k[0][0][2] only"""
    s, _ = solver((2, 2, 3))
    s.set_bound_constraints(*box((2, 2, 3), False))
    s.set_option(option, value)
    s.set_option("prefetch", 1)
    check(s, dict(path="regs", ub=0, half=0, prefetch=0), what=(option, value))


@pytest.mark.parametrize("shape", [(4, 1, 10), (4, 2, 10)], ids=str)
def test_cone_kubsoc_on_a_full_shape_run_time_instantiated_without_ub_on_a_lean_one(shape):
    """The UB rung does not fall through: a LEAN shape has no kubsoc, so its cone variant is instantiated -- from a key without UB"""
    s, _ = solver(shape)
    s.set_bound_constraints(*box(shape, False))
    s.set_cone_constraints([0], [3], [0.7], [], [], [])            # (rows 0..2 of the state: the projection handles dimension 3 only)
    s.update_settings(max_iter=20, en_state_soc=1)
    lean = shape in LEAN
    check(s, dict(path="regs", ub=int(not lean), half=0, prefetch=0), instantiated=name(shape, soc=1) if lean else None, what=shape)


@pytest.mark.parametrize("count", [4, 8])
def test_shared_halfspaces_klin_at_four_per_knot_instantiated_at_eight(count):
    shape = (2, 2, 3)
    s, rng = solver(shape)
    s.set_bound_constraints(*box(shape, False))
    s.set_linear_constraints(*halfspaces(rng, count, 2), *halfspaces(rng, count, 2))
    s.update_settings(max_iter=20, en_state_linear=1, en_input_linear=1)
    check(s, dict(path="regs", ub=0, half=0, prefetch=0), instantiated=name(shape, lin=1, kmax=8) if count == 8 else None, what=count)


@pytest.mark.parametrize("shape,het_ub", [((2, 2, 3), 1), ((2, 2, 3), 0), ((4, 2, 10), 1)], ids=str)
def test_per_instance_data_khetub_khet_and_the_run_time_ub_form_of_a_lean_shape(shape, het_ub):
    s, _ = solver(shape, hetero=True)
    s.set_bound_constraints(*box(shape, False))
    s.set_option("het_ub", het_ub)
    check(s, dict(path="regs", ub=het_ub, half=0, prefetch=0), instantiated=name(shape, het=1, ub=1) if shape in LEAN else None, what=(shape, het_ub))


def test_adaptive_rho_kadapt():
    s, _ = solver((2, 2, 3))
    s.set_bound_constraints(*box((2, 2, 3), False))
    s.set_adaptive_rho(1, 0.1, 10.0, 1)
    s.compute_sensitivity()
    check(s, dict(path="regs", ub=0, half=0, prefetch=0))


def test_per_instance_box_is_instantiated_in_its_ub_form():
    shape = (2, 2, 3)
    s, _ = solver(shape)
    s.set_instance_bounds(*[np.broadcast_to(a, (B,) + a.shape) * (1.0 + 0.01 * np.arange(B))[:, None, None] for a in box(shape, False)])
    check(s, dict(path="jit", ub=1, half=0, prefetch=0), instantiated=name(shape, ub=1, pb=1))


def test_per_instance_halfspaces_are_instantiated_at_the_blocks_own_stride():
    shape = (2, 2, 3)
    s, rng = solver(shape)
    s.set_bound_constraints(*box(shape, False))
    s.set_instance_linear_constraints(*halfspaces(rng, 2, 2, (B,)), *halfspaces(rng, 2, 2, (B,)))
    s.update_settings(max_iter=20, en_state_linear=1, en_input_linear=1)
    check(s, dict(path="jit", ub=0, half=0, prefetch=0), instantiated=name(shape, lin=1, kmax=2, pl=1))
