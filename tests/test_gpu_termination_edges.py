"""GPU: the termination test (admm.cpp:310-328) of every kernel form with each single (row, knot, residual kind) in turn as the ONLY
entry that keeps a solve open -- the batches of tests/termination_ref.py, whose preconditions tests/test_termination_ref_cpu.py asserts
on the oracle.  Every test compares with the oracle run of the same suite.

The one-row kernel probes two slots before it forms the residuals, AND-folds a ballot per DPP row (per half row on the HALF forms),
forces a full test on the last check of a launch or stage, and has two residual paths (formed inside the test for N <= 12, accumulated
in the forward sweep for longer horizons); the tile kernel reduces over an instance's W x R rows under an instance mask with an escape
for lanes without a row and, on some forms, reads v back from its HBM record; the coverage kernel has a third version.  A kernel that
misses an offender reports iter = 1, solved = 1 where the oracle has 3 or more; one that hears a neighbour's offender, a dummy slot or
a pad lane leaves a control open.  The decision has a factor 4 of margin on one side and exact zeros on the other: no rounding
difference between the two implementations can flip it.  Every test asserts which kernel form ran."""
import functools
import os

import numpy as np
import pytest

import scenarios as sc
import termination_ref as tr
from cpu_solvers import OracleSolver
from hip_runner import IN_FIELDS, make_batch
from test_gpu_parity import RTOL

pytestmark = pytest.mark.gpu

ONE_ROW = {"no_tile": 1, "repack_after": 0}
# (id, dims, options, what must have run: kernel_path() values, then option read-backs)
FORMS = [
    ("one_row_12_4_10_lazy", (12, 4, 10), dict(ONE_ROW), dict(path=("regs",), last_half_rows=0, last_prefetch=0)),
    ("one_row_4_2_10_full_rows", (4, 2, 10), dict(ONE_ROW, half_rows=0), dict(path=("regs",), last_half_rows=0)),
    ("one_row_4_2_10_half_rows", (4, 2, 10), dict(ONE_ROW, half_rows=1), dict(path=("regs",), last_half_rows=1)),
    ("one_row_4_2_30_sweep", (4, 2, 30), dict(ONE_ROW, half_rows=0), dict(path=("regs",), last_half_rows=0)),
    ("one_row_4_2_30_sweep_half_rows", (4, 2, 30), dict(ONE_ROW, half_rows=1), dict(path=("regs",), last_half_rows=1)),
    ("one_row_12_4_10_prefetch_one_wave", (12, 4, 10), dict(ONE_ROW, prefetch=1, prefetch_waves=1), dict(path=("regs",), last_prefetch=1, last_prefetch_grid=1)),
    ("one_row_12_4_10_split_at_2", (12, 4, 10), dict(ONE_ROW, repack_after=2), dict(path=("regs",))),
    ("one_row_4_2_30_split_at_2", (4, 2, 30), dict(ONE_ROW, repack_after=2), dict(path=("regs",))),
    ("one_row_4_2_30_one_wave_per_cu", (4, 2, 30), dict(ONE_ROW, grid_waves_per_cu=1), dict(path=("regs",))),
] + [
    ("tile_%d_%d_%d_w%d_dyn%d" % (dims + (w, dyn)), dims, dict(prefer_tile=1, tile_w=w, tile_dyn=dyn),
     dict(path=("tile",), tile_w=w, tile_r=1, last_tile_dyn=dyn))
    for dims in ((4, 2, 10), (4, 2, 30)) for w in (0, 1) for dyn in (0, 1)
] + [
    ("tile_20_4_10_two_rows_wide", (20, 4, 10), {}, dict(path=("tile",), last_tile_form=2001000)),
    ("tile_4_2_50_v_in_its_record", (4, 2, 50), {}, dict(path=("tile",), last_tile_form=1023)),
    ("tile_4_2_50_two_rows_long", (4, 2, 50), dict(tile_r=2), dict(path=("tile",), tile_w=1, tile_r=2)),
    ("tile_12_8_30_wide_v_in_its_record", (12, 8, 30), {}, dict(path=("tile",), last_tile_form=2001020)),
    ("tile_12_8_30_wide_two_rows_long", (12, 8, 30), dict(tile_r=2), dict(path=("tile",), tile_w=2, tile_r=2)),
    ("tile_12_4_50_dyn0", (12, 4, 50), dict(tile_dyn=0), dict(path=("tile",), tile_w=1, tile_r=2, last_tile_dyn=0)),
    ("tile_12_4_50_dyn1", (12, 4, 50), dict(tile_dyn=1), dict(path=("tile",), tile_w=1, tile_r=2, last_tile_dyn=1)),
    ("cover_4_2_10_forced", (4, 2, 10), dict(force_general=1), dict(path=("cover",))),
    ("cover_5_3_7_no_compiled_form", (5, 3, 7), dict(no_jit=1), dict(path=("cover",))),
]
FORM_IDS = [f[0] for f in FORMS]
CHECK_FORMS = [f for f in FORMS if f[1] in ((4, 2, 10), (4, 2, 30))]


def tile_dims_has(dims, w):
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tinympc_amd", "csrc", "tile_dims.txt")
    rows = [ln.split("#")[0].split() for ln in open(path)]
    return any(len(r) >= 5 and tuple(map(int, r[:4])) == dims + (w,) for r in rows)


def launch(suite, options, expect, what):
    """one launch of the whole suite; -> the status arrays, the residuals as they were before the solve, and what the dispatcher reports.
    Skips when tile_dims.txt has no entry of the (shape, W) asked for; every other difference between the form asked for and the
    form that ran is a failure."""
    if "tile_w" in options and not tile_dims_has(tuple(suite["problem"][k] for k in ("nx", "nu", "N")), options["tile_w"]):
        pytest.skip("tile_dims.txt has no W = %d entry of this shape: the form does not exist" % options["tile_w"])
    cases = suite["cases"]
    s = make_batch(suite)
    for k, v in options.items():
        s.set_option(k, v)
    s.set_x0(cases["x0"])
    for f in IN_FIELDS:
        s.set(f, cases[f])
    before = s.status()
    s.solve()
    st = s.status()
    ran = dict(path=s.kernel_path())
    for k in ("last_tile_form", "last_half_rows", "last_prefetch", "last_prefetch_grid", "last_tile_dyn"):
        ran[k] = s.get_option(k)
    s.close()
    if ran["path"] == "tile":
        ran["tile_w"], ran["tile_r"] = ran["last_tile_form"] // 1000000, ran["last_tile_form"] // 1000 % 1000
    for k, v in expect.items():
        assert (ran[k] in v) if k == "path" else (ran.get(k) == v), (what, "asked for", options, "expected", expect, "ran", ran)
    out = {k: np.asarray(st[k], dtype=float) for k in tr.RESIDUALS}
    out.update(iter=st["iter"].astype(int), sol_solved=st["solved"].astype(int), status=st["status"].astype(int))
    return out, before, ran


@functools.lru_cache(maxsize=None)
def oracle(dims, max_iter, check=1):
    suite, table = tr.position_suite(*dims, max_iter=max_iter, check_termination=check)
    ref = sc.run_cases(OracleSolver, suite, fields=("vnew", "znew"))
    floor = tr.noise_floor(suite["problem"], dict(vnew=np.maximum(np.abs(ref["vnew"]), np.abs(suite["cases"]["v"])),
                                                  znew=np.maximum(np.abs(ref["znew"]), np.abs(suite["cases"]["z"]))), RTOL)
    return suite, table, ref, floor


def assert_decisions(out, ref, table, what):
    for k in ("iter", "sol_solved", "status"):
        bad = np.flatnonzero(out[k] != ref[k].astype(int))
        assert bad.size == 0, "%s: %s differs on %d of %d instances; first: %s: got %d, oracle %d" % (
            what, k, bad.size, len(table), tr.describe(table, bad[0]), out[k][bad[0]], ref[k][bad[0]])


def assert_residuals(out, ref, table, floor, what):
    """a residual is a maximum of differences of fields that agree with the oracle's to RTOL of their largest entry: it matches at RTOL of
    its own size, or -- where it is (nearly) zero -- to the noise floor RTOL rho max|vnew| of those fields"""
    for k in tr.RESIDUALS:
        err = np.abs(out[k] - ref[k])
        bad = np.flatnonzero(~(err <= np.maximum(RTOL * np.abs(ref[k]), floor)))
        assert bad.size == 0, "%s: %s differs on %d of %d instances; first: %s: got %.17g, oracle %.17g" % (
            what, k, bad.size, len(table), tr.describe(table, bad[0]), out[k][bad[0]], ref[k][bad[0]])


# ---- 1. every position as the sole offender, solved to the end
@pytest.mark.parametrize("name,dims,options,expect", FORMS, ids=FORM_IDS)
def test_every_position_alone_keeps_its_solve_open(name, dims, options, expect):
    """max_iter = 40, check_termination = 1: iter, solved, status of every instance are the oracle's (controls 1, offenders 3 or more), the
    four residuals of the stopping test match.  A missed position shows as iter = 1 at that (j, k); an offender heard in a neighbour's
    row, a dummy slot or a pad lane in the maximum as a control that runs on."""
    suite, table, ref, floor = oracle(dims, 40)
    out, _, ran = launch(suite, options, expect, name)
    what = "%s %s %s" % (name, dims, ran)
    assert_decisions(out, ref, table, what)
    assert_residuals(out, ref, table, floor, what)
    off = table[:, 0] != tr.CTL
    print("termination edges: %s B %d offender iterations %s" % (what, len(table), dict(zip(*[a.tolist() for a in np.unique(out["iter"][off], return_counts=True)]))))


# ---- 2. the launch ends on its first test | one test before its last
@pytest.mark.parametrize("name,dims,options,expect", FORMS, ids=FORM_IDS)
def test_residuals_of_the_first_test_when_it_is_the_last_and_when_it_is_not(name, dims, options, expect):
    """max_iter = 1: the only test is the launch's last one (a full test whatever the probe says); max_iter = 2: the test of iteration 1 is
    not.  At max_iter = 1 an offender of kind c at a state row reports the state residual of kind c of the oracle at RTOL and the three
    others at most RTOL rho max|vnew| (the kernel's vnew agrees with the oracle's v only to RTOL), input rows likewise: the state |
    input split at rows nx - 1 | nx and nx + nu - 1 | pad.  At max_iter = 2 the residuals are those of iteration 2, the oracle's."""
    nx = dims[0]
    for max_iter in (1, 2):
        suite, table, ref, floor = oracle(dims, max_iter)
        out, _, ran = launch(suite, options, expect, name)
        what = "%s %s max_iter=%d %s" % (name, dims, max_iter, ran)
        assert_decisions(out, ref, table, what)
        if max_iter == 2:
            assert_residuals(out, ref, table, floor, what)
            continue
        got = np.stack([out[k] for k in tr.RESIDUALS], axis=1)
        want = np.stack([ref[k] for k in tr.RESIDUALS], axis=1)
        for b in range(len(table)):
            c = tr.residual_index(table[b, 0], table[b, 1], nx) if table[b, 0] != tr.CTL else -1
            for i, k in enumerate(tr.RESIDUALS):
                if i == c:
                    assert abs(got[b, i] - want[b, i]) <= RTOL * want[b, i], "%s: %s of %s: got %.17g, oracle %.17g" % (what, k, tr.describe(table, b), got[b, i], want[b, i])
                else:
                    assert want[b, i] == 0.0 and abs(got[b, i]) <= floor, "%s: %s of %s: got %.3g where the oracle has 0 (bound %.3g)" % (what, k, tr.describe(table, b), got[b, i], floor)


# ---- 3. the check phase
@pytest.mark.parametrize("name,dims,options,expect", CHECK_FORMS, ids=[f[0] for f in CHECK_FORMS])
def test_checks_every_second_and_third_iteration(name, dims, options, expect):
    """check_termination 2 | 3 with max_iter 1, 2, 3, 4, 7: tests at iterations 2, 4, 6 | 3, 6 only, the last one of a launch not always at its
    last iteration: iter, solved, status and the four residuals are the oracle's -- the residuals of the last test that ran, and what they
    were before the solve (a fresh handle: 0) where none ran."""
    for check in (2, 3):
        for max_iter in (1, 2, 3, 4, 7):
            suite, table, ref, floor = oracle(dims, max_iter, check)
            tol = np.array([suite["config"]["abs_pri_tol"], suite["config"]["abs_dua_tol"]] * 2)
            reported = np.stack([ref[k] for k in tr.RESIDUALS], axis=1)
            # (precondition: no reported residual of the oracle within 1e-6 of its tolerance -- no decision a rounding could flip)
            assert np.all(np.abs(reported / tol - 1.0) > 1e-6)
            out, before, ran = launch(suite, options, expect, name)
            what = "%s %s check_termination=%d max_iter=%d %s" % (name, dims, check, max_iter, ran)
            assert_decisions(out, ref, table, what)
            if max_iter < check:
                assert np.all(ref["iter"] == max_iter) and not ref["sol_solved"].any()
                for k in tr.RESIDUALS:
                    assert np.array_equal(out[k], before[k]), (what, k, "no test ran: the residuals must be untouched")
            else:
                assert_residuals(out, ref, table, floor, what)


# ---- 4. strictness
@pytest.mark.parametrize("name,dims,options,expect", FORMS, ids=FORM_IDS)
def test_a_residual_equal_to_its_tolerance_keeps_the_solve_open(name, dims, options, expect):
    """x0 = 0, references 0: x = u = 0 on any implementation, so a warm v | z entry of DELTA is a dual residual of exactly fl(DELTA rho) (every
    position, the probe's slots included) and g[j,0] = DELTA a primal residual of exactly DELTA.  Tolerance EQUAL to the residual: iter = 2
    (strict <, in the probe and in the full test alike); the next double above it: iter = 1.  The residuals are exact, so they are
    compared with ==.  (Primal equality on input rows and at k > 0 cannot be made exact without reading the code under test.)"""
    for kind in (tr.PRI, tr.DUA):
        for above in (False, True):
            suite, table = tr.strict_suite(*dims, kind, above)
            ref = sc.run_cases(OracleSolver, suite, fields=())
            off = table[:, 0] != tr.CTL
            assert np.all(ref["iter"][off] == (1 if above else 2)) and np.all(ref["iter"][~off] == 1) and np.all(ref["sol_solved"] == 1)
            out, _, ran = launch(suite, options, expect, name)
            what = "%s %s strict %s, tolerance %s the residual %s" % (name, dims, tr.KIND[kind], "just above" if above else "equal to", ran)
            assert_decisions(out, ref, table, what)
            for k in tr.RESIDUALS:
                bad = np.flatnonzero(out[k] != ref[k])
                assert bad.size == 0, "%s: %s: first %s: got %.17g, oracle %.17g" % (what, k, tr.describe(table, bad[0]), out[k][bad[0]], ref[k][bad[0]])
