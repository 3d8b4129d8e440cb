"""Every kernel at the edges of the shapes it claims to hold (tests/shape_edges.py: the table, the reasons and the two suites per
shape).  The kernel each shape must run on is not written down anywhere: tests/test_shape_edges_cpu.py derives it from the project's
own host code (jit_shape_fits, jit_tile_shape, tiny_batch_setup's choice, decide_path) and kernel_path() must name it BEFORE and AFTER
the solve -- a formula that admits a shape its kernel cannot hold makes the dispatcher fall back to a slower kernel without a word, and
then kernel_path() changes.  Results against the oracle at the project's bar, rel_err < 1e-9, iteration counts and flags exactly."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import scenarios as sc  # noqa: E402
import shape_edges as se  # noqa: E402
import test_shape_edges_cpu as rules  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402
from hip_runner import IN_FIELDS, LIN_IN, LIN_OUT, OUT_FIELDS, SOC_OUT, TV_IN, TV_OUT, make_batch  # noqa: E402

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                       # the project's bar (tests/test_gpu_jit.py)
RESIDUALS = ("primal_residual_state", "primal_residual_input", "dual_residual_state", "dual_residual_input")
FLAGS = ("iter", "sol_solved", "status")
ID = se.shape_id


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def run(suite, options=None):
    """one launch over all cases (as hip_runner.run_cases_hip), with kernel_path() read before and after the solve on the same handle"""
    cases, cfg = suite["cases"], suite["config"]
    s = make_batch(suite)
    for k, v in (options or {}).items():
        s.set_option(k, v)
    before = s.kernel_path()
    s.set_x0(cases["x0"])
    lin = cfg.get("en_state_linear", 0) or cfg.get("en_input_linear", 0)
    tvl = cfg.get("en_tv_state_linear", 0) or cfg.get("en_tv_input_linear", 0)
    soc = cfg["en_state_soc"] or cfg["en_input_soc"]
    for f in IN_FIELDS + (LIN_IN if lin else ()) + (TV_IN if tvl else ()):
        if f in cases:
            s.set(f, cases[f])
    s.solve()
    fields = OUT_FIELDS + (SOC_OUT if soc else ()) + (LIN_OUT if lin else ()) + (TV_OUT if tvl else ())
    out = {f: s.get(f) for f in fields}
    st = s.status()
    out.update(iter=st["iter"].astype(float), sol_solved=st["solved"].astype(float), status=st["status"].astype(float))
    for k in RESIDUALS:
        out[k] = st[k]
    out.update(path_before=before, path_after=s.kernel_path(), half_rows=s.get_option("last_half_rows"), fields=fields)
    s.close()
    return out


def check(out, ref, want, what):
    assert (out["path_before"], out["path_after"]) == (want, want), (what, want, out["path_before"], out["path_after"])
    for k in FLAGS:
        assert np.array_equal(out[k].astype(int), ref[k].astype(int)), (what, k, out[k], ref[k])
    for k in RESIDUALS + out["fields"]:
        assert np.all(np.isfinite(ref[k])), (what, k)
        err = rel_err(out[k], ref[k])
        assert err < RTOL, (what, k, err)


def solve_both(suite, ref, again, ref2, want, what, options=None):
    """the suite's solve and the second solve from the state the first one left, with x0 * 0.8; where the one-row kernel packed two
    instances into a DPP row, the one-per-row form as well, bit for bit"""
    for name, su, r in (("first", suite, ref), ("second", again, ref2)):
        out = run(su, options)
        check(out, r, want, (what, name))
        if out["half_rows"] == 1:
            full = run(su, dict(options or {}, half_rows=0))
            assert full["half_rows"] == 0 and full["path_after"] == want, (what, name)
            for k in FLAGS + RESIDUALS + out["fields"]:
                assert np.array_equal(out[k], full[k]), (what, name, k)


@pytest.fixture(scope="module")
def box_paths():
    return rules.expected_paths(se.SHAPES)


# ---- a. the plain box solve on the kernel the rules name
@pytest.mark.parametrize("kind", ["cold", "warm"])
@pytest.mark.parametrize("shape", se.SHAPES, ids=ID)
def test_box_solve_runs_the_kernel_the_rules_name_and_matches_the_oracle(shape, kind, box_paths):
    solve_both(*se.solved(shape, kind), box_paths[shape]["path"], (shape, kind))


# ---- b. the coverage kernel claims every one of these shapes (the entries it serves anyway are in a.)
FORCED = [s for s in se.SHAPES if se.one_row_fits(*s) or se.tile_shape(*s)]


@pytest.mark.parametrize("kind", ["cold", "warm"])
@pytest.mark.parametrize("shape", FORCED, ids=ID)
def test_box_solve_on_the_coverage_kernel(shape, kind, box_paths):
    assert box_paths[shape]["path"] != "cover"
    assert rules.expected_paths([shape], force_general=1)[shape]["path"] == "cover"
    solve_both(*se.solved(shape, kind), "cover", (shape, kind, "force_general"), options={"force_general": 1})


# ---- c. across each boundary
@pytest.mark.parametrize("last,first,rule", se.PAIRS, ids=lambda v: ID(v) if isinstance(v, tuple) else v)
def test_the_kernel_changes_across_each_boundary_and_both_sides_match(last, first, rule):
    cone = rule == "soc"
    want = rules.expected_paths([last, first], soc=cone)
    assert want[last]["path"] != want[first]["path"]
    got = []
    for shape in (last, first):
        suite, ref, _, _ = se.solved(shape, "warm", cone)
        out = run(suite)
        check(out, ref, want[shape]["path"], (shape, rule))
        got.append(out["path_after"])
    assert got[0] != got[1]


# ---- d. variants at the last rows
# the budget helpers of the dispatcher (csrc/admm_kernel.hip.h solve_kernel_lin_lds, csrc/tile_kernel.hip.h tile_variant_lds_bytes,
# both against 64 KiB - 512 of static LDS), restated for a knot-varying box and up to four half-spaces per knot and family (KMAX = 4)
LDS_STATIC_LIMIT = 64 * 1024 - 512


def one_row_planes_fit(nx, nu, N, soc, lin, kmax=4, pl=False):
    csl, tabs = (nx + nu + 1) | 1, (4 if pl else 1)
    lds = 8 * (nx * 16 + 2 * N * 16 + ((tabs * 3 * kmax * 16 + 2 * 4 * N * csl) if lin & 1 else 0) +
               ((tabs * 3 * N * kmax * 16 + 2 * 4 * N * csl) if lin & 2 else 0) + ((4 * N + 1) * 3 * csl if soc else 0))
    return lin != 0 and lds <= LDS_STATIC_LIMIT


def tile_variant_fits(nx, nu, N, W, R, lin, kmax=4):
    lw, ipw, csl = 16 * W, 4 // (W * R), (nx + nu + 1) | 1
    d = 2 * N * lw + (N // R) * 64
    if lin & 1:
        d += 3 * kmax * lw + 2 * ipw * N * csl
    if lin & 2:
        d += 3 * N * kmax * lw + 2 * ipw * N * csl
    return 8 * d <= LDS_STATIC_LIMIT


def halfspace_path(shape, lin):
    """the driver's answer for shared half-spaces of the families `lin` (bit 0 static, bit 1 time-varying), fed the facts path_facts
    would read off the handle"""
    nx, nu, N = shape
    tile = rules.expected_paths([shape])[shape]
    facts = dict(lin_families=lin, lin_kmax=4, planes_fit=int(one_row_planes_fit(nx, nu, N, False, lin)),
                 pl_planes_fit=int(one_row_planes_fit(nx, nu, N, False, lin, pl=True)),
                 tile_lin=int(bool(tile["tile_is_jit"]) and tile_variant_fits(nx, nu, N, tile["W"], tile["R"], lin)))
    return rules.expected_paths([shape], **facts)[shape]


def halfspace_config(shape, lin, rng):
    """two static and one time-varying half-space per family"""
    nx, nu, N = shape
    kw = {}
    if lin & 1:
        kw.update(en_state_linear=1, en_input_linear=1,
                  linear=(rng.standard_normal((2, nx)), rng.uniform(0.2, 1.0, 2), rng.standard_normal((2, nu)), rng.uniform(0.2, 0.6, 2)))
    if lin & 2:
        kw.update(en_tv_state_linear=1, en_tv_input_linear=1,
                  tv_linear=(rng.standard_normal((N, nx)), rng.uniform(0.3, 1.0, (1, N)), rng.standard_normal((N - 1, nu)), rng.uniform(0.2, 0.6, (1, N - 1))))
    return kw


def variant_case(name):
    """(suite, the driver's answer)"""
    if name == "13_3_4_cones_on_the_last_rows":       # state rows 10..12, inputs 0..2 = lanes 13..15
        shape = (13, 3, 4)
        kw = dict(en_state_soc=1, en_input_soc=1, state_cone=([10], [3], [0.7]), input_cone=se.INPUT_CONE)
        return se.warm_suite(shape, **kw), rules.expected_paths([shape], soc=True)[shape]
    if name.endswith("input_cone"):
        shape = tuple(map(int, name.split("_")[:3]))
        return se.solved(shape, "warm", True)[0], rules.expected_paths([shape], soc=True)[shape]
    shape, lin = tuple(map(int, name.split("_")[:3])), int(name.split("_lin")[1])
    rng = np.random.default_rng(4000 + 100 * shape[0] + 10 * shape[1] + shape[2] + lin)
    return se.warm_suite(shape, **halfspace_config(shape, lin, rng)), halfspace_path(shape, lin)


VARIANTS = {
    "13_3_4_cones_on_the_last_rows": "jit", "6_3_26_input_cone": "jit", "6_3_27_input_cone": "cover",
    "15_1_4_lin3": "jit", "1_15_4_lin3": "jit", "16_16_2_lin3": "tile-jit", "24_8_36_lin1": "tile-jit", "24_8_36_lin3": "cover",
}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_cone_and_halfspace_variants_at_the_last_rows(name):
    """VARIANTS names the kernel the issue of this test expects; it holds only where the host driver, fed the facts of the launch,
    gives the same answer -- (24,8,36) with both half-space sets is the coverage kernel's because the per-knot tables of a 32-lane
    tile do not fit the wave's LDS (tile_variant_lds_bytes), and the driver says so"""
    suite, want = variant_case(name)
    assert want["path"] == VARIANTS[name], (name, want)
    ref = sc.run_cases(OracleSolver, suite)
    again = se.second_suite(suite, ref)
    solve_both(suite, ref, again, sc.run_cases(OracleSolver, again), want["path"], name)


# ---- e. closed loop at N = 2 and at the width edges
T = 5


def closed_loop(suite, fused, window):
    """T MPC steps with the plant step on the device, in one launch or in T: every field, x0, the per-step iteration counts (negative:
    not converged) and kernel_path() before / after"""
    c = suite["cases"]
    s = make_batch(suite)
    s.set_x0(c["x0"]); s.set("Xref", c["Xref"]); s.set("Uref", c["Uref"])
    if window is not None:
        s.set_reference_trajectory(*window)
        s.set_option("reset_duals", 1)
    s.set_option("advance_x0", 1)
    s.set_option("step_log", 1)
    s.set_option("steps_per_launch", T if fused else 1)
    before, its = s.kernel_path(), []
    for _ in range(1 if fused else T):
        s.solve_async()
        if fused:
            its.append(s.step_log(T)[0])
        else:
            st = s.status()
            its.append((st["iter"] * np.where(st["solved"] == 1, 1, -1))[None, :])
    out = {k: s.get(k) for k in OUT_FIELDS + ("x0",)}
    out.update(its=np.concatenate(its), path=(before, s.kernel_path()))
    s.close()
    return out


def oracle_loop(suite, window):
    """the oracle's loop, instance by instance: solve, x0 = X[1] -- at N = 2 the terminal knot"""
    prob, cfg, c = suite["problem"], suite["config"], suite["cases"]
    nx, nu, N = prob["nx"], prob["nu"], prob["N"]
    B = c["x0"].shape[0]
    its, x0s = np.zeros((T, B), dtype=int), np.zeros((B, nx))
    for b in range(B):
        o = sc.make_solver(OracleSolver, prob, cfg)
        o["Xref"], o["Uref"] = c["Xref"][b], c["Uref"][b]
        xb = c["x0"][b].copy()
        for k in range(T):
            if window is not None:
                traj, offs = window
                o["Xref"] = traj[np.minimum(np.arange(N) + k + offs[b], len(traj) - 1)].T
                o["g"] = np.zeros((nx, N)); o["y"] = np.zeros((nu, N - 1))
            o["x"][:, 0] = xb
            o.solve()
            it = int(o.get("sol_iter"))
            its[k, b] = it if int(o.get("sol_solved")) else -it
            xb = np.array(o["x"])[:, 1].copy()
        x0s[b] = xb
        o.close()
    return its, x0s


@pytest.mark.parametrize("window", [False, True], ids=["fixed_reference", "moving_window_reset_duals"])
@pytest.mark.parametrize("shape", se.CLOSED_LOOP_SHAPES, ids=ID)
def test_closed_loop_fused_steps_equal_single_steps_and_the_oracle(shape, window):
    nx, nu, N = shape
    suite = se.cold_suite(shape)
    rng = np.random.default_rng(99 + nx)
    win = (rng.normal(0, 0.3, (N + T + 3, nx)), rng.integers(0, 3, se.B).astype(np.int32)) if window else None
    # a reference window and reset_duals are the tile kernel's EXT form where the one-row kernel does not hold the shape
    want = rules.expected_paths([shape], tile_ext=int(window))[shape]["path"]
    assert want in ("jit", "tile-jit")
    single, fused = closed_loop(suite, False, win), closed_loop(suite, True, win)
    assert single["path"] == (want, want) and fused["path"] == (want, want), (want, single["path"], fused["path"])
    for k in OUT_FIELDS + ("x0", "its"):
        assert np.array_equal(single[k], fused[k]), (shape, k)
    its, x0 = oracle_loop(suite, win)
    assert np.all(np.isfinite(x0)) and np.max(np.abs(its)) > 1
    assert np.array_equal(fused["its"], its), (shape, fused["its"], its)
    assert rel_err(fused["x0"], x0) < RTOL, (shape, rel_err(fused["x0"], x0))
