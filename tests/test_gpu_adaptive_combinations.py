"""GPU: adaptive rho TOGETHER with everything a launch reads next to it.  (a) every combination it is refused with, end to end: the text,
the handle's records and per-instance cache untouched by the refused call, the next solve as a fresh handle's; (b) every launch form
and option it is served with leaves, bit for bit, the state seven default single-step launches leave; (c) the constraint kinds it is
served with are in effect, against the oracle.  The margins of the preconditions (all checked here on the oracle, before the device is
asked): profiles/adaptive_combinations.md.

Shapes: the quadrotor (12, 4, 10) -- the compiled-in adaptive instantiation; (5, 3, 7) -- the one made at run time; per-instance data at
(6, 3, 10) -- the per-instance adaptive form, tables from compute_sensitivity.  B = 9: two full tiles of four rows and a partial one.
max_iter = 60 with check_termination = 1: rho is re-estimated every fifth iteration, the solves here take 8 to 60."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import scenarios as sc  # noqa: E402
import tinympc_amd as tm  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402
from hip_runner import make_batch, run_cases_hip  # noqa: E402

pytestmark = pytest.mark.gpu
B, T = 9, 7
FIELDS = ("x", "u", "vnew", "znew", "g", "y", "v", "z")
CACHE = ("rho", "Kinf", "Pinf", "C1", "C2")
ONE_ROW = ("regs", "jit")


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


# ---- the three suites (numpy only)
@functools.lru_cache(maxsize=None)
def quad_suite():
    return sc.tracking_adaptive_suite(B=B, seed=777, rho_min=0.5, rho_max=40.0, clip=1, max_iter=60)


RAND_DIMS = (5, 3, 7)


@functools.lru_cache(maxsize=None)
def rand_suite():
    """(5, 3, 7): sc.random_problem's system, a knot-invariant box that binds, random sensitivity tables of the size tools/fuzz_parity.py
    adaptive_trial draws"""
    nx, nu, N = RAND_DIMS
    prob, _ = sc.random_problem(nx, nu, N)
    prob = dict(prob, rho=5.0)
    rng = np.random.default_rng(5370)
    sens = {"dKinf_drho": rng.normal(0, 2e-3, (nu, nx)), "dPinf_drho": rng.normal(0, 5e-2, (nx, nx)),
            "dC1_drho": rng.normal(0, 1e-3, (nu, nu)), "dC2_drho": rng.normal(0, 1e-3, (nx, nx))}
    cfg = sc.default_config(prob, max_iter=60, x_min=np.full((nx, 1), -0.65), x_max=np.full((nx, 1), 0.65), u_min=np.full((nu, 1), -0.3), u_max=np.full((nu, 1), 0.3))
    cfg = sc.adaptive_cfg(cfg, rho_min=0.02, rho_max=20.0, clip=1, sensitivity=sens)
    cases = sc.zero_cases(prob, B)
    cases["x0"] = 0.7 * rng.uniform(-1, 1, (B, nx))          # (some start outside the +-0.65 box: those never converge)
    cases["Xref"] = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    cases["Uref"] = rng.normal(0, 0.05, (B, nu, N - 1))
    return dict(problem=prob, config=cfg, cases=cases)


def load(s, suite):
    c = suite["cases"]
    s.set_x0(c["x0"]); s.set("Xref", c["Xref"]); s.set("Uref", c["Uref"])
    return s


def settings(s, cfg, **over):
    c = dict(cfg, **over)
    s.update_settings(c["abs_pri_tol"], c["abs_dua_tol"], c["max_iter"], c["check_termination"], c["en_state_bound"], c["en_input_bound"],
                      c["en_state_soc"], c["en_input_soc"], c.get("en_state_linear", 0), c.get("en_input_linear", 0),
                      c.get("en_tv_state_linear", 0), c.get("en_tv_input_linear", 0))


def snapshot(s):
    out = {k: s.get(k) for k in FIELDS}
    out.update({k: s.get_cache_state(k) for k in CACHE})
    return out


def same(a, b, what, skip=()):
    for k in a:
        if k not in skip:
            assert np.array_equal(a[k], b[k]), (what, k)


@functools.lru_cache(maxsize=None)
def oracle_of(name):
    """one cold solve of every case of a suite on the oracle (computed once; nobody writes into it)"""
    return sc.run_cases(OracleSolver, {"quad": quad_suite, "rand": rand_suite}[name]())


def assert_rho_moved(ref, suite, least=2):
    """the precondition of every test here: the oracle's solves re-estimate rho, and the instances do not all end at one value"""
    assert np.all(ref["iter"] >= 5)
    assert np.any(ref["rho"] != suite["problem"]["rho"])
    assert len(np.unique(ref["rho"])) >= least, ref["rho"]


# =====================================================================================================================================
# a. every refusal, end to end
# =====================================================================================================================================
NX, NU, N = 12, 4, 10
TEXT_BOX = "per-instance bounds (tiny_batch_set_instance_bounds)"
TEXT_LIN = "does not combine with heterogeneous data / half-spaces / one_shot / repack_after"
TEXT_CONES = "overlapping cones run on the coverage kernel"


def halfspace_rows(n, width, seed, first_axis, first_offset):
    """n unit normals: row 0 is `z[first_axis] <= first_offset` (the one the tests count on), the others random and far out"""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(n, width))
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    b = rng.uniform(3.0, 6.0, n)
    A[0] = 0.0
    A[0, first_axis] = 1.0
    b[0] = first_offset
    return A, b


def static_set(n_state, n_input, seed=1):
    """state row 0: y <= 1 (the quadrotor suite's references run along the y axis, up to y = 4); input row 0: u_0 <= 0.1"""
    Ax, bx = halfspace_rows(n_state, NX, seed, 1, 1.0)
    Au, bu = halfspace_rows(n_input, NU, seed + 1, 0, 0.1)
    return Ax, bx, Au, bu


def tv_set(n_state, n_input, seed=11):
    Ax, bx, Au, bu = static_set(n_state, n_input, seed)
    return (np.tile(Ax, (N, 1)), np.repeat(bx[:, None], N, axis=1) + 0.01 * np.arange(N)[None, :], np.tile(Au, (N - 1, 1)),
            np.repeat(bu[:, None], N - 1, axis=1) + 0.01 * np.arange(N - 1)[None, :])


def violation(Ax, bx, x):
    """largest a' x_k - b over rows, instances and knots; x [B, nx, N]"""
    return float(np.max(np.einsum("rn,bnk->brk", Ax, x) - np.asarray(bx).reshape(1, -1, 1)))


class Offender:
    """something adaptive rho is refused with: how it is installed on a handle, how it is taken away again, the text"""
    def __init__(self, text, install, remove, dropped=None, misrouted=False):
        self.text, self.install, self.remove, self.dropped, self.misrouted = text, install, remove, dropped, misrouted


def shared_halfspaces(static=None, tv=None, flags=None, options=(), misrouted=False):
    def install(s, cfg):
        if static:
            s.set_linear_constraints(*static)
        if tv:
            s.set_tv_linear_constraints(*tv)
        for k in options:
            s.set_option(k, 1)
        settings(s, cfg, **flags)

    def remove(s, cfg):
        settings(s, cfg)
        for k in options:
            s.set_option(k, 0)
    return Offender(TEXT_LIN, install, remove, dropped=static if static and flags.get("en_state_linear") else None, misrouted=misrouted)


def option(name, value, default):
    return Offender(TEXT_LIN, lambda s, cfg: s.set_option(name, value), lambda s, cfg: s.set_option(name, default))


def instance_box():
    def install(s, cfg):
        w = 1.0 + 0.05 * np.arange(B).reshape(B, 1, 1)
        s.set_instance_bounds(cfg["x_min"][None] * w, cfg["x_max"][None] * w, cfg["u_min"][None] * w, cfg["u_max"][None] * w)
    return Offender(TEXT_BOX, install, lambda s, cfg: s.set_bound_constraints(cfg["x_min"], cfg["x_max"], cfg["u_min"], cfg["u_max"]))


def instance_halfspaces():
    Ax, bx, Au, bu = static_set(1, 1, seed=21)

    def install(s, cfg):
        w = 1.0 + 0.05 * np.arange(B)
        s.set_instance_linear_constraints(np.tile(Ax[None], (B, 1, 1)), bx[None] * w[:, None], np.tile(Au[None], (B, 1, 1)), bu[None] * w[:, None])
        settings(s, cfg, en_state_linear=1, en_input_linear=1)

    def remove(s, cfg):
        s.set_linear_constraints(Ax, bx, Au, bu)          # (one set for all frees the per-instance one; it stays switched off)
        settings(s, cfg)
    return Offender(TEXT_LIN, install, remove)


def overlapping_cones():
    def install(s, cfg):
        s.set_cone_constraints([0, 2], [3, 3], [0.5, 0.5], [], [], [])
        settings(s, cfg, en_state_soc=1)
    return Offender(TEXT_CONES, install, lambda s, cfg: settings(s, cfg))


STATE_ON, INPUT_ON = dict(en_state_linear=1), dict(en_input_linear=1)
TV_ON = dict(en_tv_state_linear=1, en_tv_input_linear=1)
OFFENDERS = {
    "static_state_1": shared_halfspaces(static=static_set(1, 1), flags=STATE_ON),
    "static_input_1": shared_halfspaces(static=static_set(1, 1), flags=INPUT_ON),
    "static_5": shared_halfspaces(static=static_set(5, 5), flags=dict(STATE_ON, **INPUT_ON)),
    "tv_1": shared_halfspaces(tv=tv_set(1, 1), flags=TV_ON),
    "tv_5": shared_halfspaces(tv=tv_set(5, 5), flags=TV_ON),
    "static_and_tv": shared_halfspaces(static=static_set(1, 1), tv=tv_set(1, 1), flags=dict(STATE_ON, **INPUT_ON, **TV_ON)),
    # the three that ran WITHOUT their half-spaces before decide_path refused them
    "static_33": shared_halfspaces(static=static_set(33, 1), flags=STATE_ON, misrouted=True),
    "static_1_force_general": shared_halfspaces(static=static_set(1, 1), flags=STATE_ON, options=("force_general",), misrouted=True),
    "static_5_no_jit": shared_halfspaces(static=static_set(5, 1), flags=STATE_ON, options=("no_jit",), misrouted=True),
    "one_shot": option("one_shot", 1, 0),
    "repack_after_8": option("repack_after", 8, -1),
    "instance_box": instance_box(),
    "instance_halfspaces": instance_halfspaces(),
    "overlapping_cones": overlapping_cones(),
}


@functools.lru_cache(maxsize=None)
def fresh_handle_two_solves():
    """what a handle nobody offended holds after its first and after its second solve of the quadrotor suite"""
    s = load(make_batch(quad_suite()), quad_suite())
    out = []
    for _ in range(2):
        s.solve()
        out.append(dict(snapshot(s), iter=s.status()["iter"].copy()))
    assert s.kernel_path() == "regs"
    s.close()
    return out


@pytest.mark.parametrize("name", list(OFFENDERS))
def test_refused_combination_says_why_and_leaves_the_handle_as_it_was(name):
    """One solve (the cache has moved), then the offender: (i) solve() raises with the table's text, read through tiny_batch_last_error too;
    (ii) the eight record arrays and the five cache members are bit for bit what they were; (iii) with the offender gone the next
    solve leaves what a fresh handle's second solve leaves, rho included.  The kernel path is answered all the same.
    For a state half-space set the oracle's solution WITHOUT it violates row 0 (y <= 1) by more than 1e-3 -- measured: 3.0 -- so a
    solve that returned OK there (static_33, static_1_force_general, static_5_no_jit before the refusal was complete) was a wrong
    answer, not a missing error."""
    off = OFFENDERS[name]
    suite = quad_suite()
    cfg = suite["config"]
    ref = oracle_of("quad")
    assert_rho_moved(ref, suite)
    if off.dropped is not None or off.misrouted:
        v = violation(off.dropped[0], off.dropped[1], ref["x"])
        print(name, "violation of the dropped half-spaces by the oracle's solution without them", v)
        assert v > 1e-3, v
    first, second = fresh_handle_two_solves()
    s = load(make_batch(suite), suite)
    s.solve()
    before = snapshot(s)
    same(before, first, "first solve", skip=("iter",))
    assert np.any(before["rho"] != suite["problem"]["rho"])
    off.install(s, cfg)
    with pytest.raises(tm.TinyMPCError) as err:
        s.solve()
    L = tm.lib()
    assert L.tiny_batch_solve(s._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(s._h).decode()
    assert off.text in msg and off.text in str(err.value) and "adaptive rho" in msg, msg
    assert s.kernel_path() in ("regs", "jit", "cover")
    same(before, snapshot(s), "after the refused call")
    off.remove(s, cfg)
    s.solve()
    after = dict(snapshot(s), iter=s.status()["iter"].copy())
    same(second, after, "the solve after the offender was removed")
    assert s.kernel_path() == "regs"
    s.close()


def test_halfspaces_installed_but_switched_off_are_not_refused():
    """both sets installed, all four en_*_linear at 0: served, and bit for bit the suite without them"""
    suite = quad_suite()
    first, _ = fresh_handle_two_solves()
    s = load(make_batch(suite), suite)
    s.set_linear_constraints(*static_set(5, 5))
    s.set_tv_linear_constraints(*tv_set(33, 1))
    settings(s, suite["config"])
    assert s.get_option("n_state_linear") == 5 and s.get_option("n_tv_state_linear") == 33
    s.solve()
    same(first, dict(snapshot(s), iter=s.status()["iter"].copy()), "switched off")
    assert s.kernel_path() == "regs"
    s.close()


# =====================================================================================================================================
# b. the forms adaptive rho is served with leave the same state
# =====================================================================================================================================
HET_DIMS = (6, 3, 10)


@functools.lru_cache(maxsize=None)
def het_inputs():
    from test_gpu_sensitivity import het_data
    return het_data(*HET_DIMS, B=B)


def make_het():
    from test_gpu_sensitivity import BOX, hetero_batch
    nx, nu, n = HET_DIMS
    fams, x0, Xref, Uref = het_inputs()
    s = hetero_batch(fams, n)
    s.set_bound_constraints(np.full((nx, 1), BOX["x_min"]), np.full((nx, 1), BOX["x_max"]), np.full((nu, 1), BOX["u_min"]), np.full((nu, 1), BOX["u_max"]))
    s.update_settings(max_iter=60)
    s.compute_sensitivity()
    s.set_adaptive_rho(1, 0.7, 6.0, 1)
    s.set_x0(x0); s.set_x_ref(Xref); s.set_u_ref(Uref)
    return s


MAKE = {"quad": lambda: load(make_batch(quad_suite()), quad_suite()), "rand": lambda: load(make_batch(rand_suite()), rand_suite()), "het": make_het}
DIMS = {"quad": (NX, NU, N), "rand": RAND_DIMS, "het": HET_DIMS}


def broadcast_reference(kind):
    def pre(s):
        c = het_inputs() if kind == "het" else None
        Xref, Uref = (c[2][0], c[3][0]) if c else ({"quad": quad_suite, "rand": rand_suite}[kind]()["cases"][k][0] for k in ("Xref", "Uref"))
        s.set_x_ref(Xref, broadcast=True)
        s.set_u_ref(Uref, broadcast=True)
    return pre


def reference_window(kind):
    def pre(s):
        nx, _, n = DIMS[kind]
        rng = np.random.default_rng(97)
        s.set_reference_trajectory(rng.normal(0, 0.2, (n + T + 3, nx)), rng.integers(0, 3, B).astype(np.int32))
    return pre


def closed_loop(kind, opts=(), fused=False, pre=None):
    """T closed-loop MPC steps (advance_x0 = 1) after reset(): T single-step launches, or one launch of T fused steps"""
    s = MAKE[kind]()
    s.reset()
    x0 = het_inputs()[1] if kind == "het" else {"quad": quad_suite, "rand": rand_suite}[kind]()["cases"]["x0"]
    s.set_x0(x0)
    if pre:
        pre(s)
    s.set_option("advance_x0", 1)
    for k, v in opts:
        s.set_option(k, v)
    rho0 = s.get_cache_state("rho")
    steps = []
    if fused:
        s.set_option("steps_per_launch", T)
        s.solve()
    else:
        for _ in range(T):
            s.solve()
            st = s.status()
            steps.append((st["iter"].copy(), st["solved"].copy(), s.get("u")[:, :, 0].copy()))
    out = {k: s.get(k) for k in FIELDS + ("x0",)}
    out.update({k: s.get_cache_state(k) for k in CACHE})
    out["iter"] = s.status()["iter"].copy()
    out["acc"] = s.reduce_stats()[7:9].copy()
    info = dict(path=s.kernel_path(), half=s.get_option("last_half_rows"), prefetch=s.get_option("last_prefetch"),
                stretches=s.get_option("step_regroup_stretches"), steps=steps, rho0=rho0)
    if dict(opts).get("step_log"):
        info["log"] = s.step_log(T)
    if dict(opts).get("debug"):
        info["debug"] = {k: s.get(k) for k in ("q", "r", "p", "d")}
    s.close()
    return out, info


BASELINES = {"default": dict(), "reset_duals": dict(opts=(("reset_duals", 1),)), "broadcast": dict(opts=(("share_ref", 0),), pre=broadcast_reference),
             "window": dict(pre=reference_window)}
_baseline = {}


def baseline(kind, key):
    """seven single-step launches (computed once per shape and kind of reference; nobody writes into it)"""
    if (kind, key) not in _baseline:
        spec = BASELINES[key]
        _baseline[kind, key] = closed_loop(kind, spec.get("opts", ()), False, spec["pre"](kind) if "pre" in spec else None)
    return _baseline[kind, key]


ALL = ("quad", "rand", "het")
# name: (shapes, options, fused, baseline, fields not compared)
VARIANTS = {
    "fused": (ALL, (), True, "default", ()),
    "regroup_2": (ALL, (("step_regroup", 2),), True, "default", ()),
    "regroup_3": (ALL, (("step_regroup", 3),), True, "default", ()),
    "regroup_2_two_streams": (ALL, (("step_regroup", 2), ("step_regroup_streams", 2)), True, "default", ()),
    "step_log": (ALL, (("step_log", 1),), True, "default", ()),
    "regroup_3_step_log": (ALL, (("step_regroup", 3), ("step_log", 1)), True, "default", ()),
    "reset_duals": (ALL, (("reset_duals", 1),), True, "reset_duals", ()),
    "store_primal_0": (ALL, (("store_primal", 0),), True, "default", ("x", "u")),
    "store_primal_2": (ALL, (("store_primal", 2),), True, "default", ("x", "u")),
    "store_primal_0_regroup_2": (ALL, (("store_primal", 0), ("step_regroup", 2)), True, "default", ("x", "u")),
    "share_ref": (ALL, (("share_ref", 1),), False, "broadcast", ()),
    "share_ref_fused": (ALL, (("share_ref", 1),), True, "broadcast", ()),
    "grid_waves_per_cu": (ALL, (("grid_waves_per_cu", 1),), False, "default", ()),
    "grid_waves_per_cu_fused": (ALL, (("grid_waves_per_cu", 1),), True, "default", ()),
    "force_general": (ALL, (("force_general", 1),), False, "default", ()),
    "no_tile": (ALL, (("no_tile", 1),), False, "default", ()),
    "prefer_tile": (ALL, (("prefer_tile", 1),), False, "default", ()),
    "half_rows": (ALL, (("half_rows", 1),), False, "default", ()),
    "prefetch": (ALL, (("prefetch", 1),), False, "default", ()),
    "prefetch_waves": (ALL, (("prefetch", 1), ("prefetch_waves", 3)), False, "default", ()),
    "dpp_mode_0": (ALL, (("dpp_mode", 0),), False, "default", ()),
    "dpp_mode_1": (ALL, (("dpp_mode", 1),), False, "default", ()),
    "uniform_bounds_off": (ALL, (("uniform_bounds", 0),), False, "default", ()),
    "het_ub_off": (("het",), (("het_ub", 0),), False, "default", ()),
    "auto_cold_off": (ALL, (("auto_cold", 0),), False, "default", ()),
    "auto_cold_off_fused": (ALL, (("auto_cold", 0),), True, "default", ()),
    "window_fused": (ALL, (), True, "window", ()),
    "window_regroup_2": (ALL, (("step_regroup", 2),), True, "window", ()),
    "debug": (("quad",), (("debug", 1),), False, "default", ()),          # (the compiled-in kadapt[1])
    "debug_fused": (("quad",), (("debug", 1),), True, "default", ()),
}
VARIANT_CASES = [(kind, name) for name, v in VARIANTS.items() for kind in v[0]]


def test_the_baseline_episodes_adapt():
    """what every comparison below rests on: in the seven default single-step launches rho leaves its setup value on every shape, the
    instances end at different values, and the first step is the oracle's solve (iteration counts equal, rho to 1e-9 / 1e-7)"""
    for kind in ALL:
        out, info = baseline(kind, "default")
        assert info["path"] in ONE_ROW and info["half"] == 0 and info["prefetch"] == 0, (kind, info["path"])
        # (per-instance data: every instance has its own system and start value; most end at the lower clip, 0.7)
        assert np.sum(out["rho"] != info["rho0"]) >= 5 and len(np.unique(out["rho"])) >= (3 if kind == "het" else 5), (kind, out["rho"], info["rho0"])
        assert out["acc"][0] == sum(int(st[0].sum()) for st in info["steps"])
    for kind, tol in (("quad", 1e-9), ("rand", 1e-7)):
        suite = {"quad": quad_suite, "rand": rand_suite}[kind]()
        ref = oracle_of(kind)
        assert_rho_moved(ref, suite, least=5)
        out = run_cases_hip(suite)
        assert np.array_equal(out["iter"].astype(int), ref["iter"].astype(int)), kind
        assert np.array_equal(baseline(kind, "default")[1]["steps"][0][0], ref["iter"].astype(int)), kind
        assert np.allclose(out["rho"], ref["rho"], rtol=tol, atol=0.0)
    # per-instance data: each instance's oracle with the tables the device computed for it
    from test_gpu_sensitivity import NAMES, oracle_runs
    fams, x0, Xref, Uref = het_inputs()
    s = make_het()
    tables = [{k: s.sensitivity_instance(i, k) for k in NAMES} for i in range(B)]
    s.close()
    first = baseline("het", "default")[1]["steps"][0][0]
    moved = 0
    for i in range(B):
        rec = oracle_runs(fams[i], tables[i], x0[i], Xref[i], Uref[i], 1, max_iter=60)[0]
        assert rec["iter"] == first[i], (i, rec["iter"], first[i])
        moved += rec["rho"][0] != fams[i]["rho"]
    assert moved >= 5, moved


@pytest.mark.parametrize("kind,name", VARIANT_CASES, ids=["%s-%s" % c for c in VARIANT_CASES])
def test_served_form_leaves_the_state_of_seven_default_single_step_launches(kind, name):
    """Records, x0, the five cache members, the last step's iteration counts and the accumulated iteration / solved counts: bit for bit.
    No option selects another kernel form: the path stays the one-row kernel, never its HALF or PREFETCH form."""
    _, opts, fused, key, skip = VARIANTS[name]
    want, winfo = baseline(kind, key)
    spec = BASELINES[key]
    got, info = closed_loop(kind, opts, fused, spec["pre"](kind) if "pre" in spec else None)
    assert info["path"] == winfo["path"] and info["path"] in ONE_ROW, info["path"]
    assert info["half"] == 0 and info["prefetch"] == 0
    if "step_regroup" in dict(opts):
        assert info["stretches"] > 2, info["stretches"]              # (one step of all, then stretches through perm)
    same(want, got, (kind, name), skip=skip)
    if "log" in info:
        it, u0 = info["log"]
        for t, (iters, solved, u) in enumerate(winfo["steps"]):
            assert np.array_equal(np.abs(it[t]), iters) and np.array_equal(it[t] > 0, (solved != 0) & (iters > 0)), (kind, name, t)
            assert np.array_equal(u0[t], u), (kind, name, t)


def test_debug_outputs_of_the_adaptive_kernel_match_the_oracle():
    """debug = 1 is another instantiation (kadapt[1]): q, r, p, d of one cold solve against the oracle at the 1e-9 of
    tests/test_gpu_adaptive.py, and everything else bit for bit what the plain instantiation leaves"""
    suite, ref = quad_suite(), oracle_of("quad")
    out = run_cases_hip(suite, debug=True)
    plain = fresh_handle_two_solves()[0]
    assert np.array_equal(out["iter"].astype(int), ref["iter"].astype(int))
    for k in FIELDS + CACHE:
        assert np.array_equal(out[k], plain[k]), k
    for k in ("q", "r", "p", "d"):
        for b in range(B):
            assert rel_err(out[k][b], ref[k][b]) < 1e-9, (k, b, rel_err(out[k][b], ref[k][b]))


# =====================================================================================================================================
# c. the constraint kinds adaptive rho is served with are in effect
# =====================================================================================================================================
def constrained(kind, **kw):
    suite = {"quad": quad_suite, "rand": rand_suite}[kind]()
    return dict(suite, config=dict(suite["config"], **kw))


def knot_varying(lo, hi, cols):
    """a box that tightens from `hi` x the bound at knot 0 to `lo` x at the last knot (another value at every knot)"""
    return np.linspace(hi, lo, cols)[None, :]


def constraint_cases():
    q, r = quad_suite()["config"], rand_suite()["config"]
    qn, rn = N, RAND_DIMS[2]
    off = dict(en_state_bound=0, en_input_bound=0)
    return {
        # quadrotor: a cone on the position (x, y against z) and one on the first three thrusts; the +-5 / +-0.5 box never binds: off
        "quad_input_cone": ("quad", 1e-9, dict(off, en_input_soc=1, input_cone=([0], [3], [0.3]))),
        "quad_state_cone": ("quad", 1e-9, dict(off, en_state_soc=1, state_cone=([0], [3], [0.5]))),
        "quad_both_cones": ("quad", 1e-9, dict(off, en_state_soc=1, en_input_soc=1, state_cone=([0], [3], [0.5]), input_cone=([0], [3], [0.3]))),
        "quad_box_knot_invariant": ("quad", 1e-9, dict(x_min=np.full((NX, qn), -1.0), x_max=np.full((NX, qn), 1.0), u_min=np.full((NU, qn - 1), -0.2), u_max=np.full((NU, qn - 1), 0.2))),
        "quad_box_knot_varying": ("quad", 1e-9, dict(x_min=-1.0 * knot_varying(0.6, 1.4, qn) * np.ones((NX, 1)), x_max=knot_varying(0.6, 1.4, qn) * np.ones((NX, 1)),
                                                     u_min=-0.2 * knot_varying(0.5, 1.5, qn - 1) * np.ones((NU, 1)), u_max=0.2 * knot_varying(0.5, 1.5, qn - 1) * np.ones((NU, 1)))),
        "rand_input_cone": ("rand", 1e-7, dict(en_input_soc=1, input_cone=([0], [3], [0.6]))),
        "rand_state_cone": ("rand", 1e-7, dict(en_state_soc=1, state_cone=([1], [3], [0.8]))),
        "rand_both_cones": ("rand", 1e-7, dict(en_state_soc=1, en_input_soc=1, state_cone=([1], [3], [0.8]), input_cone=([0], [3], [0.6]))),
        "rand_box_knot_invariant": ("rand", 1e-7, dict()),
        "rand_box_knot_varying": ("rand", 1e-7, dict(x_min=r["x_min"] * knot_varying(0.3, 0.9, rn), x_max=r["x_max"] * knot_varying(0.3, 0.9, rn),
                                                     u_min=r["u_min"] * knot_varying(0.5, 1.2, rn - 1), u_max=r["u_max"] * knot_varying(0.5, 1.2, rn - 1))),
    }


# the dual of a family after the solve IS (unprojected value - slack) of the last iteration: y_new = y_old + u - znew, znew = proj(u + y_old)
FAMILY_DUAL = {"en_state_bound": "g", "en_input_bound": "y", "en_state_soc": "gc", "en_input_soc": "yc"}


def active_sets(cfg, ref):
    """per enabled family: the number of (instance, knot) pairs whose slack differs from the unprojected value by more than 1e-6"""
    return {f: int(np.sum(np.max(np.abs(ref[d]), axis=1) > 1e-6)) for f, d in FAMILY_DUAL.items() if cfg[f]}


@pytest.mark.parametrize("name", list(constraint_cases()))
def test_served_constraint_kinds_are_in_effect_and_match_the_oracle(name):
    """Precondition, on the oracle alone: every enabled family binds on at least one instance and knot, and rho moves.  Then the device:
    iteration counts equal, rho, the records, the cone records and the cache within 1e-9 (quadrotor) / 1e-7 (random shape) per
    instance -- the numbers of tests/test_gpu_adaptive.py and tools/fuzz_parity.py adaptive_trial."""
    kind, tol, kw = constraint_cases()[name]
    suite = constrained(kind, **kw)
    cfg = suite["config"]
    ref = sc.run_cases(OracleSolver, suite)
    act = active_sets(cfg, ref)
    print(name, "active (instance, knot) pairs per enabled family", act, "distinct rho", len(np.unique(ref["rho"])), "iterations", ref["iter"].astype(int).tolist())
    assert act and all(n > 0 for n in act.values()), act
    assert_rho_moved(ref, suite)
    out = run_cases_hip(suite)
    assert np.array_equal(out["iter"].astype(int), ref["iter"].astype(int)), (out["iter"], ref["iter"])
    assert np.array_equal(out["sol_solved"].astype(int), ref["sol_solved"].astype(int))
    assert np.allclose(out["rho"], ref["rho"], rtol=tol, atol=0.0), (out["rho"], ref["rho"])
    soc = ("vcnew", "zcnew", "gc", "yc") if cfg["en_state_soc"] or cfg["en_input_soc"] else ()
    for k in FIELDS + soc + CACHE[1:]:
        for b in range(B):
            assert rel_err(out[k][b], ref[k][b]) < tol, (k, b, rel_err(out[k][b], ref[k][b]))
