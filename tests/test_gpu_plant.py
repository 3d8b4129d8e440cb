"""GPU tests of a plant model of its own at the plant step (tiny_batch_set_plant) and of the state log (option "state_log"): the one-row
kernel's PP forms and the helper kernel behind the coverage kernel.  Cases, reference plant step and oracle loops: tests/plant_cases.py
(batches of 13, 11 and 2: the last tile has 1, 3 or 2 rows; T = 5 fused MPC steps).
  a. every instance against its own oracle closed loop stepped by the reference plant, within the project's 1e-9;
  b. every launch form, bit for bit, against the host-in-the-loop form: the same library without a plant, single-step solves, the
     reference plant step applied in Python, set_x0 -- iteration log, u0 log, state log, final records and x0;
  c. a plant equal to the model, shared and per instance, on a batch with per-instance problem data: the bits of the same handle with
     nothing installed;
  d. the coverage path (force_general, a (20,8,10) tile shape) against the host form on the same kernel, and every logged state against
     the reference plant step of the logged u0: the same bits as the PP forms produce;
  e. composition with a disturbance, a per-instance box and per-instance problem data;
  f. the state log with nothing installed and with max_iter = 0;
  g. the setter, the getter, the refusal, reset and the lifecycle;  h. a sharded group.
Every test asserts the kernel path and the read-backs, so that none passes on the wrong path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import disturbance_cases as dc
import plant_cases as pc
import tinympc_amd as tm

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                        # the project's parity contract (README.md)
T, KEYS = pc.T, pc.KEYS


def make(c, group=False, own_box=False):
    """a handle for case c with everything but the plant set"""
    if group:
        s = tm.TinyGroupSolver.from_problem(c["fams"][0], c["B"], devices=[0, 0], n_shards=2, interleaved=True)
    elif c["hetero"]:
        s = tm.TinyBatchSolver.hetero(*[np.stack([f[k] for f in c["fams"]]) for k in ("A", "B", "f", "Q", "R")], np.array([f["rho"] for f in c["fams"]]), c["N"])
    else:
        s = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    if own_box:
        s.set_instance_bounds(*c["own_box"])
    else:
        s.set_bound_constraints(*[a[0] for a in c["box"]])
    s.update_settings(max_iter=pc.MAX_ITER, en_state_bound=1, en_input_bound=1)
    s.set_x0(c["x0"])
    s.set_x_ref(c["Xref"])
    s.set_u_ref(c["Uref"])
    return s


def snapshot(s, keys=KEYS):
    st = s.status()
    out = {k: s.get(k) for k in keys}
    out.update(iter=st["iter"].copy(), solved=st["solved"].copy(), x0=s.get("x0"))
    return out


def assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b), (sorted(a), sorted(b))
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, float(np.max(np.abs(np.asarray(a[k], dtype=float) - np.asarray(b[k], dtype=float)))))


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def assert_applied(s, path, kind=2):
    """the last solve's launches took their plant step through the plant on the kernel `path` names, on full rows, not in the PREFETCH form"""
    assert (s.get_option("plant"), s.get_option("last_plant")) == (kind, 1), (s.get_option("plant"), s.get_option("last_plant"))
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


def assert_host_form(r, path="regs"):
    assert (r.get_option("plant"), r.get_option("last_plant"), r.get_option("disturbance")) == (0, 0, 0)
    assert r.kernel_path() == path, r.kernel_path()


def fused(s, steps=T):
    s.set_option("steps_per_launch", steps)
    s.set_option("step_log", 1)
    s.set_option("state_log", 1)
    s.solve()
    it, u0 = s.step_log(steps)
    return dict(log_iter=it.copy(), log_u0=u0.copy(), log_x0=s.state_log(steps))


def advance(s, steps=T):
    s.set_option("advance_x0", 1)
    s.set_option("state_log", 1)
    its, u0s, xs = [], [], []
    for _ in range(steps):
        s.solve()
        st = s.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0s.append(s.get("u")[:, :, 0].copy())
        xs.append(s.state_log(1)[0])
    return dict(log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs))


def host_loop(r, plant, w=None, steps=T):
    """the host-in-the-loop form on handle r (nothing installed): `steps` single-step solves, the reference plant step (plant None: the
    solver's own x1) plus the disturbance row, where there is one, in Python, set_x0"""
    its, u0s, xs = [], [], []
    for k in range(steps):
        x0 = r.get("x0")
        r.solve()
        st = r.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0 = r.get("u")[:, :, 0].copy()
        u0s.append(u0)
        xn = r.get("x")[:, :, 1].copy() if plant is None else pc.plant_step_batch(plant, x0, u0)
        if w is not None and k < len(w):
            xn = xn + w[k]
        xs.append(xn)
        r.set_x0(xn)
    return dict(log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs))


def assert_log_follows_the_reference_plant(c, plant, run, w=None):
    """every logged state is the reference plant step of the state before it and the logged u0, bit for bit (whatever kernel solved)"""
    x0 = c["x0"]
    for k in range(len(run["log_x0"])):
        want = pc.plant_step_batch(plant, x0, run["log_u0"][k])
        if w is not None and k < len(w):
            want = want + w[k]
        assert np.array_equal(run["log_x0"][k], want), (k, float(np.max(np.abs(run["log_x0"][k] - want))))
        x0 = run["log_x0"][k]


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pc.ORACLE_CASES + pc.EDGE_CASES)
def test_every_instance_follows_its_own_oracle_loop_under_its_own_plant(name):
    pc.check_case(name)                                              # (the oracle alone: before anything runs on the GPU)
    c, want = pc.case(name), pc.oracle_case(name)
    s = make(c)
    s.set_plant(*c["plant"])
    run = fused(s)
    got = snapshot(s)
    assert_applied(s, "jit")
    for i in range(c["B"]):
        assert np.array_equal(run["log_iter"][:, i], want[i]["iter"]), (i, run["log_iter"][:, i], want[i]["iter"])
        for k in KEYS:
            e = rel_err(got[k][i], want[i]["rec"][k])
            assert e < RTOL, (i, k, e)
        assert rel_err(run["log_u0"][:, i], want[i]["u0"]) < RTOL and rel_err(got["x0"][i], want[i]["x0"]) < RTOL, i
        assert rel_err(run["log_x0"][:, i], want[i]["states"]) < RTOL, i
    assert np.array_equal(run["log_x0"][-1], got["x0"])
    s.close()


# ---- b. ------------------------------------------------------------------------------------------------------------------------------
def _regroup(streams):
    def drive(s):
        s.set_option("step_regroup", 2)
        s.set_option("step_regroup_streams", streams)
        out = fused(s)
        assert s.get_option("step_regroup_stretches") > 1
        return out
    return drive


def _capped(s):
    s.set_option("grid_waves_per_cu", 1)
    return fused(s)


FORMS = {"fused": fused, "advance_x0": advance, "step_regroup": _regroup(1), "step_regroup_two_streams": _regroup(2), "grid_waves_per_cu": _capped}


@functools.lru_cache(maxsize=None)
def host_reference(name, option=None):
    """the host-in-the-loop run of a case under its plants, computed once and shared (never modified)"""
    c = pc.case(name)
    r = make(c)
    if option:
        r.set_option(option, 1)
    want = dict(host_loop(r, c["plant"]))
    want.update(snapshot(r))
    assert_host_form(r, "cover" if option or c["nx"] + c["nu"] > 16 else "jit" if name == "5_3_7" else "regs")      # ((5,3,7) is not compiled in)
    r.close()
    return want


@pytest.mark.parametrize("name,form", [(n, f) for n in pc.ORACLE_CASES for f in FORMS])
def test_launch_forms_equal_the_host_in_the_loop_form_bit_for_bit(name, form):
    c = pc.case(name)
    s = make(c)
    s.set_plant(*c["plant"])
    run = FORMS[form](s)
    got = dict(snapshot(s), **run)
    assert_applied(s, "jit")
    s.close()
    assert_same_bits(got, host_reference(name), (name, form))


# ---- c. ------------------------------------------------------------------------------------------------------------------------------
def test_a_plant_equal_to_the_model_gives_the_bits_of_the_run_without_a_plant():
    # per-instance problem data, every instance stepped by its own model
    c = pc.case("12_4_10_hetero")
    r = make(c)
    want = dict(fused(r))
    want.update(snapshot(r))
    assert (r.get_option("plant"), r.get_option("last_plant")) == (0, 0) and r.kernel_path() == "jit"      # (the state log alone: a PD form, empty sequence)
    r.close()
    s = make(c)
    s.set_plant(*c["model"])
    got = dict(fused(s))
    got.update(snapshot(s))
    assert_applied(s, "jit")
    s.close()
    assert_same_bits(got, want, "every instance its own model as its plant")
    # one model for all, installed once
    c = pc.case("12_4_10")
    r = make(c)
    want = dict(fused(r))
    want.update(snapshot(r))
    r.close()
    for kind, plant in ((1, tuple(m[0] for m in c["model"])), (2, c["model"])):
        s = make(c)
        s.set_plant(*plant)
        got = dict(fused(s))
        got.update(snapshot(s))
        assert_applied(s, "jit", kind=kind)
        s.close()
        assert_same_bits(got, want, ("the shared model as the plant", kind))
    # ... and without the log on the reference side: the compiled-in form's records
    r = make(c)
    r.set_option("steps_per_launch", T)
    r.solve()
    assert r.kernel_path() == "regs"
    plain = snapshot(r)
    r.close()
    assert_same_bits({k: want[k] for k in plain}, plain, "the PD form with an empty sequence against the compiled-in form")


# ---- d. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,option", [("5_3_7", "force_general"), ("20_8_10", None)])
def test_the_coverage_path_takes_the_same_plant_step(name, option):
    c = pc.case(name)
    for drive in (fused, advance):
        s = make(c)
        if option:
            s.set_option(option, 1)
        s.set_plant(*c["plant"])
        run = drive(s)
        got = dict(snapshot(s), **run)
        assert_applied(s, "cover")
        s.close()
        assert_same_bits(got, host_reference(name, option or "force_general"), (name, drive.__name__))
        assert_log_follows_the_reference_plant(c, c["plant"], run)
    if option:                                                       # where both exist: the PP form's states obey the same reference, bit for bit
        s = make(c)
        s.set_plant(*c["plant"])
        run = fused(s)
        assert_applied(s, "jit")
        s.close()
        assert_log_follows_the_reference_plant(c, c["plant"], run)


# ---- e. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["disturbance", "instance_box", "hetero", "disturbance_cover"])
def test_pp_composes(what):
    c = pc.case("12_4_10_hetero" if what == "hetero" else "6_3_10")
    w = c["w"] if what.startswith("disturbance") else None
    cover = what.endswith("cover")
    def handle():
        h = make(c, own_box=what == "instance_box")
        if cover:
            h.set_option("force_general", 1)
        return h
    s = handle()
    s.set_plant(*c["plant"])
    if w is not None:
        s.set_disturbance(w)
    run = fused(s)
    got = dict(snapshot(s), **run)
    assert_applied(s, "cover" if cover else "jit")
    assert s.get_option("last_disturbance") == int(w is not None) and s.get_option("last_instance_bounds") == int(what == "instance_box")
    s.close()
    r = handle()
    want = dict(host_loop(r, c["plant"], w))
    want.update(snapshot(r))
    assert (r.get_option("plant"), r.get_option("last_plant")) == (0, 0)
    r.close()
    assert_same_bits(got, want, what)
    assert_log_follows_the_reference_plant(c, c["plant"], run, w)


def make_own(c):
    """a handle for a composition case of tests/disturbance_cases.py: every instance its own half-spaces (PL) or cone coefficients (PC)"""
    s = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    box, cones, lin = int("box" in c["has"]), int("cones" in c["has"]), int("lin" in c["has"])
    if cones:
        s.set_cone_constraints(c["Acx"], [3], c["cx"][0], c["Acu"], [3], c["cu"][0])
        s.set_instance_cone_coefficients(c["cx"], c["cu"])
    if lin:
        s.set_instance_linear_constraints(*c["linear"])
    s.update_settings(max_iter=dc.MAX_ITER, en_state_bound=box, en_input_bound=box, en_state_soc=cones, en_input_soc=cones, en_state_linear=lin, en_input_linear=lin)
    s.set_x0(c["x0"])
    s.set_x_ref(c["Xref"])
    s.set_u_ref(c["Uref"])
    return s


@pytest.mark.parametrize("name,own,with_disturbance", [("6_3_10_pl", "lin", False), ("6_3_10_pc", "cones", False), ("6_3_10_pl", "lin", True), ("6_3_10_pc", "cones", True)])
def test_pp_composes_with_per_instance_halfspaces_and_cone_coefficients(name, own, with_disturbance):
    """the PP bit on the PL and the PC form (their own tables and LDS rows next to the plant row), alone and with the PD bit as well"""
    c = dc.case(name)
    assert c["own"] == (own,) and c["path"] == "jit"
    keys, plant = dc.keys(c), pc.plant_for(c)
    w = 0.1 * c["w"] if with_disturbance else None
    s = make_own(c)
    s.set_plant(*plant)
    if w is not None:
        s.set_disturbance(w)
    run = fused(s)
    got = dict(snapshot(s, keys), **run)
    assert_applied(s, "jit")
    assert (s.get_option("last_instance_linear"), s.get_option("last_instance_cones"), s.get_option("last_disturbance")) == \
        (int(own == "lin"), int(own == "cones"), int(with_disturbance))
    s.close()
    r = make_own(c)
    want = dict(host_loop(r, plant, w))
    want.update(snapshot(r, keys))
    assert (r.get_option("plant"), r.get_option("last_plant"), r.get_option("disturbance")) == (0, 0, 0) and r.kernel_path() == "jit"
    assert (r.get_option("last_instance_linear"), r.get_option("last_instance_cones")) == (int(own == "lin"), int(own == "cones"))
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0      # (something iterates, nothing diverges)
    assert_same_bits(got, want, (name, with_disturbance))
    assert_log_follows_the_reference_plant(c, plant, run, w)


# ---- f. ------------------------------------------------------------------------------------------------------------------------------
def test_state_log_with_nothing_installed_and_with_no_iteration():
    c = pc.case("5_3_7")
    r = make(c)
    want = host_loop(r, None)
    assert_host_form(r, "jit")                                       # ((5,3,7) is not compiled in)
    r.close()
    for drive in (fused, advance):
        s = make(c)
        run = drive(s)
        assert (s.get_option("plant"), s.get_option("last_plant"), s.get_option("last_disturbance")) == (0, 0, 0) and s.kernel_path() == "jit"
        assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0
        assert_same_bits(run, want, drive.__name__)
        s.close()
    # max_iter = 0: no plant step, the log holds the x0 the launch left in place (one-row and coverage path)
    for option in (None, "force_general"):
        s = make(c)
        if option:
            s.set_option(option, 1)
        s.set_plant(*c["plant"])
        s.update_settings(max_iter=0, en_state_bound=1, en_input_bound=1)
        run = advance(s, 2)
        assert_applied(s, "cover" if option else "jit")
        assert np.array_equal(run["log_x0"], np.broadcast_to(c["x0"], run["log_x0"].shape)) and np.array_equal(s.get("x0"), c["x0"])
        s.close()
    # the log off: nothing recorded
    s = make(c)
    s.set_plant(*c["plant"])
    s.set_option("advance_x0", 1)
    s.solve()
    assert tm.lib().tiny_batch_get_state_log(s._h, None, 1) == tm.ERR_ARG
    s.close()


# ---- g. ------------------------------------------------------------------------------------------------------------------------------
def _run(s):
    run = fused(s)
    return dict(snapshot(s), **run)


def test_setter_getter_broadcast_removal_failed_call_refusal_and_reset():
    c = pc.case("4_2_10")                                            # (compiled in: without a plant step's extras the launch is the compiled-in form)
    B, nx, nu = c["B"], c["nx"], c["nu"]
    A, Bm, f = c["plant"]
    L = tm.lib()
    s = make(c)
    assert L.tiny_batch_get_plant(s._h, 0, None, None, None) == tm.ERR_ARG                      # none installed
    s.set_plant(A, Bm, f)
    for i in (0, 4, B - 1):
        gA, gB, gf = s.get_plant(i)
        assert np.array_equal(gA, A[i]) and np.array_equal(gB, Bm[i]) and np.array_equal(gf, f[i])
    assert L.tiny_batch_get_plant(s._h, B, None, None, None) == tm.ERR_ARG and L.tiny_batch_get_plant(s._h, -1, None, None, None) == tm.ERR_ARG
    own = _run(s)
    assert_applied(s, "jit")
    # one plant for all against the same plant repeated: the same bits; f_p = None is zero
    one = (A[3], Bm[3], None)
    full = (np.repeat(A[3:4], B, 0), np.repeat(Bm[3:4], B, 0), np.zeros((B, nx)))
    a, b = make(c), make(c)
    a.set_plant(*one)
    b.set_plant(*full)
    assert a.get_option("plant") == 1 and b.get_option("plant") == 2
    gA, gB, gf = a.get_plant(B - 1)
    assert np.array_equal(gA, A[3]) and np.array_equal(gB, Bm[3]) and np.array_equal(gf, np.zeros(nx))
    bc = _run(a)
    assert_applied(a, "jit", kind=1)
    assert_same_bits(bc, _run(b), "TINY_BROADCAST against the repeated plant")
    assert not np.array_equal(bc["x0"], own["x0"])
    a.close()
    b.close()
    # a failed call (B_p == NULL) leaves what was installed
    flat = np.ascontiguousarray(A.transpose(0, 2, 1)).ravel()
    assert L.tiny_batch_set_plant(s._h, flat.ctypes.data_as(C.c_void_p), None, None, tm.HOST) == tm.ERR_ARG
    assert s.get_option("plant") == 2 and np.array_equal(s.get_plant(4)[1], Bm[4])
    # reset keeps the plant: the same episode again
    s.reset()
    s.set_x0(c["x0"])
    assert s.get_option("plant") == 2
    assert_same_bits(_run(s), own, "after reset")
    # adaptive rho on a launch with a plant step is refused with its own text; without a plant step it runs
    c6 = pc.case("6_3_10")
    q = tm.TinyBatchSolver.from_problem(c6["fams"][0], c6["B"])
    q.update_settings(max_iter=pc.MAX_ITER, en_state_bound=0, en_input_bound=0)
    q.set_x0(c6["x0"])
    q.set_plant(*c6["plant"])
    q.set_adaptive_rho(1)
    q.solve()
    assert q.get_option("last_plant") == 0
    q.set_option("advance_x0", 1)
    assert L.tiny_batch_solve(q._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(q._h).decode()
    assert "adaptive rho does not combine with a plant of its own" in msg, msg
    q.set_adaptive_rho(0)
    q.solve()
    assert_applied(q, "jit")
    q.close()
    # remove, then replace: the run without a plant on the compiled-in form, then the first run again
    s.set_plant(None)
    assert s.get_option("plant") == 0 and L.tiny_batch_get_plant(s._h, 0, None, None, None) == tm.ERR_ARG
    s.reset()
    s.set_x0(c["x0"])
    s.set_option("state_log", 0)
    s.set_option("steps_per_launch", T)
    s.solve()
    assert s.get_option("last_plant") == 0 and s.kernel_path() == "regs"
    assert not np.array_equal(s.get("x0"), own["x0"])
    s.set_plant(A, Bm, f)
    s.reset()
    s.set_x0(c["x0"])
    assert_same_bits(_run(s), own, "removed and installed again")
    s.close()


def _hip_runtime():
    """the HIP runtime the library itself is linked against (already loaded with it: the same handle)"""
    for name in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise OSError("libamdhip64 not found")


def test_device_pointers_give_the_bits_of_host_arrays():
    """TINY_DEVICE: per instance and one for all; the caller's buffers are freed right after the call (the arrays are copied)"""
    c = pc.case("5_3_7")
    B = c["B"]
    A, Bm, f = c["plant"]
    hip = _hip_runtime()

    def on_device(a):
        flat = np.ascontiguousarray(a, dtype=np.float64).ravel()
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(flat.nbytes)) == 0
        assert hip.hipMemcpy(p, flat.ctypes.data_as(C.c_void_p), C.c_size_t(flat.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return p
    for kind, host, cm in ((2, (A, Bm, f), (A.transpose(0, 2, 1), Bm.transpose(0, 2, 1), f)), (1, (A[2], Bm[2], f[2]), (A[2].T, Bm[2].T, f[2]))):
        a, b = make(c), make(c)
        a.set_plant(*host)
        ptrs = [on_device(m) for m in cm]                            # (column-major per instance, as the C ABI takes them)
        b.set_plant_device(ptrs[0].value, ptrs[1].value, ptrs[2].value, broadcast=kind == 1)
        for p in ptrs:
            assert hip.hipFree(p) == 0
        for i in (0, B - 1):
            for got, want in zip(b.get_plant(i), a.get_plant(i)):
                assert np.array_equal(got, want), (kind, i)
        want = _run(a)
        assert_same_bits(_run(b), want, ("TINY_DEVICE against TINY_HOST", kind))
        assert_applied(b, "jit", kind=kind)
        a.close()
        b.close()


def test_install_replace_remove_reinstall_equals_a_fresh_handle():
    c = pc.case("5_3_7")
    A, Bm, f = c["plant"]
    other = (A[::-1].copy(), Bm[::-1].copy(), None)
    fresh = make(c)
    fresh.set_plant(A, Bm, f)
    want = _run(fresh)
    assert_applied(fresh, "jit")
    fresh.close()
    s = make(c)
    for plant in ((A[0], Bm[0], f[0]), other, None, (A, Bm, f)):
        if plant is None:
            s.set_plant(None)
        else:
            s.set_plant(*plant)
        s.reset()
        s.set_x0(c["x0"])
        got = _run(s)
    assert_applied(s, "jit")
    s.close()
    assert_same_bits(got, want, "install, replace, remove, reinstall")


# ---- h. ------------------------------------------------------------------------------------------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    c = pc.case("6_3_10")                                            # 11 instances: shards of 6 and 5
    g, s = make(c, group=True), make(c)
    for h in (g, s):
        h.set_plant(*c["plant"])
        h.set_option("steps_per_launch", 3)
        h.set_option("state_log", 1)
        h.solve()
    st, gst = s.status(), g.status()
    for k in KEYS + ("x0",):
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(gst["iter"], st["iter"]) and np.array_equal(gst["solved"], st["solved"])
    assert np.array_equal(g.state_log(3), s.state_log(3))
    assert_applied(s, "jit")
    for k in range(g.shards):
        h = tm.lib().tiny_group_shard(g._h, k)
        opt = lambda n: int(tm.lib().tiny_batch_get_option(h, n))
        assert (opt(b"plant"), opt(b"last_plant"), opt(b"last_half_rows"), opt(b"last_prefetch"), tm.lib().tiny_batch_kernel_path(h)) == (2, 1, 0, 0, 3)
    for i in (0, 1, 10):
        for got, want in zip(g.get_plant(i), (m[i] for m in c["plant"])):
            assert np.array_equal(got, want), i
    g.close()
    s.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------------
def test_model_mismatch_example_spreads_the_end_states_under_mismatch_only():
    """examples/model_mismatch_closed_loop.c (C99, built by __graft_entry__.build()): double integrators whose true actuator gain and
    mass differ per instance, 60 fused steps on a PP form with the state log, then with the model as the plant; its exit status checks
    the two spreads"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "model_mismatch_closed_loop")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/model_mismatch_closed_loop is missing: __graft_entry__.build() produces it")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "kernel path 3, plant 2, applied 1" in p.stdout and "kernel path 3, plant 1, applied 1" in p.stdout, p.stdout
