"""GPU tests of measurement noise at the plant step of a closed loop (tiny_batch_set_measurement_noise): the one-row kernel's PM forms and
the helper kernels around the coverage kernel.  Cases, noise and oracle loops: tests/measurement_cases.py on the problems of
tests/plant_cases.py (batches of 13, 11 and 2: the last tile has 1, 3 or 2 rows; T = 5 MPC steps).
  a. every launch form, bit for bit, against the host-in-the-loop form: the same library with nothing installed, per MPC step
     set_x0(fl(x + v[k])), one single-step solve, u[:,0] read back, x = the reference plant step of the TRUE x (by the plant, or with
     none by the model) -- every record, the step log, the state log and the final x0;
  b. every instance against its own oracle loop within the project's 1e-9;
  c. a sequence that never applies (every row outside the counter; no plant step) gives the bits of a handle with nothing installed;
  d. composition with a plant of its own, a disturbance, per-instance problem data, PB, PL and PC, and the coverage path;
  e. the state log holds the TRUE states, x[:,0] the measurement; the counter; max_iter = 0;
  f. setter, getter, broadcast, device pointers, removal, a failed call, reset, the lifecycle; the refusal text;  g. a sharded group;
  h. the example.
Every test asserts the kernel path and the read-backs, so that none passes on the wrong path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import disturbance_cases as dc
import measurement_cases as mc
import plant_cases as pc
import tinympc_amd as tm
from test_gpu_plant import _hip_runtime, assert_same_bits, make, make_own, rel_err, snapshot

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                        # the project's parity contract (README.md)
T, KEYS = mc.T, mc.KEYS


def assert_applied(s, path, plant=0, steps=T):
    """the last solve's launches applied the sequence on the kernel `path` names, on full rows, not in the PREFETCH form"""
    assert (s.get_option("measurement_noise"), s.get_option("last_measurement_noise")) == (steps, 1)
    assert (s.get_option("plant"), s.get_option("last_plant")) == (plant, int(plant != 0))
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


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


def _regroup(streams):
    def drive(s):
        s.set_option("step_regroup", 2)
        s.set_option("step_regroup_streams", streams)
        out = fused(s)
        assert s.get_option("step_regroup_stretches") > 1
        return out
    return drive


def _mode0(s):
    s.set_option("dpp_mode", 0)
    return fused(s)


FORMS = {"fused": fused, "advance_x0": advance, "step_regroup": _regroup(1), "step_regroup_two_streams": _regroup(2), "dpp_mode_0": _mode0}


def host_loop(r, c, v, plant=None, w=None, steps=T, keys=KEYS):
    """the host-in-the-loop form on handle r (nothing installed): per MPC step set_x0(fl(x + v[k])) where the row exists, one single-step
    solve, u[:,0] read back, x = the reference plant step of the true x plus the disturbance row, in Python.  Returns the logs, the
    records after the last solve and the final TRUE state as x0"""
    plant = plant or mc.model_of(c)
    x = c["x0"].copy()
    its, u0s, xs = [], [], []
    for k in range(steps):
        r.set_x0(x + v[k] if k < len(v) else x)
        r.solve()
        st = r.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0 = r.get("u")[:, :, 0].copy()
        u0s.append(u0)
        x = pc.plant_step_batch(plant, x, u0)
        if w is not None and k < len(w):
            x = x + w[k]
        xs.append(x)
    out = dict(snapshot(r, keys), log_iter=np.array(its), log_u0=np.array(u0s), log_x0=np.array(xs))
    out["x0"] = x
    assert (r.get_option("measurement_noise"), r.get_option("last_measurement_noise"), r.get_option("plant"), r.get_option("disturbance")) == (0, 0, 0, 0)
    return out


def assert_log_follows_the_reference_plant(c, run, plant=None):
    """every logged state is the reference plant step of the TRUE state before it and the logged u0, bit for bit (whatever kernel solved)"""
    x = c["x0"]
    for k in range(len(run["log_x0"])):
        x = pc.plant_step_batch(plant or mc.model_of(c), x, run["log_u0"][k])
        assert np.array_equal(run["log_x0"][k], x), (k, float(np.max(np.abs(run["log_x0"][k] - x))))


@functools.lru_cache(maxsize=None)
def host_reference(name, option=None, value=1):
    """the host-in-the-loop run of a case under its noise and its model, computed once and shared (never modified)"""
    c = pc.case(name)
    r = make(c)
    if option:
        r.set_option(option, value)
    want = host_loop(r, c, mc.noise(name))
    r.close()
    return want


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [(n, f) for n in mc.ORACLE_CASES for f in FORMS])
def test_launch_forms_equal_the_host_in_the_loop_form_bit_for_bit(name, form):
    c = pc.case(name)
    s = make(c)
    s.set_measurement_noise(mc.noise(name))
    run = FORMS[form](s)
    got = dict(snapshot(s), **run)
    assert_applied(s, "jit")
    assert s.get_option("measurement_step") == T
    s.close()
    assert_same_bits(got, host_reference(name, "dpp_mode", 0) if form == "dpp_mode_0" else host_reference(name), (name, form))


# ---- b. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mc.ORACLE_CASES + mc.EDGE_CASES)
def test_every_instance_follows_its_own_oracle_loop(name):
    c, want = pc.case(name), mc.oracle_case(name)
    s = make(c)
    s.set_measurement_noise(mc.noise(name))
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


# ---- c. ------------------------------------------------------------------------------------------------------------------------------
def test_a_sequence_that_never_applies_gives_the_bits_of_a_handle_with_nothing_installed():
    c = pc.case("12_4_10")
    v = mc.noise("12_4_10")

    def run(h, steps):
        h.set_option("steps_per_launch", steps)
        h.set_option("step_log", 1)
        h.solve()
        out = snapshot(h)
        if steps > 1:
            out["log_iter"], out["log_u0"] = (a.copy() for a in h.step_log(steps))
        return out
    r = make(c)
    want = run(r, T)
    assert r.kernel_path() == "regs"
    r.close()
    for start in (T, -T, 10**12):                                    # every row outside the counter: x0 itself is handed on, nothing is added
        s = make(c)
        s.set_measurement_noise(v)
        s.set_option("measurement_step", start)
        got = run(s, T)
        assert_applied(s, "jit")
        assert s.get_option("measurement_step") == start + T
        s.close()
        assert_same_bits(got, want, ("rows outside the counter", start))
    # no plant step: nothing is read, the counter stays, the compiled-in form runs
    r = make(c)
    want = run(r, 1)
    r.close()
    s = make(c)
    s.set_measurement_noise(v)
    got = run(s, 1)
    assert (s.get_option("measurement_noise"), s.get_option("last_measurement_noise"), s.get_option("measurement_step")) == (T, 0, 0)
    assert s.kernel_path() == "regs"
    s.close()
    assert_same_bits(got, want, "a launch without a plant step")


# ---- d. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["plant", "disturbance", "plant_and_disturbance", "hetero", "instance_box"])
def test_pm_composes(what):
    name = "12_4_10_hetero" if what == "hetero" else "6_3_10"
    c, v = pc.case(name), mc.noise(name)
    plant = c["plant"] if "plant" in what else None
    w = c["w"] if "disturbance" in what else None
    s = make(c, own_box=what == "instance_box")
    s.set_measurement_noise(v)
    if plant:
        s.set_plant(*plant)
    if w is not None:
        s.set_disturbance(w)
    run = fused(s)
    got = dict(snapshot(s), **run)
    assert_applied(s, "jit", plant=2 if plant else 0)
    assert s.get_option("last_disturbance") == int(w is not None) and s.get_option("last_instance_bounds") == int(what == "instance_box")
    s.close()
    r = make(c, own_box=what == "instance_box")
    want = host_loop(r, c, v, plant, w)
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0
    assert_same_bits(got, want, what)


@pytest.mark.parametrize("name,own", [("6_3_10_pl", "lin"), ("6_3_10_pc", "cones")])
def test_pm_composes_with_per_instance_halfspaces_and_cone_coefficients(name, own):
    c = dc.case(name)
    assert c["own"] == (own,) and c["path"] == "jit"
    keys = dc.keys(c)
    v = mc.noise_for(c["B"], c["nx"], 4711)
    s = make_own(c)
    s.set_measurement_noise(v)
    run = fused(s)
    got = dict(snapshot(s, keys), **run)
    assert_applied(s, "jit")
    assert (s.get_option("last_instance_linear"), s.get_option("last_instance_cones")) == (int(own == "lin"), int(own == "cones"))
    s.close()
    r = make_own(c)
    want = host_loop(r, c, v, keys=keys)
    assert r.kernel_path() == "jit"
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0      # (something iterates, nothing diverges)
    assert_same_bits(got, want, name)


@pytest.mark.parametrize("name,option", [("5_3_7", "force_general"), ("20_8_10", None)])
def test_the_coverage_path_measures_and_steps_the_same_way(name, option):
    c, v = pc.case(name), mc.noise(name)
    for drive in (fused, advance):
        s = make(c)
        if option:
            s.set_option(option, 1)
        s.set_measurement_noise(v)
        run = drive(s)
        got = dict(snapshot(s), **run)
        assert_applied(s, "cover")
        s.close()
        assert_same_bits(got, host_reference(name, option or "force_general"), (name, drive.__name__))
        assert_log_follows_the_reference_plant(c, run)
    if option:                                                       # where both exist: the PM form's states obey the same reference, bit for bit
        s = make(c)
        s.set_measurement_noise(v)
        run = fused(s)
        assert_applied(s, "jit")
        s.close()
        assert_log_follows_the_reference_plant(c, run)


# ---- e. ------------------------------------------------------------------------------------------------------------------------------
def test_the_state_log_holds_true_states_x_holds_the_measurement_and_the_counter_moves():
    c, v = pc.case("5_3_7"), mc.noise("5_3_7")
    s = make(c)
    s.set_measurement_noise(v)
    run = fused(s)
    assert_applied(s, "jit")
    assert_log_follows_the_reference_plant(c, run)                   # every logged state: the reference plant step of the TRUE state before it
    x = run["log_x0"][T - 1]
    assert np.array_equal(s.get("x0"), x)
    assert np.array_equal(s.get("x")[:, :, 0], run["log_x0"][T - 2] + v[T - 1])      # work->x[:,0] of the last solve: its measurement
    assert not np.array_equal(s.get("x")[:, :, 0], run["log_x0"][T - 2])
    # the counter: advanced by T, moved back by the option, rewound by the setter; a single step takes row 2 then
    assert s.get_option("measurement_step") == T
    s.set_option("measurement_step", 2)
    assert s.get_option("measurement_step") == 2
    s.set_option("steps_per_launch", 1)
    s.set_option("advance_x0", 1)
    s.solve()
    assert s.get_option("measurement_step") == 3 and np.array_equal(s.get("x")[:, :, 0], x + v[2])
    s.set_measurement_noise(v)
    assert s.get_option("measurement_step") == 0
    s.close()
    # max_iter = 0: the step sees its measurement in x[:,0] and takes no plant step (one-row and coverage path)
    for option in (None, "force_general"):
        s = make(c)
        if option:
            s.set_option(option, 1)
        s.set_measurement_noise(v)
        s.update_settings(max_iter=0, en_state_bound=1, en_input_bound=1)
        run = advance(s, 2)
        assert_applied(s, "cover" if option else "jit")
        assert np.array_equal(run["log_x0"], np.broadcast_to(c["x0"], run["log_x0"].shape)) and np.array_equal(s.get("x0"), c["x0"])
        assert np.array_equal(s.get("x")[:, :, 0], c["x0"] + v[1]) and s.get_option("measurement_step") == 2
        s.close()
    s = make(c)                                                      # ... and fused
    s.set_measurement_noise(v)
    s.update_settings(max_iter=0, en_state_bound=1, en_input_bound=1)
    run = fused(s, 3)
    assert_applied(s, "jit")
    assert np.array_equal(run["log_x0"], np.broadcast_to(c["x0"], run["log_x0"].shape)) and np.array_equal(s.get("x0"), c["x0"])
    assert np.array_equal(s.get("x")[:, :, 0], c["x0"] + v[2])
    s.close()


# ---- f. ------------------------------------------------------------------------------------------------------------------------------
def _run(s):
    run = fused(s)
    return dict(snapshot(s), **run)


def test_setter_getter_broadcast_device_pointers_removal_failed_call_and_reset():
    c, v = pc.case("4_2_10"), mc.noise("4_2_10")
    B, nx = c["B"], c["nx"]
    L = tm.lib()
    out = np.zeros(nx)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    s = make(c)
    assert L.tiny_batch_get_measurement_noise(s._h, 0, 0, dp) == tm.ERR_ARG                     # none installed
    s.set_measurement_noise(v)
    for k, i in ((0, 0), (2, 4), (T - 1, B - 1)):
        assert np.array_equal(s.get_measurement_noise(k, i), v[k, i])
    for k, i, p in ((T, 0, dp), (-1, 0, dp), (0, B, dp), (0, -1, dp), (0, 0, None)):
        assert L.tiny_batch_get_measurement_noise(s._h, k, i, p) == tm.ERR_ARG
    own = _run(s)
    assert_applied(s, "jit")
    # one sequence for all against the same sequence repeated, from host arrays and from device pointers: the same bits
    one = v[:, 3]
    full = np.repeat(one[:, None], B, axis=1)
    hip = _hip_runtime()

    def on_device(a):
        flat = np.ascontiguousarray(a, dtype=np.float64).ravel()
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(flat.nbytes)) == 0
        assert hip.hipMemcpy(p, flat.ctypes.data_as(C.c_void_p), C.c_size_t(flat.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return p
    runs = []
    for how in ("broadcast", "full", "device", "device_broadcast"):
        h = make(c)
        if how == "broadcast":
            h.set_measurement_noise(one)
        elif how == "full":
            h.set_measurement_noise(full)
        else:
            p = on_device(one if how == "device_broadcast" else full)
            h.set_measurement_noise_device(p.value, T, broadcast=how == "device_broadcast")
            assert hip.hipFree(p) == 0                               # (the array is copied)
        assert np.array_equal(h.get_measurement_noise(1, B - 1), one[1])
        runs.append(_run(h))
        assert_applied(h, "jit")
        h.close()
    for other in runs[1:]:
        assert_same_bits(other, runs[0], "one sequence for all, four ways")
    assert not np.array_equal(runs[0]["x0"], own["x0"])
    # a failed call leaves what was installed: a sequence no device memory holds
    s.set_option("measurement_step", 2)
    flat = np.ascontiguousarray(one).ravel()
    rc = L.tiny_batch_set_measurement_noise(s._h, flat.ctypes.data_as(C.c_void_p), 2**31 - 1, tm.HOST | tm.BROADCAST)
    assert rc != tm.OK, rc
    assert (s.get_option("measurement_noise"), s.get_option("measurement_step")) == (T, 2)
    assert np.array_equal(s.get_measurement_noise(1, 4), v[1, 4])
    # reset keeps the sequence and its counter: rewound by hand, the same episode again
    s.reset()
    assert (s.get_option("measurement_noise"), s.get_option("measurement_step")) == (T, 2)
    s.set_option("measurement_step", 0)
    s.set_x0(c["x0"])
    assert_same_bits(_run(s), own, "after reset")
    # removal, by None and by n_steps = 0: the run without noise on the compiled-in form
    s.set_measurement_noise(None)
    assert (s.get_option("measurement_noise"), s.get_option("measurement_step")) == (0, 0)
    assert L.tiny_batch_get_measurement_noise(s._h, 0, 0, dp) == tm.ERR_ARG
    s.set_measurement_noise(v)
    assert L.tiny_batch_set_measurement_noise(s._h, flat.ctypes.data_as(C.c_void_p), 0, tm.HOST) == tm.OK and s.get_option("measurement_noise") == 0
    s.reset()
    s.set_x0(c["x0"])
    s.set_option("state_log", 0)
    s.set_option("steps_per_launch", T)
    s.solve()
    assert s.get_option("last_measurement_noise") == 0 and s.kernel_path() == "regs"
    assert not np.array_equal(s.get("x0"), own["x0"])
    s.close()


def test_install_replace_remove_reinstall_equals_a_fresh_handle():
    c, v = pc.case("5_3_7"), mc.noise("5_3_7")
    fresh = make(c)
    fresh.set_measurement_noise(v)
    want = _run(fresh)
    assert_applied(fresh, "jit")
    fresh.close()
    s = make(c)
    for seq in (v[:, 0], v[::-1].copy(), None, v):
        s.set_measurement_noise(seq)
        s.reset()
        s.set_x0(c["x0"])
        got = _run(s)
    assert_applied(s, "jit")
    s.close()
    assert_same_bits(got, want, "install, replace, remove, reinstall")


def test_adaptive_rho_is_refused_on_a_launch_with_a_plant_step_only():
    c = pc.case("6_3_10")
    L = tm.lib()
    q = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    q.update_settings(max_iter=pc.MAX_ITER, en_state_bound=0, en_input_bound=0)
    q.set_x0(c["x0"])
    q.set_measurement_noise(mc.noise("6_3_10"))
    q.set_adaptive_rho(1)
    q.solve()                                                        # no plant step: the sequence does not apply, adaptive rho runs
    assert q.get_option("last_measurement_noise") == 0
    q.set_option("advance_x0", 1)
    assert L.tiny_batch_solve(q._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(q._h).decode()
    assert "adaptive rho does not combine with measurement noise (tiny_batch_set_measurement_noise)" in msg, msg
    assert q.get_option("measurement_step") == 0
    q.set_adaptive_rho(0)
    q.solve()
    assert_applied(q, "jit")
    assert q.get_option("measurement_step") == 1
    q.close()


# ---- g. ------------------------------------------------------------------------------------------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    c, v = pc.case("6_3_10"), mc.noise("6_3_10")                     # 11 instances: shards of 6 and 5
    g, s = make(c, group=True), make(c)
    for h in (g, s):
        h.set_measurement_noise(v)
        h.set_option("measurement_step", 1)                          # (forwarded to every shard)
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
        assert (opt(b"measurement_noise"), opt(b"measurement_step"), opt(b"last_measurement_noise"), opt(b"last_half_rows"), opt(b"last_prefetch"),
                tm.lib().tiny_batch_kernel_path(h)) == (T, 4, 1, 0, 0, 3)
    g.close()
    s.close()


# ---- h. ------------------------------------------------------------------------------------------------------------------------------
def test_sensor_noise_example_spreads_the_end_states_under_noise_only():
    """examples/sensor_noise_closed_loop.c (C99, built by __graft_entry__.build()): double integrators that solve from noisy readings, 60
    fused steps on a PM form with the state log, then with the exact state; its exit status checks the two spreads"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "sensor_noise_closed_loop")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/sensor_noise_closed_loop is missing: __graft_entry__.build() produces it")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "kernel path 3, sequence of 60 steps, applied 1" in p.stdout and "kernel path 3, sequence of 0 steps, applied 0" in p.stdout, p.stdout
