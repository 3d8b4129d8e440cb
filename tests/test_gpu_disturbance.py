"""GPU tests of the per-instance disturbance sequence at the plant step (tiny_batch_set_disturbance): the one-row kernel's PD forms and the
coverage kernel's addition.  Batches of 13, 11 and 2: up to four tiles, the last one with 1, 3 or 2 rows; T = 5 fused MPC steps under a
sequence of 4 rows, so that the last step is undisturbed.
  a. every instance against its own oracle closed loop (tests/disturbance_cases.py asserts, from the oracle alone, that a row read from
     the wrong instance, grid slot or step moves the next u0), on every case;
  b. every launch form, bit for bit, against the host-in-the-loop form: the same library without a sequence, single-step solves and
     x0 = get("x")[:, :, 1] + w[k] added in numpy;
  c. PD together with PB, PL and PC (and PL + PC on the coverage kernel);
  d. the step counter;  e. the setter, the getter and the refusal;  f. a sharded group.
Every test asserts the kernel path and the read-backs, so that none passes on the wrong path."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import disturbance_cases as dc
import tinympc_amd as tm

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                        # the project's parity contract (README.md)
T, N_STEPS = dc.T, dc.N_STEPS


def settings(c, max_iter=dc.MAX_ITER):
    box, cones, lin = int("box" in c["has"]), int("cones" in c["has"]), int("lin" in c["has"])
    return dict(max_iter=max_iter, en_state_bound=box, en_input_bound=box, en_state_soc=cones, en_input_soc=cones, en_state_linear=lin, en_input_linear=lin)


def make(c, group=False):
    """a handle for case c with everything but the disturbance set"""
    if group:
        s = tm.TinyGroupSolver.from_problem(c["fams"][0], c["B"], devices=[0, 0], n_shards=2, interleaved=True)
    elif c["hetero"]:
        s = tm.TinyBatchSolver.hetero(*[np.stack([f[k] for f in c["fams"]]) for k in ("A", "B", "f", "Q", "R")], np.array([f["rho"] for f in c["fams"]]), c["N"])
    else:
        s = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    if "box" in c["has"]:
        if "box" in c["own"]:
            s.set_instance_bounds(*c["box"])
        else:
            s.set_bound_constraints(*[a[0] for a in c["box"]])
    if "cones" in c["has"]:
        s.set_cone_constraints(c["Acx"], [3], c["cx"][0], c["Acu"], [3], c["cu"][0])
        if "cones" in c["own"]:
            s.set_instance_cone_coefficients(c["cx"], c["cu"])
    if "lin" in c["has"]:
        s.set_instance_linear_constraints(*c["linear"])
    s.update_settings(**settings(c))
    s.set_x0(c["x0"])
    s.set_x_ref(c["Xref"])
    s.set_u_ref(c["Uref"])
    if c["option"]:
        s.set_option(c["option"], 1)
    return s


def snapshot(s, keys):
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


def assert_applied(s, path, steps=N_STEPS):
    """the last solve's launches applied the sequence on the kernel `path` names, on full rows and not in the PREFETCH form"""
    assert (s.get_option("disturbance"), s.get_option("last_disturbance")) == (steps, 1), (s.get_option("disturbance"), s.get_option("last_disturbance"))
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


def assert_host_form(r):
    """the reference handle: nothing installed, nothing applied, never the coverage kernel by accident of a sequence"""
    assert (r.get_option("disturbance"), r.get_option("last_disturbance"), r.get_option("disturbance_step")) == (0, 0, 0)


def fused(s, steps=T):
    s.set_option("steps_per_launch", steps)
    s.set_option("step_log", 1)
    s.solve()
    it, u0 = s.step_log(steps)
    return it.copy(), u0.copy()


def host_loop(r, w, steps=T, k0=0):
    """the host-in-the-loop form on handle r (no sequence installed): `steps` single-step solves, x0 = get("x")[:, :, 1] + w[k] added in
    numpy for the rows k0 + step that exist (none: the undisturbed x1).  -> (iteration log [steps, B], u0 log [steps, B, nu])"""
    its, u0s = [], []
    for step in range(steps):
        r.solve()
        st = r.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0s.append(r.get("u")[:, :, 0].copy())
        x1 = r.get("x")[:, :, 1]
        k = k0 + step
        r.set_x0(x1 + w[k] if 0 <= k < len(w) else x1)
    return np.array(its), np.array(u0s)


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(dc.CASES))
def test_every_instance_follows_its_own_oracle_loop(name):
    dc.check_case(name)                                              # (the oracle alone: before anything runs on the GPU)
    c, want = dc.case(name), dc.oracle_case(name)
    keys = dc.keys(c)
    s = make(c)
    s.set_disturbance(c["w"])
    it, u0 = fused(s)
    got = snapshot(s, keys)
    assert_applied(s, c["path"])
    assert s.get_option("disturbance_step") == T
    assert s.get_option("last_instance_bounds") == int("box" in c["own"]) and s.get_option("last_instance_linear") == int("lin" in c["own"])
    assert s.get_option("last_instance_cones") == int("cones" in c["own"])
    for i in range(c["B"]):
        assert np.array_equal(it[:, i], want[i]["iter"]), (i, it[:, i], want[i]["iter"])
        for k in keys:
            e = rel_err(got[k][i], want[i]["rec"][k])
            assert e < RTOL, (i, k, e)
        assert rel_err(u0[:, i], want[i]["u0"]) < RTOL and rel_err(got["x0"][i], want[i]["x0"]) < RTOL, i
    s.close()


# ---- b. launch forms against the host-in-the-loop form: 6_3_10_box (iteration counts from 6 to the cap) ---------------------------------
TRAJ_POINTS = 30


def _traj(c):
    rng = np.random.default_rng(99)
    return rng.normal(0, 0.2, (TRAJ_POINTS, c["nx"])), rng.integers(0, 5, c["B"]).astype(np.int32)


def _fused(s, c):
    return fused(s)


def _advance(s, c):
    s.set_option("advance_x0", 1)
    its, u0s = [], []
    for _ in range(T):
        s.solve()
        st = s.status()
        its.append(np.where(st["solved"] != 0, st["iter"], -st["iter"]).astype(np.int32))
        u0s.append(s.get("u")[:, :, 0].copy())
    return np.array(its), np.array(u0s)


def _regroup(streams):
    def drive(s, c):
        s.set_option("step_regroup", 2)
        s.set_option("step_regroup_streams", streams)
        out = fused(s)
        assert s.get_option("step_regroup_stretches") > 1
        return out
    return drive


def _option(name, value):
    def drive(s, c):
        s.set_option(name, value)
        return fused(s)
    return drive


def _trajectory(s, c):
    traj, offs = _traj(c)
    s.set_reference_trajectory(traj, offs)
    return fused(s)


def _host_trajectory(r, c):
    traj, offs = _traj(c)
    r.set_reference_trajectory(traj, offs)


# drive on the handle with the sequence; what the host-in-the-loop handle sets before its loop (the same option, where it has a meaning
# for single-step solves); the records compared.  one_shot = 1: the fused launch takes the warm-start state as zero ONCE, at its first
# step, and promises x | u and vnew | znew only -- the host loop starts from a fresh handle, whose state is zero, without the option
FORMS = {
    "fused": (_fused, None, None),
    "advance_x0": (_advance, None, None),
    "step_regroup": (_regroup(1), None, None),
    "step_regroup_two_streams": (_regroup(2), None, None),
    "trajectory": (_trajectory, _host_trajectory, None),
    "one_shot": (_option("one_shot", 1), None, ("x", "u", "vnew", "znew")),
    "grid_waves_per_cu": (_option("grid_waves_per_cu", 1), lambda r, c: r.set_option("grid_waves_per_cu", 1), None),
    "launch_order": (_option("launch_order", 2), lambda r, c: r.set_option("launch_order", 2), None),
    "reset_duals": (_option("reset_duals", 1), lambda r, c: r.set_option("reset_duals", 1), None),
}


# (step_regroup is a launch form of the one-row kernel: the coverage kernel runs fused steps one by one, whatever the option says)
@pytest.mark.parametrize("name,form", [("6_3_10_box", f) for f in FORMS] + [("20_4_10", f) for f in FORMS if not f.startswith("step_regroup")])
def test_launch_forms_equal_the_host_in_the_loop_form_bit_for_bit(name, form):
    c = dc.case(name)
    drive, host_setup, only = FORMS[form]
    keys = dc.keys(c) if only is None else only
    s = make(c)
    s.set_disturbance(c["w"])
    it, u0 = drive(s, c)
    got = dict(snapshot(s, keys), log_iter=it, log_u0=u0)
    assert_applied(s, c["path"])
    assert s.get_option("disturbance_step") == T
    s.close()
    r = make(c)
    if c["path"] == "cover":
        r.set_option("force_general", 1)                             # (bit for bit: the same kernel on both sides -- without a sequence the shape runs on the tile kernel)
    if host_setup:
        host_setup(r, c)
    rit, ru0 = host_loop(r, c["w"])
    want = dict(snapshot(r, keys), log_iter=rit, log_u0=ru0)
    assert_host_form(r)
    assert r.kernel_path() == ("cover" if c["path"] == "cover" else "regs"), r.kernel_path()
    r.close()
    assert_same_bits(got, want, (name, form))


# ---- c. composition ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dc.COMPOSITION)
def test_pd_composes_with_the_per_instance_forms(name):
    c = dc.case(name)
    keys = dc.keys(c)
    s = make(c)
    s.set_disturbance(c["w"])
    it, u0 = fused(s)
    got = dict(snapshot(s, keys), log_iter=it, log_u0=u0)
    assert_applied(s, c["path"])
    assert (s.get_option("last_instance_bounds"), s.get_option("last_instance_linear"), s.get_option("last_instance_cones")) == \
        (int("box" in c["own"]), int("lin" in c["own"]), int("cones" in c["own"]))
    s.close()
    r = make(c)
    rit, ru0 = host_loop(r, c["w"])
    want = dict(snapshot(r, keys), log_iter=rit, log_u0=ru0)
    assert_host_form(r)
    assert r.kernel_path() == c["path"], r.kernel_path()              # (the per-instance forms are run-time instantiated without a sequence, too)
    r.close()
    assert_same_bits(got, want, name)


# ---- d. the counter -----------------------------------------------------------------------------------------------------------------
def _episode(c, keys, w, steps, prepare=None, between=None):
    """fused launches of `steps` (a list) on a fresh handle under w; prepare(s) in front, between(s, launch) in front of each launch"""
    s = make(c)
    s.set_disturbance(w)
    if prepare:
        prepare(s)
    logs = []
    for n, st in enumerate(steps):
        if between:
            between(s, n)
        logs.append(fused(s, st))
    out = dict(snapshot(s, keys), log_iter=np.concatenate([l[0] for l in logs]), log_u0=np.concatenate([l[1] for l in logs]))
    return s, out


def _host_episode(c, keys, w, rows):
    """the host-in-the-loop form with row rows[step] added behind step `step` (a row outside the sequence: none)"""
    r = make(c)
    its, u0s = [], []
    for k in rows:
        i1, u1 = host_loop(r, w, steps=1, k0=k)
        its.append(i1[0]); u0s.append(u1[0])
    out = dict(snapshot(r, keys), log_iter=np.array(its), log_u0=np.array(u0s))
    assert_host_form(r)
    r.close()
    return out


def test_counter_set_mid_episode_short_sequence_negative_rows_and_reset():
    c = dc.case("6_3_10_box")
    keys = dc.keys(c)
    w = c["w"]
    # two launches of 2 and 3 steps, the counter moved to 3 in front of the second: rows 0, 1, then 3, none, none
    def jump(s, n):
        if n == 1:
            assert s.get_option("disturbance_step") == 2
            s.set_option("disturbance_step", 3)
    s, got = _episode(c, keys, w, [2, 3], between=jump)
    assert_applied(s, "jit")
    assert s.get_option("disturbance_step") == 6
    s.close()
    assert_same_bits(got, _host_episode(c, keys, w, rows=[0, 1, 3, 4, 5]), "disturbance_step set mid-episode")
    # a sequence shorter than the episode: behind it the loop is the undisturbed one, bit for bit -- the PD form from the state the
    # disturbed steps left against the form without a sequence from that very state
    s, _ = _episode(c, keys, w[:2], [2])
    assert_applied(s, "jit", steps=2)
    mid = snapshot(s, keys)
    it, u0 = fused(s, 3)
    tail = dict(snapshot(s, keys), log_iter=it, log_u0=u0)
    assert_applied(s, "jit", steps=2)
    assert s.get_option("disturbance_step") == 5
    s.close()
    s, _ = _episode(c, keys, w[:2], [2])
    assert_same_bits(snapshot(s, keys), mid, "the same two steps")
    s.set_disturbance(None)
    assert s.get_option("disturbance") == 0
    it, u0 = fused(s, 3)
    assert s.get_option("last_disturbance") == 0 and s.kernel_path() == "regs" and s.get_option("disturbance_step") == 0
    assert_same_bits(tail, dict(snapshot(s, keys), log_iter=it, log_u0=u0), "the tail behind a short sequence")
    s.close()
    # a negative counter: rows -2, -1 add nothing, then rows 0, 1, 2
    s, got = _episode(c, keys, w, [5], prepare=lambda s: s.set_option("disturbance_step", -2))
    assert_applied(s, "jit")
    assert s.get_option("disturbance_step") == 3
    assert_same_bits(got, _host_episode(c, keys, w, rows=[-2, -1, 0, 1, 2]), "a negative counter")
    # tiny_batch_reset leaves sequence and counter alone; the setter rewinds the counter
    s.reset()
    assert (s.get_option("disturbance"), s.get_option("disturbance_step")) == (N_STEPS, 3)
    s.set_disturbance(w)
    assert s.get_option("disturbance_step") == 0
    s.close()


def test_a_launch_without_a_plant_step_reads_nothing_and_runs_the_form_it_ran():
    for name in ("6_3_10_box", "4_2_10"):
        c = dc.case(name)
        keys = dc.keys(c)
        s, r = make(c), make(c)
        s.set_disturbance(c["w"])
        s.set_option("disturbance_step", 1)
        for h in (s, r):
            h.solve()
            h.set_x0(c["x0"] * 0.9)
            h.solve()
        assert (s.get_option("disturbance"), s.get_option("last_disturbance"), s.get_option("disturbance_step")) == (N_STEPS, 0, 1)
        assert s.kernel_path() == r.kernel_path() == "regs"
        assert s.get_option("last_half_rows") == r.get_option("last_half_rows") and s.get_option("last_prefetch") == r.get_option("last_prefetch")
        assert_same_bits(snapshot(s, keys), snapshot(r, keys), name)
        s.close()
        r.close()


def test_a_half_row_shape_takes_full_rows_while_the_sequence_applies():
    c = dc.case("4_2_10")
    r = make(c)
    r.solve()
    assert r.get_option("last_half_rows") == 1                       # (what the shape runs on without a plant step)
    r.close()
    s = make(c)
    s.set_disturbance(c["w"])
    fused(s)
    assert_applied(s, "jit")
    s.close()


# ---- e. the setter ------------------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime the library itself is linked against (already loaded with it: the same handle)"""
    for name in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise OSError("libamdhip64 not found")


def _run(s, keys):
    it, u0 = fused(s)
    return dict(snapshot(s, keys), log_iter=it, log_u0=u0)


def test_broadcast_device_pointers_getter_removal_and_a_failed_call():
    c = dc.case("6_3_10_box")
    keys, B, nx = dc.keys(c), c["B"], c["nx"]
    one = np.ascontiguousarray(c["w"][:, 3])                         # [N_STEPS, nx]: one sequence for all
    full = np.ascontiguousarray(np.broadcast_to(one[:, None, :], c["w"].shape))
    a, b = make(c), make(c)
    a.set_disturbance(one)
    b.set_disturbance(full)
    for i in (0, B - 1):
        for k in (0, N_STEPS - 1):
            assert np.array_equal(a.get_disturbance(k, i), one[k]) and np.array_equal(b.get_disturbance(k, i), one[k])
    bc = _run(a, keys)
    assert_applied(a, "jit")
    assert_same_bits(bc, _run(b, keys), "TINY_BROADCAST against the expanded array")
    a.close()
    b.close()
    # device pointers give the same bits as host arrays; the caller's buffer is freed right after the call
    a, b = make(c), make(c)
    a.set_disturbance(c["w"])
    hip = _hip_runtime()
    flat = np.ascontiguousarray(c["w"]).ravel()
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(flat.nbytes)) == 0
    assert hip.hipMemcpy(p, flat.ctypes.data_as(C.c_void_p), C.c_size_t(flat.nbytes), 1) == 0      # hipMemcpyHostToDevice
    b.set_disturbance_device(p.value, N_STEPS)
    assert hip.hipFree(p) == 0
    for i in (0, 5, B - 1):
        assert np.array_equal(b.get_disturbance(2, i), c["w"][2, i])
    own = _run(a, keys)
    assert_same_bits(own, _run(b, keys), "TINY_DEVICE against TINY_HOST")
    assert_applied(b, "jit")
    # the getter's refusals
    L = tm.lib()
    out = np.zeros(nx)
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert L.tiny_batch_get_disturbance(b._h, N_STEPS, 0, dp) == tm.ERR_ARG and L.tiny_batch_get_disturbance(b._h, -1, 0, dp) == tm.ERR_ARG
    assert L.tiny_batch_get_disturbance(b._h, 0, B, dp) == tm.ERR_ARG and L.tiny_batch_get_disturbance(b._h, 0, 0, None) == tm.ERR_ARG
    # a failed call leaves what was installed: a sequence no device memory holds
    b.set_option("disturbance_step", 2)
    rc = L.tiny_batch_set_disturbance(b._h, flat.ctypes.data_as(C.c_void_p), 2**31 - 1, tm.HOST | tm.BROADCAST)
    assert rc not in (tm.OK,), rc
    assert (b.get_option("disturbance"), b.get_option("disturbance_step")) == (N_STEPS, 2)
    assert np.array_equal(b.get_disturbance(1, 4), c["w"][1, 4])
    # removal: by None, and by n_steps = 0
    b.set_disturbance(None)
    assert (b.get_option("disturbance"), b.get_option("disturbance_step")) == (0, 0)
    assert L.tiny_batch_get_disturbance(b._h, 0, 0, dp) == tm.ERR_ARG
    assert L.tiny_batch_set_disturbance(a._h, flat.ctypes.data_as(C.c_void_p), 0, tm.HOST) == tm.OK and a.get_option("disturbance") == 0
    # ... after which the loop is the undisturbed one on the compiled-in form
    b.reset()
    b.set_x0(c["x0"])
    free = _run(b, keys)
    assert b.get_option("last_disturbance") == 0 and b.kernel_path() == "regs"
    assert not np.array_equal(free["x0"], own["x0"])
    a.close()
    b.close()


def test_adaptive_rho_is_refused_on_a_launch_with_a_plant_step_only():
    c = dc.case("6_3_10_b2")
    L = tm.lib()
    s = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    s.update_settings(max_iter=dc.MAX_ITER, en_state_bound=0, en_input_bound=0)
    s.set_x0(c["x0"])
    s.set_disturbance(c["w"])
    s.set_adaptive_rho(1)
    s.solve()                                                        # no plant step: the sequence does not apply, adaptive rho runs
    assert s.get_option("last_disturbance") == 0
    s.set_option("advance_x0", 1)
    assert L.tiny_batch_solve(s._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(s._h).decode()
    assert "adaptive rho does not combine with a per-instance disturbance" in msg, msg
    assert s.get_option("disturbance_step") == 0
    s.set_adaptive_rho(0)
    s.solve()
    assert_applied(s, "jit")
    assert s.get_option("disturbance_step") == 1
    s.close()


# ---- f. a group of two shards on one GPU, round-robin, the sequence in the caller's order ------------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    c = dc.case("5_3_7")                                             # 11 instances: shards of 6 and 5
    keys = dc.keys(c)
    g, s = make(c, group=True), make(c)
    g.set_disturbance(c["w"])
    s.set_disturbance(c["w"])
    for h in (g, s):
        h.set_option("steps_per_launch", 3)
        h.solve()
        h.set_option("disturbance_step", 1)                          # (forwarded to every shard)
        h.solve()
    st, gst = s.status(), g.status()
    for k in keys + ("x0",):
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(gst["iter"], st["iter"]) and np.array_equal(gst["solved"], st["solved"])
    assert_applied(s, "jit")
    assert s.get_option("disturbance_step") == 4
    for k in range(g.shards):
        h = tm.lib().tiny_group_shard(g._h, k)
        opt = lambda n: int(tm.lib().tiny_batch_get_option(h, n))
        assert (opt(b"disturbance"), opt(b"last_disturbance"), opt(b"disturbance_step"), tm.lib().tiny_batch_kernel_path(h)) == (N_STEPS, 1, 4, 3)
    for i in (0, 1, 10):
        assert np.array_equal(g.get_disturbance(2, i), c["w"][2, i])
    g.close()
    s.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------------
def test_monte_carlo_example_spreads_the_final_states_under_noise_only():
    """examples/monte_carlo_closed_loop.c (C99, built by __graft_entry__.build()): 4 096 double integrators from one state, 60 fused steps
    under per-instance gusts on a PD form, then without them on the compiled-in form; its exit status checks the two spreads"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "monte_carlo_closed_loop")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/monte_carlo_closed_loop is missing: __graft_entry__.build() produces it")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    lines = p.stdout.splitlines()
    assert "kernel path 3, disturbance applied 1, rows used 60" in lines[0] and "kernel path 0, disturbance applied 0, rows used 0" in lines[2], p.stdout
