"""GPU tests of per-instance cone coefficients (tiny_batch_set_instance_cone_coefficients): the one-row kernel's PC forms and the
coverage kernel's per-instance read.  Batches of 2 to 13: up to four tiles, the last one with 3 rows, 2 or 1.
  a. one coefficient for all through the instance setter equals the shared setter bit for bit (cold and warm), on a one-row form and
     on the coverage kernel;
  b. every instance against its own oracle under its own coefficients (tests/instance_cone_cases.py asserts, from the oracle alone,
     that a coefficient read from the wrong instance, cone or lane moves the result), cold and warm, on every case;
  c. every launch form against 13 single-instance handles that use the SHARED setter;
  d. setter semantics: latest wins in both directions, NULL for one family, the getter, device pointers, reset, the switches;
  e. refusals;  f. a sharded group."""
import ctypes as C

import numpy as np
import pytest

import instance_cone_cases as icc
import tinympc_amd as tm

pytestmark = pytest.mark.gpu
RESID = ("primal_residual_state", "primal_residual_input", "dual_residual_state", "dual_residual_input")
RTOL = 1e-9                                        # the project's parity contract (README.md)


def settings(c, on=None, max_iter=icc.MAX_ITER):
    on = c["on"] if on is None else on
    box, lin = int(c["box"] is not None), int(c["linear"] is not None)
    return dict(max_iter=max_iter, en_state_bound=box, en_input_bound=box, en_state_soc=on[0], en_input_soc=on[1], en_state_linear=lin, en_input_linear=lin)


def make(c, only=None, group=False, coef_of=0):
    """a handle for case c: the whole batch, or (only = i) instance i alone, with the cones of the case under the SHARED coefficients of
    instance coef_of (only = i: of instance i); the per-instance ones are the caller's to set"""
    idx = list(range(c["B"])) if only is None else [only]
    if group:
        s = tm.TinyGroupSolver.from_problem(c["fams"][0], c["B"], devices=[0, 0], n_shards=2, interleaved=True)
    elif c["hetero"]:
        fams = [c["fams"][i] for i in idx]
        s = tm.TinyBatchSolver.hetero(*[np.stack([f[k] for f in fams]) for k in ("A", "B", "f", "Q", "R")], np.array([f["rho"] for f in fams]), c["N"])
    else:
        s = tm.TinyBatchSolver.from_problem(c["fams"][0], len(idx))
    j = coef_of if only is None else only
    s.set_cone_constraints(c["Acx"], [3] * len(c["Acx"]), c["cx"][j], c["Acu"], [3] * len(c["Acu"]), c["cu"][j])
    s.update_settings(**settings(c))
    s.set_x0(c["x0"][idx])
    s.set_x_ref(c["Xref"][idx])
    s.set_u_ref(c["Uref"][idx])
    if c["extra"] == "force_general":
        s.set_option("force_general", 1)
    return s


def set_rest(s, c):
    """what the case sets besides the cones: every instance its own half-spaces / box"""
    if c["linear"] is not None:
        s.set_instance_linear_constraints(*c["linear"])
    if c["box"] is not None:
        s.set_instance_bounds(*c["box"])


def snapshot(s, keys):
    st = s.status()
    out = {k: s.get(k) for k in keys}
    out.update(iter=st["iter"].copy(), solved=st["solved"].copy(), **{k: st[k].copy() for k in RESID})
    return out


def assert_same_bits(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k, float(np.max(np.abs(np.asarray(a[k], dtype=float) - np.asarray(b[k], dtype=float)))))


def rel_err(a, b):
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def assert_form(s, path, read=1):
    """the last solve read the per-instance coefficients on the kernel `path` names -- so that no test passes on the wrong path"""
    assert s.get_option("instance_cones") == 1 and s.get_option("last_instance_cones") == read, (s.get_option("instance_cones"), s.get_option("last_instance_cones"))
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["6_3_10_both", "12_4_10_hetero", "6_3_10_force_general", "12_4_10_overlap"])
def test_one_coefficient_for_all_through_the_instance_setter_equals_the_shared_setter(name):
    c = icc.case(name)
    keys = icc.keys(c)
    s, ref = make(c, coef_of=3), make(c, coef_of=0)                     # (s: the shared coefficients are NOT the ones it is held to below)
    if c["path"] == "cover":
        ref.set_option("force_general", 1)                           # (bit for bit: the same kernel on both sides)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[0], a.shape))
    s.set_instance_cone_coefficients(rep(c["cx"]), rep(c["cu"]))
    for scale, what in ((1.0, "cold"), (0.9, "warm")):
        for h in (s, ref):
            h.set_x0(c["x0"] * scale)
            h.solve()
        assert_form(s, c["path"])
        assert ref.get_option("instance_cones") == 0 and ref.get_option("last_instance_cones") == 0
        assert ref.kernel_path() in (("cover",) if c["path"] == "cover" else ("regs", "jit"))
        assert_same_bits(snapshot(s, keys), snapshot(ref, keys), (name, what))
    s.close()
    ref.close()


# ---- b. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(icc.CASES))
def test_every_instance_against_its_own_oracle_under_its_own_coefficients(name):
    icc.check_case(name)                                             # (the oracle alone: before anything runs on the GPU)
    c, want = icc.case(name), icc.oracle_case(name)
    keys = icc.keys(c)
    s = make(c, coef_of=(c["B"] - 1))
    set_rest(s, c)
    s.set_instance_cone_coefficients(c["cx"], c["cu"])
    got = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"] * scale)
        s.solve()
        got.append(snapshot(s, keys))
    assert_form(s, c["path"])
    assert s.get_option("last_instance_bounds") == int(c["box"] is not None) and s.get_option("last_instance_linear") == int(c["linear"] is not None)
    for i in range(c["B"]):
        for k_solve, what in ((0, "cold"), (1, "warm")):
            rec, it, solved = want[i][k_solve]
            assert (it, solved) == (got[k_solve]["iter"][i], got[k_solve]["solved"][i]), (i, what)
            for k in keys:
                e = rel_err(got[k_solve][k][i], rec[k])
                assert e < RTOL, (i, what, k, e)
    s.close()


# ---- c. launch forms: 6_3_10_both -----------------------------------------------------------------------------------------------------
TRAJ_POINTS = 30


def _traj(c):
    rng = np.random.default_rng(99)
    return rng.normal(0, 0.2, (TRAJ_POINTS, c["nx"])), rng.integers(0, 5, c["B"]).astype(np.int32)


def _drive_scales(s, c, idx, keys, scales=(1.0, 0.9)):
    out = []
    for scale in scales:
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s, keys))
    return out


def _drive_two_warm(s, c, idx, keys):
    return _drive_scales(s, c, idx, keys, (1.0, 0.9, 0.8))           # cold, then two warm launches: the third walks the batch in reverse again


def _drive_fused(s, c, idx, keys):
    s.set_option("steps_per_launch", 5)
    s.set_option("step_log", 1)
    s.solve()
    it, u0 = s.step_log(5)
    return [dict(snapshot(s, keys), log_iter=it.T.copy(), log_u0=u0.transpose(1, 0, 2).copy(), x0=s.get("x0"))]


def _drive_advance(s, c, idx, keys):
    s.set_option("advance_x0", 1)
    out = []
    for _ in range(2):
        s.solve()
        out.append(dict(snapshot(s, keys), x0=s.get("x0")))
    return out


def _drive_one_shot(s, c, idx, keys):
    s.set_option("one_shot", 1)
    s.solve()
    return [snapshot(s, ("x", "u", "vnew", "znew"))]


def _drive_traj(s, c, idx, keys):
    traj, offs = _traj(c)
    s.set_reference_trajectory(traj, offs[idx])
    s.set_option("steps_per_launch", 3)
    out = []
    for _ in range(2):
        s.solve()
        out.append(dict(snapshot(s, keys), x0=s.get("x0")))
    return out


def _drive_reset_duals(s, c, idx, keys):
    s.set_option("reset_duals", 1)
    return _drive_scales(s, c, idx, keys)


def _drive_repack(s, c, idx, keys):
    if len(idx) > 1:
        s.set_option("repack_after", 10)                             # (a single-instance handle solves unsplit: the split is bit-identical)
    s.solve()
    out = snapshot(s, keys)
    if len(idx) > 1:
        assert out["iter"].min() < 10 < out["iter"].max(), out["iter"]     # the batch straddles the split point
    return [out]


def _drive_regroup(s, c, idx, keys):
    s.set_option("steps_per_launch", 8)
    s.set_option("step_log", 1)
    if len(idx) > 1:
        s.set_option("step_regroup", 2)
    s.solve()
    if len(idx) > 1:
        assert s.get_option("step_regroup_stretches") > 1
    it, u0 = s.step_log(8)
    return [dict(snapshot(s, keys), log_iter=it.T.copy(), log_u0=u0.transpose(1, 0, 2).copy(), x0=s.get("x0"))]


def _drive_capped_grid(s, c, idx, keys):
    s.set_option("grid_waves_per_cu", 1)
    return _drive_scales(s, c, idx, keys)


def _drive_descending(s, c, idx, keys):
    s.set_option("launch_order", 2)
    return _drive_scales(s, c, idx, keys)


DRIVES = {"two_warm": _drive_two_warm, "fused_steps": _drive_fused, "advance_x0": _drive_advance, "one_shot": _drive_one_shot, "trajectory": _drive_traj,
          "reset_duals": _drive_reset_duals, "repack_after": _drive_repack, "step_regroup": _drive_regroup, "grid_waves_per_cu": _drive_capped_grid,
          "launch_order": _drive_descending}


@pytest.mark.parametrize("drive", list(DRIVES))
def test_launch_forms_equal_single_instance_handles_with_the_shared_setter(drive):
    c = icc.launch_case()
    B, keys = c["B"], icc.keys(c)
    s = make(c)
    s.set_instance_cone_coefficients(c["cx"], c["cu"])
    got = DRIVES[drive](s, c, list(range(B)), keys)
    assert_form(s, "jit")
    s.close()
    singles = []
    for i in range(B):
        r = make(c, only=i)
        singles.append(DRIVES[drive](r, c, [i], keys))
        assert r.get_option("instance_cones") == 0 and r.get_option("last_instance_cones") == 0
        r.close()
    for step, g in enumerate(got):
        want = {k: np.concatenate([singles[i][step][k] for i in range(B)]) for k in g}
        assert_same_bits(g, want, (drive, step))


# ---- d. setter semantics -----------------------------------------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime the library itself is linked against (already loaded with it: the same handle)"""
    for name in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise OSError("libamdhip64 not found")


def _solve_snapshot(s, c, keys):
    s.reset()
    s.set_x0(c["x0"])
    s.solve()
    return snapshot(s, keys)


def _shared_cones(s, c, i):
    s.set_cone_constraints(c["Acx"], [3] * len(c["Acx"]), c["cx"][i], c["Acu"], [3] * len(c["Acu"]), c["cu"][i])


def test_latest_setter_wins_and_null_keeps_the_shared_family():
    c = icc.case("6_3_10_both")
    keys, B = icc.keys(c), c["B"]
    rep = lambda a, i: np.ascontiguousarray(np.broadcast_to(a[i], a.shape))
    ref = make(c, coef_of=0)
    want0 = _solve_snapshot(ref, c, keys)
    s = make(c, coef_of=0)
    s.set_instance_cone_coefficients(c["cx"], c["cu"])
    own = _solve_snapshot(s, c, keys)
    assert_form(s, "jit")
    assert not np.array_equal(own["vcnew"], want0["vcnew"]) and not np.array_equal(own["zcnew"], want0["zcnew"])
    # a later instance setter replaces the earlier one
    s.set_instance_cone_coefficients(rep(c["cx"], 0), rep(c["cu"], 0))
    assert_same_bits(_solve_snapshot(s, c, keys), want0, "a second instance setter")
    assert_form(s, "jit")
    # a later shared setter drops the per-instance coefficients
    s.set_instance_cone_coefficients(c["cx"], c["cu"])
    _shared_cones(s, c, 0)
    assert s.get_option("instance_cones") == 0
    assert_same_bits(_solve_snapshot(s, c, keys), want0, "the shared setter after the instance setter")
    assert s.get_option("last_instance_cones") == 0 and s.kernel_path() in ("regs", "jit")
    # ... and the instance setter after it installs them again
    s.set_instance_cone_coefficients(c["cx"], c["cu"])
    assert_same_bits(_solve_snapshot(s, c, keys), own, "the instance setter after the shared setter")
    # NULL for one family keeps that family's shared coefficient for every instance: the state cones of all on instance 0's (shared)
    # coefficient, the input cones on their own -- against single-instance handles under exactly those shared numbers
    s.set_instance_cone_coefficients(None, c["cu"])
    mixed = _solve_snapshot(s, c, keys)
    assert_form(s, "jit")
    for i in (0, 5, B - 1):
        cx, cu = s.get_instance_cone_coefficients(i)
        assert np.array_equal(cx, c["cx"][0]) and np.array_equal(cu, c["cu"][i])
        r = tm.TinyBatchSolver.from_problem(c["fams"][0], 1)
        r.set_cone_constraints(c["Acx"], [3], c["cx"][0], c["Acu"], [3], c["cu"][i])
        r.update_settings(**settings(c))
        r.set_x_ref(c["Xref"][[i]])
        r.set_u_ref(c["Uref"][[i]])
        one = _solve_snapshot(r, dict(c, x0=c["x0"][[i]]), keys)
        assert_same_bits({k: v[[i]] for k, v in mixed.items()}, one, ("NULL state family", i))
        r.close()
    # ... and the other way round
    s.set_instance_cone_coefficients(c["cx"], None)
    cx, cu = s.get_instance_cone_coefficients(4)
    assert np.array_equal(cx, c["cx"][4]) and np.array_equal(cu, c["cu"][0])
    s.close()
    ref.close()


def test_getter_device_pointers_reset_and_the_switches():
    c = icc.case("6_3_10_both")
    keys, B = icc.keys(c), c["B"]
    a, b = make(c), make(c)
    # on a shared set the getter returns the shared values
    cx, cu = a.get_instance_cone_coefficients(B - 1)
    assert np.array_equal(cx, c["cx"][0]) and np.array_equal(cu, c["cu"][0])
    a.set_instance_cone_coefficients(c["cx"], c["cu"])
    # ... on a per-instance set what was set, whatever the switches say; either pointer may be NULL
    a.update_settings(**settings(c, on=(0, 0)))
    for i in (0, 6, B - 1):
        cx, cu = a.get_instance_cone_coefficients(i)
        assert np.array_equal(cx, c["cx"][i]) and np.array_equal(cu, c["cu"][i])
    out = np.zeros(1)
    assert tm.lib().tiny_batch_get_instance_cone_coefficients(a._h, 2, None, out.ctypes.data_as(C.POINTER(C.c_double))) == tm.OK and out[0] == c["cu"][2, 0]
    assert tm.lib().tiny_batch_get_instance_cone_coefficients(a._h, B, None, None) == tm.ERR_ARG
    # both families off: the coefficients stay installed, no kernel reads them
    a.set_x0(c["x0"])
    a.solve()
    assert a.get_option("instance_cones") == 1 and a.get_option("last_instance_cones") == 0
    a.update_settings(**settings(c))
    # device pointers give the same bits as host arrays; the caller's buffers are freed right after the call
    hip = _hip_runtime()
    dev = []
    for v in b._instance_cones(c["cx"], c["cu"]):
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(v.nbytes)) == 0
        assert hip.hipMemcpy(p, v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes), 1) == 0      # hipMemcpyHostToDevice
        dev.append(p)
    b.set_instance_cone_coefficients_device(dev[0].value, dev[1].value)
    for p in dev:
        assert hip.hipFree(p) == 0
    first = _solve_snapshot(a, c, keys)
    assert_same_bits(first, _solve_snapshot(b, c, keys), "TINY_DEVICE against TINY_HOST")
    assert_form(b, "jit")
    cx, cu = b.get_instance_cone_coefficients(7)
    assert np.array_equal(cx, c["cx"][7]) and np.array_equal(cu, c["cu"][7])
    # tiny_batch_reset leaves the coefficients alone
    assert_same_bits(_solve_snapshot(a, c, keys), first, "after a reset")
    assert_form(a, "jit")
    # one family switched off: the other one is still read per instance, as on single-instance handles with that switch off
    for on in ((1, 0), (0, 1)):
        a.update_settings(**settings(c, on=on))
        got = _solve_snapshot(a, c, keys)
        assert_form(a, "jit")
        r = make(c, only=3)
        r.update_settings(**settings(c, on=on))
        assert_same_bits({k: v[[3]] for k, v in got.items()}, _solve_snapshot(r, dict(c, x0=c["x0"][[3]]), keys), ("switches", on))
        r.close()
    a.close()
    b.close()


# ---- e. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = icc.case("6_3_10_both")
    L = tm.lib()
    flat = [np.ascontiguousarray(c["cx"]).ravel(), np.ascontiguousarray(c["cu"]).ravel()]
    ptrs = [v.ctypes.data for v in flat]
    f = L.tiny_batch_set_instance_cone_coefficients
    # no cone set installed
    s = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    assert f(s._h, ptrs[0], ptrs[1], tm.HOST) == tm.ERR_ARG
    assert s.get_option("instance_cones") == 0
    s.close()
    s = make(c)
    assert f(s._h, ptrs[0], ptrs[1], tm.HOST | tm.BROADCAST) == tm.ERR_ARG
    assert f(s._h, None, None, tm.HOST) == tm.ERR_ARG
    assert s.get_option("instance_cones") == 0
    # a failed call leaves what was installed
    s.set_instance_cone_coefficients(c["cx"], c["cu"])
    assert f(s._h, None, None, tm.HOST) == tm.ERR_ARG and f(s._h, ptrs[0], ptrs[1], tm.BROADCAST) == tm.ERR_ARG
    cx, cu = s.get_instance_cone_coefficients(5)
    assert s.get_option("instance_cones") == 1 and np.array_equal(cx, c["cx"][5]) and np.array_equal(cu, c["cu"][5])
    # adaptive rho
    s.set_adaptive_rho(1)
    assert L.tiny_batch_solve(s._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(s._h).decode()
    assert "adaptive rho does not combine with per-instance cone coefficients" in msg, msg
    s.set_adaptive_rho(0)
    s.solve()
    assert_form(s, "jit")
    s.close()


# ---- f. a group of two shards on one GPU, round-robin, coefficients in the caller's order ---------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    c = icc.case("5_3_7")                                            # 11 instances: shards of 6 and 5
    keys = icc.keys(c)
    g, s = make(c, group=True), make(c)
    g.set_instance_cone_coefficients(c["cx"], c["cu"])
    s.set_instance_cone_coefficients(c["cx"], c["cu"])
    g.solve()
    s.solve()
    st, gst = s.status(), g.status()
    for k in keys:
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(gst["iter"], st["iter"]) and np.array_equal(gst["solved"], st["solved"])
    assert_form(s, "jit")
    for i in (0, 1, 10):
        cx, cu = g.get_instance_cone_coefficients(i)
        assert np.array_equal(cx, c["cx"][i]) and np.array_equal(cu, c["cu"][i])
    g.close()
    s.close()
