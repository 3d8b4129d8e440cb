"""GPU tests of per-instance box constraints (tiny_batch_set_instance_bounds): the one-row kernel's PB forms and the coverage kernel's
per-instance read.  Batches of 11 or 13: the last tile of a launch has 3 rows or 1.
  a. the same box for every instance equals the shared setter bit for bit (cold and warm), on every shape class and both kernels;
  b. every instance against its own oracle under its own box, knot-invariant and with every bound pair distinct
     (tests/instance_bounds_cases.py asserts, from the oracle alone, that a bound read from the wrong instance, slot or lane moves
     the result), and the clamp of the first iteration bit for bit;
  c. every launch form of the box kernel against 13 single-instance handles that use the SHARED setter;
  d. the enable switches, replacement by the shared setter, device pointers, the getter;  e. refusals;  f. a sharded group."""
import ctypes as C

import numpy as np
import pytest

import instance_bounds_cases as ibc
import tinympc_amd as tm

pytestmark = pytest.mark.gpu
KEYS = ibc.KEYS
RESID = ("primal_residual_state", "primal_residual_input", "dual_residual_state", "dual_residual_input")
RTOL = 1e-9

# (nx, nu, N, per-instance problem data, batch, options of BOTH handles, expected kernel path with a per-instance box)
FORMS = {
    "12_4_10": (12, 4, 10, False, 13, {}, "jit"),
    "2_2_3": (2, 2, 3, False, 11, {}, "jit"),
    "8_8_10": (8, 8, 10, False, 11, {}, "jit"),                      # all 16 lanes in use
    "4_2_30": (4, 2, 30, False, 11, {}, "jit"),                      # one wave per SIMD; a HALF shape by default
    "6_3_10": (6, 3, 10, False, 13, {}, "jit"),                      # a HALF shape by default
    "hetero_ub": (12, 4, 10, True, 11, {"het_ub": 1}, "jit"),
    "hetero_noub": (12, 4, 10, True, 11, {"het_ub": 0}, "jit"),
    "3_2_2_no_jit": (3, 2, 2, False, 11, {"no_jit": 1}, "cover"),
    "20_8_10": (20, 8, 10, False, 11, {}, "cover"),
    # the extreme splits of a full row (instance_bounds_cases.EDGE_SHAPES): the field boundary of the [batch][16] lane blocks at lane 15 / lane 1
    "15_1_3": ibc.EDGE_SHAPES[0] + (False, 11, {}, "jit"),
    "1_15_3": ibc.EDGE_SHAPES[1] + (False, 11, {}, "jit"),
}


def make(c, batch=None, only=None):
    """a handle for case c: the whole batch, or (only = i) instance i alone"""
    idx = list(range(c["B"])) if only is None else [only]
    if c["hetero"]:
        fams = [c["fams"][i] for i in idx]
        s = tm.TinyBatchSolver.hetero(*[np.stack([f[k] for f in fams]) for k in ("A", "B", "f", "Q", "R")], np.array([f["rho"] for f in fams]), c["N"])
    else:
        s = tm.TinyBatchSolver.from_problem(c["fams"][0], len(idx))
    s.update_settings(max_iter=ibc.MAX_ITER)
    s.set_x0(c["x0"][idx])
    s.set_x_ref(c["Xref"][idx])
    s.set_u_ref(c["Uref"][idx])
    return s


def snapshot(s, keys=KEYS):
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


def assert_form(s, path, uniform):
    assert s.get_option("instance_bounds") == 1 and s.get_option("last_instance_bounds") == 1
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0
    assert s.kernel_path() == path
    assert s.get_option("last_uniform_bounds") == (1 if (uniform and path != "cover") else 0)


@pytest.mark.parametrize("form,varying", [(f, v) for f in FORMS for v in ((False, True) if f == "12_4_10" else (False,))])
def test_one_box_for_all_through_the_instance_setter_equals_the_shared_setter(form, varying):
    nx, nu, N, het, B, opts, path = FORMS[form]
    c = ibc.case(nx, nu, N, het, varying, B)
    box = [a[0] for a in c["box"]]                                   # instance 0's box for everybody
    s, ref = make(c), make(c)
    for h in (s, ref):
        for k, v in opts.items():
            h.set_option(k, v)
    ref.set_option("half_rows", 0)
    ref.set_option("prefetch", 0)
    if path == "cover":
        ref.set_option("force_general", 1)                           # (bit for bit: the same kernel on both sides)
    s.set_instance_bounds(*[np.broadcast_to(a, (B,) + a.shape) for a in box])
    ref.set_bound_constraints(*box)
    uniform = not varying and not (het and opts.get("het_ub") == 0)
    for scale, what in ((1.0, "cold"), (0.9, "warm")):
        for h in (s, ref):
            h.set_x0(c["x0"] * scale)
            h.solve()
        assert_form(s, path, uniform)
        assert ref.get_option("last_instance_bounds") == 0 and ref.get_option("instance_bounds") == 0
        assert ref.kernel_path() in (("cover",) if path == "cover" else ("regs", "jit"))
        assert_same_bits(snapshot(s), snapshot(ref), (form, what))
    s.close()
    ref.close()


@pytest.mark.parametrize("varying", [False, True])
@pytest.mark.parametrize("form", list(FORMS))
def test_every_instance_against_its_own_oracle_under_its_own_box(form, varying):
    nx, nu, N, het, B, opts, path = FORMS[form]
    ibc.check_case(nx, nu, N, het, varying, B)                       # (the oracle alone: before anything runs on the GPU)
    c, want = ibc.case(nx, nu, N, het, varying, B), ibc.oracle_case(nx, nu, N, het, varying, B)
    s = make(c)
    for k, v in opts.items():
        s.set_option(k, v)
    s.set_instance_bounds(*c["box"])
    got = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"] * scale)
        s.solve()
        got.append(snapshot(s))
    assert_form(s, path, not varying and not (het and opts.get("het_ub") == 0))
    for i in range(B):
        for k_solve, what in ((0, "cold"), (1, "warm")):
            rec, it, solved = want[i][k_solve]
            assert (it, solved) == (got[k_solve]["iter"][i], got[k_solve]["solved"][i]), (i, what)
            for k in KEYS:
                e = rel_err(got[k_solve][k][i], rec[k])
                assert e < RTOL, (i, what, k, e)
    # one iteration from zero duals: vnew = min(max(x, lo_i), hi_i) bit for bit, from the solve's own x (finite non-zero bounds)
    s.reset()
    s.update_settings(max_iter=1)
    s.set_x0(c["x0"])
    s.solve()
    x, u, vnew, znew = (s.get(k) for k in ("x", "u", "vnew", "znew"))
    assert all(np.all(np.isfinite(a)) and np.all(a != 0.0) for a in c["box"])
    assert np.array_equal(vnew, np.minimum(np.maximum(x, c["box"][0]), c["box"][1]))
    assert np.array_equal(znew, np.minimum(np.maximum(u, c["box"][2]), c["box"][3]))
    assert np.any(vnew != x) and np.any(znew != u)
    s.close()


# ---- c. launch forms: (12,4,10), batch 13, every bound pair distinct -------------------------------------------------------------
TRAJ_POINTS = 30


def _traj(c):
    rng = np.random.default_rng(99)
    return rng.normal(0, 0.2, (TRAJ_POINTS, c["nx"])), rng.integers(0, 5, c["B"]).astype(np.int32)


def _drive_two_warm(s, c, idx):
    out = []
    for scale in (1.0, 0.9, 0.8):                                    # cold, then two warm launches: the third walks the batch in reverse again
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s))
    return out


def _drive_fused(s, c, idx):
    s.set_option("steps_per_launch", 5)
    s.set_option("step_log", 1)
    s.solve()
    it, u0 = s.step_log(5)
    return [dict(snapshot(s), log_iter=it.T.copy(), log_u0=u0.transpose(1, 0, 2).copy(), x0=s.get("x0"))]


def _drive_advance(s, c, idx):
    s.set_option("advance_x0", 1)
    out = []
    for _ in range(2):
        s.solve()
        out.append(dict(snapshot(s), x0=s.get("x0")))
    return out


def _drive_one_shot(s, c, idx):
    s.set_option("one_shot", 1)
    s.solve()
    return [snapshot(s, ("x", "u", "vnew", "znew"))]


def _drive_traj(s, c, idx):
    traj, offs = _traj(c)
    s.set_reference_trajectory(traj, offs[idx])
    s.set_option("steps_per_launch", 3)
    out = []
    for _ in range(2):
        s.solve()
        out.append(dict(snapshot(s), x0=s.get("x0")))
    return out


def _drive_reset_duals(s, c, idx):
    s.set_option("reset_duals", 1)
    out = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s))
    return out


def _drive_repack(s, c, idx):
    if len(idx) > 1:
        s.set_option("repack_after", 10)                             # (a single-instance handle solves unsplit: the split is bit-identical)
    s.solve()
    out = snapshot(s)
    if len(idx) > 1:
        assert out["iter"].min() < 10 < out["iter"].max(), out["iter"]     # the batch straddles the split point
    return [out]


def _drive_regroup(s, c, idx):
    s.set_option("steps_per_launch", 8)
    s.set_option("step_log", 1)
    if len(idx) > 1:
        s.set_option("step_regroup", 2)
    s.solve()
    if len(idx) > 1:
        assert s.get_option("step_regroup_stretches") > 1
    it, u0 = s.step_log(8)
    return [dict(snapshot(s), log_iter=it.T.copy(), log_u0=u0.transpose(1, 0, 2).copy(), x0=s.get("x0"))]


def _drive_capped_grid(s, c, idx):
    s.set_option("grid_waves_per_cu", 1)
    out = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s))
    return out


DRIVES = {"two_warm": _drive_two_warm, "fused_steps": _drive_fused, "advance_x0": _drive_advance, "one_shot": _drive_one_shot, "trajectory": _drive_traj,
          "reset_duals": _drive_reset_duals, "repack_after": _drive_repack, "step_regroup": _drive_regroup, "grid_waves_per_cu": _drive_capped_grid}


@pytest.mark.parametrize("drive", list(DRIVES))
def test_launch_forms_equal_single_instance_handles_with_the_shared_setter(drive):
    c = ibc.launch_case()
    B = c["B"]
    s = make(c)
    s.set_instance_bounds(*c["box"])
    got = DRIVES[drive](s, c, list(range(B)))
    assert_form(s, "jit", False)
    s.close()
    singles = []
    for i in range(B):
        r = make(c, only=i)
        r.set_option("prefetch", 0)
        r.set_bound_constraints(*[a[i] for a in c["box"]])
        singles.append(DRIVES[drive](r, c, [i]))
        assert r.get_option("instance_bounds") == 0 and r.get_option("last_instance_bounds") == 0
        r.close()
    for step, g in enumerate(got):
        want = {k: np.concatenate([singles[i][step][k] for i in range(B)]) for k in g}
        assert_same_bits(g, want, (drive, step))


# ---- d. switches and replacement ---------------------------------------------------------------------------------------------------
def _hip_runtime():
    """the HIP runtime the library itself is linked against (already loaded with it: the same handle)"""
    for name in ("libamdhip64.so", "libamdhip64.so.7", "/opt/rocm/lib/libamdhip64.so"):
        try:
            return C.CDLL(name)
        except OSError:
            continue
    raise OSError("libamdhip64 not found")


def test_switches_replacement_device_pointers_and_getter():
    c = ibc.case(12, 4, 10, False, True, 13)
    B = c["B"]
    # the getter returns what was set, whatever the switches say
    s = make(c)
    s.set_instance_bounds(*c["box"])
    s.update_settings(max_iter=ibc.MAX_ITER, en_state_bound=0)
    for i in (0, 5, B - 1):
        assert all(np.array_equal(a, b[i]) for a, b in zip(s.instance_bounds(i), c["box"]))
    # en_state_bound = 0: only the input box acts -- one box for all against the shared handle with the same switch
    box = [a[0] for a in c["box"]]
    ref = make(c)
    ref.set_option("prefetch", 0)
    ref.update_settings(max_iter=ibc.MAX_ITER, en_state_bound=0)
    ref.set_bound_constraints(*box)
    s.set_instance_bounds(*[np.broadcast_to(a, (B,) + a.shape) for a in box])
    for h in (s, ref):
        h.solve()
    assert s.get_option("last_instance_bounds") == 1 and s.get_option("last_uniform_bounds") == 0      # (the input box varies from knot to knot)
    snap = snapshot(s)
    assert_same_bits(snap, snapshot(ref), "en_state_bound=0")
    assert np.any(np.abs(snap["vnew"]) > np.max(np.abs(np.stack(box[:2]))))      # the state box does not act
    # the shared setter afterwards replaces the per-instance box
    s.reset()
    ref.reset()
    s.set_bound_constraints(*box)
    assert s.get_option("instance_bounds") == 0
    assert all(np.array_equal(a, b) for a, b in zip(s.instance_bounds(3), box))
    s.set_option("prefetch", 0)
    for h in (s, ref):
        h.solve()
    assert s.get_option("last_instance_bounds") == 0
    assert_same_bits(snapshot(s), snapshot(ref), "shared setter after the per-instance one")
    s.close()
    ref.close()
    # device pointers give the same bits as host arrays
    a, b = make(c), make(c)
    a.set_instance_bounds(*c["box"])
    hip = _hip_runtime()
    dev = []
    for v in c["box"]:
        flat = np.ascontiguousarray(v.transpose(0, 2, 1)).ravel()   # [batch][knot][row]
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(flat.nbytes)) == 0
        assert hip.hipMemcpy(p, flat.ctypes.data_as(C.c_void_p), C.c_size_t(flat.nbytes), 1) == 0      # hipMemcpyHostToDevice
        dev.append(p)
    b.set_instance_bounds_device(*[p.value for p in dev])
    for p in dev:                                                    # (copied: the caller may free)
        assert hip.hipFree(p) == 0
    for h in (a, b):
        h.solve()
    assert b.get_option("last_instance_bounds") == 1
    assert_same_bits(snapshot(a), snapshot(b), "TINY_DEVICE against TINY_HOST")
    assert all(np.array_equal(x, y[7]) for x, y in zip(b.instance_bounds(7), c["box"]))
    a.close()
    b.close()


# ---- e. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = ibc.case(12, 4, 10, False, False, 13)
    s = make(c)
    flat = [np.ascontiguousarray(v.transpose(0, 2, 1)).ravel() for v in c["box"]]
    ptrs = [v.ctypes.data for v in flat]
    L = tm.lib()
    assert L.tiny_batch_set_instance_bounds(s._h, *ptrs, tm.HOST | tm.BROADCAST) == tm.ERR_ARG
    assert L.tiny_batch_set_instance_bounds(s._h, ptrs[0], ptrs[1], None, ptrs[3], tm.HOST) == tm.ERR_NULL
    assert s.get_option("instance_bounds") == 0
    s.set_instance_bounds(*c["box"])
    s.set_adaptive_rho(1)
    assert L.tiny_batch_solve(s._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(s._h).decode()
    assert "adaptive rho" in msg and "per-instance bounds" in msg, msg
    s.set_adaptive_rho(0)
    s.solve()
    assert s.get_option("last_instance_bounds") == 1
    s.close()


# ---- f. a group of two shards on one GPU, round-robin, boxes in the caller's order ------------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    c = ibc.case(12, 4, 10, False, True, 13)
    g = tm.TinyGroupSolver.from_problem(c["fams"][0], c["B"], devices=[0, 0], n_shards=2, interleaved=True)
    s = make(c)
    g.update_settings(max_iter=ibc.MAX_ITER)
    g.set_x0(c["x0"])
    g.set_x_ref(c["Xref"])
    g.set_u_ref(c["Uref"])
    g.set_instance_bounds(*c["box"])
    s.set_instance_bounds(*c["box"])
    g.solve()
    s.solve()
    st, gst = s.status(), g.status()
    for k in KEYS:
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(gst["iter"], st["iter"]) and np.array_equal(gst["solved"], st["solved"])
    g.close()
    s.close()
