"""GPU tests of per-instance half-space constraints (tiny_batch_set_instance_linear_constraints / ..._tv_...): the one-row kernel's PL
forms and the coverage kernel's per-instance read.  Batches of 11 or 13: more than two tiles, the last one with 3 rows or 1.
  a. one set for all through the instance setter equals the shared setter bit for bit (cold and warm), on the one-row forms and the
     coverage kernel;
  b. every instance against its own oracle under its own sets (tests/instance_halfspace_cases.py asserts, from the oracle alone, that a
     block read from the wrong instance, knot, slot or lane moves the result), cold and warm, shared and per-instance problem data;
  c. every launch form against 13 single-instance handles that use the SHARED setters;
  d. setter semantics: independent replacement of the two sets, device pointers, the getter, a padded row, the offsets-only update, a
     failed call;  e. refusals;  f. a sharded group."""
import ctypes as C

import numpy as np
import pytest

import instance_halfspace_cases as ihc
import tinympc_amd as tm

pytestmark = pytest.mark.gpu
RESID = ("primal_residual_state", "primal_residual_input", "dual_residual_state", "dual_residual_input")
RTOL = 1e-9                                        # the project's parity contract (README.md)


def settings(c, max_iter=ihc.MAX_ITER, lin=None):
    lin = c["lin"] if lin is None else lin
    box = int(c["box"] is not None)
    return dict(max_iter=max_iter, en_state_bound=box, en_input_bound=box, en_state_soc=int(c["cone"]), en_state_linear=lin & 1, en_input_linear=lin & 1,
                en_tv_state_linear=(lin >> 1) & 1, en_tv_input_linear=(lin >> 1) & 1)


def make(c, only=None, group=False):
    """a handle for case c: the whole batch, or (only = i) instance i alone; the constraints are the caller's to set"""
    idx = list(range(c["B"])) if only is None else [only]
    if group:
        s = tm.TinyGroupSolver.from_problem(c["fams"][0], c["B"], devices=[0, 0], n_shards=2, interleaved=True)
    elif c["hetero"]:
        fams = [c["fams"][i] for i in idx]
        s = tm.TinyBatchSolver.hetero(*[np.stack([f[k] for f in fams]) for k in ("A", "B", "f", "Q", "R")], np.array([f["rho"] for f in fams]), c["N"])
    else:
        s = tm.TinyBatchSolver.from_problem(c["fams"][0], len(idx))
    if c["cone"]:
        s.set_cone_constraints(*ihc.STATE_CONE, [], [], [])
    s.update_settings(**settings(c))
    s.set_x0(c["x0"][idx])
    s.set_x_ref(c["Xref"][idx])
    s.set_u_ref(c["Uref"][idx])
    return s


def set_own(s, c):
    s.set_instance_linear_constraints(*c["linear"])
    s.set_instance_tv_linear_constraints(*c["tv_linear"])
    if c["box"] is not None:
        s.set_instance_bounds(*c["box"])


def set_shared(s, c, i):
    s.set_linear_constraints(*[a[i] for a in c["linear"]])
    s.set_tv_linear_constraints(*[a[i] for a in c["tv_linear"]])
    if c["box"] is not None:
        s.set_bound_constraints(*[a[i] for a in c["box"]])


def one_for_all(c, i=0):
    """instance i's sets with a leading batch axis"""
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[i], a.shape))
    return dict(c, linear=tuple(rep(a) for a in c["linear"]), tv_linear=tuple(rep(a) for a in c["tv_linear"]),
                box=None if c["box"] is None else [rep(a) for a in c["box"]])


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


def assert_form(s, path, mask):
    """the last solve read the per-instance sets of `mask` on the kernel `path` names -- so that no test passes on the wrong path"""
    assert s.get_option("instance_linear") == 3 and s.get_option("last_instance_linear") == mask, (s.get_option("instance_linear"), s.get_option("last_instance_linear"))
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


# (case of instance_halfspace_cases.GPU_CASES order: nx, nu, N, hetero, B, lin, cone, box; options of the handles; the kernel path)
FORMS = {
    "12_4_10_lin1": ((12, 4, 10, False, 13, 1, False, False), {}, "jit"),
    "12_4_10_lin2": ((12, 4, 10, False, 13, 2, False, False), {}, "jit"),
    "12_4_10_lin3": ((12, 4, 10, False, 13, 3, False, False), {}, "jit"),
    "12_4_10_hetero": ((12, 4, 10, True, 11, 3, False, False), {}, "jit"),
    "6_3_10_cone": ((6, 3, 10, False, 13, 3, True, False), {}, "jit"),
    "5_3_7": ((5, 3, 7, False, 11, 3, False, False), {}, "jit"),
    "4_2_30_tv": ((4, 2, 30, False, 11, 2, False, False), {}, "cover"),          # four rows' tables beside the planes of N = 30 do not fit
    "20_4_10": ((20, 4, 10, False, 11, 3, False, False), {}, "cover"),           # a tile-kernel shape
    "12_4_10_box": ((12, 4, 10, False, 11, 2, False, True), {}, "cover"),        # a per-instance box at the same time
    "12_4_10_force_general": ((12, 4, 10, False, 13, 3, False, False), {"force_general": 1}, "cover"),
    "13_3_4": ((13, 3, 4, False, 11, 3, False, False), {}, "jit"),              # all 16 lanes in use, the inputs in lanes 13..15
}
assert sorted({f[0] for f in FORMS.values()}) == sorted(ihc.GPU_CASES)


@pytest.mark.parametrize("form", ["12_4_10_lin1", "12_4_10_lin2", "12_4_10_lin3", "6_3_10_cone", "12_4_10_force_general", "20_4_10"])
def test_one_set_for_all_through_the_instance_setter_equals_the_shared_setter(form):
    cs, opts, path = FORMS[form]
    c = ihc.case(*cs)
    keys = ihc.keys(c["lin"], c["cone"])
    s, ref = make(c), make(c)
    for h in (s, ref):
        for k, v in opts.items():
            h.set_option(k, v)
    if path == "cover":
        ref.set_option("force_general", 1)                           # (bit for bit: the same kernel on both sides)
    set_own(s, one_for_all(c))
    set_shared(ref, c, 0)
    for scale, what in ((1.0, "cold"), (0.9, "warm")):
        for h in (s, ref):
            h.set_x0(c["x0"] * scale)
            h.solve()
        assert_form(s, path, c["lin"])
        assert ref.get_option("instance_linear") == 0 and ref.get_option("last_instance_linear") == 0
        assert ref.kernel_path() in (("cover",) if path == "cover" else ("regs", "jit"))
        assert_same_bits(snapshot(s, keys), snapshot(ref, keys), (form, what))
    s.close()
    ref.close()


@pytest.mark.parametrize("form", [f for f in FORMS if f != "12_4_10_force_general"])
def test_every_instance_against_its_own_oracle_under_its_own_sets(form):
    cs, opts, path = FORMS[form]
    ihc.check_case(*cs)                                              # (the oracle alone: before anything runs on the GPU)
    c, want = ihc.case(*cs), ihc.oracle_case(*cs)
    keys = ihc.keys(c["lin"], c["cone"])
    s = make(c)
    for k, v in opts.items():
        s.set_option(k, v)
    set_own(s, c)
    got = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"] * scale)
        s.solve()
        got.append(snapshot(s, keys))
    assert_form(s, path, c["lin"])
    assert s.get_option("last_instance_bounds") == int(c["box"] is not None)
    for i in range(c["B"]):
        for k_solve, what in ((0, "cold"), (1, "warm")):
            rec, it, solved = want[i][k_solve]
            assert (it, solved) == (got[k_solve]["iter"][i], got[k_solve]["solved"][i]), (i, what)
            for k in keys:
                e = rel_err(got[k_solve][k][i], rec[k])
                assert e < RTOL, (i, what, k, e)
    s.close()


# ---- c. launch forms: (12,4,10), batch 13, both sets -------------------------------------------------------------------------------
TRAJ_POINTS = 30


def _traj(c):
    rng = np.random.default_rng(99)
    return rng.normal(0, 0.2, (TRAJ_POINTS, c["nx"])), rng.integers(0, 5, c["B"]).astype(np.int32)


def _drive_two_warm(s, c, idx, keys):
    out = []
    for scale in (1.0, 0.9, 0.8):                                    # cold, then two warm launches: the third walks the batch in reverse again
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s, keys))
    return out


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
    out = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s, keys))
    return out


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
    out = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s, keys))
    return out


def _drive_descending(s, c, idx, keys):
    s.set_option("launch_order", 2)
    out = []
    for scale in (1.0, 0.9):
        s.set_x0(c["x0"][idx] * scale)
        s.solve()
        out.append(snapshot(s, keys))
    return out


DRIVES = {"two_warm": _drive_two_warm, "fused_steps": _drive_fused, "advance_x0": _drive_advance, "one_shot": _drive_one_shot, "trajectory": _drive_traj,
          "reset_duals": _drive_reset_duals, "repack_after": _drive_repack, "step_regroup": _drive_regroup, "grid_waves_per_cu": _drive_capped_grid,
          "launch_order": _drive_descending}


@pytest.mark.parametrize("drive", list(DRIVES))
def test_launch_forms_equal_single_instance_handles_with_the_shared_setters(drive):
    c = ihc.launch_case()
    B, keys = c["B"], ihc.keys(c["lin"])
    s = make(c)
    set_own(s, c)
    got = DRIVES[drive](s, c, list(range(B)), keys)
    assert_form(s, "jit", 3)
    s.close()
    singles = []
    for i in range(B):
        r = make(c, only=i)
        set_shared(r, c, i)
        singles.append(DRIVES[drive](r, c, [i], keys))
        assert r.get_option("instance_linear") == 0 and r.get_option("last_instance_linear") == 0
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


def raw_set(s, tv, A_x, b_x, A_u, b_u, flags=tm.HOST):
    """the C setter's return code (None coefficients: the offsets-only update)"""
    ns, ni, a = s._instance_halfspaces(tv, A_x, b_x, A_u, b_u)
    p = [None if v is None else v.ctypes.data_as(C.c_void_p) for v in a]
    f = tm.lib().tiny_batch_set_instance_tv_linear_constraints if tv else tm.lib().tiny_batch_set_instance_linear_constraints
    return f(s._h, ns, p[0], p[1], ni, p[2], p[3], flags)


def _solve_snapshot(s, c, keys):
    s.reset()
    s.set_x0(c["x0"])
    s.solve()
    return snapshot(s, keys)


def test_static_and_time_varying_sets_are_replaced_independently():
    c = ihc.case(12, 4, 10, False, 13, 3)
    keys = ihc.keys(3)
    all0 = one_for_all(c)
    ref = make(c)
    set_shared(ref, c, 0)
    want = _solve_snapshot(ref, c, keys)
    # per-instance static set, shared time-varying set -- and the other way round: one-for-all numbers, so the shared handle is the reference
    s = make(c)
    s.set_instance_linear_constraints(*all0["linear"])
    s.set_tv_linear_constraints(*[a[0] for a in c["tv_linear"]])
    assert s.get_option("instance_linear") == 1
    assert_same_bits(_solve_snapshot(s, c, keys), want, "static per instance, time-varying shared")
    assert s.get_option("last_instance_linear") == 1 and s.kernel_path() == "jit"
    s.set_instance_tv_linear_constraints(*all0["tv_linear"])
    assert s.get_option("instance_linear") == 3
    s.set_linear_constraints(*[a[0] for a in c["linear"]])            # a later shared setter of the same set replaces the per-instance one
    assert s.get_option("instance_linear") == 2
    assert_same_bits(_solve_snapshot(s, c, keys), want, "static shared, time-varying per instance")
    assert s.get_option("last_instance_linear") == 2 and s.kernel_path() == "jit"
    s.set_tv_linear_constraints(*[a[0] for a in c["tv_linear"]])
    assert s.get_option("instance_linear") == 0
    assert_same_bits(_solve_snapshot(s, c, keys), want, "both shared again")
    assert s.get_option("last_instance_linear") == 0
    # the switches act as on shared sets: the time-varying families off on both handles
    set_own(s, all0)
    for h in (s, ref):
        h.update_settings(**settings(c, lin=1))
    assert_same_bits(_solve_snapshot(s, c, ihc.keys(1)), _solve_snapshot(ref, c, ihc.keys(1)), "time-varying families switched off")
    assert s.get_option("instance_linear") == 3 and s.get_option("last_instance_linear") == 1
    s.close()
    ref.close()


def test_getter_device_pointers_and_reset():
    c = ihc.case(12, 4, 10, False, 13, 3)
    keys = ihc.keys(3)
    a, b = make(c), make(c)
    set_own(a, c)
    # the getter returns what was set, whatever the switches say
    a.update_settings(**settings(c, lin=0))
    for i in (0, 5, c["B"] - 1):
        for tv, src in ((0, c["linear"]), (1, c["tv_linear"])):
            assert all(np.array_equal(x, y[i]) for x, y in zip(a.instance_linear_constraints(i, tv), src)), (i, tv)
    a.update_settings(**settings(c))
    # device pointers give the same bits as host arrays; the caller's buffers are freed right after the call
    hip = _hip_runtime()
    for tv, src in ((0, c["linear"]), (1, c["tv_linear"])):
        ns, ni, flat = b._instance_halfspaces(tv, *src)
        dev = []
        for v in flat:
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), C.c_size_t(v.nbytes)) == 0
            assert hip.hipMemcpy(p, v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes), 1) == 0      # hipMemcpyHostToDevice
            dev.append(p)
        setter = b.set_instance_tv_linear_constraints_device if tv else b.set_instance_linear_constraints_device
        setter(ns, dev[0].value, dev[1].value, ni, dev[2].value, dev[3].value)
        for p in dev:
            assert hip.hipFree(p) == 0
    first = _solve_snapshot(a, c, keys)
    assert_same_bits(first, _solve_snapshot(b, c, keys), "TINY_DEVICE against TINY_HOST")
    assert b.get_option("last_instance_linear") == 3
    assert all(np.array_equal(x, y[7]) for x, y in zip(b.instance_linear_constraints(7, 1), c["tv_linear"]))
    # tiny_batch_reset leaves the constraints alone
    assert a.get_option("instance_linear") == 3
    assert_same_bits(_solve_snapshot(a, c, keys), first, "after a reset")
    # on shared sets the getter returns the shared one
    set_shared(a, c, 4)
    assert all(np.array_equal(x, y[4]) for x, y in zip(a.instance_linear_constraints(9, 0), c["linear"]))
    assert all(np.array_equal(x, y[4]) for x, y in zip(a.instance_linear_constraints(9, 1), c["tv_linear"]))
    a.close()
    b.close()


@pytest.mark.parametrize("path", ["jit", "cover"])
def test_a_padded_row_is_inert(path):
    """a = 0, b = +inf as one more half-space equals the batch without it, bit for bit (cv = 0 > +inf is false).  Padded: the static input
    family and both time-varying ones, 1 -> 2 per knot -- the static state family has 2 already, so both batches run the same form
    (KMAX = 2) and the padded one applies one more half-space per time-varying column"""
    c = ihc.case(12, 4, 10, False, 13, 3)
    keys = ihc.keys(3)
    N, B = c["N"], c["B"]
    Ax, bx, Au, bu = c["linear"]
    tAx, tbx, tAu, tbu = c["tv_linear"]
    pad_rows = lambda a: np.concatenate([a, np.zeros((B, 1, a.shape[2]))], axis=1)
    pad_inf = lambda b: np.concatenate([b, np.full((B, 1) + b.shape[2:], np.inf)], axis=1)

    def pad_tv(a, knots):                                            # one zero row behind every knot's rows
        per = a.shape[1] // knots
        return np.concatenate([a.reshape(B, knots, per, -1), np.zeros((B, knots, 1, a.shape[2]))], axis=2).reshape(B, knots * (per + 1), -1)
    s, ref = make(c), make(c)
    if path == "cover":
        s.set_option("force_general", 1)
        ref.set_option("force_general", 1)
    set_own(ref, c)
    s.set_instance_linear_constraints(Ax, bx, pad_rows(Au), pad_inf(bu))
    s.set_instance_tv_linear_constraints(pad_tv(tAx, N), pad_inf(tbx), pad_tv(tAu, N - 1), pad_inf(tbu))
    assert [s.get_option(k) for k in ("n_state_linear", "n_input_linear", "n_tv_state_linear", "n_tv_input_linear")] == [2, 2, 2, 2]
    assert_same_bits(_solve_snapshot(s, c, keys), _solve_snapshot(ref, c, keys), "padded")
    assert s.get_option("last_instance_linear") == 3 and s.kernel_path() == ref.kernel_path() == path
    s.close()
    ref.close()


@pytest.mark.parametrize("path", ["jit", "cover"])
def test_offsets_only_update_equals_a_full_reset_of_the_sets(path):
    c = ihc.case(12, 4, 10, False, 13, 3)
    keys = ihc.keys(3)
    Ax, bx, Au, bu = c["linear"]
    tAx, tbx, tAu, tbu = c["tv_linear"]
    L = tm.lib()
    s, ref = make(c), make(c)
    if path == "cover":
        s.set_option("force_general", 1)
        ref.set_option("force_general", 1)
    # nothing installed: TINY_ERR_ARG, and nothing is installed afterwards
    assert raw_set(s, 0, None, bx, None, bu) == tm.ERR_ARG and raw_set(s, 1, None, tbx, None, tbu) == tm.ERR_ARG
    assert s.get_option("instance_linear") == 0
    set_own(s, c)
    first = _solve_snapshot(s, c, keys)
    # other counts: TINY_ERR_ARG, the installed sets stay (a failed call leaves what was installed)
    assert raw_set(s, 0, None, bx[:, :1], None, bu) == tm.ERR_ARG
    assert raw_set(s, 1, None, np.concatenate([tbx, tbx], axis=1), None, tbu) == tm.ERR_ARG
    assert L.tiny_batch_set_instance_linear_constraints(s._h, -1, None, None, 0, None, None, tm.HOST) != 0
    assert s.get_option("instance_linear") == 3
    assert all(np.array_equal(x, y[3]) for x, y in zip(s.instance_linear_constraints(3, 0), c["linear"]))
    assert_same_bits(_solve_snapshot(s, c, keys), first, "after failed calls")
    # the closed-loop pattern: only b moves
    bx2, bu2, tbx2, tbu2 = bx * 0.9, bu * 1.1, tbx * 0.95, tbu * 1.05
    s.set_instance_linear_constraints(None, bx2, None, bu2)
    s.set_instance_tv_linear_constraints(None, tbx2, None, tbu2)
    ref.set_instance_linear_constraints(Ax, bx2, Au, bu2)
    ref.set_instance_tv_linear_constraints(tAx, tbx2, tAu, tbu2)
    moved = _solve_snapshot(s, c, keys)
    assert_same_bits(moved, _solve_snapshot(ref, c, keys), "offsets only against a full re-set")
    assert s.kernel_path() == path and s.get_option("last_instance_linear") == 3
    assert not np.array_equal(moved["vnew"], first["vnew"])
    assert all(np.array_equal(x, y[5]) for x, y in zip(s.instance_linear_constraints(5, 1), (tAx, tbx2, tAu, tbu2)))
    # one family's offsets alone (the other family's arrays given in full)
    s.set_instance_linear_constraints(None, bx, Au, bu)
    ref.set_instance_linear_constraints(Ax, bx, Au, bu)
    assert_same_bits(_solve_snapshot(s, c, keys), _solve_snapshot(ref, c, keys), "one family's offsets only")
    s.close()
    ref.close()


# ---- e. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals():
    c = ihc.case(12, 4, 10, False, 13, 3)
    s = make(c)
    L = tm.lib()
    for tv, src in ((0, c["linear"]), (1, c["tv_linear"])):
        ns, ni, flat = s._instance_halfspaces(tv, *src)
        ptrs = [v.ctypes.data for v in flat]
        f = L.tiny_batch_set_instance_tv_linear_constraints if tv else L.tiny_batch_set_instance_linear_constraints
        assert f(s._h, ns, ptrs[0], ptrs[1], ni, ptrs[2], ptrs[3], tm.HOST | tm.BROADCAST) == tm.ERR_ARG
        assert f(s._h, -1, ptrs[0], ptrs[1], ni, ptrs[2], ptrs[3], tm.HOST) != 0
        assert f(s._h, ns, ptrs[0], ptrs[1], -2, ptrs[2], ptrs[3], tm.HOST) != 0
        assert f(s._h, ns, ptrs[0], None, ni, ptrs[2], ptrs[3], tm.HOST) == tm.ERR_NULL
    assert s.get_option("instance_linear") == 0
    set_own(s, c)
    s.set_adaptive_rho(1)
    assert L.tiny_batch_solve(s._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(s._h).decode()
    assert "adaptive rho does not combine with" in msg and "half-spaces" in msg, msg
    s.set_adaptive_rho(0)
    s.solve()
    assert s.get_option("last_instance_linear") == 3
    s.close()


# ---- f. a group of two shards on one GPU, round-robin, sets in the caller's order ----------------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    c = ihc.case(5, 3, 7, False, 11, 3)                              # 11 instances: shards of 6 and 5
    keys = ihc.keys(3)
    g, s = make(c, group=True), make(c)
    g.set_instance_linear_constraints(*c["linear"])
    g.set_instance_tv_linear_constraints(*c["tv_linear"])
    set_own(s, c)
    g.solve()
    s.solve()
    st, gst = s.status(), g.status()
    for k in keys:
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(gst["iter"], st["iter"]) and np.array_equal(gst["solved"], st["solved"])
    assert s.get_option("last_instance_linear") == 3
    g.close()
    s.close()
