"""GPU tests of the per-instance closed-loop score at the plant step (tiny_batch_set_score): the one-row kernel's PS forms and the helper
kernel behind the coverage kernel.  Cases, setups and the reference: tests/score_cases.py on the problems of tests/plant_cases.py
(batches of 13, 11 and 2: the last tile has 1, 3 or 2 rows; T = 5 MPC steps).  The yardstick is never the code under test: the reference
(score_cases.score_reference, plain Python floats) is applied to the state log and the step log's u0 of a handle WITHOUT a score.
  1. every launch form gives the reference's four arrays bit for bit and the counter reads T; everything else -- records, step log,
     state log, final x0 -- equals the handle without a score;
  2. every instance against the reference applied to its own ORACLE loop: cost within the project's 1e-9, counts equal;
  3. composition: plant + disturbance, measurement noise + estimator (the TRUE state is scored), per-instance problem data, PB, PL, PC;
  4. the coverage path;  5. no limits;  6. the counter moved;  7. max_iter = 0;  8. a launch without a plant step;
  9. setter and getters;  10. the refusal;  11. a sharded group;  12. the example.
Every test asserts the kernel path and the read-backs, so that none passes on the wrong path."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import disturbance_cases as dc
import estimator_cases as ec
import measurement_cases as mc
import plant_cases as pc
import score_cases as scs
import tinympc_amd as tm
from test_gpu_plant import FORMS as PLANT_FORMS, _hip_runtime, advance, assert_same_bits, fused, make, make_own, rel_err, snapshot

pytestmark = pytest.mark.gpu
RTOL = 1e-9                                        # the project's parity contract (README.md)
T, KEYS = scs.T, pc.KEYS
NAMES = ("cost", "worst", "violated_steps", "first_violation")


def assert_scored(s, path, kind=2, counter=T):
    """the last solve's launches scored on the kernel `path` names, on full rows, not in the PREFETCH form, and the counter reads `counter`"""
    assert (s.get_option("score"), s.get_option("last_score"), s.get_option("score_step")) == (kind, 1, counter), (s.get_option("score"), s.get_option("last_score"), s.get_option("score_step"))
    assert s.kernel_path() == path, s.kernel_path()
    assert s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0


def assert_record(got, want, what):
    """the four arrays, bit for bit"""
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name, g, w)


def reference_of(run, setup, **kw):
    """the reference applied to the logs of a run: state log and step log"""
    return scs.score_reference_batch(run["log_x0"], run["log_u0"], setup, **kw)


def setup_around(run, seed):
    """a per-instance setup whose limits are drawn around the trajectories a run logged (score_cases.limits_around)"""
    z = np.concatenate([run["log_x0"], run["log_u0"]], axis=2).swapaxes(0, 1)
    B, _, nz = z.shape
    nx = run["log_x0"].shape[2]
    rng = np.random.default_rng(seed)
    lo, hi = scs.limits_around(z, nx, nz - nx, seed + 1)
    return rng.uniform(0.5, 2.0, (B, nz)), rng.uniform(-0.3, 0.3, (B, nz)), lo, hi


def _two_launches(s):
    a, b = fused(s, 2), fused(s, 3)
    return {k: np.concatenate([a[k], b[k]]) for k in a}


def _mode0(s):
    s.set_option("dpp_mode", 0)
    return fused(s)


FORMS = dict(PLANT_FORMS, two_plus_three=_two_launches, dpp_mode_0=_mode0)


@functools.lru_cache(maxsize=None)
def plain(name, option=None, value=1):
    """the case under its plant on a handle WITHOUT a score, fused, both logs on: computed once and shared (never modified)"""
    c = pc.case(name)
    r = make(c)
    if option:
        r.set_option(option, value)
    r.set_plant(*c["plant"])
    want = dict(fused(r))
    want.update(snapshot(r))
    assert (r.get_option("score"), r.get_option("last_score")) == (0, 0)
    r.close()
    return want


def scoring(name, drive=fused, option=None, setup=None, before=None):
    """the same on a handle with the case's score installed -> (records and logs, the four arrays, the handle)"""
    c = pc.case(name)
    s = make(c)
    if option:
        s.set_option(option, 1)
    s.set_plant(*c["plant"])
    s.set_score(*(setup or scs.setup(name)))
    if before:
        before(s)
    run = drive(s)
    return dict(snapshot(s), **run), s.get_score(), s


# ---- 1. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,form", [(n, f) for n in scs.ORACLE_CASES for f in FORMS])
def test_every_launch_form_gives_the_references_record_and_moves_nothing_else(name, form):
    want = plain(name, "dpp_mode", 0) if form == "dpp_mode_0" else plain(name)      # (the solve's own bits follow dpp_mode; the score's sum does not)
    got, rec, s = scoring(name, FORMS[form])
    assert_scored(s, "jit")
    s.close()
    assert_same_bits(got, want, (name, form))
    assert_record(rec, reference_of(want, scs.setup(name)), (name, form))
    assert np.any(rec[2] > 0) and np.any(rec[2] == 0) and np.all(rec[0] > 0.0)


# ---- 2. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scs.ORACLE_CASES + scs.EDGE_CASES)
def test_every_instance_scores_what_its_own_oracle_loop_scores(name):
    scs.check_case(name)                                             # (the reference and the oracle alone: before anything runs on the GPU)
    cost, worst, steps, first = scs.oracle_scores(name)
    got, rec, s = scoring(name)
    assert_scored(s, "jit")
    s.close()
    for i in range(pc.case(name)["B"]):
        e = abs(rec[0][i] - cost[i]) / abs(cost[i])
        assert e < RTOL, (name, i, e)
    assert np.array_equal(rec[2], steps) and np.array_equal(rec[3], first), (name, rec[2], steps, rec[3], first)
    assert_same_bits(got, plain(name), name)
    assert_record(rec, reference_of(plain(name), scs.setup(name)), name)


# ---- 3. ------------------------------------------------------------------------------------------------------------------------------
def _compose(build, prepare, keys=KEYS, seed=900, path="jit"):
    """a run without a score, a setup around what it logged, the run again with that score: nothing but the record differs, and the
    record is the reference's"""
    r = build()
    prepare(r)
    want = dict(fused(r))
    want.update(snapshot(r, keys))
    assert r.get_option("score") == 0 and r.kernel_path() == path
    r.close()
    assert np.max(np.abs(want["log_iter"])) > 1 and np.max(np.abs(want["x"])) < 100.0      # (something iterates, nothing diverges)
    setup = setup_around(want, seed)
    s = build()
    prepare(s)
    s.set_score(*setup)
    got = dict(fused(s))
    got.update(snapshot(s, keys))
    rec = s.get_score()
    assert_scored(s, path)
    assert_same_bits(got, want, "everything but the record")
    ref = reference_of(want, setup)
    assert_record(rec, ref, "the record")
    assert np.any(ref[2] > 0) and np.any(ref[2] == 0)
    return s, want, setup, rec


def test_ps_composes_with_a_plant_and_a_disturbance():
    c = pc.case("6_3_10")

    def prepare(h):
        h.set_plant(*c["plant"])
        h.set_disturbance(c["w"])
    s, want, setup, rec = _compose(lambda: make(c), prepare)
    assert (s.get_option("last_plant"), s.get_option("last_disturbance")) == (1, 1)
    s.close()
    # the disturbance is part of what is scored: the undisturbed plant step scores otherwise
    bare = pc.plant_step_batch(c["plant"], c["x0"], want["log_u0"][0])
    assert not np.array_equal(bare, want["log_x0"][0])


def test_ps_under_measurement_noise_and_an_estimator_scores_the_true_state():
    name = "6_3_10"
    c, v = pc.case(name), mc.noise(name)
    M, xp0 = ec.gain_for(c["B"], c["nx"], 321), ec.estimate_for(c["x0"], 123)

    def prepare(h):
        h.set_measurement_noise(v)
        h.set_plant(*c["plant"])
        h.set_estimator(M)
        h.set_estimate(xp0)
        h.set_option("estimate_log", 1)
    s, want, setup, rec = _compose(lambda: make(c), prepare)
    assert (s.get_option("last_estimator"), s.get_option("last_measurement_noise"), s.get_option("last_plant")) == (1, 1, 1)
    xhat = s.estimate_log(T)
    s.close()
    # the state log holds TRUE states; the estimates the solver saw one step later would score otherwise
    assert not np.array_equal(xhat[1:], want["log_x0"][:-1])
    other = scs.score_reference_batch(xhat[1:], want["log_u0"][:-1], setup)
    assert not np.array_equal(other[0], reference_of(dict(log_x0=want["log_x0"][:-1], log_u0=want["log_u0"][:-1]), setup)[0])


@pytest.mark.parametrize("what", ["hetero", "instance_box"])
def test_ps_composes_with_per_instance_problem_data_and_boxes(what):
    c = pc.case("12_4_10_hetero" if what == "hetero" else "6_3_10")
    s, _, _, _ = _compose(lambda: make(c, own_box=what == "instance_box"), lambda h: None, seed=901)      # (nothing else installed: the PD form, empty sequence)
    assert (s.get_option("last_plant"), s.get_option("last_disturbance"), s.get_option("last_instance_bounds")) == (0, 0, int(what == "instance_box"))
    s.close()


@pytest.mark.parametrize("name,own", [("6_3_10_pl", "lin"), ("6_3_10_pc", "cones")])
def test_ps_composes_with_per_instance_halfspaces_and_cone_coefficients(name, own):
    c = dc.case(name)
    assert c["own"] == (own,) and c["path"] == "jit"
    plant = pc.plant_for(c)
    s, _, _, _ = _compose(lambda: make_own(c), lambda h: h.set_plant(*plant), keys=dc.keys(c), seed=902)
    assert (s.get_option("last_instance_linear"), s.get_option("last_instance_cones"), s.get_option("last_plant")) == (int(own == "lin"), int(own == "cones"), 1)
    s.close()


# ---- 4. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,option", [(scs.COVER_CASE, None), ("5_3_7", "force_general")])
def test_the_coverage_path_scores_the_same_way(name, option):
    scs.check_case(name)
    want = plain(name, option)
    for drive in (fused, advance):
        got, rec, s = scoring(name, drive, option)
        assert_scored(s, "cover")
        s.close()
        assert_same_bits(got, want, (name, drive.__name__))
        assert_record(rec, reference_of(want, scs.setup(name)), (name, drive.__name__))
    if option:                                                       # where both exist: the helper kernel and the PS form agree on the same states
        got, rec, s = scoring(name)
        assert_scored(s, "jit")
        s.close()
        assert_record(rec, reference_of(got, scs.setup(name)), "the PS form on its own logs")


# ---- 5. 6. ---------------------------------------------------------------------------------------------------------------------------
def test_no_limits_score_the_cost_alone_and_a_moved_counter_moves_every_first_violation():
    name = "5_3_7"
    w, tg, lo, hi = scs.setup(name)
    want = plain(name)
    got, rec, s = scoring(name, setup=(w, tg, None, None))
    assert_scored(s, "jit")
    B = len(w)
    assert np.array_equal(rec[1], np.zeros(B)) and np.array_equal(rec[2], np.zeros(B, dtype=np.int32)) and np.array_equal(rec[3], np.full(B, -1, dtype=np.int32))
    assert np.array_equal(rec[0], reference_of(want, scs.setup(name))[0])
    for out, none in zip(s.get_score_setup(3)[2:], (-np.inf, np.inf)):
        assert np.array_equal(out, np.full(w.shape[1], none))
    s.close()
    # one side only
    got, rec, s = scoring(name, setup=(w, None, None, hi))
    assert_record(rec, reference_of(want, (w, None, None, hi)), "no target, no lower limits")
    s.close()
    # the counter moved to 7 before the launch
    got, rec, s = scoring(name, before=lambda h: h.set_option("score_step", 7))
    assert_scored(s, "jit", counter=7 + T)
    s.close()
    ref = reference_of(want, scs.setup(name))
    assert_record(rec, ref[:3] + (np.where(ref[3] >= 0, ref[3] + 7, -1).astype(np.int32),), "score_step = 7")
    assert_record(rec, reference_of(want, scs.setup(name), k0=7), "score_step = 7, by the reference")
    assert np.any(ref[3] >= 0)


# ---- 7. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("option,drive,steps", [(None, fused, 3), (None, advance, 2), ("force_general", fused, 2)])
def test_a_step_without_an_iteration_is_not_scored_and_the_counter_advances(option, drive, steps):
    name = "5_3_7"
    c = pc.case(name)
    B = c["B"]

    def no_iteration(h):
        h.update_settings(max_iter=0, en_state_bound=1, en_input_bound=1)
    got, rec, s = scoring(name, lambda h: drive(h, steps), option, before=no_iteration)
    assert_scored(s, "cover" if option else "jit", counter=steps)
    assert_record(rec, (np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)), "max_iter = 0")
    assert np.array_equal(got["x0"], c["x0"]) and np.all(got["log_iter"] == 0)
    # ... and the steps after it are scored under the counter's value
    s.update_settings(max_iter=pc.MAX_ITER, en_state_bound=1, en_input_bound=1)
    run = drive(s, 2)
    rec = s.get_score()
    assert_scored(s, "cover" if option else "jit", counter=steps + 2)
    s.close()
    assert_record(rec, reference_of(run, scs.setup(name), k0=steps), "after the idle steps")


# ---- 8. ------------------------------------------------------------------------------------------------------------------------------
def test_a_launch_without_a_plant_step_leaves_record_and_counter_alone():
    name = "4_2_10"
    c = pc.case(name)
    r = make(c)
    r.solve()
    want = snapshot(r)
    path = r.kernel_path()
    r.close()
    s = make(c)
    s.set_score(*scs.setup(name))
    s.solve()
    assert (s.get_option("score"), s.get_option("last_score"), s.get_option("score_step")) == (2, 0, 0) and s.kernel_path() == path == "regs"
    assert tm.lib().tiny_batch_kernel_path(s._h) == 0                 # (a compiled-in shape keeps the compiled-in form)
    B = c["B"]
    assert_record(s.get_score(), (np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32)), "no plant step")
    assert_same_bits(snapshot(s), want, "no plant step")
    # ... after a scored episode too: the record and the counter stay
    s.set_plant(*c["plant"])
    fused(s)
    before = s.get_score()
    s.set_option("steps_per_launch", 1)
    s.set_option("state_log", 0)
    s.solve()
    assert (s.get_option("last_score"), s.get_option("score_step")) == (0, T)
    assert_record(s.get_score(), before, "a single solve behind an episode")
    s.close()


# ---- 9. ------------------------------------------------------------------------------------------------------------------------------
def test_setter_getters_broadcast_device_pointers_replacing_removal_failed_call_and_resets():
    name = "4_2_10"
    c, setup = pc.case(name), scs.setup(name)
    B, nz = c["B"], c["nx"] + c["nu"]
    L = tm.lib()
    want = plain(name)
    ref = reference_of(want, setup)
    zero = (np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int32), np.full(B, -1, dtype=np.int32))
    dp = np.zeros(B).ctypes.data_as(C.POINTER(C.c_double))
    s = make(c)
    s.set_plant(*c["plant"])
    assert L.tiny_batch_get_score(s._h, dp, None, None, None) == tm.ERR_ARG and L.tiny_batch_reset_score(s._h) == tm.ERR_ARG        # none installed
    assert L.tiny_batch_get_score_setup(s._h, 0, dp, None, None, None) == tm.ERR_ARG
    s.set_score(*setup)
    for i in (0, 4, B - 1):
        for got, given in zip(s.get_score_setup(i), setup):
            assert np.array_equal(got, given[i])
    for i in (B, -1):
        assert L.tiny_batch_get_score_setup(s._h, i, dp, None, None, None) == tm.ERR_ARG
    assert L.tiny_batch_get_score(s._h, None, None, None, None) == tm.OK                                                             # (any output may be null)
    assert_record(s.get_score(), zero, "installed")
    fused(s)
    assert_scored(s, "jit")
    assert_record(s.get_score(), ref, "the episode")
    # a failed call leaves what was installed: setup, record and counter
    flat = np.ascontiguousarray(setup[0]).ravel()
    assert L.tiny_batch_set_score(s._h, flat.ctypes.data_as(C.c_void_p), None, None, None, 64) == tm.ERR_ARG
    assert "flags" in L.tiny_batch_last_error(s._h).decode()
    with pytest.raises(ValueError):
        s.set_score(setup[0][:, :-1])
    assert (s.get_option("score"), s.get_option("score_step")) == (2, T) and np.array_equal(s.get_score_setup(2)[0], setup[0][2])
    assert_record(s.get_score(), ref, "after a failed call")
    # tiny_batch_reset leaves setup, record and counter alone; reset_score zeroes the record, rewinds the counter and keeps the setup
    s.reset()
    assert (s.get_option("score"), s.get_option("score_step")) == (2, T)
    assert_record(s.get_score(), ref, "after tiny_batch_reset")
    s.reset_score()
    assert (s.get_option("score"), s.get_option("score_step")) == (2, 0) and np.array_equal(s.get_score_setup(B - 1)[3], setup[3][B - 1])
    assert_record(s.get_score(), zero, "after reset_score")
    s.set_x0(c["x0"])
    fused(s)
    assert_record(s.get_score(), ref, "the episode again")
    # replacing zeroes the record and rewinds the counter
    other = tuple(a[::-1].copy() for a in setup)
    s.set_score(*other)
    assert (s.get_option("score"), s.get_option("score_step")) == (2, 0) and np.array_equal(s.get_score_setup(0)[1], setup[1][B - 1])
    assert_record(s.get_score(), zero, "replaced")
    s.reset()
    s.set_x0(c["x0"])
    fused(s)
    assert_record(s.get_score(), reference_of(want, other), "the other setup")
    # removal: the record goes with it, the run is the one without a score
    s.set_score(None)
    assert s.get_option("score") == 0 and L.tiny_batch_get_score(s._h, dp, None, None, None) == tm.ERR_ARG
    s.reset()
    s.set_x0(c["x0"])
    got = dict(fused(s))
    got.update(snapshot(s))
    assert s.get_option("last_score") == 0 and s.kernel_path() == "jit"
    assert_same_bits(got, want, "removed")
    s.close()
    # one setup for all against the same repeated, from host arrays and from device pointers: the same record
    one = tuple(a[5] for a in setup)
    full = scs.broadcast(one, B)
    hip = _hip_runtime()

    def on_device(a):
        a = np.ascontiguousarray(a, dtype=np.float64).ravel()
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), C.c_size_t(a.nbytes)) == 0
        assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0      # hipMemcpyHostToDevice
        return p
    for how in ("broadcast", "full", "device", "device_broadcast"):
        h = make(c)
        h.set_plant(*c["plant"])
        bc = how.endswith("broadcast")
        if how == "broadcast":
            h.set_score(*one)
        elif how == "full":
            h.set_score(*full)
        else:
            ps = [on_device(a) for a in (one if bc else full)]
            h.set_score_device(*[p.value for p in ps], broadcast=bc)
            for p in ps:
                assert hip.hipFree(p) == 0                             # (the arrays are copied)
        for got, given in zip(h.get_score_setup(B - 1), one):
            assert np.array_equal(got, given)
        fused(h)
        assert_scored(h, "jit", kind=1 if bc else 2)
        assert_record(h.get_score(), reference_of(want, full), how)
        h.close()


def test_install_remove_reinstall_equals_a_fresh_handle():
    name = "5_3_7"
    c, setup = pc.case(name), scs.setup(name)
    want = plain(name)
    s = make(c)
    s.set_plant(*c["plant"])
    for given in (tuple(a[0] for a in setup), None, setup):
        s.reset()
        s.set_x0(c["x0"])
        s.set_score(*(given if given is not None else (None,)))
        got = dict(fused(s))
        got.update(snapshot(s))
    assert_scored(s, "jit")
    rec = s.get_score()
    s.close()
    assert_same_bits(got, want, "install, remove, reinstall")
    assert_record(rec, reference_of(want, setup), "install, remove, reinstall")


# ---- 10. -----------------------------------------------------------------------------------------------------------------------------
def test_adaptive_rho_is_refused_on_a_launch_with_a_plant_step_only():
    c = pc.case("6_3_10")
    L = tm.lib()
    q = tm.TinyBatchSolver.from_problem(c["fams"][0], c["B"])
    q.update_settings(max_iter=pc.MAX_ITER, en_state_bound=0, en_input_bound=0)
    q.set_x0(c["x0"])
    q.set_score(*scs.setup("6_3_10"))
    q.set_adaptive_rho(1)
    q.solve()                                                        # no plant step: the score does not apply, adaptive rho runs
    assert q.get_option("last_score") == 0
    q.set_option("advance_x0", 1)
    assert L.tiny_batch_solve(q._h) == tm.ERR_UNSUPPORTED
    msg = L.tiny_batch_last_error(q._h).decode()
    assert "adaptive rho does not combine with a closed-loop score (tiny_batch_set_score)" in msg, msg
    assert q.get_option("score_step") == 0 and np.array_equal(q.get_score()[0], np.zeros(c["B"]))
    q.set_adaptive_rho(0)
    q.solve()
    assert_scored(q, "jit", counter=1)
    q.close()


# ---- 11. -----------------------------------------------------------------------------------------------------------------------------
def test_group_with_interleaved_shards_equals_the_single_batch():
    name = "6_3_10"
    c, setup = pc.case(name), scs.setup(name)                         # 11 instances: shards of 6 and 5
    g, s = make(c, group=True), make(c)
    for h in (g, s):
        h.set_plant(*c["plant"])
        h.set_score(*setup)
        h.set_option("score_step", 2)                                # (forwarded to every shard)
        h.set_option("steps_per_launch", 3)
        h.set_option("state_log", 1)
        h.set_option("step_log", 1)
        h.solve()
    for k in KEYS + ("x0",):
        assert np.array_equal(g.get(k), s.get(k)), k
    assert np.array_equal(g.state_log(3), s.state_log(3))
    assert_record(g.get_score(), s.get_score(), "group")
    it, u0 = s.step_log(3)
    assert_record(s.get_score(), scs.score_reference_batch(s.state_log(3), u0, setup, k0=2), "the single batch")
    assert_scored(s, "jit", counter=5)
    assert np.any(s.get_score()[2] > 0)
    for k in range(g.shards):
        h = tm.lib().tiny_group_shard(g._h, k)
        opt = lambda n: int(tm.lib().tiny_batch_get_option(h, n))
        assert (opt(b"score"), opt(b"last_score"), opt(b"score_step"), opt(b"last_half_rows"), opt(b"last_prefetch"), tm.lib().tiny_batch_kernel_path(h)) == (2, 1, 5, 0, 0, 3)
    # one setup for all shards, and removal
    g.set_score(*[a[2] for a in setup])
    h = tm.lib().tiny_group_shard(g._h, 1)
    assert int(tm.lib().tiny_batch_get_option(h, b"score")) == 1 and np.array_equal(g.get_score()[3], np.full(c["B"], -1, dtype=np.int32))
    g.reset_score()
    g.set_score(None)
    assert int(tm.lib().tiny_batch_get_option(h, b"score")) == 0
    g.close()
    s.close()


# ---- 12. -----------------------------------------------------------------------------------------------------------------------------
def test_the_example_prints_what_the_reference_scores_on_its_own_logs(tmp_path):
    """examples/closed_loop_score.c (C99, built by __graft_entry__.build()): point masses holding a hover point in gusts, behind sensor
    noise and an estimator, 60 fused steps on a PS form with no log on; with a file name it flies the episode again without the score and
    writes both logs -- the numbers it printed are the reference's on those logs, bit for bit"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "closed_loop_score")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/closed_loop_score is missing: __graft_entry__.build() produces it")
    dump = str(tmp_path / "logs.bin")
    p = subprocess.run([exe, dump], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "kernel path 3, score 2 (applied 1, counter 60), state_log 0" in p.stdout and "logs: kernel path 3, score 0 (applied 0)" in p.stdout, p.stdout
    raw = open(dump, "rb").read()
    steps, B, nx, nu = np.frombuffer(raw[:16], dtype=np.int32)
    nz = nx + nu
    body = np.frombuffer(raw[16:], dtype=np.float64)
    assert body.size == 4 * B * nz + steps * B * nz
    setup = tuple(body[i * B * nz:(i + 1) * B * nz].reshape(B, nz) for i in range(4))
    states = body[4 * B * nz:4 * B * nz + steps * B * nx].reshape(steps, B, nx)
    u0 = body[4 * B * nz + steps * B * nx:].reshape(steps, B, nu)
    # (4 096 instances x 60 steps in plain Python floats would take a minute: the same three roundings per term and the same order,
    # vectorised over the instances -- numpy's elementwise double operations are the IEEE ones)
    cost, worst, count = np.zeros(B), np.zeros(B), np.zeros(B, dtype=int)
    w, tg, lo, hi = setup
    for k in range(steps):
        z = np.concatenate([states[k], u0[k]], axis=1)
        for c in range(nz):
            d = z[:, c] - tg[:, c]
            cost = cost + (w[:, c] * d) * d
        m = np.maximum(np.max(np.maximum(z - hi, lo - z), axis=1), 0.0)
        worst = np.maximum(worst, m)
        count += m > 0.0
    some = [0, 1, B // 2, B - 1]                                      # ... checked against the plain-float reference on a few instances
    for i in some:
        r = scs.score_reference(states[:, i], u0[:, i], tuple(a[i] for a in setup))
        assert (r[0], r[1], r[2]) == (cost[i], worst[i], count[i]), i
    line = {ln.split()[1]: ln for ln in p.stdout.splitlines() if ln.startswith("score: ")}
    assert "score: %d of %d instances ever left their corridor" % (int(np.sum(count > 0)), B) in p.stdout and "%d violated steps" % int(np.sum(count)) in p.stdout
    assert 0 < int(np.sum(count > 0)) < B
    assert float(line["largest"].split()[-1]) == np.max(worst)
    words = line["cost"].split()
    ordered = np.sort(cost)
    assert (float(words[3]), float(words[5]), float(words[7])) == (ordered[0], ordered[B // 2], ordered[-1])
