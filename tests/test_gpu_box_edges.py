"""GPU: the box clamp of update_slack + update_dual (admm.cpp:85-98, 222-225) on every kernel form, bit for bit against tests/box_ref.py
(the numpy model that tests/test_box_ref_cpu.py pins to the oracle bit for bit and to the real reference on tests/golden/box_edges.npz).

The project spells the clamp many ways: inside the inline-asm fused forward steps of the one-row kernel (max and min split around a DPP
chain, back to back in the INPLACE form, a copy of its own in the half-row form), vclamp64 and vmin64(hi, vmax64(lo, t)) elsewhere in
that kernel, vmin64 / vmax64 in three places of the tile kernel with the bounds from LDS or -- the UB forms -- from registers, fmin /
fmax twice in the coverage kernel; and the host writes the bound tables three times, input bounds one slot late.  The step is exact
arithmetic -- one rounded add, one max, one min, one rounded subtract -- so every form must give the model's bits: from zeros (x0 = 0,
references 0, warm vnew = g: x = u = 0 on any implementation and t = g) on batches where every (row, knot) has a bound pair of its
own and where every class of (lo, hi, t) meets every (row, knot); from its own x, u on real dynamics; through the single-phase entry
points; with a family switched off; and carried over three iterations.  The kernels follow IEEE maxNum / minNum, the reference a pair
of ternaries: the two differ on a NaN bound and in the sign of a zero when a zero bound meets a zero t -- there the
kernels are held to the maxNum / minNum model as numbers, and to each other bit for bit.  Every test asserts which kernel form ran."""
import ctypes as C
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import box_ref as br  # noqa: E402
from hip_runner import IN_FIELDS  # noqa: E402
from test_gpu_termination_edges import FORMS, ONE_ROW, tile_dims_has  # noqa: E402

pytestmark = pytest.mark.gpu

# (id, dims, options, what must have run, extra): the termination suite's forms (those tile_dims.txt has), then the box's own.
# extra: ub = the form has a UB variant (dispatcher: dpp_mode 2, no debug outputs; the coverage kernel has none), hetero = per-instance
# problem data (every instance the same problem), cone = a state cone next to the box
BOX_FORMS = [(n, d, o, e, dict(ub=e["path"] != ("cover",))) for n, d, o, e in FORMS if "tile_w" not in o or tile_dims_has(d, o["tile_w"])] + [
    ("one_row_12_4_10_dpp_mode_0", (12, 4, 10), dict(ONE_ROW, dpp_mode=0), dict(path=("regs",), last_half_rows=0), dict(ub=False)),
    ("one_row_12_4_10_dpp_mode_1", (12, 4, 10), dict(ONE_ROW, dpp_mode=1), dict(path=("regs",), last_half_rows=0), dict(ub=False)),
    ("one_row_12_4_10_debug", (12, 4, 10), dict(ONE_ROW, debug=1), dict(path=("regs",), last_half_rows=0), dict(ub=False)),
    ("one_row_8_8_10_full_row", (8, 8, 10), dict(ONE_ROW), dict(path=("regs",), last_half_rows=0), dict(ub=True)),
    ("one_row_4_1_10_one_input", (4, 1, 10), dict(ONE_ROW), dict(path=("regs",)), dict(ub=True)),
    ("one_row_2_2_3", (2, 2, 3), dict(ONE_ROW), dict(path=("regs",)), dict(ub=True)),
    ("one_row_6_3_10_cone", (6, 3, 10), dict(ONE_ROW), dict(path=("regs",)), dict(ub=True, cone=True)),
    ("one_row_12_4_10_per_instance_data_het_ub1", (12, 4, 10), dict(ONE_ROW, het_ub=1), dict(path=("regs",)), dict(ub=True, hetero=True)),
    ("one_row_12_4_10_per_instance_data_het_ub0", (12, 4, 10), dict(ONE_ROW, het_ub=0), dict(path=("regs",)), dict(ub=False, hetero=True)),
    ("tile_20_8_10_widest", (20, 8, 10), {}, dict(path=("tile",), tile_w=2), dict(ub=True)),
    ("cover_3_2_2_two_knots", (3, 2, 2), dict(no_jit=1), dict(path=("cover",)), dict(ub=False)),
]
BOX_IDS = [f[0] for f in BOX_FORMS]
assert {f[1] for f in BOX_FORMS} <= set(br.GPU_DIMS)
BY_ID = {f[0]: f for f in BOX_FORMS}
READ_BACKS = ("last_tile_form", "last_half_rows", "last_prefetch", "last_prefetch_grid", "last_tile_dyn", "last_uniform_bounds")
# what v_max_f64 / v_min_f64 returned for a zero bound meeting a zero t, as the forms that ran so far found it: pattern -> (sign of
# the slack, the form that first saw it).  Every form must find the same
ZERO_TIES = {}


def make(suite, extra):
    import tinympc_amd as tm
    prob, cfg = suite["problem"], suite["config"]
    B = suite["cases"]["x0"].shape[0]
    if extra.get("hetero"):
        rep = lambda a: np.stack([np.asarray(a, dtype=float)] * B)                  # noqa: E731
        s = tm.TinyBatchSolver.hetero(rep(prob["A"]), rep(prob["B"]), rep(prob["f"]), rep(prob["Q"]), rep(prob["R"]), np.full(B, prob["rho"]), prob["N"])
    else:
        s = tm.TinyBatchSolver.from_problem(prob, B)
    if cfg.get("bounds_set", True):
        s.set_bound_constraints(cfg["x_min"], cfg["x_max"], cfg["u_min"], cfg["u_max"])
    if extra.get("cone"):
        s.set_cone_constraints([0], [3], [0.5], [], [], [])
    s.update_settings(cfg["abs_pri_tol"], cfg["abs_dua_tol"], cfg["max_iter"], cfg["check_termination"], cfg["en_state_bound"], cfg["en_input_bound"],
                      1 if extra.get("cone") else 0, 0)
    return s


def solve(suite, form, uniform_bounds=1):
    """one launch of the suite on the form -> its fields, status, and what the dispatcher reports; the form that ran is asserted, the UB
    decision too: a UB form ran exactly when the option is on, the form has one and box_is_uniform holds for the enabled families"""
    name, dims, options, expect, extra = form
    cases, cfg = suite["cases"], suite["config"]
    s = make(suite, extra)
    for k, v in dict(options, uniform_bounds=uniform_bounds).items():
        s.set_option(k, v)
    s.set_x0(cases["x0"])
    for f in IN_FIELDS:
        s.set(f, cases[f])
    s.solve()
    out = {k: s.get(k) for k in ("x", "u") + br.FIELDS}
    st = s.status()
    ran = dict(path=s.kernel_path())
    for k in READ_BACKS:
        ran[k] = s.get_option(k)
    s.close()
    if ran["path"] == "tile":
        ran["tile_w"], ran["tile_r"] = ran["last_tile_form"] // 1000000, ran["last_tile_form"] // 1000 % 1000
    what = (name, "asked for", options, "uniform_bounds", uniform_bounds, "expected", expect, "ran", ran)
    for k, v in expect.items():
        assert (ran[k] in v) if k == "path" else (ran.get(k) == v), what
    want_ub = bool(uniform_bounds and extra["ub"] and options.get("het_ub", 1) and br.box_uniform(cfg, dims[2]))
    assert ran["last_uniform_bounds"] == int(want_ub), what
    out.update({k: np.asarray(st[k], dtype=float) for k in br.RESIDUALS})
    out.update(iter=st["iter"].astype(int), solved=st["solved"].astype(int))
    return out, ran


def first_difference(got, want, labels=None):
    same = br.same_bits(got, want)
    if same.all():
        return None
    at = tuple(np.argwhere(~same)[0])
    return dict(entries=int((~same).sum()), of=int(same.size), first=at, got=float(got[at]).hex(), want=float(want[at]).hex(),
                classes=None if labels is None else sorted({br.CLASSES[c] for c in labels[~same]}))


def note_zero_ties(who, cfg, field, t, slack, labels):
    """the zero-tie entries of one slack field: equal to the model as numbers (a zero), and the sign the hardware chose for each pattern
    of signs is the one every other form found"""
    lo, hi = (np.broadcast_to(a, t.shape[1:]) for a in br.bounds_at(cfg, field))
    for b, j, k in np.argwhere(labels == br.CLASSES.index("zero_tie")):
        assert slack[b, j, k] == 0.0 and t[b, j, k] == 0.0, (who, field, (b, j, k), slack[b, j, k])
        pat = br.zero_tie_pattern(lo[j, k], hi[j, k], t[b, j, k])
        sign = "-0" if np.signbit(slack[b, j, k]) else "+0"
        first = ZERO_TIES.setdefault(pat, (sign, who))
        assert first[0] == sign, ("forms disagree on a zero tie", pat, "here", who, sign, "before", first)


def check_first_iteration(suite, out, who, labels=None):
    """the six fields of a max_iter = 1 solve through the model from the solve's OWN x, u: bit for bit, except that a zero-tie entry's
    slack is compared as a number (and across forms, note_zero_ties) and what follows from it -- its dual, v | z -- through that slack;
    the four residuals == the model's (a NaN slack -- both bounds NaN -- is passed over by the maxima, as the oracle's do)"""
    assert np.all(out["iter"] == 1), (who, out["iter"])
    cfg, cases = suite["config"], suite["cases"]
    want = br.first_iteration(suite, out["x"], out["u"])
    assert np.array_equal(out["solved"], want["solved"]), who
    for slack, dual, prev, src, warm in (("vnew", "g", "v", "x", "g"), ("znew", "y", "z", "u", "y")):
        lab = None if labels is None else labels[warm]
        tie = np.zeros(out[slack].shape, dtype=bool) if lab is None else lab == br.CLASSES.index("zero_tie")
        with np.errstate(all="ignore"):
            t = out[src] + cases[warm]
        if tie.any():
            note_zero_ties(who, cfg, slack, t, out[slack], lab)
            for k in (slack, dual, prev):
                want[k] = want[k].copy()
            want[slack][tie] = out[slack][tie]
            want[dual][tie] = (t - out[slack])[tie]
            want[prev][tie] = np.where(want["solved"][:, None, None] == 1, cases[prev], out[slack])[tie]
        for k in (slack, dual, prev):
            d = first_difference(out[k], want[k], lab)
            assert d is None, (who, k, d)
    for k in br.RESIDUALS:
        bad = np.flatnonzero(~br.same_bits(np.abs(out[k]), np.abs(want[k])))
        assert bad.size == 0, (who, k, "instance", int(bad[0]), "got", out[k][bad[0]], "model", want[k][bad[0]])


# ---- (a) every position's bound on its own
@pytest.mark.parametrize("form", BOX_FORMS, ids=BOX_IDS)
def test_every_position_is_clamped_by_its_own_bound_pair(form):
    """max_iter = 1 from zeros.  Knot-varying box: every (row, knot) has a bound pair no other entry has and every entry of every
    instance lies outside its own, so each slack IS its own table entry -- a bound read from a neighbouring knot, row or slot differs
    in the bits; no UB form may run.  Knot-invariant box, one pair per row: instance (j, k) has a directed t at (j, k); with
    uniform_bounds = 1 a UB form must run (where the form has one), with 0 the table form.  vnew, znew, g, y, v, z are the model's bit
    for bit, x and u zeros, the four residuals == the model's.  The last instances are quiet controls: every entry inside its pair and
    tiny, so they -- and only they -- stop at iteration 1 with v, z untouched, unless a lane that holds no entry is clamped onto a
    bound that excludes 0 and reaches a residual."""
    name, dims = form[0], form[1]
    t0 = time.time()
    for uniform in (False, True):
        suite, labels, table = br.position_batch(*dims, uniform)
        for ub in ((1, 0) if uniform else (1,)):
            out, ran = solve(suite, form, ub)
            who = "%s %s position batch uniform=%s uniform_bounds=%d %s" % (name, dims, uniform, ub, ran)
            assert not np.any(out["x"]) and not np.any(out["u"]), who
            check_first_iteration(suite, out, who, labels)
            assert np.array_equal(out["solved"], (table[:, 0] < 0).astype(int)), (who, "the controls stop, nothing else does", out["solved"])
            print("box edges: %s B %d classes %s" % (who, len(table), br.class_counts(labels)))
    print("box edges: %s seconds %.2f" % (name, time.time() - t0))


@pytest.mark.parametrize("form", BOX_FORMS, ids=BOX_IDS)
def test_one_entry_an_ulp_off_the_common_pair_is_not_a_uniform_box(form):
    """one pair per row, except that ONE (row, knot) -- the first and the last knot of either family, one in the middle; a launch
    each -- has both bounds one ulp further out: no solution moves by 1e-9, but no UB form may run (solve() asserts it), and the row of
    the odd entry carries t on and around both pairs at every knot: bit for bit the model's"""
    name, dims = form[0], form[1]
    for spot, suite, labels in br.odd_one_out_suites(*dims):
        out, ran = solve(suite, form)
        who = "%s %s odd one out at %s %s" % (name, dims, spot, ran)
        assert ran["last_uniform_bounds"] == 0 and not np.any(out["x"]) and not np.any(out["u"]), who
        check_first_iteration(suite, out, who, labels)
        print("box edges: %s B %d classes %s" % (who, len(out["iter"]), br.class_counts(labels)))


# ---- (b) every class at every (row, knot)
@pytest.mark.parametrize("form", BOX_FORMS, ids=BOX_IDS)
def test_every_class_of_bound_and_t_at_every_row_and_knot(form):
    """max_iter = 1 from zeros, the class rounds: over the rounds every (row, knot) of both families meets every kind of bound pair --
    ordinary, one-signed, three ulps wide, equal, crossed, infinite, +-1e17, subnormal, a zero of either sign, NaN -- with t on, one
    ulp inside and outside, and far from each bound.  Bit for bit against the maxNum / minNum model; a zero bound meeting a zero t as
    a number, with the sign every other form found.  Knot-invariant rounds with uniform_bounds 1 and 0."""
    name, dims = form[0], form[1]
    t0 = time.time()
    counts, launches, ub_ran = {}, 0, 0
    for uniform in (False, True):
        for m, (suite, labels) in enumerate(br.class_rounds(*dims, uniform)):
            for ub in ((1, 0) if uniform else (1,)):
                out, ran = solve(suite, form, ub)
                who = "%s %s class round %d uniform=%s uniform_bounds=%d %s" % (name, dims, m, uniform, ub, ran)
                assert not np.any(out["x"]) and not np.any(out["u"]), who
                check_first_iteration(suite, out, who, labels)
                launches += 1
                ub_ran += ran["last_uniform_bounds"]
            for k, n in br.class_counts(labels).items():
                counts[k] = counts.get(k, 0) + n
    print("box edges: %s %s launches %d (UB forms %d) classes %s seconds %.2f" % (name, dims, launches, ub_ran, counts, time.time() - t0))
    print("box edges: zero ties on the hardware so far: %s" % {p: s for p, (s, _) in sorted(ZERO_TIES.items())})
    assert set(counts) == set(br.CLASSES) - set(br.PHASE_ONLY)


# ---- (c) the own-output identity on real dynamics
@pytest.mark.parametrize("form", BOX_FORMS, ids=BOX_IDS)
def test_own_outputs_reproduce_the_slacks_and_duals_on_real_dynamics(form):
    """random x0, references and warm state, max_iter = 1, a third of the entries pushed below, a third above their bounds: the
    kernel's own x, u and the warm g, y give its vnew, znew, g, y, v, z and its four residuals through the model, bit for bit -- a t
    formed from the wrong knot's x, or from u and y of different slots, does not.  Knot-varying and knot-invariant bounds."""
    name, dims = form[0], form[1]
    for uniform in (False, True):
        suite = br.identity_suite(*dims, uniform)
        for ub in ((1, 0) if uniform else (1,)):
            out, ran = solve(suite, form, ub)
            who = "%s %s identity uniform=%s uniform_bounds=%d %s" % (name, dims, uniform, ub, ran)
            assert np.any(out["x"][:, :, 1:]) and np.any(out["u"]), who
            check_first_iteration(suite, out, who)
            low, high, inside = br.shares(suite["config"], out["x"] + suite["cases"]["g"], out["u"] + suite["cases"]["y"])[0]
            print("box edges: %s state entries low %.2f high %.2f inside %.2f" % (who, low, high, inside))


# ---- (d) the single-phase entry points
def phase_check(who, suite, labels, got):
    x, u, g, y = br.phase_inputs(suite)
    want = br.step(suite["config"], x, u, g, y)
    for slack, dual, src in (("vnew", "g", x), ("znew", "y", u)):
        lab = labels[dual][:got[slack].shape[0]]
        tie = lab == br.CLASSES.index("zero_tie")
        with np.errstate(all="ignore"):
            t = (src + suite["cases"][dual])[:got[slack].shape[0]]
            own = t - got[slack]
        note_zero_ties(who, suite["config"], slack, t, got[slack], lab)
        ws, wd = want[slack][:len(lab)].copy(), want[dual][:len(lab)].copy()
        ws[tie], wd[tie] = got[slack][tie], own[tie]
        for k, w in ((slack, ws), (dual, wd)):
            d = first_difference(got[k], w, lab)
            assert d is None, (who, k, d)


@pytest.mark.parametrize("dims", [br.FIXTURE_DIMS, (4, 2, 10), (12, 4, 10), (20, 4, 10)])
def test_phase_kernel_update_slack_then_update_dual_on_every_class(dims):
    """tiny_batch_phase("update_slack"), then "update_dual", with x, u, g, y set directly (x | u carry half of t on odd instances): every
    class, t = NaN and t = +-inf included, bit for bit against the maxNum / minNum model.  (tiny_batch_phase launches the coverage
    kernel's single-phase form whatever the shape; kernel_path() describes solves only -- nothing to assert.)"""
    counts = {}
    for uniform in (False, True):
        for m, (suite, labels) in enumerate(br.class_rounds(*dims, uniform, phase=True)):
            s = make(suite, {})
            for k, v in zip(("x", "u", "g", "y"), br.phase_inputs(suite)):
                s.set(k, v)
            s.phase("update_slack")
            got = dict(vnew=s.get("vnew"), znew=s.get("znew"))
            assert np.all(br.same_bits(s.get("g"), suite["cases"]["g"])) and np.all(br.same_bits(s.get("y"), suite["cases"]["y"]))
            s.phase("update_dual")
            got.update(g=s.get("g"), y=s.get("y"))
            s.close()
            phase_check("phase kernel %s round %d uniform=%s" % (dims, m, uniform), suite, labels, got)
            for k, n in br.class_counts(labels).items():
                counts[k] = counts.get(k, 0) + n
    print("box edges: phase kernel %s classes %s" % (dims, counts))
    print("box edges: zero ties on the hardware so far: %s" % {p: s for p, (s, _) in sorted(ZERO_TIES.items())})
    assert set(counts) == set(br.CLASSES)


def test_exported_update_slack_and_update_dual_on_a_solver_struct():
    """update_slack(TinySolver*), then update_dual(TinySolver*), called as a reference caller would on ONE solver struct whose bounds
    are set anew for every round (tiny_set_bound_constraints) and whose x, u, g, y are written directly: the first three instances of
    every phase round of the fixture's shape, bit for bit against the maxNum / minNum model"""
    import pod
    import tinympc_amd as tm
    from test_gpu_phases import _pod_solver
    L = tm.lib()
    nx, nu, N = br.FIXTURE_DIMS
    keep, sp, counts = [], None, {}
    for name in ("update_slack", "update_dual"):
        getattr(L, name).argtypes, getattr(L, name).restype = [C.POINTER(pod.TinySolver)], None
    for uniform in (False, True):
        for m, (suite, labels) in enumerate(br.class_rounds(nx, nu, N, uniform, phase=True)):
            cfg = dict(suite["config"], en_state_soc=0, en_input_soc=0)
            if sp is None:
                sp = _pod_solver(L, pod, suite["problem"], cfg, keep)
            bs = [pod.mat(cfg[k]) for k in ("x_min", "x_max", "u_min", "u_max")]
            keep.append(bs)
            assert L.tiny_set_bound_constraints(sp, *[C.byref(b[0]) for b in bs]) == 0
            w = sp.contents.work.contents
            ins = dict(zip(("x", "u", "g", "y"), br.phase_inputs(suite)))
            got = {k: np.zeros((3,) + ins[k2].shape[1:]) for k, k2 in (("vnew", "g"), ("znew", "y"), ("g", "g"), ("y", "y"))}
            for b in range(3):
                for k, v in ins.items():
                    pod.to_np(getattr(w, k))[...] = v[b]
                L.update_slack(sp)
                got["vnew"][b], got["znew"][b] = pod.to_np(w.vnew), pod.to_np(w.znew)
                L.update_dual(sp)
                got["g"][b], got["y"][b] = pod.to_np(w.g), pod.to_np(w.y)
            phase_check("exported symbols round %d uniform=%s" % (m, uniform), suite, labels, got)
            for k, n in br.class_counts({k: v[:3] for k, v in labels.items()}).items():
                counts[k] = counts.get(k, 0) + n
    L.tiny_destroy.argtypes = [C.POINTER(pod.TinySolver)]
    L.tiny_destroy(sp)
    print("box edges: exported update_slack / update_dual %s classes %s" % (br.FIXTURE_DIMS, counts))
    print("box edges: zero ties on the hardware so far: %s" % {p: s for p, (s, _) in sorted(ZERO_TIES.items())})
    assert set(counts) == set(br.CLASSES)


# ---- (e) the switches
@pytest.mark.parametrize("name", ["one_row_12_4_10_lazy", "tile_20_4_10_two_rows_wide", "cover_4_2_10_forced"])
def test_a_disabled_family_passes_t_through_and_only_enabled_families_decide_ub(name):
    """finite, tight bounds set, then en_state_bound = 0 | en_input_bound = 0 | both 0 | bounds never set, each with the state box
    knot-invariant and the input box knot-varying, and the reverse: every field through the own-output identity bit for bit -- a
    disabled family's slack is fl(x + g) untouched, its dual t - t -- and a UB form runs exactly when box_is_uniform holds for the
    families that are ON (solve() asserts it)"""
    form = BY_ID[name]
    ubs = []
    for case, suite in br.enable_suites(*form[1]):
        out, ran = solve(suite, form)
        who = "%s %s switches %s %s" % (name, form[1], case, ran)
        check_first_iteration(suite, out, who)
        cfg, cases = suite["config"], suite["cases"]
        for flag, slack, dual, src, warm in (("en_state_bound", "vnew", "g", "x", "g"), ("en_input_bound", "znew", "y", "u", "y")):
            if not cfg[flag] or not cfg["bounds_set"]:
                t = out[src] + cases[warm]
                assert first_difference(out[slack], t) is None and not np.any(out[dual]), (who, slack)
            else:
                assert np.any(out[dual]), (who, dual, "an enabled family that clamps nothing")
        ubs.append(ran["last_uniform_bounds"])
        print("box edges: %s box_is_uniform %s" % (who, br.box_uniform(cfg, form[1][2])))
    assert form[4]["ub"] == (0 < sum(ubs) < len(ubs)), (name, ubs)


# ---- (f) carried state
@pytest.mark.parametrize("name", ["one_row_12_4_10_lazy", "one_row_4_2_10_half_rows", "tile_4_2_50_v_in_its_record", "cover_4_2_10_forced"])
def test_three_iterations_of_the_pure_map_family_iterate_the_box_map(name):
    """A = B = 0: x is x0 at knot 0 and +0 afterwards in every iteration, so after 3 iterations the state rows' vnew, g and v are the
    model's map iterated from the warm g, bit for bit -- the dual a form carries from one iteration to the next is the one it wrote"""
    form = BY_ID[name]
    suite = br.pure_map_suite(*form[1])
    out, ran = solve(suite, form)
    who = "%s %s pure map %s" % (name, form[1], ran)
    assert np.all(out["iter"] == 3) and not out["solved"].any(), who
    assert np.array_equal(out["x"][:, :, 0], suite["cases"]["x0"]) and not np.any(out["x"][:, :, 1:]), who
    want = br.pure_map_want(suite)
    for k in ("vnew", "g", "v"):
        assert first_difference(out[k], want[k]) is None, (who, k, first_difference(out[k], want[k]))
    one = br.pure_map_want(dict(suite, config=dict(suite["config"], max_iter=1)))
    print("box edges: %s B %d entries whose dual moved after iteration 1: %.2f" % (who, out["g"].shape[0], float(np.mean(one["g"] != want["g"]))))
