"""CPU: the numpy model of the box step of update_slack + update_dual (tests/box_ref.py) against the C restatement's phases, bit for
bit, and against the real reference's recorded answers (tests/golden/box_edges.npz) on every class of bound pair and t; which of the
two clamp rules -- the ternaries of oracle/tinympc_oracle.c:363 or IEEE maxNum / minNum -- the real reference follows where they
differ (a NaN bound; a zero bound meeting a zero t); and the preconditions of the batches tests/test_gpu_box_edges.py launches, on the
oracle, for every shape it launches them at."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import box_ref as br  # noqa: E402
import scenarios as sc  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "box_edges.npz")
SMALL_DIMS = ((4, 2, 10), (3, 2, 4), (12, 4, 10), (2, 2, 3), (3, 2, 2))
OUT = (("vnew", "g"), ("znew", "y"), ("g", "g"), ("y", "y"))         # (output field, the label array that goes with it)


def oracle_phases(suite, x, u, g, y):
    """update_slack, then update_dual, in the oracle on x, u, g, y set directly, per instance -> {vnew, znew, g, y}"""
    o = sc.make_solver(OracleSolver, suite["problem"], suite["config"])
    out = {k: np.zeros_like(g if k in ("vnew", "g") else y) for k in ("vnew", "znew", "g", "y")}
    for b in range(g.shape[0]):
        o["x"], o["u"], o["g"], o["y"] = x[b], u[b], g[b], y[b]
        o.phase("update_slack")
        out["vnew"][b], out["znew"][b] = o["vnew"], o["znew"]
        o.phase("update_dual")
        out["g"][b], out["y"][b] = o["g"], o["y"]
    o.close()
    return out


def assert_bits(got, want, what, mask=None):
    same = br.same_bits(got, want)
    if mask is not None:
        same = same | ~mask
    assert same.all(), (what, int((~same).sum()), "of", same.size, "first", tuple(np.argwhere(~same)[0]), got[~same][:3], want[~same][:3])


def value_compared(labels):
    return np.isin(labels, [br.CLASSES.index(c) for c in br.VALUE_COMPARED])


def all_rounds(dims, phase):
    return [(u, m, s, l) for u in (False, True) for m, (s, l) in enumerate(br.class_rounds(*dims, u, phase=phase))]


# ---- the model is the oracle
@pytest.mark.parametrize("dims", SMALL_DIMS)
def test_ternary_model_equals_the_oracles_phases_on_every_class(dims):
    """update_slack + update_dual alone on the phase rounds (x | u nonzero on odd instances, t = NaN and +-inf included): vnew, znew, g, y
    bit for bit, NaN equal to NaN; and on every class but the two value-compared ones the two rules give the same bits"""
    seen = set()
    for uniform, m, suite, labels in all_rounds(dims, True):
        x, u, g, y = br.phase_inputs(suite)
        got = oracle_phases(suite, x, u, g, y)
        tern, mm = br.step(suite["config"], x, u, g, y, "ternary"), br.step(suite["config"], x, u, g, y, "minmaxnum")
        for k, lab in OUT:
            assert_bits(got[k], tern[k], (dims, uniform, m, k))
            assert_bits(mm[k], tern[k], (dims, uniform, m, k, "the rules differ outside zero_tie and nan_bound"), ~value_compared(labels[lab]))
        seen |= set(br.class_counts(labels))
    assert seen == set(br.CLASSES), set(br.CLASSES) - seen


@pytest.mark.parametrize("dims", SMALL_DIMS)
def test_every_class_at_every_row_and_at_the_end_knots(dims):
    """over the rounds of a class batch every class other than the phase-only ones occurs at every row, and at state knots 0 and N - 1
    and input knots 0 and N - 2; zero_tie and nan_bound together are at most 10 % of the entries; a uniform round's box is uniform"""
    nx, nu, N = dims
    want = set(range(len(br.CLASSES))) - {br.CLASSES.index(c) for c in br.PHASE_ONLY}
    for uniform in (False, True):
        rounds = br.class_rounds(*dims, uniform)
        for fam, rows, last in (("g", nx, N - 1), ("y", nu, N - 2)):
            lab = np.stack([l[fam] for _, l in rounds])                    # (rounds, B, rows, knots)
            need = want - ({br.CLASSES.index("nan_bound")} if uniform else set())
            for j in range(rows):
                assert need <= set(lab[:, :, j].ravel().tolist()), (dims, uniform, fam, j)
            for k in {0, last}:
                assert need <= set(lab[:, :, :, k].ravel().tolist()), (dims, uniform, fam, k)
        lab = np.concatenate([np.concatenate([l["g"].ravel(), l["y"].ravel()]) for _, l in rounds])
        assert value_compared(lab).mean() <= 0.10, value_compared(lab).mean()
        assert all(br.box_uniform(s["config"], N) == (uniform and N >= 2) for s, _ in rounds)


# ---- the real reference
def test_the_golden_file_is_the_model_and_names_the_references_rule():
    """tests/golden/box_edges.npz (the REAL reference's update_slack + update_dual on the phase rounds of FIXTURE_DIMS): the inputs are
    the builder's, the outputs the model's bit for bit on every class but zero_tie and nan_bound.  On those two the file shows which
    rule the reference follows -- the test finds it and holds the ORACLE, which claims to restate the reference, to the file bit for
    bit there too.  (The kernels follow IEEE maxNum / minNum; INTEGRATION.md states the divergence.)"""
    z = np.load(GOLDEN)
    assert tuple(z["dims"]) == br.FIXTURE_DIMS
    agree = {r: {c: [0, 0] for c in br.VALUE_COMPARED} for r in ("ternary", "minmaxnum")}
    entries = 0
    for tag, suite, labels in br.fixture_rounds():
        ins = dict(zip(("x", "u", "g", "y"), br.phase_inputs(suite)))
        for k in ("x_min", "x_max", "u_min", "u_max"):
            assert br.same_bits(z["%s.%s" % (tag, k)], suite["config"][k]).all(), (tag, k)
        for k, v in ins.items():
            assert br.same_bits(z["%s.in.%s" % (tag, k)], v).all(), (tag, k)
        for k, v in labels.items():
            assert np.array_equal(z["%s.label.%s" % (tag, k)], v), (tag, k)
        model = {r: br.step(suite["config"], *ins.values(), rule=r) for r in agree}
        ora = oracle_phases(suite, *ins.values())
        for k, lab in OUT:
            ref = z["%s.out.%s" % (tag, k)]
            vc = value_compared(labels[lab])
            assert_bits(ref, model["minmaxnum"][k], (tag, k, "model"), ~vc)
            assert_bits(ref, ora[k], (tag, k, "the oracle against the real reference, every class"))
            for r in agree:
                same = br.same_bits(ref, model[r][k])
                for c in br.VALUE_COMPARED:
                    at = labels[lab] == br.CLASSES.index(c)
                    agree[r][c][0] += int(same[at].sum())
                    agree[r][c][1] += int(at.sum())
            entries += ref.size
    print("box edges golden: %d outputs; agreement with the real reference on the value-compared classes: %s" % (entries, agree))
    for c in br.VALUE_COMPARED:
        assert agree["ternary"][c][1] > 0 and agree["ternary"][c][0] == agree["ternary"][c][1], ("the reference does not follow the ternaries on", c, agree)
    # and the two rules do differ there: the file decides between them
    assert agree["minmaxnum"]["nan_bound"][0] < agree["minmaxnum"]["nan_bound"][1]
    assert agree["minmaxnum"]["zero_tie"][0] < agree["minmaxnum"]["zero_tie"][1]
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "halfspace_edges.npz"))


# ---- the preconditions of the GPU batches, on the oracle
def solve(suite, fields=("x", "u") + br.FIELDS):
    return sc.run_cases(OracleSolver, suite, fields=fields)


def check_first_iteration(suite, out, what, labels=None):
    """the oracle's solve against the model through the oracle's own x, u: fields and residuals bit for bit (ternary), and against the
    minmaxnum model outside the value-compared classes"""
    assert np.all(out["iter"] == 1), what
    for rule in ("ternary", "minmaxnum"):
        want = br.first_iteration(suite, out["x"], out["u"], rule)
        for k in br.FIELDS:
            lab = None if labels is None else labels["g" if k in ("vnew", "g", "v") else "y"]
            mask = None if (rule == "ternary" or lab is None) else ~value_compared(lab)
            assert_bits(out[k], want[k], (what, rule, k), mask)
        if rule == "ternary":
            for k in br.RESIDUALS:
                assert_bits(out[k], want[k], (what, k))
            assert np.array_equal(out["sol_solved"].astype(int), want["solved"]), what
            assert br.margin_to_tolerance(suite["config"], want) > 1e-6, (what, "a residual within 1e-6 of its tolerance")


@pytest.mark.parametrize("dims", br.GPU_DIMS)
def test_zero_trajectory_batches_on_the_oracle(dims):
    """position batches and class rounds: x and u are zeros, so t = g wherever g is not a zero; the oracle's fields and residuals are
    the model's; in the knot-varying position batch every entry's slack differs from what the bound pair of ANY neighbour (row +- 1,
    knot +- 1, the diagonals too) would have given"""
    nx, nu, N = dims
    for uniform in (False, True):
        suite, labels, table = br.position_batch(*dims, uniform)
        out = solve(suite)
        assert not np.any(out["x"]) and not np.any(out["u"]), (dims, uniform)
        check_first_iteration(suite, out, (dims, "position", uniform), labels)
        assert len(table) == nx * N + nu * (N - 1) + br.CONTROLS
        quiet = table[:, 0] < 0
        assert np.all(out["sol_solved"][quiet] == 1) and not np.any(out["sol_solved"][~quiet]), (dims, uniform, "the controls stop, nothing else does")
        if not uniform:
            cfg = suite["config"]
            lo = np.full((nx + nu, N), np.nan)
            hi = np.full((nx + nu, N), np.nan)
            lo[:nx], hi[:nx], lo[nx:, :-1], hi[nx:, :-1] = cfg["x_min"], cfg["x_max"], cfg["u_min"], cfg["u_max"]
            t = np.full((len(table) - br.CONTROLS, nx + nu, N), np.nan)
            t[:, :nx], t[:, nx:, :-1] = suite["cases"]["g"][~quiet], suite["cases"]["y"][~quiet]
            own = br.clamp(lo, hi, t)
            assert not br.box_uniform(cfg, N) and np.all((own == lo) | (own == hi) | np.isnan(lo))
            for dj in (-1, 0, 1):
                for dk in (-1, 0, 1):
                    if (dj, dk) == (0, 0):
                        continue
                    nlo, nhi = np.roll(lo, (dj, dk), axis=(0, 1)), np.roll(hi, (dj, dk), axis=(0, 1))      # (wraps: one more neighbour each)
                    other = br.clamp(nlo, nhi, t)
                    ok = (other != own) | np.isnan(lo) | np.isnan(nlo)
                    assert ok.all(), (dims, dj, dk)
    for uniform in (False, True):
        for m, (suite, labels) in enumerate(br.class_rounds(*dims, uniform)):
            out = solve(suite)
            assert not np.any(out["x"]) and not np.any(out["u"]), (dims, uniform, m)
            check_first_iteration(suite, out, (dims, "classes", uniform, m), labels)
    # one entry an ulp off the common pair: not uniform, and taking it for uniform changes bits at that entry
    for name, suite, labels in br.odd_one_out_suites(*dims):
        out = solve(suite)
        assert not np.any(out["x"]) and not np.any(out["u"]), (dims, name)
        check_first_iteration(suite, out, (dims, name), labels)
        assert not br.box_uniform(suite["config"], N) and br.box_uniform(suite["common_config"], N)
        as_uniform = br.first_iteration(dict(suite, config=suite["common_config"]), out["x"], out["u"])
        assert any(not br.same_bits(as_uniform[k], out[k]).all() for k in ("vnew", "znew")), (dims, name)


@pytest.mark.parametrize("dims", br.GPU_DIMS)
def test_identity_and_switch_suites_on_the_oracle(dims):
    """real dynamics: the oracle's own x, u and the warm duals give its slacks, duals, v, z and residuals through the model; at least a
    quarter of the state and of the input entries clamp low, a quarter high, a quarter stay inside; the switch suites pass a disabled
    family's t through"""
    for uniform in (False, True):
        suite = br.identity_suite(*dims, uniform)
        out = solve(suite)
        check_first_iteration(suite, out, (dims, "identity", uniform))
        assert br.box_uniform(suite["config"], dims[2]) == (uniform and dims[2] >= 2)
        for low, high, inside in br.shares(suite["config"], out["x"] + suite["cases"]["g"], out["u"] + suite["cases"]["y"]):
            assert min(low, high, inside) >= 0.25, (dims, uniform, low, high, inside)
    for name, suite in br.enable_suites(*dims):
        out = solve(suite)
        check_first_iteration(suite, out, (dims, name))
        cfg = suite["config"]
        if not cfg["en_state_bound"] or not cfg["bounds_set"]:
            assert_bits(out["vnew"], out["x"] + suite["cases"]["g"], (dims, name, "state t passes through"))
        if not cfg["en_input_bound"] or not cfg["bounds_set"]:
            assert_bits(out["znew"], out["u"] + suite["cases"]["y"], (dims, name, "input t passes through"))


@pytest.mark.parametrize("dims", ((12, 4, 10), (4, 2, 10), (4, 2, 50)))
def test_pure_map_family_iterates_the_box_map_on_the_oracle(dims):
    """A = B = 0, 3 iterations: the oracle's state rows are the model's map iterated, bit for bit, and the map does move: the dual
    grows at knot 0 where x0 lies outside its bounds"""
    suite = br.pure_map_suite(*dims)
    out = solve(suite)
    assert np.all(out["iter"] == 3)
    want = br.pure_map_want(suite, "ternary")
    for k in want:
        assert_bits(out[k], want[k], (dims, k))
        assert_bits(want[k], br.pure_map_want(suite)[k], (dims, k, "rules"))
    assert np.array_equal(out["x"][:, :, 0], suite["cases"]["x0"]) and not np.any(out["x"][:, :, 1:])
    one = br.pure_map_want(dict(suite, config=dict(suite["config"], max_iter=1)))
    assert np.mean(one["g"] != want["g"]) > 0.05
