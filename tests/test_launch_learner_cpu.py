"""CPU: the rules by which the dispatch learns a batch's launch form (csrc/launch_learner.hpp), checked on the learner itself.  It is plain
C++ without a HIP call, so tests/dropin/launch_learner_driver.cpp feeds it a script of events -- named after its transitions -- and prints
the whole state and every query's answer after each.  The expected states below are restated from the rules (each named beside its
table), not read off the learner: a silent change of a threshold, of a reset's field list or of the order of the steps of a probe's
arrival costs speed, never correctness, so no result test sees it (profiles/launch_learner.md)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
FIELDS = ("auto_verdict auto_cap auto_cap_max_iter auto_growth growth_alt growth_verdict auto_probes auto_since auto_last_cap auto_plain_rate "
          "auto_split_rate auto_gain tile_verdict tile_since tile_rate regroup_verdict regroup_since lockstep_ratio probe_was_tile probe_was_growth hist_copy").split()
# iteration histograms: BASELINE config 3 and the uniform one of tests/test_split_model.py; ONE = a single instance of one iteration,
# so that a probe's rate (ms / sum of i * hist[i]) is its ms exactly -- and no split can beat its plain launch: K = 0, ratio 1, growth 2
H3 = {7: 9000, 8: 61000, 9: 98000, 10: 58000, 11: 14000, 12: 5000, 14: 3000, 18: 3000, 25: 3500, 40: 3500, 70: 3000, 100: 1144}
UNI = {9: 262144}
ONE = {1: 1}
JUST_UNDER_97 = 96.99999237060547            # the float below 97 (a clock reading is a float of milliseconds)


def hist_line(h):
    return "hist " + " ".join("%d:%d" % kv for kv in sorted(h.items()))


def hist_id(h):
    """what the driver prints for hist_copy: its length and the FNV-1a hash of its bytes"""
    a = np.zeros(1024, np.uint32)
    for k, v in h.items():
        a[k] = v
    x = 1469598103934665603
    for byte in a.tobytes():
        x = ((x ^ byte) * 1099511628211) & (2 ** 64 - 1)
    return (1024, x)


@pytest.fixture(scope="module")
def drive(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("launch_learner") / "driver")
    csrc = os.path.join(ROOT, "tinympc_amd", "csrc")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O1", "-I", csrc, os.path.join(ROOT, "tests", "dropin", "launch_learner_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)

    def run(*script):
        """the script's events through a fresh learner -> one dict per line: fields, queries, what the event returned"""
        lines = [ln for part in script for ln in ([part] if isinstance(part, str) else part)]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
        assert len(out) == len(lines)
        rows = []
        for ln in out:
            r = dict(w.split("=", 1) for w in ln.split())
            for k, v in r.items():
                if k == "hist_copy":
                    r[k] = tuple(int(x) for x in v.split(":"))
                elif k != "event":
                    r[k] = float(v) if ("." in v or "e" in v or "n" in v) else int(v)
            rows.append(r)
        return rows
    return run


def state(r):
    return {k: r[k] for k in FIELDS}


def changed(before, after):
    """the fields an event changed, with their new values"""
    return {k: after[k] for k in FIELDS if after[k] != before[k]}


# a kept split of K = 10 with both clock readings behind it, the growth question open (auto_probes comes in as max(2, 0): readings count)
KEPT = "plan_import 1 0 auto_verdict=1 auto_cap=10 auto_cap_max_iter=100 auto_plain_rate=100 auto_split_rate=90"
# every field away from its default: what a reset leaves alone must show
FULL = [hist_line(H3),
        "plan_import 1 0 auto_verdict=1 auto_cap=10 auto_cap_max_iter=100 auto_growth=2 growth_verdict=1 auto_probes=5 auto_plain_rate=100 auto_split_rate=90 "
        "auto_gain=0.8 tile_verdict=1 tile_rate=80 regroup_verdict=1 lockstep_ratio=1.2 hist_valid=1 hist=1",
        "one_row_solve_counted 1", "one_row_solve_counted 1", "tile_solve_counted", "tile_solve_counted", "tile_solve_counted",
        "fused_solve_counted 1", "fused_solve_counted 1", "fused_solve_counted 1", "fused_solve_counted 1",
        "timed_launch_recorded 10", "growth_probe_on_trial", "tile_probe_enqueued"]
FULL_STATE = dict(auto_verdict=1, auto_cap=10, auto_cap_max_iter=100, auto_growth=2, growth_alt=4, growth_verdict=1, auto_probes=5, auto_since=2, auto_last_cap=10,
                  auto_plain_rate=100.0, auto_split_rate=90.0, auto_gain=0.8, tile_verdict=1, tile_since=3, tile_rate=80.0, regroup_verdict=1, regroup_since=4,
                  lockstep_ratio=1.2, probe_was_tile=1, probe_was_growth=1, hist_copy=hist_id(H3))


def test_the_first_reading_of_a_handle_is_discarded(drive):
    """Rule: the first timed solve carries one-time costs (code object load): it is counted and not used.  Its histogram still gives the
    open question its K."""
    r = drive(hist_line(ONE), "timed_launch_recorded 0", "probe_arrived 1 100 100")
    assert changed(state(r[1]), state(r[2])) == dict(auto_probes=1, auto_cap_max_iter=100, auto_gain=1.0, hist_copy=hist_id(ONE))
    assert r[2]["auto_plain_rate"] == 0.0 and r[2]["auto_split_rate"] == 0.0 and r[2]["fresh"] == 0 and r[0]["fresh"] == 1


@pytest.mark.parametrize("split_ms,verdict", [(JUST_UNDER_97, 1), (97.0, -1), (98.0, -1)])
def test_plain_then_split_reading_the_split_is_kept_when_3_percent_faster(drive, split_ms, verdict):
    """Rule: a split reading with a plain reading behind it closes the question: 1 when split < 0.97 x plain (0.97 * 100.0 is 97.0 exactly),
    -1 at or above it."""
    assert 0.97 * 100.0 == 97.0
    r = drive(hist_line(ONE), "probe_arrived 1 50 100", "timed_launch_recorded 0", "probe_arrived 1 100 100", "timed_launch_recorded 5",
              "probe_arrived 1 %r 100" % split_ms)
    assert changed(state(r[2]), state(r[3])) == dict(auto_probes=2, auto_plain_rate=100.0)              # the plain reading alone decides nothing
    assert changed(state(r[4]), state(r[5])) == dict(auto_probes=3, auto_split_rate=split_ms, auto_verdict=verdict)


def test_readings_that_decide_nothing(drive):
    """Rules: a split reading without a plain rate leaves the verdict open; a probe whose clock could not be read, or read 0, stores no
    rate but counts."""
    r = drive(hist_line(ONE), "probe_arrived 1 50 100", "timed_launch_recorded 5", "probe_arrived 1 97 100", "probe_arrived 0 80 100", "probe_arrived 1 0 100")
    assert changed(state(r[2]), state(r[3])) == dict(auto_probes=2, auto_split_rate=97.0)
    assert changed(state(r[3]), state(r[4])) == dict(auto_probes=3) and changed(state(r[4]), state(r[5])) == dict(auto_probes=4)
    # an empty histogram (no iteration was run): no rate either
    r = drive("probe_arrived 1 50 100", "probe_arrived 1 60 100")
    assert r[1]["auto_probes"] == 2 and r[1]["auto_plain_rate"] == 0.0


@pytest.mark.parametrize("ctx,imported,wanted", [
    ("", "", 1),
    ("repack_growth=2", "", 0),                     # the caller fixed the schedule
    ("", "auto_cap=0", 0),                          # nothing to schedule
    ("max_iter=50", "", 0),                         # the cap was made for another max_iter
    ("hist_pending=1", "", 0),                      # a probe is in flight
    ("auto_split=0", "", 0),
    ("", "growth_verdict=1", 0),                    # asked already
])
def test_a_kept_split_wants_exactly_one_growth_probe(drive, ctx, imported, wanted):
    """Rule: growth_probe = auto_split && !hist_pending && verdict 1 && growth_verdict 0 && repack_growth < 2 && cap > 0 && the cap's max_iter
    is this solve's && a split rate exists; a growth probe is an auto probe."""
    r = drive("ctx " + ctx, KEPT + " " + imported)
    assert (r[1]["growth_probe_wanted"], r[1]["auto_probe_wanted"]) == (wanted, wanted)


@pytest.mark.parametrize("reading,after", [
    ("1 87 100", dict(auto_growth=4, auto_split_rate=87.0)),       # 87 < 0.97 x 90 = 87.3: the other schedule and its rate are taken
    ("1 88 100", dict()),                                          # not 3 % faster: the schedule in use stays
    ("0 0 100", dict()),                                           # the clock could not be read: asked once all the same
])
def test_the_growth_probes_reading(drive, reading, after):
    """Rule: the trial takes the other schedule of 2 | 4; its reading replaces auto_growth and auto_split_rate only under 0.97 x the split's
    rate; growth_verdict is 1 afterwards whatever became of the reading; a kept split keeps its K and histogram."""
    r = drive(hist_line(ONE), KEPT, "growth_probe_on_trial", "probe_arrived " + reading)
    assert changed(state(r[1]), state(r[2])) == dict(growth_alt=4, probe_was_growth=1) and r[2]["returned"] == 4
    assert changed(state(r[2]), state(r[3])) == dict(auto_probes=3, growth_verdict=1, probe_was_growth=0, **after)
    assert r[3]["growth_probe_wanted"] == 0 and r[3]["auto_probe_wanted"] == 0
    assert drive(KEPT + " auto_growth=4", "growth_probe_on_trial")[1]["returned"] == 2


SETTLED = {"rejected": ("plan_import 1 0 auto_verdict=-1 auto_cap=10 auto_plain_rate=100 auto_split_rate=90", ""),
           "plain predicted as fast": ("plan_import 1 0 auto_cap=0 auto_plain_rate=100", ""),
           "kept, schedule compared": (KEPT + " growth_verdict=1", ""),
           "kept, schedule fixed by the caller": (KEPT, "repack_growth=2")}


@pytest.mark.parametrize("way", list(SETTLED))
def test_a_tile_probe_is_wanted_once_the_one_row_question_is_settled(drive, way):
    """Rule: one_row_settled = a plain rate && (verdict -1 || cap 0 || (verdict 1 && (growth_verdict != 0 || repack_growth >= 2)));
    tile probe = tile_verdict 0 && settled && no histogram pending."""
    imported, ctx = SETTLED[way]
    r = drive("ctx " + ctx, imported, "ctx hist_pending=1", "ctx hist_pending=0", "plan_import 1 0 tile_verdict=-1")
    assert [(x["one_row_settled"], x["tile_probe_wanted"]) for x in r[1:]] == [(1, 1), (1, 0), (1, 1), (1, 0)]


def test_no_tile_probe_while_the_one_row_question_is_open(drive):
    r = drive(KEPT,                                                           # kept, the other schedule untried
              "plan_import 1 0 auto_verdict=0 auto_cap=10",                   # plain or split undecided
              "plan_import 1 0 auto_verdict=-1 auto_cap=0 auto_plain_rate=0")  # no plain rate (the import opens such a verdict)
    assert [(x["one_row_settled"], x["tile_probe_wanted"]) for x in r] == [(0, 0)] * 3


@pytest.mark.parametrize("imported,ms,verdict", [
    (KEPT + " growth_verdict=1", 87, 1), (KEPT + " growth_verdict=1", 88, -1),      # kept split: against its rate, 0.97 x 90 = 87.3
    (SETTLED["rejected"][0], 96, 1), (SETTLED["rejected"][0], 97, -1),             # otherwise against the plain rate, 0.97 x 100 = 97
])
def test_the_tile_verdict_is_judged_against_the_best_one_row_rate(drive, imported, ms, verdict):
    r = drive(hist_line(ONE), imported, "tile_probe_enqueued", "probe_arrived 1 %d 100" % ms)
    assert changed(state(r[1]), state(r[2])) == dict(probe_was_tile=1)
    assert changed(state(r[2]), state(r[3])) == dict(auto_probes=3, probe_was_tile=0, tile_rate=float(ms), tile_verdict=verdict)


def test_full_state_is_what_its_script_says(drive):
    assert state(drive(FULL)[-1]) == FULL_STATE


def test_the_one_row_drift_reset_fires_on_the_32nd_eligible_solve_with_its_own_field_list(drive):
    """Rule (launch_solve): auto_split && verdict != 0 && ++auto_since >= 32 -> auto_since, auto_verdict, growth_verdict, auto_plain_rate,
    tile_verdict.  tile_since, auto_split_rate and the rest stay (inherited)."""
    r = drive(FULL, ["one_row_solve_counted 0"] * 3, ["one_row_solve_counted 1"] * 30)
    assert all(changed(FULL_STATE, state(x)) == {} for x in r[len(FULL):len(FULL) + 3])                 # not eligible: not counted
    assert changed(FULL_STATE, state(r[-2])) == dict(auto_since=31)
    assert changed(FULL_STATE, state(r[-1])) == dict(auto_since=0, auto_verdict=0, growth_verdict=0, auto_plain_rate=0.0, tile_verdict=0)
    assert r[-1]["tile_since"] == 3 and r[-1]["auto_split_rate"] == 90.0
    assert drive("one_row_solve_counted 1")[0]["auto_since"] == 0                                        # an open verdict counts nothing


def test_the_tile_drift_reset_fires_on_the_32nd_solve_with_its_own_field_list(drive):
    """Rule (try_tile_alternative): tile_verdict 1 && ++tile_since >= 32 -> tile_since, tile_verdict, auto_verdict, growth_verdict,
    auto_plain_rate, auto_since; the solve then goes back to the one-row kernel.  auto_split_rate and tile_rate stay (inherited)."""
    r = drive(FULL, ["tile_solve_counted"] * 29)
    assert changed(FULL_STATE, state(r[-2])) == dict(tile_since=31) and r[-2]["returned"] == 0
    assert changed(FULL_STATE, state(r[-1])) == dict(tile_since=0, tile_verdict=0, auto_verdict=0, growth_verdict=0, auto_plain_rate=0.0, auto_since=0)
    assert r[-1]["returned"] == 1 and r[-1]["auto_split_rate"] == 90.0 and r[-1]["tile_rate"] == 80.0
    assert drive("tile_solve_counted")[0]["tile_since"] == 0                                             # (a probe, verdict 0: not counted)


def test_the_regroup_drift_reset_fires_on_the_64th_fused_solve(drive):
    """Rule: regroup_auto && verdict != 0 && ++regroup_since >= 64 -> regroup_since, regroup_verdict."""
    r = drive(FULL, "fused_solve_counted 0", ["fused_solve_counted 1"] * 60)
    assert changed(FULL_STATE, state(r[len(FULL)])) == {}
    assert changed(FULL_STATE, state(r[-2])) == dict(regroup_since=63)
    assert changed(FULL_STATE, state(r[-1])) == dict(regroup_since=0, regroup_verdict=0)


@pytest.mark.parametrize("option,cleared", [
    ("repack_after_set", dict(auto_cap=0, hist_copy=(0, 0), auto_verdict=0, growth_verdict=0, auto_plain_rate=0.0, auto_split_rate=0.0, auto_probes=0)),
    ("repack_growth_set", dict(growth_verdict=0)),
    ("step_regroup_set", dict(regroup_verdict=0, regroup_since=0)),
])
def test_each_option_reset_clears_its_field_list_and_nothing_else(drive, option, cleared):
    r = drive(FULL, option)
    assert changed(FULL_STATE, state(r[-1])) == cleared


def test_the_lock_step_estimate(drive):
    """Rule: ratio = rows x largest total / totals, 1.0 when nothing was counted; an open verdict becomes 1 at >= 1.05, else -1; a decided
    one only takes the ratio."""
    r = drive("lockstep_estimate_arrived 105 100", "lockstep_estimate_arrived 104 100", "step_regroup_set", "lockstep_estimate_arrived 104 100",
              "step_regroup_set", "lockstep_estimate_arrived 0 0")
    assert [(x["lockstep_ratio"], x["regroup_verdict"]) for x in r] == [(1.05, 1), (1.04, 1), (1.04, 0), (1.04, -1), (1.04, 0), (1.0, -1)]
    assert changed(state(r[2]), state(r[3])) == dict(regroup_verdict=-1)


def model_answer(h, ct=1):
    """tiny_predict_split for the quadrotor shape (two waves per SIMD, 256 CUs) -- or, without the library, None"""
    try:
        import tinympc_amd as tm
        a = np.zeros(1024, np.int64)
        for k, v in h.items():
            a[k] = v
        return tm.predict_split(a, 12, 4, 10, max_iter=100, check_termination=ct)
    except (OSError, ImportError):
        return None


def test_k_ratio_and_growth_are_the_cost_models(drive):
    """Rule: while the verdict is open a fresh histogram re-chooses K, the predicted ratio and the stage growth together -- what
    tiny_predict_split answers for the same inputs (tests/test_split_model.py pins those)."""
    r = drive(hist_line(H3), "choose_split", "probe_arrived 1 100 100", hist_line(UNI), "choose_split", "probe_arrived 1 100 100",
              "model 12 4 10 2 100 5 0 256", hist_line(H3), "choose_split")
    for row, learnt, h, ct in ((r[1], r[2], H3, 1), (r[4], r[5], UNI, 1), (r[8], None, H3, 5)):
        want = model_answer(h, ct)
        if want is not None:
            assert (row["k"], row["ratio"]) == (want[0], want[1])
        assert row["growth"] in (2, 4) and row["k"] % ct == 0
        if learnt:
            assert (learnt["auto_cap"], learnt["auto_gain"], learnt["auto_growth"], learnt["auto_cap_max_iter"]) == (row["k"], row["ratio"], row["growth"], 100)
            assert learnt["hist_copy"] == hist_id(h)
    assert 6 <= r[1]["k"] <= 24 and 0.75 < r[1]["ratio"] < 0.95                     # what tests/test_split_model.py pins for these histograms
    assert r[4]["k"] == 0 and r[5]["solve_cap"] == 0


def test_the_diagnostic_histogram_path(drive):
    """Rule (get_option "auto_split_k"): the probe's flags are cleared and its reading dropped, auto_probes and the rates stay; K, ratio,
    growth and the histogram are re-chosen only while the verdict is open."""
    r = drive(hist_line(H3), "probe_arrived 1 50 100", "probe_arrived 1 100 100", "tile_probe_enqueued", "growth_probe_on_trial", hist_line(UNI), "choose_split",
              "histogram_read_back 77")
    assert r[4]["auto_cap"] > 0 and r[4]["solve_cap"] == r[4]["auto_cap"]           # (a plain rate and an open verdict: the model's K is tried)
    # the uniform histogram: no split beats the plain launch -- K = 0, ratio 1, the default schedule 2
    want = dict(probe_was_tile=0, probe_was_growth=0, auto_cap=0, auto_cap_max_iter=77, auto_gain=1.0, hist_copy=hist_id(UNI))
    assert changed(state(r[4]), state(r[7])) == dict(want, **(dict(auto_growth=2) if r[4]["auto_growth"] != 2 else {}))
    assert (r[6]["k"], r[6]["ratio"], r[6]["growth"]) == (0, 1.0, 2)
    assert (r[7]["auto_probes"], r[7]["auto_plain_rate"], r[7]["auto_split_rate"]) == (2, 100.0 / sum(i * c for i, c in H3.items()), 0.0)
    r = drive(FULL, hist_line(UNI), "histogram_read_back 77")                       # a decided batch keeps its K and its schedule
    assert changed(FULL_STATE, state(r[-1])) == dict(probe_was_tile=0, probe_was_growth=0)


EXPORTED = [f for f in FIELDS if f not in ("growth_alt", "auto_since", "auto_last_cap", "tile_since", "regroup_since", "probe_was_tile", "probe_was_growth")]


def test_a_plan_round_trip_gives_back_every_exported_field(drive):
    """Rule: from_plan(to_plan(state)) under the same settings -- verdicts with their readings behind them stand; the counters, the flags
    and auto_last_cap start afresh."""
    r = drive(FULL, "plan_import 1 0")                                               # settled
    assert r[-1]["in_range"] == 1
    assert changed(FULL_STATE, state(r[-1])) == dict(auto_since=0, tile_since=0, regroup_since=0, probe_was_tile=0, probe_was_growth=0, auto_last_cap=0)
    r = drive(hist_line(H3), "probe_arrived 1 50 100", "probe_arrived 1 100 100", "plan_import 1 0")   # unsettled: a plain rate, the split untried
    assert {k: r[3][k] for k in EXPORTED} == {k: r[2][k] for k in EXPORTED} and r[2]["auto_verdict"] == 0 and r[2]["auto_cap"] > 0
    assert r[2]["open_questions"] == 1 and r[3]["plan_open_questions"] == 1


@pytest.mark.parametrize("imported,ctx,want", [
    (SETTLED["rejected"][0], "", 0),                              # nothing open
    (KEPT + " growth_verdict=1", "", 0),
    ("plan_import 1 0 auto_cap=0 auto_plain_rate=100", "", 0),    # undecided, but no split is on the table
    ("plan_import 1 0 auto_cap=10 auto_plain_rate=100", "", 1),   # plain or split undecided
    ("plan_import 1 0", "", 1),                                   # a fresh handle
    (KEPT, "", 1),                                                # the other stage schedule of a kept split untried
    (KEPT, "repack_growth=2", 0),                                 # ... unless the caller fixed it
])
def test_open_questions_as_get_plan_counts_them(drive, imported, ctx, want):
    """Rule: (verdict 0 && !(plain rate && cap 0)) + (verdict 1 && growth_verdict 0 && repack_growth < 2)."""
    assert drive("ctx " + ctx, imported)[1]["open_questions"] == want


@pytest.mark.parametrize("name,value", [
    ("auto_verdict", 2), ("tile_verdict", -2), ("regroup_verdict", 3), ("growth_verdict", 7), ("auto_cap", -1), ("auto_cap", 4000), ("auto_growth", 3),
    ("auto_probes", -5), ("auto_cap_max_iter", -1), ("batch", 0), ("hist_valid", 2), ("auto_plain_rate", "nan"), ("auto_split_rate", -1.0), ("auto_gain", "inf"),
    ("tile_rate", "nan"), ("lockstep_ratio", -0.5)])
def test_a_plan_field_out_of_range_is_refused(drive, name, value):
    """The fields tests/test_gpu_repack.py sends through tiny_batch_set_plan: verdicts in {-1, 0, 1}, counts non-negative, K below the
    histogram's length, growth 2 | 4, readings finite and non-negative."""
    r = drive(FULL, "plan_import 1 0 %s=%s" % (name, value), "plan_import 1 0 auto_cap=1023 auto_growth=4 auto_probes=0 auto_cap_max_iter=0 tile_rate=1e299")
    assert r[-2]["in_range"] == 0 and state(r[-2]) == FULL_STATE
    assert r[-1]["in_range"] == 1


@pytest.mark.parametrize("how,opened", [
    ("0 0", dict(auto_verdict=0, growth_verdict=0, tile_verdict=0)),                                    # other max_iter / check_termination: the regroup verdict stands
    ("1 1", dict(auto_verdict=0, growth_verdict=0, tile_verdict=0, regroup_verdict=0)),                 # a batch of another order of magnitude
    ("1 0 auto_split_rate=0", dict(auto_verdict=0, growth_verdict=0, auto_split_rate=0.0)),             # a kept split without its reading
    ("1 0 auto_plain_rate=0", dict(auto_verdict=0, growth_verdict=0, auto_plain_rate=0.0)),
    ("1 0 tile_rate=0", dict(tile_verdict=0, tile_rate=0.0)),                                           # a kept tile form without its reading
    ("1 0 tile_rate=0 tile_verdict=-1", dict(tile_verdict=-1, tile_rate=0.0)),                          # (a rejection needs none)
    ("1 0 auto_probes=0", dict(auto_probes=2)),                                                         # auto_probes = max(2, imported): its readings count
    ("1 0 auto_probes=7", dict(auto_probes=7)),
    ("1 0 hist_valid=0", dict(hist_copy=(0, 0))),
])
def test_an_import_opens_the_verdicts_it_cannot_trust(drive, how, opened):
    """Rule (set_plan): the split and tile verdicts need same_settings, !far_batch and their supporting reading; the regroup verdict only
    !far_batch; growth_verdict goes with a kept split."""
    r = drive(FULL, "plan_import " + how)
    afresh = dict(auto_since=0, tile_since=0, regroup_since=0, probe_was_tile=0, probe_was_growth=0, auto_last_cap=0)
    assert r[-1]["in_range"] == 1 and changed(FULL_STATE, state(r[-1])) == dict(afresh, **opened)
