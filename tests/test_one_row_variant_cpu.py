"""CPU: which instantiation of admm_solve_kernel a launch on the one-row kernel runs (csrc/one_row_variant.hpp), checked on the function
itself.  It is plain C++ without a HIP call, so tests/dropin/one_row_variant_driver.cpp answers for any set of facts and any of the slot
patterns a compiled-in entry can have, and counts the answers over every consistent combination.  The expected answers below are restated
from the rungs (profiles/one_row_variant.md lists them in order), not read off the driver: the GPU suite pins the choice only at the
shapes and options its tests happen to use."""
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("one_row_variant") / "driver")
    csrc = os.path.join(ROOT, "tinympc_amd", "csrc")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", csrc, os.path.join(ROOT, "tests", "dropin", "one_row_variant_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


TEXT = ("slot", "prefetch", "fallback")


def words(line):
    r = dict(w.split("=", 1) for w in line.split())
    return {k: (v if k in TEXT else int(v)) for k, v in r.items()}


@pytest.fixture(scope="module")
def ask(driver):
    def run(*queries):
        """each query: a dict of facts and entry words (unnamed ones are 0) -> the driver's answer as a dict; every query must be consistent"""
        lines = [" ".join("%s=%d" % kv for kv in q.items()) for q in queries]
        out = subprocess.run([driver], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
        assert len(out) == len(lines)
        rows = [words(ln) for ln in out]
        assert all(r.pop("consistent") == 1 for r in rows), [q for q, ln in zip(queries, out) if "consistent=0" in ln]
        return rows
    return run


def choice(slot="NONE", **over):
    """the answer for the plain box launch at the default settings (mode 2, stride 4), with what differs"""
    return dict(dict(soc=0, dbg=0, mode=2, lin=0, het=0, kmax=4, adapt=0, ub=0, pb=0, pl=0, slot=slot, ipw=4, prefetch="NONE", ub_form=0, fallback="NONE"), **over)


def check(ask, cases):
    got = ask(*[c[0] for c in cases])
    for (facts, want), have in zip(cases, got):
        assert have == want, (facts, have, want)


# the slot patterns (kernel_entry.hpp): KERNELS_FOR fills every slot, KERNELS_LEAN k[0][0][2] and kub; none: a shape outside kernel_dims.txt.
# OPT: the shape-dependent HALF / PREFETCH slots.  dpp_mode 2 is the handle's default; the driver's default for a fact not named is 0.
FULL, LEAN, NO_ENTRY = dict(entry=2, dpp_mode=2), dict(entry=1, dpp_mode=2), dict(entry=0, dpp_mode=2)
OPT = dict(half=1, pf=1, halfpf=1)
PF_LAUNCH = dict(prefetch_on=1, single_step=1, no_ref_window=1, default_grid=1)
LIN4 = dict(lin=1, lin_kmax=4)


def test_rung_1_adaptive_rho_asks_kadapt_by_debug_only(ask):
    """In front of every other rung; with a cone or per-instance data the variant is instantiated; mode is forced to 2."""
    base = dict(FULL, adaptive=1, uniform_ub=1)
    check(ask, [(base, choice("KADAPT[0]", adapt=1)), (dict(base, debug=1), choice("KADAPT[1]", adapt=1, dbg=1)),
                (dict(base, dpp_mode=0), choice("KADAPT[0]", adapt=1)), (dict(base, dpp_mode=1, debug=1), choice("KADAPT[1]", adapt=1, dbg=1)),
                (dict(base, soc=1), choice(adapt=1, soc=1)), (dict(base, hetero=1), choice(adapt=1, het=1)),
                (dict(base, hetero=1, het_ub=1), choice(adapt=1, het=1)),                     # (not the HET-UB form either: ub stays 0)
                (dict(base, entry=1), choice(adapt=1)), (dict(base, entry=0), choice(adapt=1)),
                (dict(base, adaptive=0), choice("KUB", ub_form=1))])


def test_rung_2_knot_invariant_box_takes_the_ub_slot_and_does_not_fall_through(ask):
    """kub / kubsoc without debug, at mode 2, with bounds_uniform && use_ub: each term alone moves the launch to k[soc][dbg][mode].  A LEAN
    shape has no kubsoc: the cone goes to run-time instantiation, from a key WITHOUT ub -- not to k[1][0][2] (which it has not either)."""
    base = dict(FULL, uniform_ub=1)
    check(ask, [(base, choice("KUB", ub_form=1)), (dict(base, soc=1), choice("KUBSOC", soc=1, ub_form=1)),
                (dict(base, uniform_ub=0), choice("K[0][0][2]")), (dict(base, debug=1), choice("K[0][1][2]", dbg=1)),
                (dict(base, dpp_mode=1), choice("K[0][0][1]", mode=1)), (dict(base, dpp_mode=0), choice("K[0][0][0]", mode=0)),
                (dict(base, hetero=1), choice("KHET[0]", het=1)), (dict(base, **LIN4), choice("KLIN[0][1]", lin=1)),
                (dict(LEAN, uniform_ub=1), choice("KUB", ub_form=1)), (dict(LEAN, uniform_ub=1, soc=1), choice(soc=1)),
                (dict(LEAN, uniform_ub=0, soc=1), choice(soc=1)), (dict(NO_ENTRY, uniform_ub=1), choice())])


def test_rung_3_k_soc_dbg_mode_with_the_mode_clamped(ask):
    """Every one of the twelve on a FULL shape, only k[0][0][2] on a LEAN one; dpp_mode outside 0..2 counts as 0."""
    cases = []
    for soc, dbg, mode in itertools.product((0, 1), (0, 1), (0, 1, 2)):
        q = dict(soc=soc, debug=dbg, dpp_mode=mode)
        cases.append((dict(FULL, **q), choice("K[%d][%d][%d]" % (soc, dbg, mode), soc=soc, dbg=dbg, mode=mode)))
        cases.append((dict(LEAN, **q), choice("K[0][0][2]" if (soc, dbg, mode) == (0, 0, 2) else "NONE", soc=soc, dbg=dbg, mode=mode)))
    cases += [(dict(FULL, dpp_mode=m), choice("K[0][0][0]", mode=0)) for m in (-1, 3)]
    cases += [(dict(FULL, dpp_mode=3, uniform_ub=1), choice("K[0][0][0]", mode=0))]           # (clamped BEFORE the UB rung asks for mode 2)
    check(ask, cases)


def test_rung_4_shared_halfspaces_klin_only_at_the_compiled_in_stride_without_debug(ask):
    """klin[soc][lin] at kmax == 4, no debug, no per-instance data; mode forced to 2; HET together with lin is always instantiated."""
    cases = [(dict(FULL, lin=lin, lin_kmax=4, soc=soc, dpp_mode=mode, uniform_ub=1), choice("KLIN[%d][%d]" % (soc, lin), lin=lin, soc=soc))
             for lin in (1, 2, 3) for soc in (0, 1) for mode in (0, 2)]
    base = dict(FULL, **LIN4)
    cases += [(dict(base, lin_kmax=km), choice(lin=1, kmax=km)) for km in (8, 16, 32)]
    cases += [(dict(base, debug=1), choice(lin=1, dbg=1)), (dict(base, hetero=1), choice(lin=1, het=1)),
              (dict(base, hetero=1, het_ub=1, uniform_ub=1), choice(lin=1, het=1)),
              (dict(base, entry=1), choice(lin=1)), (dict(base, entry=0), choice(lin=1))]
    check(ask, cases)


def test_rung_5_per_instance_data_khetub_run_time_ub_form_or_khet(ask):
    """khetub[soc] with het_ub on a knot-invariant box where the slot exists; where it does not (LEAN), the UB form is instantiated
    (key.ub = 1) -- only with !no_jit && !variant_jit_failed, else khet[soc] is asked (which a LEAN shape has not: instantiated with
    ub = 0).  Without debug only."""
    base = dict(FULL, hetero=1, het_ub=1, uniform_ub=1)
    lean = dict(base, entry=1)
    check(ask, [(base, choice("KHETUB[0]", het=1, ub_form=1)), (dict(base, soc=1), choice("KHETUB[1]", het=1, soc=1, ub_form=1)),
                (dict(base, het_ub=0), choice("KHET[0]", het=1)), (dict(base, uniform_ub=0), choice("KHET[0]", het=1)),
                (dict(base, soc=1, het_ub=0), choice("KHET[1]", het=1, soc=1)), (dict(base, dpp_mode=0), choice("KHETUB[0]", het=1, ub_form=1)),
                (dict(base, no_jit=1), choice("KHETUB[0]", het=1, ub_form=1)),                # (the compiled-in slot needs no instantiation)
                (dict(base, debug=1), choice(het=1, dbg=1)),
                (lean, choice(het=1, ub=1, ub_form=1)), (dict(lean, no_jit=1), choice(het=1)), (dict(lean, variant_jit_failed=1), choice(het=1)),
                (dict(lean, het_ub=0), choice(het=1)), (dict(lean, uniform_ub=0), choice(het=1)), (dict(lean, debug=1), choice(het=1, dbg=1)),
                (dict(base, entry=0), choice(het=1))])


def test_rung_0_per_instance_box_and_halfspaces_never_ask_the_entry(ask):
    """PB: ub = bounds_uniform && use_ub && (!hetero || het_ub), no HALF, no PREFETCH; PL: the blocks' own stride."""
    everything = dict(FULL, **OPT, **PF_LAUNCH, half_rows=1)
    pb = dict(everything, pb=1)
    pl = dict(everything, lin=1, pl=1, lin_kmax=4, il_km=2)
    check(ask, [(dict(pb, uniform_ub=1), choice(pb=1, ub=1, ub_form=1)), (pb, choice(pb=1)),
                (dict(pb, uniform_ub=1, hetero=1), choice(pb=1, het=1)), (dict(pb, uniform_ub=1, hetero=1, het_ub=1), choice(pb=1, het=1, ub=1, ub_form=1)),
                (dict(pb, dpp_mode=1), choice(pb=1, mode=1)), (dict(pb, entry=0, half=0, pf=0, halfpf=0, uniform_ub=1), choice(pb=1, ub=1, ub_form=1)),
                (pl, choice(lin=1, pl=1, kmax=2)), (dict(pl, il_km=32, lin_kmax=0, lin=3), choice(lin=3, pl=1, kmax=32)),
                (dict(pl, soc=1, hetero=1, uniform_ub=1, het_ub=1, dpp_mode=0), choice(lin=1, pl=1, kmax=2, soc=1, het=1)),
                (dict(pl, pl=0, il_km=0), choice("KLIN[0][1]", lin=1))])


def test_half_upgrade_only_from_kub_or_k002_with_the_option_and_the_slot(ask):
    base = dict(FULL, **OPT, half_rows=1)
    ub = dict(base, uniform_ub=1)
    check(ask, [(ub, choice("KHALF[1]", ipw=8, ub_form=1)), (base, choice("KHALF[0]", ipw=8)),
                (dict(ub, entry=1), choice("KHALF[1]", ipw=8, ub_form=1)), (dict(base, entry=1), choice("KHALF[0]", ipw=8)),
                (dict(ub, half_rows=0), choice("KUB", ub_form=1)), (dict(base, half_rows=0), choice("K[0][0][2]")),
                (dict(ub, half=0, halfpf=0), choice("KUB", ub_form=1)), (dict(base, half=0, halfpf=0), choice("K[0][0][2]")),
                (dict(ub, soc=1), choice("KUBSOC", soc=1, ub_form=1)), (dict(base, soc=1), choice("K[1][0][2]", soc=1)),
                (dict(base, debug=1), choice("K[0][1][2]", dbg=1)), (dict(base, dpp_mode=1), choice("K[0][0][1]", mode=1)),
                (dict(ub, adaptive=1), choice("KADAPT[0]", adapt=1)), (dict(ub, **LIN4), choice("KLIN[0][1]", lin=1)),
                (dict(ub, hetero=1), choice("KHET[0]", het=1)), (dict(ub, hetero=1, het_ub=1), choice("KHETUB[0]", het=1, ub_form=1)),
                (dict(ub, entry=0, half=0, pf=0, halfpf=0), choice())])


def test_prefetch_slot_the_four_candidates_and_every_launch_term(ask):
    base = dict(FULL, **OPT, **PF_LAUNCH)
    ub = dict(base, uniform_ub=1)
    cases = [(ub, choice("KUB", ub_form=1, prefetch="KPF[1]")), (base, choice("K[0][0][2]", prefetch="KPF[0]")),
             (dict(ub, half_rows=1), choice("KHALF[1]", ipw=8, ub_form=1, prefetch="KHALFPF[1]")), (dict(base, half_rows=1), choice("KHALF[0]", ipw=8, prefetch="KHALFPF[0]")),
             (dict(ub, entry=1), choice("KUB", ub_form=1, prefetch="KPF[1]")),
             (dict(ub, pf=0), choice("KUB", ub_form=1)), (dict(base, pf=0, half_rows=1), choice("KHALF[0]", ipw=8, prefetch="KHALFPF[0]")),
             (dict(ub, halfpf=0, half_rows=1), choice("KHALF[1]", ipw=8, ub_form=1)),          # (the HALF form does not go back to kpf)
             (dict(ub, soc=1), choice("KUBSOC", soc=1, ub_form=1)), (dict(base, debug=1), choice("K[0][1][2]", dbg=1)),
             (dict(base, dpp_mode=1), choice("K[0][0][1]", mode=1)), (dict(ub, adaptive=1), choice("KADAPT[0]", adapt=1)),
             (dict(ub, **LIN4), choice("KLIN[0][1]", lin=1)), (dict(ub, hetero=1, het_ub=1), choice("KHETUB[0]", het=1, ub_form=1)),
             (dict(ub, hetero=1), choice("KHET[0]", het=1))]
    cases += [(dict(ub, **{term: 0}), choice("KUB", ub_form=1)) for term in PF_LAUNCH]
    cases += [(dict(base, half_rows=1, **{term: 0}), choice("KHALF[0]", ipw=8)) for term in PF_LAUNCH]
    check(ask, cases)


def test_inherited_behaviour_is_kept(ask):
    """The list of the issue, one case each (most have their sole-offender cases above)."""
    check(ask, [
        # mode forced to 2 for lin / het / adapt, after the clamp
        (dict(FULL, dpp_mode=1, **LIN4), choice("KLIN[0][1]", lin=1)), (dict(FULL, dpp_mode=7, hetero=1), choice("KHET[0]", het=1)),
        (dict(FULL, dpp_mode=-1, adaptive=1), choice("KADAPT[0]", adapt=1)), (dict(FULL, dpp_mode=7), choice("K[0][0][0]", mode=0)),
        # PB and PL never ask the entry
        (dict(FULL, pb=1), choice(pb=1)), (dict(FULL, lin=1, pl=1, lin_kmax=4, il_km=4), choice(lin=1, pl=1, kmax=4)),
        # jk.ub of PB
        (dict(FULL, pb=1, uniform_ub=1, hetero=1, het_ub=0), choice(pb=1, het=1)), (dict(FULL, pb=1, uniform_ub=1, hetero=1, het_ub=1), choice(pb=1, het=1, ub=1, ub_form=1)),
        # the UB rung does not fall through
        (dict(LEAN, soc=1, uniform_ub=1), choice(soc=1)),
        # kadapt is indexed by debug only
        (dict(FULL, adaptive=1, debug=1), choice("KADAPT[1]", adapt=1, dbg=1)),
        # HET together with lin: always instantiated
        (dict(FULL, hetero=1, **LIN4), choice(lin=1, het=1)),
        # HALF only from kub / k[0][0][2], with half_rows and the slot
        (dict(FULL, **OPT, half_rows=1, soc=1, uniform_ub=1), choice("KUBSOC", soc=1, ub_form=1)), (dict(FULL, half_rows=1), choice("K[0][0][2]")),
        # the HET-UB run-time form only with !no_jit && !variant_jit_failed
        (dict(LEAN, hetero=1, het_ub=1, uniform_ub=1), choice(het=1, ub=1, ub_form=1)), (dict(LEAN, hetero=1, het_ub=1, uniform_ub=1, no_jit=1), choice(het=1)),
        (dict(LEAN, hetero=1, het_ub=1, uniform_ub=1, variant_jit_failed=1), choice(het=1))])


def test_last_ub_ipw_and_prefetch_follow_from_the_slot(ask):
    """Every compiled-in slot a launch can end on, with everything on that could add HALF / PREFETCH: (ub_form, ipw, prefetch) is a
    function of the slot -- UB forms are kub, kubsoc, khetub[], khalf[1]; eight per wave are khalf[]; PREFETCH forms have kub, k[0][0][2],
    khalf[].  A run-time instantiated variant is a UB form where its key says so."""
    on = dict(FULL, **OPT, **PF_LAUNCH)
    of_slot = {"KUB": (1, 4, "KPF[1]"), "K[0][0][2]": (0, 4, "KPF[0]"), "KHALF[1]": (1, 8, "KHALFPF[1]"), "KHALF[0]": (0, 8, "KHALFPF[0]"), "KUBSOC": (1, 4, "NONE"),
               "KHETUB[0]": (1, 4, "NONE"), "KHETUB[1]": (1, 4, "NONE"), "KHET[0]": (0, 4, "NONE"), "KHET[1]": (0, 4, "NONE"), "KADAPT[0]": (0, 4, "NONE"),
               "KADAPT[1]": (0, 4, "NONE")}
    of_slot.update({"KLIN[%d][%d]" % (s, l): (0, 4, "NONE") for s in (0, 1) for l in (1, 2, 3)})
    of_slot.update({"K[%d][%d][%d]" % k: (0, 4, "NONE") for k in itertools.product((0, 1), (0, 1), (0, 1, 2)) if k != (0, 0, 2)})
    queries = [dict(on, soc=s, debug=d, dpp_mode=m, uniform_ub=u, half_rows=h) for s, d, m, u, h in itertools.product((0, 1), (0, 1), (0, 1, 2), (0, 1), (0, 1))]
    queries += [dict(on, soc=s, lin=l, lin_kmax=4, uniform_ub=1, half_rows=1) for s in (0, 1) for l in (1, 2, 3)]
    queries += [dict(on, soc=s, hetero=1, het_ub=h, uniform_ub=1, half_rows=1) for s in (0, 1) for h in (0, 1)]
    queries += [dict(on, adaptive=1, debug=d, uniform_ub=1, half_rows=1) for d in (0, 1)]
    got = ask(*queries)
    assert {g["slot"] for g in got} == set(of_slot)
    for q, g in zip(queries, got):
        assert (g["ub_form"], g["ipw"], g["prefetch"]) == of_slot[g["slot"]], (q, g)
    jit = ask(dict(on, entry=0, half=0, pf=0, halfpf=0, uniform_ub=1, half_rows=1), dict(on, pb=1, uniform_ub=1, half_rows=1), dict(on, entry=1, hetero=1, het_ub=1, uniform_ub=1))
    assert [(g["slot"], g["ub"], g["ub_form"], g["ipw"], g["prefetch"]) for g in jit] == [("NONE", 0, 0, 4, "NONE"), ("NONE", 1, 1, 4, "NONE"), ("NONE", 1, 1, 4, "NONE")]


# ---- the sweep: the whole function restated over arrays, one element per consistent combination of facts
FREE = ("hetero", "uniform_ub", "het_ub", "half_rows", "prefetch_on", "single_step", "no_ref_window", "default_grid")
PATTERNS = [dict(entry=0, half=0, pf=0, halfpf=0)] + [dict(entry=e, half=o, pf=o, halfpf=o) for e in (1, 2) for o in (0, 1)] + \
    [dict(entry=2, half=0, pf=1, halfpf=0), dict(entry=1, half=1, pf=0, halfpf=0)]      # (what (12,4,10) has; HALF without PREFETCH: (4,2,30))


def consistent_space():
    """dict fact -> array, broadcastable to (tied facts, free facts): variant_facts_consistent restated (the driver's value lists)"""
    tied = []
    for lin, pl, pb, soc, dbg, adapt, nojit, vjf in itertools.product(range(4), *[(0, 1)] * 7):
        if (pl and not lin) or (pb and (pl or soc or lin or dbg)) or (pl and dbg) or ((pb or pl) and (nojit or vjf)) or (adapt and (pb or pl or lin)):
            continue
        for km in (0, 4, 8, 16, 32):
            if (not lin and km) or (lin and not pl and not km):
                continue
            for ikm in (0, 1, 4, 32):
                if bool(pl) != bool(ikm):
                    continue
                tied.append((lin, pl, pb, soc, dbg, adapt, nojit, vjf, km, ikm))
    tied = np.array(tied, dtype=np.int64)
    names = "lin pl pb soc debug adaptive no_jit variant_jit_failed lin_kmax il_km".split()
    f = {n: tied[:, i][:, None, None] for i, n in enumerate(names)}
    f["dpp_mode"] = np.array([-1, 0, 1, 2, 3])[None, :, None]
    grid = np.array(list(itertools.product((0, 1), repeat=len(FREE))), dtype=np.int64)
    for i, n in enumerate(FREE):
        f[n] = grid[:, i][None, None, :]
    return f, (len(tied), 5, len(grid))


NONE, K, KUB, KUBSOC, KLIN, KHET, KHETUB, KADAPT, KHALF, KPF, KHALFPF = range(11)
SLOT_NAME = ["NONE", "K", "KUB", "KUBSOC", "KLIN", "KHET", "KHETUB", "KADAPT", "KHALF", "KPF", "KHALFPF"]
SLOT_INDICES = [0, 3, 0, 0, 2, 1, 1, 1, 1, 1, 1]


def slot_text(kind, i, j, l):
    return SLOT_NAME[kind] + "".join("[%d]" % v for v in (i, j, l)[:SLOT_INDICES[kind]])


def restated_choice(f, shape, pattern):
    """-> the answer's fields, one array each, in the order the driver prints them (a slot: kind, i, j, l)"""
    full, entry = pattern["entry"] == 2, pattern["entry"] != 0
    B = {k: np.broadcast_to(np.asarray(v) != 0, shape) for k, v in f.items() if k not in ("lin", "dpp_mode", "lin_kmax", "il_km")}
    I = {k: np.broadcast_to(np.asarray(f[k]), shape) for k in ("lin", "dpp_mode", "lin_kmax", "il_km")}
    lin, soc, dbg, het, adapt = I["lin"], B["soc"], B["debug"], B["hetero"], B["adaptive"]
    zero = np.zeros(shape, dtype=np.int64)
    # the key
    pl = B["pl"] & (lin != 0)
    mode = np.where((I["dpp_mode"] >= 0) & (I["dpp_mode"] <= 2), I["dpp_mode"], 0)
    mode = np.where((lin != 0) | het | adapt, 2, mode)
    kmax = np.where(lin == 0, 4, np.where(pl, I["il_km"], I["lin_kmax"]))
    pb = B["pb"]
    ub = pb & B["uniform_ub"] & (~het | B["het_ub"])
    # the rungs, in order: (condition, slot kind, i, j, l, the slot is in the pattern)
    asks = entry & ~pb & ~pl
    plain = ~(lin != 0) & ~het
    ub_rung = plain & ~dbg & (mode == 2) & B["uniform_ub"]
    het_rung = het & (lin == 0) & ~dbg
    want_ub = B["het_ub"] & B["uniform_ub"]
    het_jit = asks & ~adapt & het_rung & want_ub & (not full) & ~B["no_jit"] & ~B["variant_jit_failed"]
    lean_k = ~soc & ~dbg & (mode == 2)
    rungs = [(~asks, NONE, zero, zero, zero, False),
             (adapt & (soc | het), NONE, zero, zero, zero, False), (adapt, KADAPT, dbg, zero, zero, full),
             (ub_rung & soc, KUBSOC, zero, zero, zero, full), (ub_rung, KUB, zero, zero, zero, True),
             (plain, K, soc, dbg, mode, lean_k | full),
             ((lin != 0) & ~het & ~dbg & (kmax == 4), KLIN, soc, lin, zero, full),
             (het_rung & want_ub & full, KHETUB, soc, zero, zero, full), (het_jit, NONE, zero, zero, zero, False), (het_rung, KHET, soc, zero, zero, full),
             (np.ones(shape, bool), NONE, zero, zero, zero, False)]
    which = np.select([np.broadcast_to(r[0], shape) for r in rungs], range(len(rungs)))
    present = np.select([which == n for n in range(len(rungs))], [np.broadcast_to(r[5], shape) for r in rungs])
    kind = np.where(present, np.array([r[1] for r in rungs])[which], NONE)
    at = [np.where(present, np.select([which == n for n in range(len(rungs))], [np.broadcast_to(r[c], shape) for r in rungs]), 0).astype(np.int64) for c in (2, 3, 4)]
    ub = ub | het_jit
    # HALF, PREFETCH, ub_form, fallback
    k002 = (kind == K) & (at[0] == 0) & (at[1] == 0) & (at[2] == 2)
    half = B["half_rows"] & ((kind == KUB) | k002) & bool(pattern["half"])
    at[0] = np.where(half, kind == KUB, at[0]).astype(np.int64)
    at[1], at[2] = np.where(half, 0, at[1]), np.where(half, 0, at[2])
    kind = np.where(half, KHALF, kind)
    ipw = np.where(half, 8, 4)
    launch = B["prefetch_on"] & B["single_step"] & B["no_ref_window"] & B["default_grid"]
    k002 = (kind == K) & (at[0] == 0) & (at[1] == 0) & (at[2] == 2)
    pf_kind = np.select([launch & ((kind == KUB) | k002) & bool(pattern["pf"]), launch & (kind == KHALF) & bool(pattern["halfpf"])], [KPF, KHALFPF], NONE)
    pf_i = np.where(pf_kind == KPF, kind == KUB, np.where(pf_kind == KHALFPF, at[0], 0)).astype(np.int64)
    ub_form = np.where(kind == NONE, ub, (kind == KUB) | (kind == KUBSOC) | (kind == KHETUB) | ((kind == KHALF) & (at[0] == 1)))
    fallback = het_jit & full                                       # khet[soc] where the entry has it: no pattern that exists has khet without khetub
    cols = [soc, dbg, mode, lin, het, kmax, adapt, ub, pb, pl, kind, at[0], at[1], at[2], ipw, pf_kind, pf_i, ub_form, np.where(fallback, KHET, NONE), np.where(fallback, soc, 0)]
    return np.stack([np.broadcast_to(c, shape).astype(np.int64).ravel() for c in cols], axis=1)


@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: "entry%d_half%d_pf%d_halfpf%d" % (p["entry"], p["half"], p["pf"], p["halfpf"]))
def test_sweep_every_consistent_combination_counts_agree(driver, pattern):
    f, shape = consistent_space()
    assert shape == (315, 5, 256)          # (33 tied combinations without half-spaces, 3 x 64 with shared ones, 3 x 30 with per-instance ones)
    fields = restated_choice(f, shape, pattern)
    radix = fields.max(axis=0) + 1
    keys, counts = np.unique(np.ravel_multi_index(tuple(fields.T), radix), return_counts=True)
    want = {}
    for r, c in zip(np.stack(np.unravel_index(keys, radix), axis=1).tolist(), counts.tolist()):
        line = "soc=%d dbg=%d mode=%d lin=%d het=%d kmax=%d adapt=%d ub=%d pb=%d pl=%d" % tuple(r[:10])
        line += " slot=%s ipw=%d prefetch=%s ub_form=%d fallback=%s" % (slot_text(*r[10:14]), r[14], slot_text(r[15], r[16], 0, 0), r[17], slot_text(r[18], r[19], 0, 0))
        want[line] = c
    out = subprocess.run([driver, "sweep"] + ["%s=%d" % kv for kv in pattern.items()], check=True, capture_output=True, text=True, timeout=120).stdout.splitlines()
    assert out[-1] == "total=%d" % (shape[0] * shape[1] * shape[2])
    have = {ln.rsplit(" count=", 1)[0]: int(ln.rsplit(" count=", 1)[1]) for ln in out[:-1]}
    assert have == want
