"""CPU: per-instance cone coefficients (tiny_batch_set_instance_cone_coefficients) as far as they can be checked without a GPU -- the
exported entry points and their NULL returns; the fill rule of the block the one-row kernel reads (csrc/lane_tables.hpp cone_entry,
dumped by tests/dropin/instance_cones_dump.cpp) against the layout restated here in numpy and against VEC_CONE_MU of the shared lane
table; the path and variant rules (tests/dropin/instance_cones_path_driver.cpp), and that with the feature off both choices are the
ones of the headers before it; that the PC forms of the one-row kernel (run-time instantiated only) compile for gfx950, that the flag
without a cone is refused by name, and what the forms cost in registers, scratch and occupancy; the oracle-side conditions of every case
the GPU tests use."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import instance_cone_cases as icc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("tiny_batch_set_instance_cone_coefficients", "tiny_batch_get_instance_cone_coefficients", "tiny_group_set_instance_cone_coefficients")


def pc_name(nx, nu, N, het=False, soc=True, pc=True, ub=False):
    """the instantiation name csrc/jit.hip builds for a cone variant at MODE 2: PC is bit 4 of the MODE argument, UB the last one"""
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, 0, %s, 4, false%s>" % (nx, nu, N, "true" if soc else "false", 18 if pc else 2,
                                                                                              "true" if het else "false", ", true" if ub else "")


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_set_instance_cone_coefficients(None, None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_instance_cone_coefficients(None, 0, None, None) == tm.ERR_NULL
    assert L.tiny_group_set_instance_cone_coefficients(None, None, None, tm.HOST) == tm.ERR_NULL
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        assert callable(cls.set_instance_cone_coefficients) and callable(cls.get_instance_cone_coefficients)
    assert callable(tm.TinyBatchSolver.set_instance_cone_coefficients_device)


@pytest.mark.parametrize("name", list(icc.CASES))
def test_the_cases_of_the_gpu_tests_meet_their_conditions(name):
    icc.check_case(name)
    c = icc.case(name)
    if c["coef"] == "random":
        drawn = np.concatenate([c["cx"].ravel(), c["cu"].ravel()])
        assert np.unique(drawn).size == drawn.size and drawn.min() >= 0.2 and drawn.max() <= 1.5


# ---- the fill rule ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("instance_cones") / "dump")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, "-x", "hip", os.path.join(ROOT, "tests", "dropin", "instance_cones_dump.cpp"),
                    os.path.join(CSRC, "batch_tables.hip"), "-o", exe], check=True, capture_output=True, timeout=600)

    def run(shape, en, Acx, Acu):
        words = [str(v) for v in shape] + [str(int(v)) for v in en] + [",".join(map(str, a)) or "-" for a in (Acx, Acu)]
        out = subprocess.run([exe] + words, check=True, capture_output=True, text=True, timeout=60).stdout
        rule, table = {}, {}
        for ln in out.splitlines():
            w = ln.split()
            if w[0] == "R":
                rule[int(w[1])] = float(w[2])
            else:
                table[int(w[1])] = (float(w[2]), float(w[3]))
        return rule, table
    return run


# (shape, first rows of the state cones, of the input cones): the rocket's, the quadrotor shape with two state cones, a 32-lane shape
LAYOUTS = [((6, 3, 10), [1], [0]), ((6, 3, 10), [3], []), ((12, 4, 10), [1, 6], [0]), ((12, 4, 10), [9, 0], [1]), ((20, 8, 10), [2, 17], [5, 0])]


@pytest.mark.parametrize("shape,Acx,Acu", LAYOUTS)
def test_fill_rule_puts_every_coefficient_in_the_lanes_of_its_cone(dump, shape, Acx, Acu):
    nx, nu, N = shape
    lw = 16 * ((nx + nu + 15) // 16)
    # the dump's one instance: cx[k] = 101 + k, cu[k] = 201 + k.  The layout: the three rows of state cone k are lanes Acx[k] .. + 2, those of
    # input cone k lanes nx + Acu[k] .. + 2; 1.0 on every other lane; the block does not depend on the enable switches
    want = np.ones(lw)
    for k, first in enumerate(Acx):
        want[first:first + 3] = 101.0 + k
    for k, first in enumerate(Acu):
        want[nx + first:nx + first + 3] = 201.0 + k
    for en in ((1, 1), (1, 0), (0, 1), (0, 0)):
        rule, table = dump(shape, en, Acx, Acu)
        assert sorted(rule) == sorted(table) == list(range(lw))
        assert np.array_equal(np.array([rule[j] for j in range(lw)]), want), en
        # the shared table under the switches: the same coefficient on the lanes of an enabled family's cones (where VEC_CONE_BASE names
        # the cone's first lane), 0.0 and no cone everywhere else -- the positions are the block's
        for j in range(lw):
            mu, base = table[j]
            family_on = en[0] if j < nx else (en[1] if j < nx + nu else 0)
            if family_on and want[j] != 1.0:
                assert mu == want[j] and 0 <= j - base <= 2, (en, j)
            else:
                assert mu == 0.0 and base == -1.0, (en, j)


def test_fill_rule_on_cones_that_share_rows_is_the_shared_table_s(dump):
    """where cones share rows the last one in the caller's order holds the lane, as in the shared table (no register kernel runs such a
    set: the coverage kernel walks the cones by index with the caller's dense arrays)"""
    rule, table = dump((12, 4, 10), (1, 1), [0, 2, 1], [0, 1])
    want = np.ones(16)
    want[[0]] = 101.0                                                 # cone 0 keeps row 0 only; cone 2 (rows 1..3) came last, cone 1 keeps row 4
    want[1:4] = 103.0
    want[4] = 102.0
    want[12] = 201.0
    want[13:16] = 202.0
    assert np.array_equal(np.array([rule[j] for j in range(16)]), want)
    assert all(table[j][0] == (want[j] if want[j] != 1.0 else 0.0) for j in range(16))


# ---- the path and the variant choice ----------------------------------------------------------------------------------------------------
def _parent_commit():
    """the commit before the one that brought per-instance cone coefficients (a work tree that has not committed them yet: HEAD)"""
    git = lambda *a: subprocess.run(["git", "-C", ROOT] + list(a), capture_output=True, text=True, timeout=60)
    if git("rev-parse", "HEAD").returncode != 0:
        return None
    first = git("log", "--format=%H", "--reverse", "-Sinst_cones", "--", "tinympc_amd/csrc/kernel_path.hpp").stdout.split()
    rev = first[0] + "^" if first else "HEAD"
    return rev if git("cat-file", "-e", rev + ":tinympc_amd/csrc/kernel_path.hpp").returncode == 0 else None


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    rev = _parent_commit()
    if rev is None:
        pytest.skip("no git history to take the parent's headers from")
    d = tmp_path_factory.mktemp("instance_cones_path")
    os.makedirs(d / "parent")
    for h in ("kernel_path.hpp", "one_row_variant.hpp"):
        text = subprocess.run(["git", "-C", ROOT, "show", "%s:tinympc_amd/csrc/%s" % (rev, h)], check=True, capture_output=True, text=True, timeout=60).stdout
        assert "inst_cones" not in text and not re.search(r"\b(int|bool) pc\b", text), h       # (the headers before the feature)
        (d / "parent" / h).write_text(text)
    exe = str(d / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, "-I", str(d), os.path.join(ROOT, "tests", "dropin", "instance_cones_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _lines(exe, mode, stdin=None):
    out = subprocess.run([exe, mode], input=stdin, check=True, capture_output=True, text=True, timeout=900).stdout.splitlines()
    return [dict(w.split("=", 1) for w in ln.split()) for ln in out]


JIT = dict(fits_box=1, fits=1, soc=1, inst_cones=1)


def test_path_rules_with_per_instance_cone_coefficients(driver):
    cases = [
        (JIT, ("ONE_ROW", "one_row:pc", 1, 3, 0)),
        (dict(JIT, hetero=1), ("ONE_ROW", "one_row:pc", 1, 3, 0)),
        (dict(JIT, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:pc", 1, 3, 0)),                    # a compiled-in entry is not asked
        (dict(JIT, cones_overlap=1), ("COVERAGE", "cones_overlap", 0, 2, 0)),
        (dict(JIT, inst_bounds=1), ("COVERAGE", "cover:pb", 0, 2, 0)),
        (dict(JIT, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1, inst_lin=1), ("COVERAGE", "cover:pc_with_halfspaces", 0, 2, 0)),
        (dict(JIT, lin_families=1, lin_kmax=4, planes_fit=1), ("COVERAGE", "cover:pc", 0, 2, 0)),       # shared half-spaces
        (dict(JIT, debug=1), ("COVERAGE", "cover:pc", 0, 2, 0)),
        (dict(JIT, force_general=1), ("COVERAGE", "cover:pc", 0, 2, 0)),
        (dict(JIT, no_jit=1), ("COVERAGE", "cover:pc", 0, 2, 0)),
        (dict(JIT, variant_jit_failed=1), ("COVERAGE", "cover:pc", 0, 2, 0)),
        (dict(JIT, jit_failed=1), ("COVERAGE", "cover:pc", 0, 2, 0)),
        (dict(soc=1, inst_cones=1, has_tile=1), ("COVERAGE", "cover:pc", 0, 2, 0)),                     # a tile-kernel shape
        (dict(JIT, adaptive=1), ("ONE_ROW", "one_row:pc", 1, 3, 5)),                                   # refused: REFUSE_ADAPTIVE_INSTANCE_CONES
        (dict(JIT, adaptive=1, cones_overlap=1), ("COVERAGE", "cones_overlap", 0, 2, 5)),               # ... reported before the overlapping cones
        (dict(JIT, adaptive=1, inst_bounds=1), ("COVERAGE", "cover:pb", 0, 2, 1)),
        (dict(JIT, adaptive=1, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1, inst_lin=1), ("COVERAGE", "cover:pc_with_halfspaces", 0, 2, 2)),
        (dict(JIT, inst_cones=0), ("ONE_ROW", "one_row:plain", 0, 3, 0)),
        (dict(JIT, inst_cones=0, adaptive=1, cones_overlap=1), ("COVERAGE", "cones_overlap", 0, 2, 3)),
    ]
    stdin = "".join(" ".join("%s=%d" % kv for kv in f.items()) + "\n" for f, _ in cases)
    got = _lines(driver, "path", stdin)
    assert len(got) == len(cases)
    for (f, (kernel, rule, pc, code, refusal)), g in zip(cases, got):
        assert (g["kernel"], g["rule"], int(g["pc"]), int(g["code"]), int(g["refusal"]), g["consistent"]) == (kernel, rule, pc, code, refusal, "1"), (f, g)
        assert (g["lin"], g["pl"], g["pb"]) == ("0", "0", "0"), (f, g)
    # inst_cones without a cone family on is nothing path_facts can produce
    assert _lines(driver, "path", "inst_cones=1 fits=1 fits_box=1\n")[0]["consistent"] == "0"
    out = subprocess.run([driver, "message"], check=True, capture_output=True, text=True, timeout=60).stdout.strip()
    assert out.startswith("5 adaptive rho does not combine with per-instance cone coefficients (tiny_batch_set_instance_cone_coefficients)"), out


def test_path_sweep_follows_the_rules_and_equals_the_parent_without_the_feature(driver):
    rows = _lines(driver, "paths")
    tail = {k: int(v) for r in rows if len(r) == 1 for k, v in r.items()}
    assert tail["parent_compared"] > 1000000 and tail["parent_differ"] == 0, tail
    assert tail["with_cones"] > 100000 and tail["violations"] == 0, tail
    rules = {r["rule"] for r in rows if "rule" in r}
    assert rules == {"cones_overlap", "cover:pb", "cover:pc_with_halfspaces", "one_row:pc", "cover:pc"}, rules
    for r in (r for r in rows if "rule" in r):
        assert (r["pc"] == "1") == (r["rule"] == "one_row:pc") and r["code"] == ("3" if r["rule"] == "one_row:pc" else "2"), r


def test_variant_sweep_keys_the_pc_form_and_equals_the_parent_without_it(driver):
    rows = _lines(driver, "variants")
    tail = {k: int(v) for r in rows if len(r) == 1 for k, v in r.items()}
    assert tail["parent_compared"] > 100000 and tail["parent_differ"] == 0, tail
    assert tail["with_pc"] > 0 and tail["key_order"] == 1, tail
    forms = [r for r in rows if "slot" in r]
    assert forms
    for r in forms:
        # run-time instantiated only (whatever the entry holds), full rows, no PREFETCH slot, no fallback; never with pb, pl, lin, debug, adaptive
        assert r["pc"] == "1" and r["soc"] == "1" and r["slot"].startswith("NONE") and r["ipw"] == "4" and r["prefetch"].startswith("NONE"), r
        assert r["fallback"].startswith("NONE") and (r["pb"], r["pl"], r["lin"], r["dbg"], r["adapt"]) == ("0", "0", "0", "0", "0"), r
        assert r["het"] == r["hetero"] and r["ub_form"] == r["ub"] and (r["het"] == "0" or r["mode"] == "2"), r
    assert {(r["het"], r["ub"]) for r in forms} == {("0", "0"), ("0", "1"), ("1", "0"), ("1", "1")}


# ---- the PC forms ------------------------------------------------------------------------------------------------------------------------
CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
import tinympc_amd as tm
out = []
for name in sys.argv[2:]:
    try:
        n, hit = tm.jit_compile(name)
        out.append({"name": name, "bytes": n})
    except RuntimeError as e:
        out.append({"name": name, "error": str(e)[:1500]})
print(json.dumps(out))
'''

PC_VARIANTS = [pc_name(6, 3, 10), pc_name(6, 3, 10, het=True), pc_name(6, 3, 10, ub=True), pc_name(12, 4, 10, het=True, ub=True), pc_name(5, 3, 7)]


def test_pc_variants_compile_and_the_flag_without_a_cone_is_refused():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PC_VARIANTS, capture_output=True, text=True, timeout=1500, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert [r["name"] for r in res] == PC_VARIANTS
    bad = [r for r in res if "error" in r]
    assert not bad, bad
    assert all(r["bytes"] > 1000 for r in res)
    # (a tree whose kernel does not know the flag refuses MODE 18 for every name: its static_assert ends at 16.  What tells the PC forms
    # here is the text of the refusal: the flag without a cone, and with per-instance half-spaces)
    refused = [pc_name(6, 3, 10, soc=False), "tinympc_amd::admm_solve_kernel<6, 3, 10, true, false, 26, 1, false, 1, false>"]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + refused, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert "error" in res[0] and "per-instance cone coefficients: a cone variant (SOC)" in res[0]["error"], res[0]
    assert "error" in res[1] and "per-instance cone coefficients: not with per-instance half-spaces" in res[1]["error"], res[1]


def test_pc_forms_cost_no_occupancy_no_lds_and_at_6_3_10_no_scratch(tmp_path):
    """the cone variant of (6,3,10) and of (12,4,10), plain and HET, knot-invariant box or not, with and without PC, compiled side by
    side: the reference is the form without PC as THIS tree compiles it, not a fixed number.  Waves per SIMD and static LDS are the
    shared form's by construction (the launch attribute and the shared arrays do not see the flag).  Scratch: a PC form carries
    item_mu through the iteration loop as the shared form does, and item_rmu not at all, so it should spill no more -- which holds at
    (6,3,10), the shape of the rocket landing, where only the HET + UB form spills at all.  At (12,4,10), where every cone form sits at
    256 registers and spills 72 to 196 B/lane already, the compiler disagrees: 72 / 108 / 192 / 216 B/lane against 72 / 92 / 172 / 196
    (profiles/instance_cones.md); those figures are printed, not asserted"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    import register_audit
    for nx, nu, N, hets in ((6, 3, 10, (False, True)), (12, 4, 10, (False, True))):
        names = [pc_name(nx, nu, N, het=het, pc=pc, ub=ub) for het in hets for ub in (False, True) for pc in (False, True)]
        src = tmp_path / ("pc_audit_%d_%d.hip" % (nx, nu))
        src.write_text('#define TINYMPC_FUSED_NX %d\n#define TINYMPC_FUSED_NU %d\n#include "%s"\n' % (nx, nu, os.path.join(CSRC, "admm_kernel.hip.h")) +
                       "".join("template __global__ void tinympc_amd::%s(const tinympc_amd::SolveArgs);\n" % n[n.index("admm_"):] for n in names))
        rows = register_audit.usage(str(src), cwd=str(tmp_path))
        # template arguments as the symbol spells them: <NX,NU,N,SOC,DBG,MODE | 16 PC,LIN,HET,KMAX,ADAPT,UB,HALF,PF>
        by = {(r["args"][7], r["args"][10], r["args"][5] >> 4): r for r in rows}
        assert len(by) == len(names) == len(rows), [r["name"] for r in rows]
        for het in (0, 1):
            for ub in (0, 1):
                ref, pc = by[(het, ub, 0)], by[(het, ub, 1)]
                print((nx, nu, N), "het", het, "ub", ub, "shared", {k: ref[k] for k in ("vgpr", "agpr", "scratch", "occ", "lds")},
                      "pc", {k: pc[k] for k in ("vgpr", "agpr", "scratch", "occ", "lds")})
                assert pc["occ"] == ref["occ"] and pc["lds"] == ref["lds"], (het, ub, pc, ref)
                if (nx, nu, N) == (6, 3, 10):
                    assert pc["scratch"] <= ref["scratch"], (het, ub, pc, ref)
