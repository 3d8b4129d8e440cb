"""CPU: the per-instance disturbance sequence at the plant step (tiny_batch_set_disturbance) as far as it can be checked without a GPU --
the exported entry points and their NULL returns; the path and variant rules (tests/dropin/disturbance_path_driver.cpp), and that with
the feature off both choices are the ones of the headers before it; that the PD forms of the one-row kernel (run-time instantiated only)
compile for gfx950, that an ADAPT, HALF or PF name carrying the bit is refused by name, and what the forms cost in registers, scratch and
occupancy; the argument block's fixed layout; the oracle-side conditions of every case the GPU tests use."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import disturbance_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("tiny_batch_set_disturbance", "tiny_batch_get_disturbance", "tiny_group_set_disturbance")
PD = 32                                            # bit 5 of the kernel's MODE argument


def pd_name(nx, nu, N, soc=False, mode=2, lin=0, het=False, kmax=4, adapt=False, ub=False, tail=""):
    """the instantiation name csrc/jit.hip builds: <NX, NU, N, SOC, DBG, MODE | 4 PB | 8 PL | 16 PC | 32 PD, LIN, HET, KMAX, ADAPT[, UB[, HALF[, PF]]]>"""
    b = lambda v: "true" if v else "false"
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, %d, %s, %d, %s%s%s>" % (nx, nu, N, b(soc), mode, lin, b(het), kmax, b(adapt), ", true" if ub else "", tail)


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_set_disturbance(None, None, 0, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_disturbance(None, 0, 0, None) == tm.ERR_NULL
    assert L.tiny_group_set_disturbance(None, None, 0, tm.HOST) == tm.ERR_NULL
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        assert callable(cls.set_disturbance) and callable(cls.get_disturbance)
    assert callable(tm.TinyBatchSolver.set_disturbance_device)


def test_the_argument_block_keeps_its_size_and_offsets_and_the_fields_lie_over_pf_base(tmp_path):
    src = open(os.path.join(CSRC, "admm_kernel.hip.h")).read()
    assert "sizeof(SolveArgs) == 472" in src
    assert "__builtin_offsetof(SolveArgs, pf_counter) == 432 && __builtin_offsetof(SolveArgs, pf_base) == 440" in src
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    prog = ('#include <cstdio>\n#include "%s"\nusing tinympc_amd::SolveArgs;\nint main() { printf("%%zu %%zu %%zu %%zu %%zu\\n", sizeof(SolveArgs), '
            '__builtin_offsetof(SolveArgs, pf_base), __builtin_offsetof(SolveArgs, dist), __builtin_offsetof(SolveArgs, dist_steps), '
            '__builtin_offsetof(SolveArgs, dist_step0)); return 0; }\n' % os.path.join(CSRC, "admm_kernel.hip.h"))
    exe, cpp = str(tmp_path / "layout"), tmp_path / "layout.hip"
    cpp.write_text(prog)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", str(cpp), "-o", exe], check=True, capture_output=True, timeout=600)
    words = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=60).stdout.split()
    assert [int(w) for w in words] == [472, 440, 440, 448, 452], words


@pytest.mark.parametrize("name", list(dc.CASES))
def test_the_cases_of_the_gpu_tests_meet_their_conditions(name):
    dc.check_case(name)
    c = dc.case(name)
    w = c["w"]
    assert w.shape == (dc.N_STEPS, c["B"], c["nx"]) and dc.N_STEPS < dc.T
    assert np.unique(w).size == w.size and 0.5 <= np.abs(w).min() and np.abs(w).max() <= 1.0      # distinct, of the size of x0
    assert 0.5 <= np.abs(c["x0"]).min() and np.abs(c["x0"]).max() <= 1.0


def test_the_batches_end_in_tiles_of_one_three_and_two_rows():
    assert {c["B"] % 4 for c in dc.CASES.values()} == {1, 3, 2} and max(c["B"] for c in dc.CASES.values()) == 13


# ---- the path and the variant choice ----------------------------------------------------------------------------------------------------
def _parent_commit():
    """the commit before the one that brought the disturbance (a work tree that has not committed it yet: HEAD)"""
    git = lambda *a: subprocess.run(["git", "-C", ROOT] + list(a), capture_output=True, text=True, timeout=60)
    if git("rev-parse", "HEAD").returncode != 0:
        return None
    first = git("log", "--format=%H", "--reverse", "-SREFUSE_ADAPTIVE_DISTURBANCE", "--", "tinympc_amd/csrc/kernel_path.hpp").stdout.split()
    rev = first[0] + "^" if first else "HEAD"
    return rev if git("cat-file", "-e", rev + ":tinympc_amd/csrc/kernel_path.hpp").returncode == 0 else None


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    rev = _parent_commit()
    if rev is None:
        pytest.skip("no git history to take the parent's headers from")
    d = tmp_path_factory.mktemp("disturbance_path")
    os.makedirs(d / "parent")
    for h in ("kernel_path.hpp", "one_row_variant.hpp"):
        text = subprocess.run(["git", "-C", ROOT, "show", "%s:tinympc_amd/csrc/%s" % (rev, h)], check=True, capture_output=True, text=True, timeout=60).stdout
        assert "disturbance" not in text and not re.search(r"\b(int|bool) pd\b", text), h       # (the headers before the feature)
        (d / "parent" / h).write_text(text)
    exe = str(d / "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-I", CSRC, "-I", str(d), os.path.join(ROOT, "tests", "dropin", "disturbance_path_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def _lines(exe, mode, stdin=None):
    out = subprocess.run([exe, mode], input=stdin, check=True, capture_output=True, text=True, timeout=900).stdout.splitlines()
    return [dict(w.split("=", 1) for w in ln.split()) for ln in out]


BOX = dict(fits_box=1, fits=1, disturbance=1)
CONE = dict(BOX, soc=1)
LIN = dict(BOX, lin_families=1, lin_kmax=4, planes_fit=1, pl_planes_fit=1)


def test_path_rules_with_a_disturbance(driver):
    # facts -> (kernel, rule, (lin, pl, pb, pc, pd), path code, refusal)
    cases = [
        (BOX, ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1), 3, 0)),
        (dict(BOX, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1), 3, 0)),           # a compiled-in entry is not asked
        (dict(BOX, hetero=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1), 3, 0)),
        (CONE, ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1), 3, 0)),
        (dict(LIN, has_entry=1, entry_klin=1), ("ONE_ROW", "one_row:pd", (1, 0, 0, 0, 1), 3, 0)),            # shared half-spaces: the LIN variant's PD form
        # composition with the per-instance rules: their forms take the bit and keep their rule
        (dict(BOX, inst_bounds=1), ("ONE_ROW", "one_row:pb", (0, 0, 1, 0, 1), 3, 0)),
        (dict(LIN, inst_lin=1), ("ONE_ROW", "one_row:pl", (1, 1, 0, 0, 1), 3, 0)),
        (dict(CONE, inst_cones=1), ("ONE_ROW", "one_row:pc", (0, 0, 0, 1, 1), 3, 0)),
        # ... and a coverage answer stays coverage
        (dict(CONE, **LIN, inst_lin=1, inst_cones=1), ("COVERAGE", "cover:pc_with_halfspaces", (0, 0, 0, 0, 0), 2, 0)),
        (dict(CONE, inst_bounds=1), ("COVERAGE", "cover:pb", (0, 0, 0, 0, 0), 2, 0)),
        (dict(CONE, cones_overlap=1), ("COVERAGE", "cones_overlap", (0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, force_general=1), ("COVERAGE", "cover:force_general", (0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, debug=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, no_jit=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0), 2, 0)),  # no hipRTC: not the compiled-in form, which adds nothing
        (dict(BOX, variant_jit_failed=1, has_entry=1, entry_plain=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, jit_failed=1), ("COVERAGE", "cover:no_register_form", (0, 0, 0, 0, 0), 2, 0)),
        # never the tile kernel while the fact is on: its shapes run on the coverage kernel
        (dict(disturbance=1, has_tile=1), ("COVERAGE", "cover:no_register_form", (0, 0, 0, 0, 0), 2, 0)),
        (dict(BOX, has_tile=1, prefer_tile=1), ("ONE_ROW", "one_row:pd", (0, 0, 0, 0, 1), 3, 0)),
        (dict(has_tile=1), ("TILE", "tile:no_register_form", (0, 0, 0, 0, 0), 1, 0)),
        # adaptive rho: refused with the new value, appended last -- what was refused before keeps its value
        (dict(BOX, adaptive=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0), 2, 6)),
        (dict(BOX, adaptive=1, inst_bounds=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0), 2, 1)),
        (dict(LIN, adaptive=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0), 2, 2)),
        (dict(CONE, adaptive=1, inst_cones=1), ("COVERAGE", "cover:pd", (0, 0, 0, 0, 0), 2, 5)),
        (dict(CONE, adaptive=1, cones_overlap=1), ("COVERAGE", "cones_overlap", (0, 0, 0, 0, 0), 2, 3)),
        # the fact off: the parent's answers
        (dict(BOX, disturbance=0), ("ONE_ROW", "one_row:plain", (0, 0, 0, 0, 0), 3, 0)),
        (dict(BOX, disturbance=0, has_entry=1, entry_plain=1), ("ONE_ROW", "one_row:plain", (0, 0, 0, 0, 0), 0, 0)),
        (dict(BOX, disturbance=0, adaptive=1), ("ONE_ROW", "one_row:adaptive", (0, 0, 0, 0, 0), 3, 0)),
    ]
    stdin = "".join(" ".join("%s=%d" % kv for kv in f.items()) + "\n" for f, _ in cases)
    got = _lines(driver, "path", stdin)
    assert len(got) == len(cases)
    for (f, (kernel, rule, forms, code, refusal)), g in zip(cases, got):
        assert (g["kernel"], g["rule"], int(g["code"]), int(g["refusal"]), g["consistent"]) == (kernel, rule, code, refusal, "1"), (f, g)
        assert tuple(int(g[k]) for k in ("lin", "pl", "pb", "pc", "pd")) == forms, (f, g)
    p = subprocess.run([driver, "message"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and p.stdout.strip() == "6 adaptive rho does not combine with a per-instance disturbance", (p.returncode, p.stdout)


def test_path_sweep_follows_the_rule_pair_and_equals_the_parent_without_the_fact(driver):
    rows = _lines(driver, "paths")
    tail = {k: int(v) for r in rows if len(r) == 1 for k, v in r.items()}
    assert tail["parent_compared"] > 1000000 and tail["parent_differ"] == 0, tail
    assert tail["with_disturbance"] == tail["parent_compared"] and tail["violations"] == 0, tail
    answers = [r for r in rows if "rule" in r]
    assert {r["rule"] for r in answers if r["kernel"] == "ONE_ROW"} == {"one_row:pd", "one_row:pb", "one_row:pl", "one_row:pc"}
    assert "cover:pd" in {r["rule"] for r in answers} and not any(r["kernel"] == "TILE" for r in answers)
    for r in answers:
        assert (r["pd"] == "1") == (r["kernel"] == "ONE_ROW") and r["code"] == ("3" if r["kernel"] == "ONE_ROW" else "2"), r
        assert r["kernel"] != "ONE_ROW" or r["refusal"] == "0", r                # (what is refused never names a PD form)
    assert {r["refusal"] for r in answers} == {"0", "1", "2", "3", "4", "5", "6"}


def test_variant_sweep_keys_the_pd_form_and_equals_the_parent_without_it(driver):
    rows = _lines(driver, "variants")
    tail = {k: int(v) for r in rows if len(r) == 1 for k, v in r.items()}
    assert tail["parent_compared"] > 100000 and tail["parent_differ"] == 0, tail
    assert tail["with_pd"] > 0 and tail["base_differs"] == 0 and tail["key_order"] == 1, tail
    forms = [r for r in rows if "slot" in r]
    assert forms
    for r in forms:
        # run-time instantiated only (whatever the entry holds), full rows, no PREFETCH slot, no fallback; never with debug or adaptive rho
        assert r["pd"] == "1" and r["slot"].startswith("NONE") and r["ipw"] == "4" and r["prefetch"].startswith("NONE") and r["fallback"].startswith("NONE"), r
        assert (r["dbg"], r["adapt"]) == ("0", "0") and r["het"] == r["hetero"] and r["ub_form"] == r["ub"], r
        # the knot-invariant box in registers where the form it rides on keeps it there (half-space variants never do)
        assert r["ub"] == "0" or r["lin"] == "0", r
    assert {(r["pb"], r["pl"], r["pc"]) for r in forms} == {("0", "0", "0"), ("1", "0", "0"), ("0", "1", "0"), ("0", "0", "1")}
    assert {r["ub"] for r in forms} == {"0", "1"} and {r["soc"] for r in forms} == {"0", "1"} and {r["lin"] for r in forms} == {"0", "1", "2", "3"}


# ---- the PD forms ------------------------------------------------------------------------------------------------------------------------
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
        out.append({"name": name, "error": str(e)[:3000]})
print(json.dumps(out))
'''

# the forms the GPU tests launch: (6,3,10) box (knot-invariant: UB), both cones, PB, PL (static half-spaces, two per knot), PC;
# (12,4,10) per-instance data; (5,3,7) a run-time shape; (4,2,10) a half-row shape on full rows
PD_VARIANTS = [pd_name(6, 3, 10, mode=2 | PD, ub=True), pd_name(6, 3, 10, mode=2 | PD), pd_name(6, 3, 10, soc=True, mode=2 | PD), pd_name(6, 3, 10, mode=2 | 4 | PD, ub=True),
               pd_name(6, 3, 10, mode=2 | 8 | PD, lin=1, kmax=2), pd_name(6, 3, 10, soc=True, mode=2 | 16 | PD), pd_name(6, 3, 10, mode=2 | PD, lin=1),
               pd_name(12, 4, 10, mode=2 | PD, het=True, ub=True), pd_name(5, 3, 7, mode=2 | PD, ub=True), pd_name(4, 2, 10, mode=2 | PD, ub=True)]


def test_pd_variants_compile_and_adapt_half_and_pf_names_are_refused():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PD_VARIANTS, capture_output=True, text=True, timeout=3000, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert [r["name"] for r in res] == PD_VARIANTS
    bad = [r for r in res if "error" in r]
    assert not bad, bad
    assert all(r["bytes"] > 1000 for r in res)
    # (a tree whose kernel does not know the flag refuses MODE 34 for every name: its static_assert ends at 32.  What tells the PD forms
    # here is the text of the refusal)
    refused = [(pd_name(6, 3, 10, mode=2 | PD, adapt=True), "per-instance disturbance: not with adaptive rho"),
               (pd_name(4, 2, 10, mode=2 | PD, tail=", false, true"), "per-instance disturbance: not the half-row form"),
               (pd_name(6, 3, 10, mode=2 | PD, tail=", false, false, true"), "per-instance disturbance: not the prefetch form")]
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + [n for n, _ in refused], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    for r, (_, text) in zip(res, refused):
        assert "error" in r and text in r["error"], r


def test_pd_forms_keep_the_waves_per_simd_and_static_lds_of_their_base_forms(tmp_path):
    """every PD form compiled next to the form it rides on: waves per SIMD and static LDS are the base form's (the launch attribute and
    the shared arrays do not see the flag); registers and scratch are printed for each.  Measured at this commit: +2 VGPRs on the box /
    cone forms (no scratch in either), none on the half-space forms; the per-instance-data forms of (12,4,10), which sit at 256
    registers and spill already, spill 8 and 16 B/lane more (52 -> 60, 76 -> 92): profiles/disturbance.md"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    import register_audit
    forms = {(6, 3, 10): [dict(), dict(ub=True), dict(soc=True), dict(soc=True, ub=True), dict(mode=2 | 4, ub=True), dict(soc=True, mode=2 | 16), dict(lin=1, mode=2 | 8, kmax=2),
                          dict(lin=1)],
             (12, 4, 10): [dict(ub=True), dict(het=True), dict(het=True, ub=True)], (5, 3, 7): [dict(ub=True)], (4, 2, 10): [dict(ub=True)]}
    for (nx, nu, N), variants in forms.items():
        names = [pd_name(nx, nu, N, **dict(v, mode=v.get("mode", 2) | pd)) for v in variants for pd in (0, PD)]
        src = tmp_path / ("pd_audit_%d_%d_%d.hip" % (nx, nu, N))
        src.write_text('#define TINYMPC_FUSED_NX %d\n#define TINYMPC_FUSED_NU %d\n#include "%s"\n' % (nx, nu, os.path.join(CSRC, "admm_kernel.hip.h")) +
                       "".join("template __global__ void tinympc_amd::%s(const tinympc_amd::SolveArgs);\n" % n[n.index("admm_"):] for n in names))
        rows = register_audit.usage(str(src), cwd=str(tmp_path))
        # template arguments as the symbol spells them: <NX,NU,N,SOC,DBG,MODE | 32 PD,LIN,HET,KMAX,ADAPT,UB,HALF,PF>
        by = {(tuple(r["args"][:5]) + (r["args"][5] & 31,) + tuple(r["args"][6:]), r["args"][5] >> 5): r for r in rows}
        assert len(by) == len(names) == len(rows), [r["name"] for r in rows]
        for (key, pd), r in sorted(by.items()):
            if pd:
                ref = by[(key, 0)]
                print((nx, nu, N), key[3:], "base", {k: ref[k] for k in ("vgpr", "agpr", "scratch", "occ", "lds")}, "pd", {k: r[k] for k in ("vgpr", "agpr", "scratch", "occ", "lds")})
                assert r["occ"] == ref["occ"] and r["lds"] == ref["lds"], (key, r, ref)
