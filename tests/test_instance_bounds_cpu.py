"""CPU: per-instance box constraints (tiny_batch_set_instance_bounds) as far as they can be checked without a GPU -- the exported
entry points and their NULL returns; that the PB forms of the one-row kernel (run-time instantiated only) compile for gfx950; the fill
rule of the array the kernels read (csrc/lane_tables.hpp box_entry, dumped by tests/dropin/instance_bounds_dump.cpp) against the slot
convention restated here and against the bounds block of the shared lane table; and that the PB form of the headline variant costs no
occupancy and no scratch over the form it is derived from."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("tiny_batch_set_instance_bounds", "tiny_batch_get_instance_bounds", "tiny_group_set_instance_bounds")


def pb_name(nx, nu, N, ub, het, pb=True):
    """the instantiation name csrc/jit.hip builds for a box variant at MODE 2: PB is bit 2 of the MODE argument, UB the last one"""
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, false, false, %d, 0, %s, 4, false%s>" % (nx, nu, N, 6 if pb else 2, "true" if het else "false",
                                                                                                ", true" if ub else "")


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_set_instance_bounds(None, None, None, None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_instance_bounds(None, 0, None, None, None, None) == tm.ERR_NULL
    assert L.tiny_group_set_instance_bounds(None, None, None, None, None) == tm.ERR_NULL


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

PB_VARIANTS = [pb_name(12, 4, 10, ub, het) for ub in (True, False) for het in (False, True)] + \
              [pb_name(2, 2, 3, True, False), pb_name(8, 8, 10, True, False), pb_name(4, 2, 30, True, False)]


# the cone register variants are out of scope: a per-instance box with a cone runs on the coverage kernel, and the kernel says so
PB_WITH_CONE = "tinympc_amd::admm_solve_kernel<12, 4, 10, true, false, 6, 0, false, 4, false, true>"


def test_pb_variants_compile():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + PB_VARIANTS, capture_output=True, text=True, timeout=1500, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert [r["name"] for r in res] == PB_VARIANTS
    bad = [r for r in res if "error" in r]
    assert not bad, bad
    assert all(r["bytes"] > 1000 for r in res)
    # (a tree whose kernel does not know the flag compiles SOME kernel for these names too: MODE is an int.  What tells the PB forms
    # from that is below -- the cone variant with the flag is refused by name, and the resource test sees the rows' bound blocks in LDS)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT, PB_WITH_CONE], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert "error" in res[0] and "per-instance box" in res[0]["error"], res


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    exe = str(tmp_path_factory.mktemp("instance_bounds") / "dump")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, "-x", "hip", os.path.join(ROOT, "tests", "dropin", "instance_bounds_dump.cpp"),
                    os.path.join(CSRC, "batch_tables.hip"), "-o", exe], check=True, capture_output=True, timeout=600)

    def run(shape, sb, ib):
        out = subprocess.run([exe] + [str(v) for v in shape] + [str(int(sb)), str(int(ib))], check=True, capture_output=True, text=True, timeout=60).stdout
        blocks = {"R": {}, "T": {}}
        for ln in out.splitlines():
            tag, s, j, lo, hi = ln.split()
            blocks[tag][(int(s), int(j))] = (float(lo), float(hi))
        return blocks
    return run


@pytest.mark.parametrize("shape", [(2, 2, 3), (12, 4, 10), (8, 8, 10), (20, 8, 10)])
def test_fill_rule_puts_every_source_element_in_its_slot_and_lane(dump, shape):
    nx, nu, N = shape
    nz, lw = nx + nu, 16 * ((nx + nu + 15) // 16)
    # the dump's one instance: every source element a distinct number ([knot][row], as the setter takes them)
    x_min, x_max = 1.0 + np.arange(N * nx).reshape(N, nx), 10001.0 + np.arange(N * nx).reshape(N, nx)
    u_min, u_max = 20001.0 + np.arange((N - 1) * nu).reshape(N - 1, nu), 30001.0 + np.arange((N - 1) * nu).reshape(N - 1, nu)
    everything = np.concatenate([v.ravel() for v in (x_min, x_max, u_min, u_max)])
    assert np.unique(everything).size == everything.size
    for sb, ib in itertools.product((1, 0), (1, 0)):
        # the convention: state lanes keep knot s in slot s; input lanes keep knot s - 1 in slot s, their slot 0 is (-inf, +inf); lanes
        # from nx + nu on and a disabled family are (-inf, +inf)
        lo, hi = np.full((N, lw), -np.inf), np.full((N, lw), np.inf)
        if sb:
            lo[:, :nx], hi[:, :nx] = x_min, x_max
        if ib:
            lo[1:, nx:nz], hi[1:, nx:nz] = u_min, u_max
        got = dump(shape, sb, ib)
        assert sorted(got["R"]) == sorted(got["T"]) == [(s, j) for s in range(N) for j in range(lw)]
        rule = np.array([[got["R"][(s, j)] for j in range(lw)] for s in range(N)])
        assert np.array_equal(rule[:, :, 0], lo) and np.array_equal(rule[:, :, 1], hi), (sb, ib)
        # ... and the bounds block fill_lane_tables writes when the same box is the SHARED one.  (Not a second witness of the rule: that
        # builder calls box_entry too.  What this pins is that a shared and a per-instance box of the same numbers are ONE block --
        # the rule itself is checked by the numpy statement above, the shared table also by tests/test_lane_tables_cpu.py)
        table = np.array([[got["T"][(s, j)] for j in range(lw)] for s in range(N)])
        assert np.array_equal(table, rule), (sb, ib)


def test_pb_form_of_the_headline_variant_costs_no_occupancy_and_no_scratch(tmp_path):
    """the UB instantiation of (12,4,10), plain and HET, with and without PB, compiled side by side: the reference is the form without
    PB as THIS tree compiles it, not a fixed number"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    import register_audit
    names = [pb_name(12, 4, 10, True, het, pb) for het in (False, True) for pb in (False, True)]
    names += [pb_name(12, 4, 10, False, False, pb) for pb in (False, True)]      # the knot-varying pair: the rows' bound blocks in LDS
    src = tmp_path / "pb_audit.hip"
    src.write_text('#define TINYMPC_FUSED_NX 12\n#define TINYMPC_FUSED_NU 4\n#include "%s"\n' % os.path.join(CSRC, "admm_kernel.hip.h") +
                   "".join("template __global__ void tinympc_amd::%s(const tinympc_amd::SolveArgs);\n" % n[n.index("admm_"):] for n in names))
    rows = register_audit.usage(str(src), cwd=str(tmp_path))
    # template arguments as the symbol spells them: <NX,NU,N,SOC,DBG,MODE | 4 PB,LIN,HET,KMAX,ADAPT,UB,HALF,PF>
    by = {(r["args"][7], r["args"][5] >> 2): r for r in rows if r["args"][10] == 1}
    assert sorted(by) == [(0, 0), (0, 1), (1, 0), (1, 1)], [r["name"] for r in rows]
    # what makes a PB form one: without UB every one of the wave's four rows has its own [lo | hi][N][16] block where the shared form
    # has one for the wave -- three more blocks of 2 x 10 x 16 doubles of static LDS, nothing else
    varying = {r["args"][5] >> 2: r for r in rows if r["args"][10] == 0}
    assert sorted(varying) == [0, 1], [r["name"] for r in rows]
    assert varying[1]["lds"] - varying[0]["lds"] == 3 * 2 * 10 * 16 * 8, (varying[1]["lds"], varying[0]["lds"])
    assert varying[1]["occ"] == varying[0]["occ"] and varying[1]["scratch"] <= varying[0]["scratch"], varying
    # ... and with UB it uses no LDS for bounds at all
    assert by[(0, 1)]["lds"] == by[(0, 0)]["lds"] and by[(1, 1)]["lds"] == by[(1, 0)]["lds"], by
    for het in (0, 1):
        ref, pb = by[(het, 0)], by[(het, 1)]
        assert ref["args"][10] == pb["args"][10] == 1
        assert pb["occ"] == ref["occ"], (het, pb, ref)
        assert pb["scratch"] <= ref["scratch"], (het, pb, ref)
