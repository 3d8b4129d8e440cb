"""CPU: per-instance half-space constraints (tiny_batch_set_instance_linear_constraints / ..._tv_...) as far as they can be checked
without a GPU -- the exported entry points and their NULL returns; that the PL forms of the one-row kernel (run-time instantiated only)
compile for gfx950 and that the combinations the kernel excludes are refused by name, with the static_assert's text; the fill rule of the
blocks the kernels read (csrc/lane_tables.hpp halfspace_entry, dumped by tests/dropin/instance_halfspaces_dump.cpp) against the layout
restated here in numpy, against halfspace_ref's row-order norm and against the half-space part of the shared lane table; the oracle-side
conditions of every case the GPU tests use; and the static LDS, scratch and occupancy of the PL form of the quadrotor's time-varying
variant against the shared form it is derived from."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import halfspace_ref as hr
import instance_halfspace_cases as ihc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("tiny_batch_set_instance_linear_constraints", "tiny_batch_set_instance_tv_linear_constraints", "tiny_batch_get_instance_linear_constraints",
               "tiny_group_set_instance_linear_constraints", "tiny_group_set_instance_tv_linear_constraints")


def lin_lds(nx, nu, n, soc, lin, kmax, pl):
    """solve_kernel_lin_lds of csrc/admm_kernel.hip.h without UB: bytes of static LDS of a half-space variant with its slack planes"""
    nz = nx + nu
    csl = cs = (nz + 1) | 1
    tabs = 4 if pl else 1
    return 8 * (nx * 16 + 2 * n * 16 + ((tabs * 3 * kmax * 16 + 8 * n * csl) if lin & 1 else 0) + ((tabs * 3 * n * kmax * 16 + 8 * n * csl) if lin & 2 else 0) +
                ((4 * n + 1) * 3 * cs if soc else 0))


def lin_waves(nx, nu, n, soc, lin, kmax, pl):
    """solve_kernel_lin_waves for the shapes used here (N <= 10: the box kernel keeps two waves per SIMD)"""
    lds = lin_lds(nx, nu, n, soc, lin, kmax, pl)
    assert n <= 10 and lds <= 64 * 1024 - 512
    return 2 if 8 * lds <= 158 * 1024 else 1


def pl_name(nx, nu, N, lin, kmax, het=False, soc=False, pl=True, mode=2, adapt=False):
    """the instantiation name csrc/jit.hip builds for a half-space variant: PL is bit 3 of the MODE argument, PB bit 2"""
    return "tinympc_amd::admm_solve_kernel<%d, %d, %d, %s, false, %d, %d, %s, %d, %s>" % (nx, nu, N, "true" if soc else "false", mode | (8 if pl else 0), lin,
                                                                                           "true" if het else "false", kmax, "true" if adapt else "false")


def test_new_symbols_are_declared_and_exported_and_refuse_null():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_set_instance_linear_constraints(None, 0, None, None, 0, None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_set_instance_tv_linear_constraints(None, 0, None, None, 0, None, None, tm.HOST) == tm.ERR_NULL
    assert L.tiny_batch_get_instance_linear_constraints(None, 0, 0, None, None, None, None) == tm.ERR_NULL
    assert L.tiny_group_set_instance_linear_constraints(None, 0, None, None, 0, None, None) == tm.ERR_NULL
    assert L.tiny_group_set_instance_tv_linear_constraints(None, 0, None, None, 0, None, None) == tm.ERR_NULL


def test_solve_args_keep_their_size_and_offsets():
    """the PL pointer shares the place of the PREFETCH form's ticket counters (the kernel header asserts the numbers; they are the parent's)"""
    src = open(os.path.join(CSRC, "admm_kernel.hip.h")).read()
    assert "static_assert(sizeof(SolveArgs) == 472 && __builtin_offsetof(SolveArgs, het_tabs) == 208 && __builtin_offsetof(SolveArgs, pf_mask) == 416 &&" in src
    assert "__builtin_offsetof(SolveArgs, pf_counter) == 432 && __builtin_offsetof(SolveArgs, pf_base) == 440" in src


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
        out.append({"name": name, "error": str(e)[:6000]})
print(json.dumps(out))
'''

# (12,4,10) with LIN 1, 2, 3 and KMAX 1, 2, 4 where the LDS rule admits the form, with and without HET; (6,3,10) with the cone; (5,3,7)
PL_VARIANTS = [pl_name(12, 4, 10, lin, km, het) for lin in (1, 2, 3) for km in (1, 2, 4) for het in (False, True)
               if lin_lds(12, 4, 10, False, lin, km, True) <= 64 * 1024 - 512] + [pl_name(6, 3, 10, 3, 2, soc=True), pl_name(5, 3, 7, 3, 2)]
# what the kernel excludes, and the words its static_assert says it with
PL_REFUSED = [(pl_name(12, 4, 10, 2, 1, adapt=True), "per-instance half-spaces: not with adaptive rho"),
              (pl_name(12, 4, 10, 2, 1, mode=6), "per-instance half-spaces: not with a per-instance box"),
              (pl_name(12, 4, 10, 0, 4), "per-instance half-spaces: a half-space variant (LIN != 0)"),
              (pl_name(12, 4, 10, 2, 4), "per-instance half-spaces: the slack planes and the four rows' tables must fit the wave's static LDS")]


def _compile(names):
    env = dict(os.environ)
    env.pop("TINYMPC_AMD_JIT_CACHE", None)
    p = subprocess.run([sys.executable, "-c", CHILD, ROOT] + names, capture_output=True, text=True, timeout=1500, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads(p.stdout.strip().splitlines()[-1])
    assert [r["name"] for r in res] == names
    return res


def test_the_rule_admits_the_forms_this_file_expects():
    assert lin_lds(12, 4, 10, False, 2, 4, True) > 64 * 1024 - 512 and lin_lds(12, 4, 10, False, 3, 4, True) > 64 * 1024 - 512     # four [N][3][4][16] tables: 61 KB
    assert len(PL_VARIANTS) == 2 * (3 + 2 + 2) + 2
    assert lin_lds(4, 2, 30, False, 2, 1, True) > 64 * 1024 - 512                 # the GPU tests' (4,2,30) case: the coverage kernel


def test_pl_variants_compile():
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    res = _compile(PL_VARIANTS)
    bad = [r for r in res if "error" in r]
    assert not bad, bad
    assert all(r["bytes"] > 1000 for r in res)


def test_excluded_combinations_are_refused_with_the_static_asserts_text():
    """(a tree whose kernel does not know the flag compiles SOME kernel for such a name, or fails without these words: MODE is an int)"""
    if not any(os.path.exists(p) for p in ("/opt/rocm/lib/libhiprtc.so", "/opt/rocm/lib/libhiprtc.so.7")):
        pytest.skip("libhiprtc not installed")
    res = _compile([n for n, _ in PL_REFUSED])
    for r, (name, text) in zip(res, PL_REFUSED):
        assert "error" in r and text in r["error"], (name, text, r.get("error", "")[-800:])


# ---- the fill rule ---------------------------------------------------------------------------------------------------------------------
COUNTS = (3, 2, 2, 3)                              # static state | input, time-varying state | input (per knot)


def sources(nx, nu, N, seed=5):
    """one instance's eight arrays in the shapes the Python setters take, every element a distinct number with a full mantissa"""
    rng = np.random.default_rng([seed, nx, nu, N])
    ns, ni, nts, nti = COUNTS
    shapes = [(ns, nx), (ns,), (ni, nu), (ni,), (nts * N, nx), (nts, N), (nti * (N - 1), nu), (nti, N - 1)]
    out = [rng.uniform(0.5, 2.0, s) * rng.choice([-1.0, 1.0], s) for s in shapes]
    everything = np.concatenate([v.ravel() for v in out])
    assert np.unique(everything).size == everything.size
    return out


def row_order_norm(a):
    """a'a as halfspace_ref.project forms it: summed from 0.0 in row order, every product rounded"""
    return float(hr.project(np.zeros(len(a)), np.asarray(a)[None, :], np.array([np.inf]))[1]["nn"][0])


def expected_blocks(src, nx, nu, N, on, km, lw):
    """{(set, slot): [3][km][lw]} restated: state lanes keep the state family's row k of knot `slot`, input lanes the input family's of knot
    slot - 1 (none in slot 0); k beyond the count or km, lanes from nx + nu on and a disabled family are blank (0, +inf, 1)"""
    Ax, bx, Au, bu, tAx, tbx, tAu, tbu = src
    ns, ni, nts, nti = COUNTS

    def block(rows_x, off_x, on_x, rows_u, off_u, on_u):
        blk = np.zeros((3, km, lw))
        blk[1], blk[2] = np.inf, 1.0
        for lane0, rows, off, en in ((0, rows_x, off_x, on_x), (nx, rows_u, off_u, on_u)):
            if rows is None or not en:
                continue
            for k in range(min(len(off), km)):
                n = rows.shape[1]
                blk[0, k, lane0:lane0 + n], blk[1, k, lane0:lane0 + n], blk[2, k, lane0:lane0 + n] = rows[k], off[k], row_order_norm(rows[k])
        return blk

    out = {(0, 0): block(Ax, bx, on[0], Au, bu, on[1])}
    for s in range(N):
        ux = (tAu[nti * (s - 1):nti * s], tbu[:, s - 1]) if s >= 1 else (None, None)
        out[(1, s)] = block(tAx[nts * s:nts * (s + 1)], tbx[:, s], on[2], ux[0], ux[1], on[3])
    return out


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    d = tmp_path_factory.mktemp("instance_halfspaces")
    exe = str(d / "dump")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", "-I", CSRC, "-x", "hip", os.path.join(ROOT, "tests", "dropin", "instance_halfspaces_dump.cpp"),
                    os.path.join(CSRC, "batch_tables.hip"), "-o", exe], check=True, capture_output=True, timeout=600)

    def run(shape, src, on, km):
        nx, nu, N = shape
        path = str(d / ("in_%d_%d_%d.bin" % shape))
        # the setters' own layout: matrices column-major
        np.concatenate([np.asarray(v, dtype=np.float64).T.ravel() for v in src]).tofile(path)
        out = subprocess.run([exe] + [str(v) for v in shape + COUNTS] + [str(int(v)) for v in on] + [str(km), path], check=True, capture_output=True, text=True,
                             timeout=60).stdout
        lw = 16 * ((nx + nu + 15) // 16)
        tkm = None
        got = {"R": {}, "T": {}}
        for ln in out.splitlines():
            f = ln.split()
            if f[0] == "KM":
                tkm = int(f[1])
                continue
            tag, st, slot, k, lane = f[0], int(f[1]), int(f[2]), int(f[3]), int(f[4])
            stride = km if tag == "R" else tkm
            blk = got[tag].setdefault((st, slot), np.full((3, stride, lw), np.nan))
            blk[:, k, lane] = [float(v) for v in f[5:8]]
        return got, tkm
    return run


@pytest.mark.parametrize("shape", [(2, 2, 3), (12, 4, 10), (8, 8, 10), (20, 8, 10)])
def test_fill_rule_puts_every_source_element_in_its_slot_lane_and_k(dump, shape):
    nx, nu, N = shape
    lw = 16 * ((nx + nu + 15) // 16)
    src = sources(nx, nu, N)
    for on in ((1, 1, 1, 1), (0, 1, 1, 0), (1, 0, 0, 1), (0, 0, 0, 0)):
        for km in (4, 2):                         # km = 2: the third static state and time-varying input half-space are dropped
            got, tkm = dump(shape, src, on, km)
            want = expected_blocks(src, nx, nu, N, on, km, lw)
            assert sorted(got["R"]) == sorted(want)
            for key in want:
                assert hr.same_bits(got["R"][key], want[key]).all(), (on, km, key)
            # ... and the half-space part of the lane table fill_lane_tables writes when the same numbers are the SHARED sets: one rule,
            # one block (the shared table itself is pinned by tests/test_lane_tables_cpu.py and the existing half-space tests)
            assert tkm == 4
            table = expected_blocks(src, nx, nu, N, on, tkm, lw)
            for key in table:
                assert hr.same_bits(got["T"][key], table[key]).all(), (on, "table", key)
            if km == tkm:
                for key in want:
                    assert hr.same_bits(got["T"][key], got["R"][key]).all(), (on, "table against rule", key)


def test_the_norm_is_the_row_order_sum_not_numpys_pairwise_one():
    """at nx = 12 (and 20) numpy's np.sum pairs the terms differently; the inputs must show that, or the test above could not tell"""
    differing = 0
    for shape in ((12, 4, 10), (20, 8, 10)):
        src = sources(*shape)
        for rows in (src[0], src[4]):
            for a in rows:
                assert len(a) > 3
                differing += row_order_norm(a) != float(np.sum(a * a))
    assert differing > 0


@pytest.mark.parametrize("case", ihc.GPU_CASES, ids=lambda c: "_".join(str(int(v)) for v in c))
def test_oracle_conditions_of_the_gpu_cases(case):
    ihc.check_case(*case)


def test_launch_case_straddles_the_split_point():
    c = ihc.launch_case()
    its = [ihc.oracle_solve(c, i)[0][1] for i in range(c["B"])]
    assert min(its) < 10 < max(its), its


def test_pl_form_of_the_time_varying_variant_against_the_shared_form(tmp_path):
    """(12,4,10), LIN = 2, the PL form and the shared LIN form at the same KMAX, both as compiled by this tree"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    import register_audit
    names = [pl_name(12, 4, 10, 2, km, pl=pl) for km in (1, 2) for pl in (False, True)]
    src = tmp_path / "pl_audit.hip"
    src.write_text('#define TINYMPC_FUSED_NX 12\n#define TINYMPC_FUSED_NU 4\n#include "%s"\n' % os.path.join(CSRC, "admm_kernel.hip.h") +
                   "".join("template __global__ void tinympc_amd::%s(const tinympc_amd::SolveArgs);\n" % n[n.index("admm_"):] for n in names))
    rows = register_audit.usage(str(src), cwd=str(tmp_path))
    # template arguments as the symbol spells them: <NX,NU,N,SOC,DBG,MODE | 4 PB | 8 PL,LIN,HET,KMAX,...>
    by = {(r["args"][8], r["args"][5] >> 3): r for r in rows}
    assert sorted(by) == [(1, 0), (1, 1), (2, 0), (2, 1)], [r["name"] for r in rows]
    for km in (1, 2):
        shared, pl = by[(km, 0)], by[(km, 1)]
        # what makes a PL form one: every one of the wave's four rows has its own [N][3][KMAX][16] tables where the shared form has one
        # set for the wave -- three more table blocks of static LDS, nothing else
        assert pl["lds"] - shared["lds"] == 3 * (3 * 10 * km * 16) * 8, (km, pl["lds"], shared["lds"])
        assert pl["scratch"] <= shared["scratch"], (km, pl, shared)
        assert shared["occ"] == lin_waves(12, 4, 10, False, 2, km, False) and pl["occ"] == lin_waves(12, 4, 10, False, 2, km, True), (km, pl, shared)
        assert shared["lds"] == lin_lds(12, 4, 10, False, 2, km, False) and pl["lds"] == lin_lds(12, 4, 10, False, 2, km, True)
