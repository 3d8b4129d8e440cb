"""CPU only: the instruction budget of the headline kernel's ADMM iteration loop, from the gfx950 assembly hipcc emits.

The quadrotor launch (admm_solve_kernel<12,4,10>, knot-invariant bounds) is bound by VALU issue: its time follows the number of
instructions one wave issues per iteration.  Per knot the mapping needs its 32 DPP FMAs (the two 16-column sweeps) and a handful
of lane-local FP64 operations; this test pins what stands around them -- accumulator copies, s_nop wait states, other FP64 work --
so that a change to the shared template cannot add issue slots to the loop unnoticed.  It also checks the wait states the DPP
broadcasts themselves need, which nothing else checks: an operand broadcast by row_newbcast must not have been written by a VALU
instruction in the two issue slots before (the one exception is the in-place, bank-masked B u chain of the forward step, whose
broadcast lanes lie in banks its bank_mask disables, so the chain never writes them)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_loop_stats  # noqa: E402

# <12,4,10, box only, dpp_mode 2, plain, knot-invariant bounds (UB)>: the form bench.py launches
HEADLINE = "ILi12ELi4ELi10ELb0ELb0ELi2ELi0ELb0ELi4ELb0ELb1ELb0ELb0EE"

# static counts of the loop body (isa_loop_stats.py row 12 4 10 false false 2 0 false 4 false true false false --fused)
BUDGET = {"total": 488, "mov": 5, "nop/wait": 4, "fp64_non_dpp": 131}
DPP_FMAS = 288          # 9 backward + 9 forward knots x 16 columns


def _regs(op):
    m = re.match(r"-?\|?v\[(\d+):(\d+)\]", op)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"-?\|?v(\d+)$", op)
    return {int(m.group(1))} if m else set()


@pytest.fixture(scope="module")
def headline_loop(tmp_path_factory):
    src = os.path.join(ROOT, "tinympc_amd", "csrc", "_gen", "u_12_4_10.hip")
    if not os.path.exists(src):
        pytest.skip("library not built through the Makefile")
    asm = str(tmp_path_factory.mktemp("isa") / "u_12_4_10.s")
    p = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S", src, "-o", asm],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    found = [(sym, lines, loop, meta) for sym, lines, loop, meta in isa_loop_stats.analyse(asm)
             if "admm_solve_kernel" in sym and HEADLINE in sym]
    assert len(found) == 1, [f[0] for f in found]
    sym, lines, loop, meta = found[0]
    assert loop is not None
    return lines[loop[0]:loop[1] + 1], meta


def test_headline_loop_instruction_budget(headline_loop):
    body, meta = headline_loop
    assert meta["private_segment_fixed_size"] == 0 and meta["next_free_vgpr"] <= 249, meta
    cls = [isa_loop_stats.classify(l) for l in body]
    dpp = sum(1 for l in body if "_f64_dpp" in l)
    got = {"total": len(body), "mov": cls.count("mov"), "nop/wait": cls.count("nop/wait"), "fp64_non_dpp": cls.count("fp64") - dpp}
    assert dpp == DPP_FMAS, dpp
    for k, v in BUDGET.items():
        assert got[k] <= v, (k, got, BUDGET)


def _dpp_fields(l):
    """(broadcast lane, bank_mask) of a row_newbcast DPP instruction (bank_mask prints as 0xf, 7, ...)."""
    lane = re.search(r"row_newbcast:([0-9+]+)", l)
    mask = re.search(r"bank_mask:(0x[0-9a-f]+|\d+)", l)
    return (sum(int(x) for x in lane.group(1).split("+")) if lane else None), (int(mask.group(1), 0) if mask else 0xF)


def _in_place_safe(l, dst, src0):
    """An in-place chain (vdst == broadcast source) is safe only where the broadcast lane's bank is one the mask disables:
    that lane is never written by the chain, so an early read returns the value a late one would."""
    lane, mask = _dpp_fields(l)
    return dst == src0 and lane is not None and not (mask >> (lane // 4)) & 1


def test_in_place_check_rejects_an_enabled_broadcast_bank():
    ok = "v_fmac_f64_dpp v[10:11], v[10:11], v[58:59] row_newbcast:12+1 row_mask:0xf bank_mask:7"
    bad = "v_fmac_f64_dpp v[10:11], v[10:11], v[58:59] row_newbcast:12+1 row_mask:0xf bank_mask:0xf"
    bad2 = "v_fmac_f64_dpp v[10:11], v[10:11], v[58:59] row_newbcast:8+1 row_mask:0xf bank_mask:7"
    r = _regs("v[10:11]")
    assert _in_place_safe(ok, r, r) and not _in_place_safe(bad, r, r) and not _in_place_safe(bad2, r, r)


def test_headline_loop_dpp_broadcast_wait_states(headline_loop):
    body, _ = headline_loop
    short = []
    for i, l in enumerate(body):
        if "_dpp" not in l:
            continue
        ops = [o.strip() for o in l.split(None, 1)[1].split(",")]
        dst, src0 = _regs(ops[0]), _regs(ops[1])
        in_place = _in_place_safe(l, dst, src0)
        states = 0
        for j in range(i - 1, -1, -1):
            p = body[j]
            if p.startswith("s_nop"):
                states += int(p.split()[1]) + 1
            elif p.startswith("v_"):
                if _regs(p.split(None, 1)[1].split(",")[0].strip()) & src0:
                    # the writer must be the same in-place chain, under the same bank mask (it leaves the broadcast lane alone too)
                    prev_in_place = "_dpp" in p and _regs(p.split(None, 1)[1].split(",")[0].strip()) == dst and \
                        _dpp_fields(p)[1] == _dpp_fields(l)[1]
                    if not (in_place and prev_in_place):
                        short.append((i, l, j, p, states))
                    break
                states += 1
            if states >= 2:
                break
    assert not short, short[:4]
