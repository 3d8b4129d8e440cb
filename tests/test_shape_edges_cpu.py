"""CPU: the two shape formulas of csrc/jit.hpp at their edges (tests/shape_edges.py holds the table and a restatement of the formulas),
asked of the project's own host code through tests/dropin/shape_rules_driver.cpp -- and, from the same driver, the kernel every table
entry must end on (tiny_batch_setup's choice of a tile shape, path_facts' shape facts, decide_path's rules), which
tests/test_gpu_shape_edges.py asserts on the GPU: expected_paths() below is what it imports.  A second test runs the oracle alone over
every entry and both suites and asserts what keeps the GPU comparison from being vacuous."""
import functools
import os
import subprocess
import tempfile

import numpy as np
import pytest

import shape_edges as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
HIP_INCLUDE = "/opt/rocm/include"                 # (jit.hpp names hipFunction_t: the HIP headers, as plain C++ -- no HIP call is made)
PATH_NAME = {0: "regs", 1: "tile", 2: "cover", 3: "jit", 4: "tile-jit"}          # tinympc_amd.TinyBatchSolver.kernel_path


@functools.lru_cache(maxsize=None)
def build_driver():
    """tests/dropin/shape_rules_driver.cpp, built the way tests/test_kernel_path_cpu.py builds kernel_path_driver.cpp; once per process"""
    exe = os.path.join(tempfile.mkdtemp(prefix="shape_rules_"), "driver")
    subprocess.run([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-D__HIP_PLATFORM_AMD__", "-I", HIP_INCLUDE, "-I", CSRC, os.path.join(ROOT, "tests", "dropin", "shape_rules_driver.cpp"), "-o", exe],
                   check=True, capture_output=True, timeout=600)
    return exe


def listed_shapes(name):
    """{(nx, nu, N): the words after them} of kernel_dims.txt / tile_dims.txt"""
    out = {}
    for line in open(os.path.join(CSRC, name)):
        w = line.split("#")[0].split()
        if len(w) >= 3:
            out.setdefault(tuple(map(int, w[:3])), []).append(w[3:])
    return out


def shape_facts(shape, soc=False):
    """what the library's tables say of a shape, for a box (or cone) launch with default options"""
    entries, tiles = listed_shapes("kernel_dims.txt"), listed_shapes("tile_dims.txt")
    lean = shape in entries and any("lean" in w for w in entries[shape])
    return dict(nx=shape[0], nu=shape[1], N=shape[2], has_entry=int(shape in entries), entry_plain=int(shape in entries and not (lean and soc)),
                tile_entry=int(shape in tiles), soc=int(soc))


def ask_paths(queries):
    """each query: a dict of names the driver's `path` mode reads -> its answer as a dict; every query must be a consistent set of facts"""
    lines = [" ".join("%s=%d" % kv for kv in q.items()) for q in queries]
    out = subprocess.run([build_driver(), "path"], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True, timeout=60).stdout.splitlines()
    assert len(out) == len(lines)
    rows = []
    for q, ln in zip(queries, out):
        r = dict(w.split("=", 1) for w in ln.split())
        r = {k: (v if k in ("kernel", "rule") else int(v)) for k, v in r.items()}
        assert r.pop("consistent") == 1, q
        r["path"] = PATH_NAME[r["code"]]
        rows.append(r)
    return rows


def expected_paths(shapes, soc=False, **facts):
    """{shape: the driver's answer (with "path", the kernel_path() string)} for a launch with the settings / options `facts`"""
    shapes = list(shapes)
    return dict(zip(shapes, ask_paths([dict(shape_facts(s, soc), **facts) for s in shapes])))


@pytest.fixture(scope="module")
def rules():
    """{(nx, nu, N): (fits_box, fits_soc, (W, R) or None)} over the whole range the driver sweeps"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    out = subprocess.run([build_driver(), "rules"], check=True, capture_output=True, text=True, timeout=120).stdout
    t = np.array(out.split(), dtype=np.int64).reshape(-1, 8)
    return {(a, b, c): (bool(d), bool(e), (int(w), int(r)) if f else None) for a, b, c, d, e, f, w, r in t.tolist()}


def test_the_driver_sweeps_the_whole_range_and_agrees_with_the_restated_formulas(rules):
    want = [(nx, nu, N) for nx in range(1, 33) for nu in range(1, 33) if nx + nu <= 33 for N in range(2, 171)]
    assert sorted(rules) == sorted(want)
    for (nx, nu, N), (box, soc, tile) in rules.items():
        assert box == se.one_row_fits(nx, nu, N, False) and soc == se.one_row_fits(nx, nu, N, True), (nx, nu, N)
        assert tile == se.tile_shape(nx, nu, N), (nx, nu, N, tile)


def test_every_table_entry_is_what_the_table_says(rules):
    for e in se.EDGES:
        box, soc, tile = rules[e["shape"]]
        got = dict(fits=box, fits_soc=soc, tile=tile)
        for k, v in e["claims"].items():
            assert got[k] == v, (e["shape"], e["why"], k, got[k])
    for last, first, rule in se.PAIRS:
        assert last in se.SHAPES and first in se.SHAPES
        assert last[:2] == first[:2] and first[2] > last[2]
        at = {"box": 0, "soc": 1, "tile": 2}[rule]
        assert rules[last][at] and not rules[first][at], (last, first, rule)
        if rule != "tile":                            # the very next N: the one-row rule is monotone (below), so this IS the boundary
            assert first[2] == last[2] + 1
    # (6,3,27): the cone form is refused, the box form is not
    assert rules[(6, 3, 27)][:2] == (True, False)
    # the tile rule's boundaries in full: every N between the pair's two shapes that some R divides is refused for its length as well
    assert [N for N in range(33, 171) if rules[(12, 4, N)][2] == (1, 1)] == list(range(33, 41))
    assert [N for N in range(41, 171) if rules[(12, 4, N)][2] == (1, 2)] == list(range(42, 81, 2))
    assert [N for N in range(81, 171) if rules[(12, 4, N)][2] == (1, 4)] == list(range(84, 161, 4))
    assert [N for N in range(2, 171) if rules[(24, 8, N)][2] == (2, 1)] == list(range(2, 35))
    assert [N for N in range(35, 171) if rules[(24, 8, N)][2] == (2, 2)] == list(range(36, 69, 2))
    shape, lds = se.LDS_LIMIT_SHAPE
    assert se.tile_lds_bytes(shape[0] + shape[1], shape[2], rules[shape][2][1]) == lds == 60 * 1024


def test_the_one_row_rule_is_monotone_in_the_horizon_and_in_the_width(rules):
    for (nx, nu, N), (box, soc, _) in rules.items():
        assert box or not soc                         # a cone costs registers
        if N > 2:                                     # a shorter horizon of the same shape fits too
            assert rules[(nx, nu, N - 1)][0] >= box and rules[(nx, nu, N - 1)][1] >= soc, (nx, nu, N)
        if nx > 1:                                    # ... and so does a narrower shape of the same horizon, whichever field loses the row
            assert rules[(nx - 1, nu, N)][0] >= box and rules[(nx - 1, nu, N)][1] >= soc, (nx, nu, N)
        if nu > 1:
            assert rules[(nx, nu - 1, N)][0] >= box and rules[(nx, nu - 1, N)][1] >= soc, (nx, nu, N)
        if nx + nu > 16:
            assert not box
    # the rule reads nx + nu only
    for (nx, nu, N), (box, soc, _) in rules.items():
        if nx > 1 and nu < 32:
            assert (box, soc) == rules[(nx - 1, nu + 1, N)][:2], (nx, nu, N)


def test_every_tile_form_the_rule_returns_is_legal(rules):
    for (nx, nu, N), (_, _, tile) in rules.items():
        nz = nx + nu
        if tile is None:
            continue
        W, R = tile
        assert W in (1, 2) and R in (1, 2, 4) and W * R <= 4 and N % R == 0, (nx, nu, N, tile)
        assert (W == 2) == (nz > 16), (nx, nu, N, tile)

        def admissible(r):
            return W * r <= 4 and N % r == 0 and 2 * (5 * (N // r) + 2 * nz) + 44 <= 512 and se.tile_lds_bytes(nz, N, r) <= 60 * 1024
        assert admissible(R) and not any(admissible(r) for r in (1, 2, 4) if r < R), (nx, nu, N, tile)
    # ... and where it returns none, no (W, R) is admissible
    for (nx, nu, N), (_, _, tile) in rules.items():
        nz, W = nx + nu, (2 if nx + nu > 16 else 1)
        if tile is None and nz <= 32:
            assert not any(W * r <= 4 and N % r == 0 and 2 * (5 * (N // r) + 2 * nz) + 44 <= 512 and se.tile_lds_bytes(nz, N, r) <= 60 * 1024 for r in (1, 2, 4))


def test_every_shape_up_to_32_rows_has_a_kernel_and_33_rows_have_none(rules):
    """nx + nu <= 32: the one-row rule, the tile rule or the coverage kernel (tiny_batch_setup admits the shape; decide_path always
    answers).  nx + nu = 33: neither rule holds it, and tiny_batch_setup refuses a shape without a compiled-in entry beyond 32 rows"""
    wide = [s for s in rules if s[0] + s[1] == 33]
    assert len(wide) == 32 * 169 and not any(rules[s][0] or rules[s][1] or rules[s][2] for s in wide)
    src = open(os.path.join(CSRC, "batch_api.hip")).read()
    assert "if (!ke && nx + nu > 32)" in src and "return TINY_ERR_UNSUPPORTED;" in src.split("if (!ke && nx + nu > 32)")[1][:400]
    # every narrower shape: one answer per shape from the rules, and it names a kernel that holds the shape
    some = [s for s in rules if s[0] + s[1] <= 32 and (s[2] in (2, 3, 32, 33, 37, 38, 40, 41, 160, 164, 170) or s in se.SHAPES)]
    for s, r in expected_paths(some).items():
        box, _, tile = rules[s]
        listed = r["path"] in ("regs", "tile")
        if r["kernel"] == "ONE_ROW":
            assert box or listed, s
        elif r["kernel"] == "TILE":
            assert (tile is not None and (r["W"], r["R"]) == tile) or listed, s
        else:
            assert r["rule"] == "cover:no_register_form" and not box and tile is None, (s, r)


def test_the_kernel_each_table_entry_ends_on():
    """derived, not written down: the table's claims only say which rule holds a shape; here the host code says which kernel that makes.
    None of the entries is compiled in, so each runs a template instantiation made at run time -- or the coverage kernel"""
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    box = expected_paths(se.SHAPES)
    for e in se.EDGES:
        r, c = box[e["shape"]], e["claims"]
        want = "jit" if c.get("fits") else "tile-jit" if c.get("tile") else "cover"
        assert r["path"] == want, (e["shape"], r)
        if want == "tile-jit":
            assert (r["W"], r["R"]) == c["tile"]
    # under force_general every entry is the coverage kernel's
    assert {r["path"] for r in expected_paths(se.SHAPES, force_general=1).values()} == {"cover"}
    # the cone rows: the last N keeps the one-row kernel; the first N refused has no tile shape either (its box form is the one-row
    # kernel's, so tiny_batch_setup chose none): the coverage kernel
    cone = expected_paths(se.CONE_SHAPES, soc=True)
    assert [cone[s]["path"] for s in se.CONE_SHAPES] == ["jit", "cover"] and cone[(6, 3, 27)]["rule"] == "cover:no_register_form"
    # across each boundary the kernel changes
    for last, first, rule in se.PAIRS:
        answers = cone if rule == "soc" else box
        assert answers[last]["path"] != answers[first]["path"], (last, first)


@pytest.mark.parametrize("kind", ["cold", "warm"])
def test_the_oracle_alone_on_every_entry(kind):
    """what keeps the GPU comparison from being vacuous, from the ORACLE's results alone: all outputs finite; warm suite: each of the
    four bound arrays is attained exactly by an entry of vnew / znew (the knot-varying tables are read, entry by entry); cold suite:
    not every instance of the table runs into max_iter (the termination test decides)"""
    iters = []
    for shape in se.SHAPES:
        for cone in (False, True) if shape in se.CONE_SHAPES else (False,):
            suite, ref, again, ref2 = se.solved(shape, kind, cone)
            for out in (ref, ref2):
                for k, v in out.items():
                    assert np.all(np.isfinite(v)), (shape, kind, cone, k)
            iters.append(ref["iter"])
            if kind == "warm":
                cfg = suite["config"]
                for bound, field in (("x_min", "vnew"), ("x_max", "vnew"), ("u_min", "znew"), ("u_max", "znew")):
                    assert np.any(ref[field] == cfg[bound][None]), (shape, cone, bound)
                assert np.all(ref["iter"] == se.WARM_MAX_ITER) or np.any(ref["sol_solved"] == 1), shape
    iters = np.concatenate(iters)
    if kind == "cold":
        assert np.any(iters < se.COLD_MAX_ITER) and len(np.unique(iters)) > 3, np.unique(iters)
