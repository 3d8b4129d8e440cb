"""The shapes at the edges of what each kernel claims to hold (host only; imported by tests/test_shape_edges_cpu.py and
tests/test_gpu_shape_edges.py).  Two formulas of csrc/jit.hpp send a shape (nx, nu, N) to the one-row kernel (jit_shape_fits), to
the tile kernel (jit_tile_shape) or, where neither holds it, to the coverage kernel; a shape outside kernel_dims.txt / tile_dims.txt is
instantiated at run time from templates nobody instantiated at those values before.  EDGES lists the shapes that sit on a limit of
either formula or on a lane boundary of the 16-lane DPP rows, each with the reason it is an edge and with what the formulas -- restated
below -- say about it.  The kernel a shape runs on is NOT written down here: tests/test_shape_edges_cpu.py derives it from the
project's own host code (tests/dropin/shape_rules_driver.cpp) and exports it to the GPU test.

Two suites per shape, both on the problems of oracle/scenarios.py (random_problem):
  cold: sweep_suite(nx, nu, N, B=9, max_iter=120) -- zero workspace, a shared knot-invariant input box
  warm: every input array random, a non-zero f, 25 iterations, knot-varying boxes on both fields: no symmetric or replicated
        structure anywhere, so a transposed or shifted table entry cannot pass (as random_state_suite)
B = 9 is ragged on every form: four instances per wave on the one-row kernel, one to four per wave on the tile kernel."""
import functools

import numpy as np

import scenarios as sc
from cpu_solvers import OracleSolver

B = 9
COLD_MAX_ITER = 120
WARM_MAX_ITER = 25
# (the draw under which every shape -- those with two or three state entries included -- has an entry on each of its four bound arrays:
# tests/test_shape_edges_cpu.py asserts it from the oracle alone)
WARM_SEED = 3
INPUT_CONE = ([0], [3], [0.6])                    # rows 0..2 of the input (the reference's project_soc handles dimension 3 only)


# ---- the formulas of csrc/jit.hpp, restated
def one_row_fits(nx, nu, N, soc=False):
    """jit_shape_fits: one instance per 16-lane row, the N-long arrays of a lane within 512 registers"""
    return nx >= 1 and nu >= 1 and nx + nu <= 16 and N >= 2 and 2 * ((8 if soc else 6) * N + 2 * (nx + nu) + 8) + 40 <= 512


def tile_lds_bytes(nz, N, R):
    """the per-wave bound and trajectory tables of jit_tile_shape"""
    W = 2 if nz > 16 else 1
    return 2 * N * 16 * W * 8 + (N // R) * 64 * 8


def tile_shape(nx, nu, N):
    """jit_tile_shape: (W, R) or None -- W rows across the knot vector, the smallest R in {1, 2, 4} with W * R <= 4 and N % R == 0
    whose N / R-long arrays fit 512 registers and whose tables fit 60 KiB of LDS"""
    nz = nx + nu
    if nx < 1 or nu < 1 or nz > 32 or N < 2:
        return None
    W = 2 if nz > 16 else 1
    for R in (1, 2, 4):
        if W * R > 4 or N % R:
            continue
        if 2 * (5 * (N // R) + 2 * nz) + 44 <= 512 and tile_lds_bytes(nz, N, R) <= 60 * 1024:
            return (W, R)
    return None


# ---- the table.  Each entry: shape, why it is an edge, and what the formulas above say of it -- `fits` (box form of the one-row
# rule), `fits_soc` (cone form), `tile` ((W, R) or None); a key that is absent is not claimed
def edge(shape, why, **claims):
    return dict(shape=shape, why=why, claims=claims)


EDGES = [
    edge((1, 1, 2), "smallest of everything", fits=True),
    edge((15, 1, 2), "nz = 16, one input in lane 15, N = 2", fits=True),
    edge((1, 15, 2), "nz = 16, one state in lane 0, N = 2", fits=True),
    edge((7, 1, 5), "nz = 8: the half-row limit", fits=True),
    edge((1, 7, 5), "nz = 8: the half-row limit, inputs from lane 1", fits=True),
    edge((8, 1, 5), "nz = 9: the first shape past the half-row limit", fits=True),
    edge((12, 4, 13), "just past two waves per SIMD (solve_kernel_waves_per_simd: one wave from N = 12 at nz = 16)", fits=True),
    edge((15, 1, 32), "last N of the one-row rule at nz = 16", fits=True),
    edge((15, 1, 33), "first N the one-row rule refuses at nz = 16", fits=False, tile=(1, 1)),
    edge((1, 1, 37), "last N of the one-row rule at nz = 2", fits=True),
    edge((1, 1, 38), "first N the one-row rule refuses at nz = 2", fits=False, tile=(1, 1)),
    edge((6, 3, 26), "last N of the one-row rule with a cone on", fits=True, fits_soc=True),
    edge((6, 3, 27), "first N the one-row rule refuses with a cone on; its box form still fits", fits=True, fits_soc=False),
    edge((16, 1, 2), "nz = 17: one lane in the second DPP row", fits=False, tile=(2, 1)),
    edge((1, 16, 3), "nz = 17: one lane in the second DPP row, an input", fits=False, tile=(2, 1)),
    edge((16, 16, 2), "each field fills a row exactly", fits=False, tile=(2, 1)),
    edge((17, 15, 7), "the state field straddles the two rows", fits=False, tile=(2, 1)),
    edge((4, 20, 10), "an input field wider than a row", fits=False, tile=(2, 1)),
    edge((31, 1, 2), "nz = 32, one input in the last lane", fits=False, tile=(2, 1)),
    edge((1, 31, 3), "nz = 32, inputs over both rows", fits=False, tile=(2, 1)),
    edge((12, 4, 33), "first N of the tile kernel at nz = 16", fits=False, tile=(1, 1)),
    edge((12, 4, 40), "last N with R = 1", fits=False, tile=(1, 1)),
    edge((12, 4, 41), "odd N past R = 1: no R serves it", fits=False, tile=None),
    edge((12, 4, 42), "R = 2", fits=False, tile=(1, 2)),
    edge((12, 4, 82), "N / 2 too long, N % 4 != 0: no R", fits=False, tile=None),
    edge((12, 4, 160), "R = 4, exactly at the LDS limit", fits=False, tile=(1, 4)),
    edge((12, 4, 164), "first N past R = 4", fits=False, tile=None),
    edge((24, 8, 34), "W = 2: last N with R = 1", fits=False, tile=(2, 1)),
    edge((24, 8, 35), "W = 2: odd N past R = 1", fits=False, tile=None),
    edge((24, 8, 36), "W = 2: R = 2", fits=False, tile=(2, 2)),
    edge((24, 8, 68), "W = 2: last N with R = 2", fits=False, tile=(2, 2)),
    edge((24, 8, 70), "W = 2: first N past R = 2", fits=False, tile=None),
]
SHAPES = [e["shape"] for e in EDGES]

# (last shape a rule admits, first it refuses, the rule): "box" / "soc" the one-row rule without / with a cone, "tile" the tile rule
PAIRS = [
    ((15, 1, 32), (15, 1, 33), "box"), ((1, 1, 37), (1, 1, 38), "box"), ((6, 3, 26), (6, 3, 27), "soc"),
    ((12, 4, 40), (12, 4, 41), "tile"), ((12, 4, 160), (12, 4, 164), "tile"), ((24, 8, 34), (24, 8, 35), "tile"), ((24, 8, 68), (24, 8, 70), "tile"),
]
LDS_LIMIT_SHAPE = ((12, 4, 160), 61440)           # (shape, bytes): sits on the 60 KiB limit to the byte
# the shapes whose cone form is an edge of its own: solved with INPUT_CONE on as well (tests/test_gpu_shape_edges.py, variants)
CONE_SHAPES = [(6, 3, 26), (6, 3, 27)]
# closed loop: N = 2 (the knot the plant step reads, X[1], is the terminal knot and N - 1 = 1) at the width edges
CLOSED_LOOP_SHAPES = [(1, 1, 2), (15, 1, 2), (1, 15, 2), (16, 16, 2), (31, 1, 2)]


def shape_id(shape):
    return "_".join(map(str, shape))


# ---- the suites
def cold_suite(shape, cone=False):
    suite = sc.sweep_suite(*shape, B=B, max_iter=COLD_MAX_ITER)
    if cone:
        suite["config"].update(en_input_soc=1, input_cone=INPUT_CONE)
    return suite


def warm_boxes(rng, nx, nu, N):
    return dict(x_min=rng.uniform(-1.0, -0.1, (nx, N)), x_max=rng.uniform(0.1, 1.0, (nx, N)),
                u_min=rng.uniform(-0.5, -0.05, (nu, N - 1)), u_max=rng.uniform(0.05, 0.5, (nu, N - 1)))


def warm_suite(shape, cone=False, **config):
    nx, nu, N = shape
    prob, _ = sc.random_problem(nx, nu, N)
    rng = np.random.default_rng(WARM_SEED + 1000 * nx + 10 * nu + N)
    prob = dict(prob, f=rng.normal(0.0, 0.05, nx))
    kw = dict(max_iter=WARM_MAX_ITER, **warm_boxes(rng, nx, nu, N))
    if cone:
        kw.update(en_input_soc=1, input_cone=INPUT_CONE)
    kw.update(config)
    cfg = sc.default_config(prob, **kw)
    cases = sc.zero_cases(prob, B)
    for k, v in cases.items():
        cases[k] = rng.normal(0.0, 0.4, v.shape)
    return dict(problem=prob, config=cfg, cases=cases)


SUITES = {"cold": cold_suite, "warm": warm_suite}
WARM_STATE = ("x", "u", "vnew", "znew", "g", "y", "v", "z")
EXTRA_STATE = ("gc", "yc", "gl", "yl", "gl_tv", "yl_tv")


def second_suite(suite, ref):
    """the second solve: from the state the first one left (the oracle's), with x0 * 0.8"""
    warm = dict(problem=suite["problem"], config=suite["config"], cases=dict(suite["cases"]))
    for k in WARM_STATE + tuple(k for k in EXTRA_STATE if k in ref and k in suite["cases"]):
        warm["cases"][k] = ref[k]
    warm["cases"]["x0"] = suite["cases"]["x0"] * 0.8
    return warm


@functools.lru_cache(maxsize=None)
def solved(shape, kind, cone=False):
    """(suite, the oracle's outputs, the second suite, the oracle's outputs of it): computed once per shape and shared; nobody writes to them"""
    suite = SUITES[kind](shape, cone)
    ref = sc.run_cases(OracleSolver, suite)
    again = second_suite(suite, ref)
    return suite, ref, again, sc.run_cases(OracleSolver, again)
