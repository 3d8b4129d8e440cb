"""numpy reference of the cache precompute (csrc/riccati_kernel.hip.h, csrc/cache.hpp): tiny_precompute_and_set_cache as tiny_setup
runs it (reference src/tinympc/tiny_api.cpp:307-381), restated plainly with the number format as an argument -- np.longdouble (x86:
64-bit mantissa, eps 1.08e-19) is the reference, np.float64 the float64 replay whose distance from it says how well float64 can know
an instance's cache at all.  Neither is the code under test, and neither shares its operation order.

    Q1 = (Q + rho) + rho, R1 = (R + rho) + rho          rho enters twice (tiny_api.cpp:117-118, then :317-318)
    P = rho I, Kprev = 0
    up to 1000 times:  K  = inv(R1 + B' P B) B' P A      products left to right
                       Pn = Q1 + A' P (A - B K)
                       stop if max|K - Kprev| < 1e-5      BEFORE Kprev = K, P = Pn
    Quu_inv = inv(R1 + B' Pn B), AmBKt = (A - B K)', APf = (AmBKt Pn) f, BPf = (B' Pn) f

The inverse is the LU with partial pivoting of cache.hpp:invert written out, so that its row exchanges can be counted.
The instance sets of tests/test_gpu_riccati.py are generated here, each a pure function of its seed; tests/test_riccati_ref_cpu.py
asserts on the reference alone that they reach the code they are meant to reach."""
import numpy as np

MEMBERS = ("Kinf", "Pinf", "Quu_inv", "AmBKt", "APf", "BPf")
LD = np.longdouble
MAX_STEPS = 1000
STOP = 1e-5


def inverse(G):
    """LU with partial pivoting (first row of the largest magnitude below the diagonal, exchanged only if strictly larger), then one
    permuted unit vector per column through both triangles -> (inverse or None where a pivot is exactly 0, row exchanges)"""
    n = G.shape[0]
    lu = G.copy()
    perm = np.arange(n)
    swaps = 0
    for k in range(n):
        p = k + int(np.argmax(np.abs(lu[k:, k])))            # (argmax: the first of equals, as the strict > of the loop)
        if lu[p, k] == 0:
            return None, swaps
        if p != k:
            lu[[k, p], :] = lu[[p, k], :]
            perm[[k, p]] = perm[[p, k]]
            swaps += 1
        lu[k + 1:, k] = lu[k + 1:, k] / lu[k, k]
        lu[k + 1:, k + 1:] = lu[k + 1:, k + 1:] - np.outer(lu[k + 1:, k], lu[k, k + 1:])
    x = np.zeros((n, n), dtype=G.dtype)
    x[np.arange(n), perm] = 1                                # row i of the right-hand sides: 1 in column perm[i]
    for i in range(n):
        x[i, :] = x[i, :] - lu[i, :i] @ x[:i, :]
    for i in range(n - 1, -1, -1):
        x[i, :] = (x[i, :] - lu[i, i + 1:] @ x[i + 1:, :]) / lu[i, i]
    return x, swaps


def precompute(fam, dtype=LD):
    """fam: dict with A (nx,nx), B (nx,nu), f (nx,), Q (nx,), R (nu,) user diagonals, rho -> dict with the six cache members (in
    dtype), riccati_iters, swaps (row exchanges of all inversions, the final one included), swaps_first (of the first step's),
    deltas (max|K - Kprev| of every step), ok (False: an inversion was refused, the members are then missing)"""
    A, B = np.asarray(fam["A"], dtype=dtype), np.asarray(fam["B"], dtype=dtype)
    nx, nu = B.shape
    f = np.zeros(nx, dtype=dtype) if fam.get("f") is None else np.asarray(fam["f"], dtype=dtype)
    rho = dtype(fam["rho"])
    Q1 = np.diag((np.asarray(fam["Q"], dtype=dtype) + rho) + rho)
    R1 = np.diag((np.asarray(fam["R"], dtype=dtype) + rho) + rho)
    At, Bt = A.T.copy(), B.T.copy()
    P = rho * np.eye(nx, dtype=dtype)
    Kprev = np.zeros((nu, nx), dtype=dtype)
    out = dict(ok=False, riccati_iters=MAX_STEPS, swaps=0, swaps_first=0, deltas=[])
    with np.errstate(all="ignore"):
        for it in range(MAX_STEPS):
            Gi, s = inverse(R1 + (Bt @ P) @ B)
            out["swaps"] += s
            if it == 0:
                out["swaps_first"] = s
            if Gi is None:
                return out
            K = ((Gi @ Bt) @ P) @ A
            Pn = Q1 + (At @ P) @ (A - B @ K)
            out["deltas"].append(float(np.max(np.abs(K - Kprev))))
            if out["deltas"][-1] < STOP:
                out["riccati_iters"] = it + 1
                break                                         # before the copies: Pn is one step ahead of the P behind K
            Kprev, P = K, Pn
        Gi, s = inverse(R1 + (Bt @ Pn) @ B)
        out["swaps"] += s
        if Gi is None:
            return out
        AmBKt = (A - B @ K).T.copy()
        out.update(ok=True, Kinf=K, Pinf=Pn, Quu_inv=Gi, AmBKt=AmBKt, APf=((AmBKt @ Pn) @ f).reshape(nx, 1), BPf=((Bt @ Pn) @ f).reshape(nu, 1))
    return out


def rel_dev(a, b):
    """max|a - b| relative to the largest entry of b, in b's format"""
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a.astype(b.dtype) - b)) / max(np.max(np.abs(b)), b.dtype.type(1e-300)))


def tolerances(ref, f64):
    """per cache member max(32 d, 1e-14), d = the float64 replay's deviation from the longdouble reference on this instance (relative to
    the member's largest entry).  The 32 is for the summation order alone: numpy's products against sequential, uncontracted dot products."""
    return {k: max(32.0 * rel_dev(f64[k], ref[k]), 1e-14) for k in MEMBERS}


_BOTH = {}


def reference(fam):
    """(longdouble reference, float64 replay) of a family, computed once per process"""
    f = np.zeros(fam["B"].shape[0]) if fam.get("f") is None else fam["f"]
    key = (fam["B"].shape,) + tuple(np.asarray(fam[k], dtype=np.float64).tobytes() for k in ("A", "B", "Q", "R")) + (np.asarray(f, dtype=np.float64).tobytes(), float(fam["rho"]))
    if key not in _BOTH:
        _BOTH[key] = (precompute(fam, LD), precompute(fam, np.float64))
    return _BOTH[key]


def margin(deltas):
    """relative distance from 1e-5 of the deciding max|K - Kprev| and of the one before it (the smaller of the two)"""
    return min(abs(d - STOP) / STOP for d in deltas[-2:])


# ---- generators: every instance a pure function of its seed
def tame_family(nx, nu, N, seed):
    """tests/test_gpu_hetero.py:random_family (A a contraction, B ~ N(0,1)/sqrt(nx), R in 0.1..1, rho in 0.5..5) with every entry of f between 0.5 and 1.5 in magnitude"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((nx, nx))
    A = M * rng.uniform(0.7, 0.99) / np.max(np.abs(np.linalg.eigvals(M)))
    return dict(nx=nx, nu=nu, N=N, rho=float(rng.uniform(0.5, 5.0)), A=A, B=rng.standard_normal((nx, nu)) / np.sqrt(nx),
                f=rng.choice([-1.0, 1.0], nx) * rng.uniform(0.5, 1.5, nx), Q=rng.uniform(1, 10, nx), R=rng.uniform(0.1, 1, nu))


def strong_family(nx, nu, N, seed):
    """strong inputs under a light weight: B ~ 3 N(0,1), R in 0.01..0.1, rho in 0.05..0.2 -- R + B'PB is far from diagonally
    dominant and its inversion exchanges rows"""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((nx, nx))
    A = M * rng.uniform(0.7, 0.99) / np.max(np.abs(np.linalg.eigvals(M)))
    return dict(nx=nx, nu=nu, N=N, rho=float(rng.uniform(0.05, 0.2)), A=A, B=3.0 * rng.standard_normal((nx, nu)),
                f=rng.choice([-1.0, 1.0], nx) * rng.uniform(0.5, 1.5, nx), Q=rng.uniform(1, 10, nx), R=rng.uniform(0.01, 0.1, nu))


EDGE_SHAPES = ((1, 1), (15, 1), (1, 15), (2, 14), (31, 1), (16, 16), (8, 16), (1, 16))      # (a): B = 9 each, N = 4
PIVOT_SHAPES = ((16, 16), (8, 16), (4, 12), (4, 2))                                           # (b): B = 8 each, N = 4
SOLVED_SHAPES = ((2, 14), (16, 16), (31, 1))                                                  # (d): the (a) batches of these are solved
# Seeds drawn so that every instance meets the input conditions tests/test_riccati_ref_cpu.py asserts (a step count float64 and longdouble
# agree on, decided at least 1 % away from 1e-5; the pivot sets: row exchanges) -- the share of instances left out of a set is zero.
EDGE_SEEDS = {(1, 1): tuple(range(100, 109)), (15, 1): (200, 201, 202, 203, 204, 205, 206, 207, 209), (1, 15): tuple(range(300, 309)),
              (2, 14): tuple(range(400, 409)), (31, 1): (500, 501, 503, 504, 505, 506, 507, 509, 510), (16, 16): tuple(range(600, 609)),
              (8, 16): tuple(range(700, 709)), (1, 16): tuple(range(800, 809))}
PIVOT_SEEDS = {(16, 16): (1601, 1602, 1607, 1609, 1611, 1612, 1613, 1617), (8, 16): tuple(range(1700, 1708)),
               (4, 12): tuple(range(1800, 1808)), (4, 2): (1905, 1908, 1911, 1917, 1942, 1950, 1953, 1954)}


def edge_set(nx, nu):
    return [tame_family(nx, nu, 4, seed) for seed in EDGE_SEEDS[(nx, nu)]]


def pivot_set(nx, nu):
    return [strong_family(nx, nu, 4, seed) for seed in PIVOT_SEEDS[(nx, nu)]]


def zero_a_family(nx, nu, N, seed):
    """A = 0: the first Kinf is exactly 0 and the recursion leaves at its first step, before any copy"""
    fam = tame_family(nx, nu, N, seed)
    fam["A"] = np.zeros((nx, nx))
    return fam


def cap_family(nx, nu, N, seed):
    """A = [[1, 0.1], [0, 0.9]], B = [[0], [1e-3]], Q = R = 1, rho = 1: a barely actuated integrator whose gain still moves by more than
    1e-5 per step after 1000 steps (every value finite, max|Pinf| 2303).  Larger shapes: that system as the first block of a block-
    diagonal one, the rest a contraction with its own inputs -- the blocks do not mix, the first one keeps the recursion running."""
    rng = np.random.default_rng(seed)
    A, B = np.zeros((nx, nx)), np.zeros((nx, nu))
    A[:2, :2] = [[1.0, 0.1], [0.0, 0.9]]
    B[1, 0] = 1e-3
    if nx > 2:
        M = rng.standard_normal((nx - 2, nx - 2))
        A[2:, 2:] = M * rng.uniform(0.7, 0.99) / np.max(np.abs(np.linalg.eigvals(M)))
        B[2:, 1:] = rng.standard_normal((nx - 2, nu - 1)) / np.sqrt(nx - 2)
    return dict(nx=nx, nu=nu, N=N, rho=1.0, A=A, B=B, f=rng.normal(0, 0.01, nx), Q=np.ones(nx), R=np.ones(nu))


STEP_SHAPES = ((2, 1, 4), (6, 3, 10))                     # (c): B = 7, the A = 0 instance at 2, the cap instance at 4
STEP_SEED = {(2, 1, 4): 2100, (6, 3, 10): 2230}
ZERO_AT, CAP_AT = 2, 4


def step_set(nx, nu, N, edges=True):
    """seven ordinary instances (f small, as random_family: these batches are solved); edges: two of them replaced"""
    seed = STEP_SEED[(nx, nu, N)]
    fams = [tame_family(nx, nu, N, seed + i) for i in range(7)]
    for fam in fams:
        fam["f"] = 0.01 * fam["f"]
    if edges:
        fams[ZERO_AT] = zero_a_family(nx, nu, N, seed + 50)
        fams[ZERO_AT]["f"] = 0.01 * fams[ZERO_AT]["f"]
        fams[CAP_AT] = cap_family(nx, nu, N, seed + 51)
    return fams


def singular_family(fam, col=0):
    """a copy with column col of B zero, rho = 1 and R[col] = -2: (R + rho) + rho is exactly 0.0 there and stays the whole pivot column"""
    bad = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in fam.items()}
    bad["B"][:, col] = 0.0
    bad["rho"] = 1.0
    bad["R"][col] = -2.0
    return bad


REFUSAL_SHAPE, REFUSAL_SEED, BAD_AT = (6, 3, 10), 2300, 3


def refusal_set():
    return [tame_family(*REFUSAL_SHAPE, REFUSAL_SEED + i) for i in range(7)]


# ---- the solves of (c) and (d): data and the oracle's own sensitivity
BOX = dict(x_min=-2.0, x_max=2.0, u_min=-0.4, u_max=0.4)
MAX_ITER = 150


def solve_data(fams, seed=5):
    """x0, Xref, Uref of a batch, as tests/test_gpu_hetero.py draws them"""
    nx, nu, N, B = fams[0]["nx"], fams[0]["nu"], fams[0]["N"], len(fams)
    rng = np.random.default_rng(seed)
    x0 = rng.uniform(-1, 1, (B, nx))
    Xref = np.repeat(rng.uniform(-0.3, 0.3, (B, nx, 1)), N, axis=2) + rng.normal(0, 0.02, (B, nx, N))
    Uref = rng.normal(0, 0.05, (B, nu, N - 1))
    return x0, Xref, Uref


FIELDS = ("x", "u", "vnew", "znew", "g", "y", "v", "z")
WARM_FIELDS = ("x", "u", "g")


def oracle_solves(fam, x0, Xref, Uref, scale=1.0):
    """the instance's own oracle: a cold box-constrained solve from x0, then a warm one from 0.9 x0; scale multiplies A and B
    -> [cold, warm], each a dict of the fields, iter and solved"""
    import scenarios as sc
    from cpu_solvers import OracleSolver
    nx, nu = fam["nx"], fam["nu"]
    fam = dict(fam, A=fam["A"] * scale, B=fam["B"] * scale)
    cfg = sc.default_config(fam, max_iter=MAX_ITER, x_min=np.full((nx, 1), BOX["x_min"]), x_max=np.full((nx, 1), BOX["x_max"]),
                            u_min=np.full((nu, 1), BOX["u_min"]), u_max=np.full((nu, 1), BOX["u_max"]))
    o = sc.make_solver(OracleSolver, fam, cfg)
    o["Xref"], o["Uref"] = Xref, Uref
    out = []
    for start, fields in ((x0, FIELDS), (0.9 * x0, WARM_FIELDS)):
        o["x"][:, 0] = start
        o.solve()
        rec = {k: o[k].copy() for k in fields}
        rec.update(iter=int(o.get("sol_iter")), solved=int(o.get("sol_solved")))
        out.append(rec)
    o.close()
    return out


def oracle_amplification(fam, x0, Xref, Uref):
    """the oracle's own amplification of a 1 + 1e-15 scaling of A and B (as tools/fuzz_parity.py:hetero_adaptive_floor measures one of
    the tables): the worst relative field difference of the two runs, inf where their counts differ or a field is not finite"""
    a, b = oracle_solves(fam, x0, Xref, Uref), oracle_solves(fam, x0, Xref, Uref, 1.0 + 1e-15)
    worst = 0.0
    for ra, rb in zip(a, b):
        if (ra["iter"], ra["solved"]) != (rb["iter"], rb["solved"]):
            return float("inf")
        for k in ra:
            if k not in ("iter", "solved"):
                if not np.all(np.isfinite(ra[k])):
                    return float("inf")
                worst = max(worst, float(np.max(np.abs(rb[k] - ra[k])) / max(np.max(np.abs(ra[k])), 1e-300)))
    return worst
