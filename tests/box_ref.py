"""TEST INFRASTRUCTURE -- the box step of update_slack + update_dual (src/tinympc/admm.cpp:85-98, 222-225) restated in numpy exactly as
oracle/tinympc_oracle.c:356 forms it, and seeded batches on which a restatement of it can go wrong without any golden noticing.

One entry meets one bound pair: t = fl(x + g), vnew = clamp(lo, hi, t), g' = fl(t - vnew) -- one rounded add, one max, one min, one rounded
subtract, so every implementation that is right is right bit for bit.  Two clamp rules: "ternary" is the oracle's (and Eigen's)
(lo < t) ? t : lo, then (m < hi) ? m : hi; "minmaxnum" is IEEE minNum(hi, maxNum(lo, t)), what v_max_f64 / v_min_f64 and fmax / fmin
compute.  They differ only where a bound is NaN and in the sign of a zero when a zero bound meets a zero t: the two VALUE_COMPARED
classes.

The box belongs to a batch handle (tiny_batch_set_bound_constraints has no instance axis), so one launch has ONE box; what varies over
the instances of a launch is the warm dual.  A batch of several boxes is a list of ROUNDS, one launch each.

step(cfg, x, u, g, y, rule)        -> {vnew, znew, g, y} of one update_slack + update_dual
first_iteration(suite, x, u, rule) -> the same plus v, z, the four residuals of the first termination test and solved
position_batch / class_rounds / identity_suite / enable_suites / pure_map_suite: see each
"""
import copy
import functools

import numpy as np

import scenarios as sc
from halfspace_ref import family
from soc_ref import same_bits  # noqa: F401  (re-exported: elementwise the same 64 bits, or both NaN)
from termination_ref import RESIDUALS

FIELDS = ("vnew", "znew", "g", "y", "v", "z")
# every shape tests/test_gpu_box_edges.py launches: tests/test_box_ref_cpu.py asserts the builders' preconditions on the oracle for each
GPU_DIMS = ((12, 4, 10), (4, 2, 10), (4, 2, 30), (20, 4, 10), (4, 2, 50), (12, 8, 30), (12, 4, 50), (5, 3, 7), (8, 8, 10), (4, 1, 10), (2, 2, 3), (6, 3, 10),
            (20, 8, 10), (3, 2, 2))
INF, NAN = np.inf, np.nan


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def clamp(lo, hi, t, rule="minmaxnum"):
    with np.errstate(all="ignore"):
        if rule == "ternary":                       # x_max.cwiseMin(x_min.cwiseMax(t)) as oracle/tinympc_oracle.c:363-364 spells it
            m = np.where(lo < t, t, lo)
            return np.where(m < hi, m, hi)
        if rule == "minmaxnum":
            return np.fmin(hi, np.fmax(lo, t))
    raise KeyError(rule)


def step(cfg, x, u, g, y, rule="minmaxnum"):
    """x, g (B, nx, N) | (nx, N); u, y likewise with (nu, N - 1): -> vnew, znew and the duals after update_dual.  A disabled family
    passes t = fl(x + g) through; its dual becomes t - t"""
    out = {}
    with np.errstate(all="ignore"):
        for src, dual, sname, dname, lo, hi, flag in ((x, g, "vnew", "g", "x_min", "x_max", "en_state_bound"), (u, y, "znew", "y", "u_min", "u_max", "en_input_bound")):
            t = np.asarray(src, dtype=np.float64) + np.asarray(dual, dtype=np.float64)                    # :85 / :88, and g + x of :222
            s = clamp(np.asarray(cfg[lo], dtype=np.float64), np.asarray(cfg[hi], dtype=np.float64), t, rule) if cfg[flag] else t
            out[sname], out[dname] = s, t - s
    return out


def _absmax(a):
    """the oracle's `if (a > m) m = a` from 0.0 over one instance's entries: a NaN term is passed over"""
    return np.fmax.reduce(np.abs(a).reshape(a.shape[0], -1), axis=1, initial=0.0)


def residuals(rho, x, u, v, z, vnew, znew):
    """the four scalars of termination_condition (oracle/tinympc_oracle.c:487-499), in its operation order: the dual ones are
    fl(rho max|v - vnew|) -- the maximum first"""
    with np.errstate(all="ignore"):
        return {"primal_residual_state": _absmax(x - vnew), "dual_residual_state": _absmax(v - vnew) * np.float64(rho),
                "primal_residual_input": _absmax(u - znew), "dual_residual_input": _absmax(z - znew) * np.float64(rho)}


def first_iteration(suite, x, u, rule="minmaxnum"):
    """what a solve with max_iter = 1 leaves behind, from ITS x, u and the warm g, y, v, z of the suite: the step, the residuals of the
    one termination test, solved, and v | z (the slack where the solve stays open, admm.cpp:445; untouched where it stops)"""
    cfg, cases, rho = suite["config"], suite["cases"], suite["problem"]["rho"]
    out = step(cfg, x, u, cases["g"], cases["y"], rule)
    out.update(residuals(rho, x, u, cases["v"], cases["z"], out["vnew"], out["znew"]))
    with np.errstate(all="ignore"):
        solved = (out["primal_residual_state"] < cfg["abs_pri_tol"]) & (out["primal_residual_input"] < cfg["abs_pri_tol"]) & \
                 (out["dual_residual_state"] < cfg["abs_dua_tol"]) & (out["dual_residual_input"] < cfg["abs_dua_tol"])
    out["solved"] = solved.astype(int)
    out["v"] = np.where(solved[:, None, None], cases["v"], out["vnew"])
    out["z"] = np.where(solved[:, None, None], cases["z"], out["znew"])
    return out


def box_uniform(cfg, N):
    """box_is_uniform (csrc/batch_tables.hip) restated: only ENABLED families count, a box never set is uniform, a NaN equals nothing"""
    if N < 2:
        return False
    if not cfg.get("bounds_set", True):
        return True
    same = lambda a: bool(np.all(np.asarray(a) == np.asarray(a)[:, :1]))        # noqa: E731
    return (not cfg["en_state_bound"] or (same(cfg["x_min"]) and same(cfg["x_max"]))) and \
           (not cfg["en_input_bound"] or (same(cfg["u_min"]) and same(cfg["u_max"])))


def margin_to_tolerance(cfg, res):
    """min over the four residuals of |r / tol - 1|: how far the nearest one is from flipping its test (inf: tolerance 0)"""
    with np.errstate(all="ignore"):
        m = [np.abs(res[k] / (cfg["abs_pri_tol"] if k.startswith("primal") else cfg["abs_dua_tol"]) - 1.0) for k in RESIDUALS]
    return float(np.nanmin(np.stack(m)))


# ---- classes of a directed entry: (lo, hi, t) ---------------------------------------------------------------------------------------
CLASSES = ("inside", "below", "above", "on_lo", "on_hi", "ulp_inside_lo", "ulp_outside_lo", "ulp_inside_hi", "ulp_outside_hi", "equal_bounds",
           "crossed", "inf_lo", "inf_hi", "inf_both", "huge", "subnormal", "zero_tie", "nan_bound", "nan_t", "inf_t")
VALUE_COMPARED = ("zero_tie", "nan_bound")
PHASE_ONLY = ("nan_t", "inf_t")
# the bound pair of an entry comes from one of these KINDS; the instances of a round walk the kind's t variants.  14 kinds: zero_tie (2
# of the 6 variants of "zero") and nan_bound (all of "nan") together are (1/3 + 1) / 14 = 9.5 % of the entries
KINDS = ("normal", "positive", "negative", "tight", "equal", "crossed", "inf_lo", "inf_hi", "inf_both", "huge", "subnormal", "zero", "wide", "nan")
UNIFORM_KINDS = KINDS[:-1]            # a NaN bound is never uniform (box_is_uniform): 13 kinds
PHASE_KINDS = ("bad_t", "bad_t_inf_lo", "bad_t_inf_hi")
B_ROUND = 12                          # instances per round: more than the 9 variants of the longest kind
TINY = 5e-324


def _up(v):
    return float(np.nextafter(v, INF))


def _dn(v):
    return float(np.nextafter(v, -INF))


def kind_bounds(kind, rng, par):
    """(lo, hi) of one entry; par: a small integer that picks among the kind's sub-forms"""
    a, c = (float(v) for v in rng.uniform(0.5, 2.0, 2))
    if kind in ("normal", "bad_t"):
        return -a, c
    if kind == "wide":
        return -8.0 * a, 8.0 * c
    if kind == "positive":
        return a, a + c
    if kind == "negative":
        return -a - c, -a
    if kind == "tight":
        lo = a if par % 2 else -a
        return lo, _up(_up(_up(lo)))
    if kind == "equal":
        return (a, a) if par % 2 else (-c, -c)
    if kind == "crossed":
        return (c, -a) if par % 2 else (a + c, a)
    if kind in ("inf_lo", "bad_t_inf_lo"):
        return -INF, c if par % 2 else -c
    if kind in ("inf_hi", "bad_t_inf_hi"):
        return (-a if par % 2 else a), INF
    if kind == "inf_both":
        return -INF, INF
    if kind == "huge":
        return -1e17, 1e17
    if kind == "subnormal":
        return -3e-310 * (1 + par % 3), 5e-310
    if kind == "zero":
        return ((0.0, c), (-0.0, c), (-a, 0.0), (-a, -0.0))[par % 4]
    if kind == "nan":
        return ((NAN, c), (-a, NAN), (NAN, NAN))[par % 3]
    raise KeyError(kind)


def kind_variants(kind, lo, hi):
    """[(class, t)] of an entry whose bounds are (lo, hi)"""
    if kind in ("normal", "positive", "negative", "wide"):
        return [("inside", lo + (hi - lo) * 0.37), ("below", lo - 0.7), ("above", hi + 1.3), ("on_lo", lo), ("on_hi", hi), ("ulp_inside_lo", _up(lo)),
                ("ulp_outside_lo", _dn(lo)), ("ulp_inside_hi", _dn(hi)), ("ulp_outside_hi", _up(hi))]
    if kind == "tight":
        return [("ulp_inside_lo", _up(lo)), ("ulp_inside_hi", _dn(hi)), ("on_lo", lo), ("on_hi", hi), ("ulp_outside_lo", _dn(lo)), ("ulp_outside_hi", _up(hi))]
    if kind == "equal":
        return [("equal_bounds", t) for t in (_dn(lo), lo, _up(lo), lo - 1.0, lo + 1.0)]
    if kind == "crossed":
        return [("crossed", t) for t in (hi - 0.5, 0.5 * (lo + hi), lo + 0.5, lo, hi)]
    if kind == "inf_lo":
        return [("inf_lo", t) for t in (-1e300, hi - 0.5, hi + 0.5, hi, _up(hi))]
    if kind == "inf_hi":
        return [("inf_hi", t) for t in (1e300, lo + 0.5, lo - 0.5, lo, _dn(lo))]
    if kind == "inf_both":
        return [("inf_both", t) for t in (1e300, -1e300, 0.75)]
    if kind == "huge":
        return [("huge", t) for t in (1.7e308, -1.7e308, 2.5, -1e17, _up(1e17))]
    if kind == "subnormal":
        return [("subnormal", t) for t in (_dn(lo), 1e-310, 9e-310, lo, hi, _up(hi), -TINY)]
    if kind == "zero":
        if lo == 0.0:
            return [("zero_tie", 0.0), ("zero_tie", -0.0), ("inside", 0.5 * hi), ("below", -0.75), ("ulp_inside_lo", TINY), ("ulp_outside_lo", -TINY)]
        return [("zero_tie", 0.0), ("zero_tie", -0.0), ("inside", 0.5 * lo), ("above", 0.75), ("ulp_inside_hi", -TINY), ("ulp_outside_hi", TINY)]
    if kind == "nan":
        c = hi if hi == hi else (lo if lo == lo else 0.5)
        return [("nan_bound", t) for t in (c - 0.5, c + 0.5, c)]
    if kind in PHASE_KINDS:
        return [("nan_t", NAN), ("inf_t", INF), ("inf_t", -INF)]
    raise KeyError(kind)


def zero_tie_pattern(lo, hi, t):
    """'lo=-0 t=+0' and the like, for the printed table of what the hardware returns"""
    z = lambda v: "-0" if np.signbit(v) else "+0"           # noqa: E731
    return ("lo=%s t=%s" % (z(lo), z(t))) if lo == 0.0 else ("hi=%s t=%s" % (z(hi), z(t)))


def class_counts(labels, only=None):
    lab = np.concatenate([np.asarray(l).ravel() for l in (labels.values() if isinstance(labels, dict) else [labels])])
    return {CLASSES[k]: int(n) for k, n in enumerate(np.bincount(lab, minlength=len(CLASSES))) if n and (only is None or CLASSES[k] in only)}


# ---- the zero-trajectory construction -------------------------------------------------------------------------------------------------
def zero_problem(nx, nu, N):
    """a sweep cell's dynamics (f = 0).  With x0 = 0, references 0 and warm vnew = g, znew = y the first update_linear_cost forms
    vnew - g = 0 exactly, so q, r, p, d, x, u are zeros on ANY implementation and t = fl(x + g) = g wherever g is not a zero -- the
    argument termination_ref.strict_suite rests on"""
    prob, _ = sc.random_problem(nx, nu, N)
    assert not np.any(prob["f"])
    return prob


def zero_suite(prob, bounds, g, y, **cfg):
    """bounds: (x_min, x_max, u_min, u_max); warm vnew = g, znew = y, v = z = 0; max_iter = 1 and the default tolerances unless given"""
    B = g.shape[0]
    cases = sc.zero_cases(prob, B)
    cases["g"], cases["y"], cases["vnew"], cases["znew"] = g.copy(), y.copy(), g.copy(), y.copy()
    kw = dict(max_iter=1, x_min=bounds[0], x_max=bounds[1], u_min=bounds[2], u_max=bounds[3])
    kw.update(cfg)
    return dict(problem=prob, config=sc.default_config(prob, **kw), cases=cases)


def _split(rec, nx):
    """a stacked record (..., nx + nu, N) -> state (..., nx, N), input (..., nu, N - 1)"""
    return rec[..., :nx, :].copy(), rec[..., nx:, :-1].copy()


def positions(nx, nu, N):
    return [(j, k) for j in range(nx) for k in range(N)] + [(nx + j, k) for j in range(nu) for k in range(N - 1)]


CONTROLS = 5                          # quiet instances at the end of a position batch (every row position of a wave of 4)


def classify(lo, hi, t):
    """the class of t against an ordinary pair lo < hi, elementwise -> indices into CLASSES"""
    c = np.where(t < lo, CLASSES.index("below"), np.where(t > hi, CLASSES.index("above"), CLASSES.index("inside")))
    for name, v in (("ulp_inside_lo", np.nextafter(lo, INF)), ("ulp_outside_lo", np.nextafter(lo, -INF)), ("ulp_inside_hi", np.nextafter(hi, -INF)),
                    ("ulp_outside_hi", np.nextafter(hi, INF)), ("on_lo", lo), ("on_hi", hi)):
        c = np.where(t == v, CLASSES.index(name), c)
    return c.astype(np.int8)


@functools.lru_cache(maxsize=None)
def _position_batch(nx, nu, N, uniform):
    prob = zero_problem(nx, nu, N)
    nz, pos = nx + nu, positions(nx, nu, N)
    B = len(pos) + CONTROLS
    rng = np.random.default_rng([nx, nu, N, int(uniform), 20261019])
    j_, k_ = np.meshgrid(np.arange(nz), np.arange(N), indexing="ij")
    g = np.zeros((B, nz, N))
    labels = np.full((B, nz, N), -1, dtype=np.int8)
    if not uniform:
        # EVERY entry has a bound pair of its own (multiples of 2^-12: exact), and every entry of every instance lies outside its own
        # pair -- alternately below and above, by 1/4 (1/2 at the instance's own (j, k)) -- so its slack is its own bound, a value no
        # other entry of the table holds, and its dual +-1/4: a clamp that reads ANY other entry of the table differs in the bits
        idx = (j_ * N + k_).astype(np.float64)
        lo, hi = -(1.0 + idx / 4096.0), 1.0 + (idx + 0.5) / 4096.0
        for b, (j, k) in enumerate(pos):
            push = np.full((nz, N), 0.25)
            push[j, k] = 0.5
            low = (j_ + k_ + b) % 2 == 0
            g[b] = np.where(low, lo - push, hi + push)
            labels[b] = np.where(low, CLASSES.index("below"), CLASSES.index("above"))
    else:
        # one pair per row; instance (j, k) has a directed class at (j, k) and values on either side of the bounds everywhere else
        row = np.arange(nz, dtype=np.float64)[:, None]
        lo, hi = np.broadcast_to(-(1.0 + row / 64.0), (nz, N)).copy(), np.broadcast_to(1.0 + (row + 0.5) / 64.0, (nz, N)).copy()
        g[:] = rng.uniform(-2.5, 2.5, (B, nz, N))
        labels[:] = classify(lo, hi, g)
        for b, (j, k) in enumerate(pos):
            v = kind_variants("normal", lo[j, k], hi[j, k])
            cls, t = v[b % len(v)]
            g[b, j, k], labels[b, j, k] = t, CLASSES.index(cls)
    # the controls: every entry inside its pair and below 2^-12, so all four residuals are below the default tolerances and the
    # solve STOPS (v | z stay as they were) -- unless a lane that holds no entry (a pad lane, the input lanes' dummy slot) is clamped
    # by a bound that excludes 0 and reaches a residual
    g[len(pos):] = rng.choice([-1.0, 1.0], (CONTROLS, nz, N)) * rng.uniform(2.0 ** -14, 2.0 ** -12, (CONTROLS, nz, N))
    labels[len(pos):] = CLASSES.index("inside")
    gx, gy = _split(g, nx)
    lx, lu = _split(labels, nx)
    bounds = _split(lo, nx) + _split(hi, nx)
    suite = zero_suite(prob, (bounds[0], bounds[2], bounds[1], bounds[3]), gx, gy)
    return suite, dict(g=lx, y=lu), np.array(pos + [(-1, -1)] * CONTROLS, dtype=np.int32)


def position_batch(nx, nu, N, uniform):
    """one instance per (row j, knot k) of the stacked record, then CONTROLS quiet ones -> (suite, labels {g, y}, table[B, 2] of (j, k),
    (-1, -1) for a control).  (Cached: a copy.)"""
    suite, labels, table = _position_batch(nx, nu, N, bool(uniform))
    return copy.deepcopy(suite), labels, table


@functools.lru_cache(maxsize=None)
def _odd_one_out_suites(nx, nu, N, B):
    prob = zero_problem(nx, nu, N)
    nz = nx + nu
    spots = list(dict.fromkeys([(0, 0), (nx - 1, N - 1), (nx, 0), (nz - 1, N - 2), (nx // 2, N // 2)]))
    row = np.arange(nz, dtype=np.float64)[:, None]
    out = []
    for j, k in spots:
        rng = np.random.default_rng([nx, nu, N, j, k, 61])
        lo, hi = np.broadcast_to(-(1.0 + row / 64.0), (nz, N)).copy(), np.broadcast_to(1.0 + (row + 0.5) / 64.0, (nz, N)).copy()
        if (N if j < nx else N - 1) < 2:
            continue                                     # (a family with one knot is uniform whatever its pair)
        common = (lo[j, k], hi[j, k])
        plain = tuple(_split(lo, nx)) + tuple(_split(hi, nx))
        lo[j, k], hi[j, k] = _dn(lo[j, k]), _up(hi[j, k])
        g = rng.uniform(-2.5, 2.5, (B, nz, N))
        ladder = (hi[j, k], lo[j, k], common[1], common[0], _up(hi[j, k]), _dn(lo[j, k]), _dn(common[1]), _up(common[0]))
        for b in range(B):
            g[b, j, :] = ladder[b % len(ladder)]         # the whole row: the odd entry and its neighbours under the common pair
        labels = classify(lo, hi, g)
        gx, gy = _split(g, nx)
        lx, lu = _split(labels, nx)
        (x_min, u_min), (x_max, u_max) = _split(lo, nx), _split(hi, nx)
        suite = zero_suite(prob, (x_min, x_max, u_min, u_max), gx, gy)
        suite["common_config"] = dict(suite["config"], x_min=plain[0], u_min=plain[1], x_max=plain[2], u_max=plain[3])
        out.append(("row_%d_knot_%d" % (j, k), suite, dict(g=lx, y=lu)))
    return out


def odd_one_out_suites(nx, nu, N, B=8):
    """[(name, suite, labels)]: a box that is one pair per row EXCEPT that one (row, knot) has each bound one ulp further out -- the first
    and the last knot of both families and one in the middle, a launch each.  No solution moves by 1e-9, but the box is not uniform:
    the row of the odd entry carries t on and around both pairs at every knot, so the odd entry clamped by the common pair, or a
    neighbour by the odd one, differs in the last bit.  suite["common_config"]: the box without the odd entry.  (Cached: copies.)"""
    return [(n, copy.deepcopy(s), l) for n, s, l in _odd_one_out_suites(nx, nu, N, B)]


@functools.lru_cache(maxsize=None)
def _class_rounds(nx, nu, N, uniform, phase):
    prob = zero_problem(nx, nu, N)
    nz = nx + nu
    kinds = (UNIFORM_KINDS if uniform else KINDS) + (PHASE_KINDS if phase else ())
    K = len(kinds)
    rounds = []
    for m in range(K):
        lo, hi = np.zeros((nz, N)), np.zeros((nz, N))
        g = np.zeros((B_ROUND, nz, N))
        x = np.zeros((B_ROUND, nz, N))
        labels = np.zeros((B_ROUND, nz, N), dtype=np.int8)
        kind_at = np.zeros((nz, N), dtype=np.int8)
        for j in range(nz):
            for k in range(N):
                # every (row, knot) meets every kind once over the K rounds; uniform: the kind and the pair belong to the row
                c = (j + m) % K if uniform else (j + 2 * k + m) % K
                rng = np.random.default_rng([nx, nu, N, m, j, 0 if uniform else k, 77])
                lo[j, k], hi[j, k] = kind_bounds(kinds[c], rng, j + m if uniform else j + k + m)
                kind_at[j, k] = c
                v = kind_variants(kinds[c], lo[j, k], hi[j, k])
                for b in range(B_ROUND):
                    cls, t = v[(b + j + 3 * k) % len(v)]
                    labels[b, j, k] = CLASSES.index(cls)
                    # phase batches: x carries half of t on odd instances where the halves add up to t exactly, and the sign of a -0
                    if phase and b % 2 and np.isfinite(t) and (0.5 * t) + (t - 0.5 * t) == t and t != 0.0:
                        x[b, j, k], g[b, j, k] = 0.5 * t, t - 0.5 * t
                    else:
                        x[b, j, k], g[b, j, k] = (-0.0 if (phase and t == 0.0 and np.signbit(t)) else 0.0), t
        gx, gy = _split(g, nx)
        lx, lu = _split(labels, nx)
        (x_min, u_min), (x_max, u_max) = _split(lo, nx), _split(hi, nx)
        suite = zero_suite(prob, (x_min, x_max, u_min, u_max), gx, gy)
        suite["cases"]["x"], suite["cases"]["u"] = _split(x, nx)
        rounds.append((suite, dict(g=lx, y=lu)))
    return rounds


def class_rounds(nx, nu, N, uniform, phase=False):
    """the class batch: [(suite, labels {g, y} (B_ROUND, rows, knots))], one round per kind rotation -- over the rounds EVERY (row, knot)
    of both families meets EVERY kind, and the instances of a round walk the kind's t variants.  uniform: one bound pair per row.
    phase: the rounds for tiny_batch_phase -- the PHASE_ONLY kinds as well, and x | u nonzero (cases["x"], cases["u"]) on odd
    instances; a solve ignores those two.  (Cached: copies.)"""
    return [(copy.deepcopy(s), l) for s, l in _class_rounds(nx, nu, N, bool(uniform), bool(phase))]


def bounds_at(cfg, field):
    """(lo, hi) broadcastable against a slack field"""
    return (cfg["x_min"], cfg["x_max"]) if field in ("vnew", "g", "v") else (cfg["u_min"], cfg["u_max"])


# ---- real dynamics ----------------------------------------------------------------------------------------------------------------
def _random_box(rng, nx, nu, N, uniform):
    kx, ku = (1, 1) if uniform else (N, N - 1)
    b = [rng.uniform(-1.0, -0.2, (nx, kx)), rng.uniform(0.2, 1.0, (nx, kx)), rng.uniform(-0.5, -0.1, (nu, ku)), rng.uniform(0.1, 0.5, (nu, ku))]
    return [np.ascontiguousarray(np.broadcast_to(a, (a.shape[0], n))) for a, n in zip(b, (N, N, N - 1, N - 1))]


@functools.lru_cache(maxsize=None)
def _identity_suite(nx, nu, N, uniform, B):
    from cpu_solvers import OracleSolver
    prob, _ = sc.random_problem(nx, nu, N)
    rng = np.random.default_rng([nx, nu, N, int(uniform), 41])
    box = _random_box(rng, nx, nu, N, uniform)
    cfg = sc.default_config(prob, max_iter=1, abs_pri_tol=0.0, abs_dua_tol=0.0, x_min=box[0], x_max=box[1], u_min=box[2], u_max=box[3])
    cases = sc.zero_cases(prob, B)
    for k in ("x0", "Xref", "Uref", "vnew", "znew", "v", "z"):
        cases[k] = rng.normal(0.0, 0.3, cases[k].shape)
    # the oracle's x, u with zero duals; then the duals that put a third of the entries below, a third above and a third inside their
    # bounds, and the warm slacks moved along so that vnew - g (what the linear cost sees) stays what it was up to a rounding
    base = sc.run_cases(OracleSolver, dict(problem=prob, config=cfg, cases=cases), fields=("x", "u"))
    for src, dual, slack, lo, hi in (("x", "g", "vnew", box[0], box[1]), ("u", "y", "znew", box[2], box[3])):
        shape = base[src].shape
        third = (np.arange(base[src][0].size).reshape(shape[1:])[None] + np.arange(B)[:, None, None]) % 3
        t = np.where(third == 0, lo - rng.uniform(0.1, 1.0, shape), np.where(third == 1, hi + rng.uniform(0.1, 1.0, shape), lo + (hi - lo) * rng.uniform(0.2, 0.8, shape)))
        cases[dual] = t - base[src]
        cases[slack] = cases[slack] + cases[dual]
    return dict(problem=prob, config=cfg, cases=cases)


def identity_suite(nx, nu, N, uniform, B=8):
    """real dynamics, random x0, references and warm state, max_iter = 1, tolerances 0 (no solve stops: iter = 1, v = vnew); knot-varying
    random bounds, or one pair per row.  At least a quarter of the state and of the input entries clamp low, a quarter high, a quarter
    stay inside on the oracle's x and u (tests/test_box_ref_cpu.py asserts it).  (Cached: a copy.)"""
    return copy.deepcopy(_identity_suite(nx, nu, N, bool(uniform), B))


def shares(cfg, t_x, t_u):
    """(low, high, inside) fractions of the state and of the input entries"""
    out = []
    for t, lo, hi in ((t_x, cfg["x_min"], cfg["x_max"]), (t_u, cfg["u_min"], cfg["u_max"])):
        out.append((float(np.mean(t < lo)), float(np.mean(t > hi)), float(np.mean((t >= lo) & (t <= hi)))))
    return out


ENABLE_CASES = (("state_off", 0, 1, True), ("input_off", 1, 0, True), ("both_off", 0, 0, True), ("never_set", 1, 1, False))


def enable_suites(nx, nu, N, B=8):
    """[(name, suite)]: the identity suite's data under en_state_bound = 0 | en_input_bound = 0 | both 0 | bounds never set (config
    entry bounds_set = False: the launcher makes no set_bound_constraints call; the reference's default box is +-1e17, which is what the
    config then holds), each with the STATE family's box knot-invariant and the input family's knot-varying, and the reverse"""
    base_u, base_v = identity_suite(nx, nu, N, True, B), identity_suite(nx, nu, N, False, B)
    out = []
    for name, en_s, en_i, have in ENABLE_CASES:
        for which in ("state_uniform", "input_uniform"):
            suite = copy.deepcopy(base_v)
            cfg = suite["config"]
            src = base_u["config"]
            for k in (("x_min", "x_max") if which == "state_uniform" else ("u_min", "u_max")):
                cfg[k] = src[k].copy()
            cfg.update(en_state_bound=en_s, en_input_bound=en_i, bounds_set=have)
            if not have:
                cfg.update(x_min=np.full((nx, N), -1e17), x_max=np.full((nx, N), 1e17), u_min=np.full((nu, N - 1), -1e17), u_max=np.full((nu, N - 1), 1e17))
            out.append(("%s-%s" % (name, which), suite))
    return out


# ---- carried state: the pure-map family ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pure_map_suite(nx, nu, N, B, iters):
    prob = family(nx, nu, N)
    rng = np.random.default_rng([nx, nu, N, 53])
    box = _random_box(rng, nx, nu, N, False)
    cfg = sc.default_config(prob, max_iter=iters, abs_pri_tol=0.0, abs_dua_tol=0.0, x_min=box[0], x_max=box[1], u_min=box[2], u_max=box[3])
    cases = sc.zero_cases(prob, B)
    cases["x0"] = rng.normal(0.0, 1.0, (B, nx))
    cases["x0"][::3] = 0.0
    cases["g"], cases["y"] = rng.normal(0.0, 1.5, cases["g"].shape), rng.normal(0.0, 0.7, cases["y"].shape)
    return dict(problem=prob, config=cfg, cases=cases)


def pure_map_suite(nx, nu, N, B=12, iters=3):
    """A = B = 0 (halfspace_ref.family): x is x0 at knot 0 and +0 at every later knot in every iteration, so the state rows of a solve
    are the box map iterated from the warm g.  Tolerances 0: no solve stops.  (Cached: a copy.)"""
    return copy.deepcopy(_pure_map_suite(nx, nu, N, B, iters))


def pure_map_want(suite, rule="minmaxnum"):
    """vnew, g, v of the state rows after max_iter iterations"""
    cfg, cases = suite["config"], suite["cases"]
    x = np.zeros_like(cases["g"])
    x[:, :, 0] = cases["x0"]
    g = cases["g"]
    vnew = v = np.zeros_like(g)
    u0, y0 = np.zeros_like(cases["y"]), np.zeros_like(cases["y"])
    for _ in range(cfg["max_iter"]):
        out = step(cfg, x, u0, g, y0, rule)
        vnew, g = out["vnew"], out["g"]
        v = vnew                                     # (admm.cpp:445: the solve stays open)
    return dict(vnew=vnew, g=g, v=v)


# ---- the fixture (oracle/gen_golden.py --box-edges) ------------------------------------------------------------------------------------
FIXTURE_DIMS = (3, 2, 4)


def fixture_rounds():
    """the rounds tests/golden/box_edges.npz holds: the phase rounds of FIXTURE_DIMS, knot-varying then uniform -> [(tag, suite, labels)]"""
    out = []
    for uniform in (False, True):
        for m, (suite, labels) in enumerate(class_rounds(*FIXTURE_DIMS, uniform, phase=True)):
            out.append(("%s%02d" % ("u" if uniform else "v", m), suite, labels))
    return out


def phase_inputs(suite):
    """x, u, g, y of a phase round"""
    c = suite["cases"]
    return c["x"], c["u"], c["g"], c["y"]
