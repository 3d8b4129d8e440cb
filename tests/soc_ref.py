"""TEST INFRASTRUCTURE -- the reference's project_soc (src/tinympc/admm.cpp:39-60) restated in numpy, and seeded generators of the
inputs at which a restatement of it can go wrong without any golden noticing.

The reference computes `mu` and the norm `a` in float: `a = (float)sqrt(s0^2 + s1^2)` (a double square root of an unfused sum, then
ONE rounding to float), `a / mu` is a float division, and the four branches compare the float `a` with the double `u0 = s2 * mu`.
numpy evaluates every ufunc on its own, so nothing here is fused; float32 arithmetic is IEEE with gradual underflow.

project(s, mu)            -> (out, branch)      s (..., 3) doubles, mu broadcast against s[..., 0]
iterate(g, mu, iters)     -> (vcnew, gc)        the cone rows of a solve whose x stays exactly 0 there (tests/test_soc_ref_cpu.py)
draw(rng, cls, mu, count) -> s (count, 3)       members of one class (CLASSES), checked against the model's own facts
"""
import numpy as np

BRANCHES = ("below", "inside", "outside", "remainder")
MARGIN = 1.0 - 2.0 ** -20                  # the all-inside fast path takes q <= u0^2 (1 - 2^-20)  (admm_kernel.hip.h: soc_all_inside)
RELS = (0.0, 1e-9, -1e-9, 3e-8, -3e-8, 2.0 ** -21, -2.0 ** -21, 2.0 ** -20, -2.0 ** -20)
MUS = (0.3, 0.5, 1.0, 1.5, 2.0 ** -60, 2.0 ** 60, 2.0 ** -61, 2.0 ** 61)      # the last two: powers of two outside the multiply path
FLT_MIN_NORMAL = 2.0 ** -126


def facts(s, mu):
    """what the reference computes on the way: u0, q, rd = the double square root, a = its float rounding (as a double)"""
    s = np.asarray(s, dtype=np.float64)
    mu32 = np.broadcast_to(np.asarray(mu, dtype=np.float64).astype(np.float32), s.shape[:-1])
    with np.errstate(all="ignore"):
        u0 = s[..., 2] * mu32.astype(np.float64)                       # :40
        q0 = s[..., 0] * s[..., 0]
        q1 = s[..., 1] * s[..., 1]
        q = q0 + q1
        rd = np.sqrt(q)
        a32 = rd.astype(np.float32)                                    # :42
    return dict(u0=u0, q=q, rd=rd, a32=a32, a=a32.astype(np.float64), mu32=mu32)


def project(s, mu):
    """-> (out (..., 3), branch (...) indices into BRANCHES)"""
    s = np.asarray(s, dtype=np.float64)
    f = facts(s, mu)
    u0, a, a32, mu32 = f["u0"], f["a"], f["a32"], f["mu32"]
    with np.errstate(all="ignore"):
        below = a <= -u0                                               # :46
        inside = ~below & (a <= u0)                                    # :49
        outside = ~below & ~inside & (a >= np.abs(u0))                 # :52
        scale = 0.5 * (1.0 + u0 / a)                                   # :55
        last = (a32 / mu32).astype(np.float64)                         # :54, a float division
        proj = np.stack([scale * s[..., 0], scale * s[..., 1], scale * last], axis=-1)
    out = np.zeros_like(s)                                             # below | :58 (only NaNs get there)
    out = np.where(inside[..., None], s, out)
    out = np.where(outside[..., None], proj, out)
    branch = np.where(below, 0, np.where(inside, 1, np.where(outside, 2, 3))).astype(np.int8)
    return out, branch


def iterate(g, mu, iters):
    """the cone rows of `iters` ADMM iterations when x is exactly +0 there: vcnew = P(x + gc) (:103, :119), gc = (gc + x) - vcnew
    (:229) -> (vcnew, gc) after the last one"""
    g = np.asarray(g, dtype=np.float64)
    v = np.zeros_like(g)
    for _ in range(int(iters)):
        with np.errstate(all="ignore"):
            s = 0.0 + g
            v, _ = project(s, mu)
            g = s - v
    return v, g


def same_bits(a, b):
    """elementwise: the same 64 bits, or both NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))


def fast_path_takes(s, mu):
    """soc_all_inside's per-item condition, restated: q <= u0^2 (1 - 2^-20), 1e-30 < u0 < 1e300, q < 1e70"""
    f = facts(s, mu)
    with np.errstate(all="ignore"):
        return (f["u0"] > 1e-30) & (f["u0"] < 1e300) & (f["q"] <= (f["u0"] * f["u0"]) * MARGIN) & (f["q"] < 1e70)


# ---- candidates: every function returns m vectors that are LIKELY members of the class; `member` decides
def _ring(rng, n, s2):
    th = rng.uniform(0.0, 2.0 * np.pi, np.shape(n))
    return np.stack([n * np.cos(th), n * np.sin(th), np.broadcast_to(s2, np.shape(n))], axis=-1)


def _mud(mu):
    return float(np.float32(mu))


def _near_u0(rng, mu, m, sign, rels):
    s2 = sign * rng.uniform(0.1, 10.0, m)
    return _ring(rng, np.abs(s2 * _mud(mu)) * (1.0 + rng.choice(rels, m)), s2)


def _log(rng, lo, hi, m):
    return 10.0 ** rng.uniform(lo, hi, m)


def _sign(rng, m):
    return rng.choice([-1.0, 1.0], m)


def _with_nonfinite(rng, mu, m, col, values):
    s = rng.normal(0.0, 1.0, (m, 3))
    s[:, 2] = np.abs(s[:, 2]) * 3.0
    c = rng.choice(col, m)
    s[np.arange(m), c] = rng.choice(values, m)
    return s


def _margin(rng, mu, m):
    s2 = rng.uniform(0.1, 10.0, m)
    return _ring(rng, s2 * _mud(mu) * np.sqrt(MARGIN) * (1.0 + _sign(rng, m) * rng.uniform(0.5, 40.0, m) * 2.0 ** -52), s2)


def _negzero(rng, mu, m):
    s = _ring(rng, np.where(rng.random(m) < 0.5, 0.0, rng.uniform(0.1, 3.0, m)), -0.0)
    return s


def _tiny_norm(lo, hi):
    def gen(rng, mu, m):                   # the last component of the norm's own size (either sign), or exactly zero
        n = _log(rng, lo, hi, m)
        s2 = np.where(rng.random(m) < 0.25, 0.0, _sign(rng, m) * n * _log(rng, -1.0, 1.0, m) / _mud(mu))
        return _ring(rng, n, s2)
    return gen


def _q_big(rng, mu, m):
    n = _log(rng, 35.2, 38.4, m)
    return _ring(rng, n, _sign(rng, m) * n * _log(rng, -1.0, 1.0, m) / _mud(mu))


def _a_overflow(rng, mu, m):
    n = np.where(rng.random(m) < 0.5, _log(rng, 199.0, 201.0, m), _log(rng, 39.0, 150.0, m))     # q = inf | q finite, (float)sqrt(q) = inf
    return _ring(rng, n, _sign(rng, m) * _log(rng, -3.0, 3.0, m))


def _quot_tiny(rng, mu, m):
    a = _mud(mu) * _log(rng, -49.0, -38.2, m)
    return _ring(rng, a, _sign(rng, m) * 0.5 * a / _mud(mu) * rng.uniform(0.0, 1.0, m))


CANDIDATES = {
    "rounded_in": lambda rng, mu, m: _near_u0(rng, mu, m, 1.0, RELS[1:5]),
    "rounded_out": lambda rng, mu, m: _near_u0(rng, mu, m, 1.0, RELS[1:5]),
    "exact": lambda rng, mu, m: _near_u0(rng, mu, m, 1.0, RELS[:1]),
    "neg_rounded_in": lambda rng, mu, m: _near_u0(rng, mu, m, -1.0, RELS[1:5]),
    "neg_rounded_out": lambda rng, mu, m: _near_u0(rng, mu, m, -1.0, RELS[1:5]),
    "neg_exact": lambda rng, mu, m: _near_u0(rng, mu, m, -1.0, RELS[:1]),
    "near": lambda rng, mu, m: _near_u0(rng, mu, m, _sign(rng, m), RELS[5:]),
    "margin_below": _margin,
    "margin_above": _margin,
    "below": lambda rng, mu, m: (lambda s2: _ring(rng, rng.uniform(0.0, 0.9, m) * s2 * _mud(mu), -s2))(rng.uniform(0.1, 10.0, m)),
    "inside": lambda rng, mu, m: (lambda s2: _ring(rng, rng.uniform(0.0, 0.9, m) * s2 * _mud(mu), s2))(rng.uniform(0.1, 10.0, m)),
    "outside": lambda rng, mu, m: (lambda s2: _ring(rng, rng.uniform(1.1, 10.0, m) * np.abs(s2) * _mud(mu), s2))(_sign(rng, m) * rng.uniform(0.1, 10.0, m)),
    "zero": lambda rng, mu, m: np.zeros((m, 3)),
    "negzero": _negzero,
    "q_big": _q_big,
    "a_overflow": _a_overflow,
    "a_denormal": _tiny_norm(-44.0, -38.2),
    "a_zero": _tiny_norm(-170.0, -150.0),
    "u0_small": lambda rng, mu, m: (lambda u0: _ring(rng, rng.uniform(0.0, 0.5, m) * u0, u0 / _mud(mu)))(_log(rng, -40.0, -30.0, m)),
    "u0_big": lambda rng, mu, m: (lambda u0: _ring(rng, _log(rng, -3.0, 30.0, m), u0 / _mud(mu)))(_log(rng, 300.0, 303.0, m)),
    "quot_tiny": _quot_tiny,
    "nan_head": lambda rng, mu, m: _with_nonfinite(rng, mu, m, [0, 1], [np.nan]),
    "nan_last": lambda rng, mu, m: _with_nonfinite(rng, mu, m, [2], [np.nan]),
    "inf_head": lambda rng, mu, m: _with_nonfinite(rng, mu, m, [0, 1], [np.inf, -np.inf]),
    "inf_last": lambda rng, mu, m: _with_nonfinite(rng, mu, m, [2], [np.inf, -np.inf]),
}
CLASSES = tuple(CANDIDATES)
NONFINITE = ("nan_head", "nan_last", "inf_head", "inf_last")


def member(cls, s, mu):
    """the class's defining property, on the model's own intermediate values"""
    f = facts(s, mu)
    u0, q, rd, a, a32, mu32 = f["u0"], f["q"], f["rd"], f["a"], f["a32"], f["mu32"]
    _, br = project(s, mu)
    fin = np.all(np.isfinite(s), axis=-1)
    with np.errstate(all="ignore"):
        thr = (u0 * u0) * MARGIN
        quot = a32 / mu32
        return {
            "rounded_in": lambda: (u0 > 0) & (rd > u0) & (a <= u0),
            "rounded_out": lambda: (u0 > 0) & (rd < u0) & (a > u0),
            "exact": lambda: (u0 > 0) & (rd == u0),
            "neg_rounded_in": lambda: (u0 < 0) & (rd > -u0) & (a <= -u0),
            "neg_rounded_out": lambda: (u0 < 0) & (rd < -u0) & (a > -u0),
            "neg_exact": lambda: (u0 < 0) & (rd == -u0),
            "near": lambda: (u0 != 0) & (np.abs(rd / np.abs(u0) - 1.0) > 2.0 ** -22) & (np.abs(rd / np.abs(u0) - 1.0) < 2.0 ** -19),
            "margin_below": lambda: (u0 > 0) & (q <= thr) & (q > thr * (1.0 - 2.0 ** -40)),
            "margin_above": lambda: (u0 > 0) & (q > thr) & (q < thr * (1.0 + 2.0 ** -40)),
            "below": lambda: (br == 0) & (u0 < 0) & (rd < -0.95 * u0),
            "inside": lambda: (br == 1) & (rd < 0.95 * u0),
            "outside": lambda: (br == 2) & (rd > 1.05 * np.abs(u0)) & (u0 != 0),
            "zero": lambda: np.all(s == 0, axis=-1) & ~np.signbit(s[..., 2]),
            "negzero": lambda: (s[..., 2] == 0) & np.signbit(s[..., 2]),
            "q_big": lambda: (q >= 1e70) & np.isfinite(a),
            "a_overflow": lambda: fin & np.isinf(a),
            "a_denormal": lambda: (a > 0) & (a < FLT_MIN_NORMAL),
            "a_zero": lambda: (a == 0) & (rd > 0),
            "u0_small": lambda: (u0 > 0) & (u0 <= 1e-30) & (br == 1),
            "u0_big": lambda: (u0 >= 1e300) & np.isfinite(u0) & (br == 1),
            "quot_tiny": lambda: (br == 2) & (a > 0) & (quot < FLT_MIN_NORMAL),
            "nan_head": lambda: np.isnan(s[..., 0]) | np.isnan(s[..., 1]),
            "nan_last": lambda: np.isnan(s[..., 2]) & ~np.isnan(q),
            "inf_head": lambda: np.isinf(q) & ~fin & np.isfinite(s[..., 2]),
            "inf_last": lambda: np.isinf(s[..., 2]) & np.isfinite(q),
        }[cls]()


def feasible(cls, mu):
    """a / mu is a float denormal only for a >= 2^-149, and u0 >= 1e300 needs s2 = u0 / mu to be a double: not at mu = 2^-60, 2^-61"""
    return not (cls in ("quot_tiny", "u0_big") and _mud(mu) < 2.0 ** -20)


def stays_finite(s, mu, iters=3):
    """every value of `iters` iterations of the map is finite, and so is what a solve's linear cost makes of it (rho (vcnew - gc),
    times a rho of at most 10): such an item cannot reach x through 0 * inf"""
    ok = np.all(np.isfinite(s), axis=-1)
    g = np.asarray(s, dtype=np.float64)
    for _ in range(iters):
        v, g2 = iterate(g, mu, 1)
        with np.errstate(all="ignore"):
            ok &= np.all(np.isfinite(v) & np.isfinite(g2) & (np.abs(v - g2) < 1e306), axis=-1)
        g = g2
    return ok


def draw(rng, cls, mu, count, finite=False):
    """`count` members of class `cls` for the coefficient mu (seeded by rng); finite: only items that stay finite through a solve"""
    assert feasible(cls, mu), (cls, mu)
    got = []
    have = 0
    for _ in range(200):
        if have >= count:
            break
        c = CANDIDATES[cls](rng, mu, max(64, 4 * count))
        keep = member(cls, c, mu)
        if finite:
            keep &= stays_finite(c, mu)
        got.append(c[keep])
        have += int(keep.sum())
    assert have >= count, ("class ran dry", cls, mu, have, count)
    return np.concatenate(got)[:count]


def classes_for(mu, finite=False, solve=False):
    """the classes that exist at mu; solve: those a solve can carry (no non-finite input); finite: ... for more than one iteration"""
    return tuple(c for c in CLASSES if feasible(c, mu) and not ((finite or solve) and c in NONFINITE) and not (finite and c == "a_overflow"))


def fill(rng, mu, shape, finite=False, shift=0):
    """an array shape + (3,) of items for one cone of coefficient mu, and its class labels (indices into CLASSES): the class of the
    item at flat index i is classes_for(mu)[(i + shift) % len] -- with `shift` advancing by one per instance every position of the
    item layout (lane, pass) meets every class"""
    cl = classes_for(mu, finite)
    n = int(np.prod(shape))
    idx = ((np.arange(n).reshape(shape) + np.asarray(shift)) % len(cl)).ravel()        # shift: broadcast against shape
    s = np.zeros((n, 3))
    lab = np.zeros(n, dtype=np.int8)
    for k, c in enumerate(cl):
        at = np.flatnonzero(idx == k)
        s[at] = draw(rng, c, mu, len(at), finite)
        lab[at] = CLASSES.index(c)
    return s.reshape(tuple(shape) + (3,)), lab.reshape(shape)


def deep_inside(rng, mu, shape, ratio=0.2):
    """items with norm <= ratio * u0, s2 in [0.1, 10]: the all-inside fast path's daily bread"""
    m = int(np.prod(shape))
    s2 = rng.uniform(0.1, 10.0, m)
    return _ring(rng, rng.uniform(0.0, ratio, m) * s2 * _mud(mu), s2).reshape(tuple(shape) + (3,))


def bridged(rng, mu, count):
    """rounded_out items whose double norm is below u0 by MORE than 2^-26 of it (and the float norm still above u0): what an all-inside
    margin narrower than a float's half ulp lets through"""
    got = np.zeros((0, 3))
    while len(got) < count:
        c = _near_u0(rng, mu, 4096, 1.0, RELS[4:5])
        f = facts(c, mu)
        got = np.concatenate([got, c[member("rounded_out", c, mu) & (f["rd"] < f["u0"] * (1.0 - 2.0 ** -26))]])
    return got[:count]


def fixture_items(seed=20, per=10):
    """the directed set of tests/golden/project_soc_edges.npz: `per` members of every feasible class at each of MUS, and 4 `per` plain
    vectors each at mu = 0.0 and mu = -0.5 (tiny_batch_set_cone_constraints does not refuse them) -> s, mu, labels, names"""
    rng = np.random.default_rng(seed)
    S, M, L = [], [], []
    for mu in MUS:
        for c in classes_for(mu):
            S.append(draw(rng, c, mu, per))
            M.append(np.full(per, mu))
            L.append(np.full(per, CLASSES.index(c), dtype=np.int8))
    names = CLASSES + ("mu_zero", "mu_negative")
    for k, mu in enumerate((0.0, -0.5)):
        s = rng.normal(0.0, 1.0, (4 * per, 3))
        s[::7] = 0.0
        S.append(s)
        M.append(np.full(4 * per, mu))
        L.append(np.full(4 * per, len(CLASSES) + k, dtype=np.int8))
    return np.concatenate(S), np.concatenate(M), np.concatenate(L), names


# ---- the family on which the cone rows of a solve ARE the map above -----------------------------------------------------------------
# A = 0, B with zero rows at the state-cone rows, f = 0, Xref = Uref = 0, no boxes, both tolerances 0: the cone rows of x are +0 at every
# knot >= 1 in every iteration (knot 0 is x0, kept 0 there), so the projection's input is 0 + gc.  A non-finite gc would reach every row
# of x through 0 * NaN in the backward pass of the reference itself -- those classes go through update_slack alone.
FORMS = {
    # name: nx, nu, N, first rows of the state cones, first row of the input cone that the "mixed" pair of a one-cone shape adds
    "one_row_6_3_10": dict(nx=6, nu=3, N=10, rows=(0, 3)),              # the compiled-in cone form of the one-row kernel, two passes
    "one_cone_6_3_10": dict(nx=6, nu=3, N=10, rows=(1,), input_row=0),   # ... with rows 0, 4, 5 in no cone
    "one_row_5_3_7": dict(nx=5, nu=3, N=7, rows=(1,), input_row=0),     # a run-time instantiated one-row form
    "half_4_3_10": dict(nx=4, nu=3, N=10, rows=(0,), input_row=0),      # nx + nu <= 8: the half-row candidate
    "wide_20_4_10": dict(nx=20, nu=4, N=10, rows=(3, 14)),              # W = 2: the cone at rows 14..16 straddles the two DPP rows
    "long_8_3_50": dict(nx=8, nu=3, N=50, rows=(1, 5)),                 # a long form, R > 1
    "tile_jit_16_8_6": dict(nx=16, nu=8, N=6, rows=(0, 6, 12)),         # a tile shape outside the compiled-in list
}
MU_SETS = {"pow2": (0.5, 0.5), "plain": (0.3, 0.3), "mixed": (0.5, 0.3),
           "pow2_60": (2.0 ** 60, 2.0 ** -60), "pow2_61": (2.0 ** 61, 2.0 ** -61)}
MIN_PER_CLASS = 32


def family(form, seed=0, dynamics=False):
    """dynamics: A is nonzero (spectral radius 0.9) on the rows and columns of no cone -- its cone rows stay zero, which is all the
    construction needs -- so that x0 matters: with A = 0 the gain Kinf is zero and a solve forgets x0 after one iteration"""
    f = FORMS[form]
    nx, nu, N = f["nx"], f["nu"], f["N"]
    rng = np.random.default_rng(seed + 1000 * nx + 10 * nu + N)
    B = rng.standard_normal((nx, nu)) / np.sqrt(nx)
    for r in f["rows"]:
        B[r:r + 3] = 0.0
    A = np.zeros((nx, nx))
    if dynamics:
        free = noncone_rows(form)
        M = rng.standard_normal((len(free), len(free)))
        A[np.ix_(free, free)] = M * 0.9 / np.max(np.abs(np.linalg.eigvals(M)))
    return dict(nx=nx, nu=nu, N=N, rho=1.0, A=A, B=B, f=np.zeros(nx), Q=rng.uniform(1.0, 10.0, nx), R=rng.uniform(0.1, 1.0, nu))


def cone_setup(form, mu_set):
    """-> (state cone triple, input cone triple or None, the state cones' coefficients)"""
    f = FORMS[form]
    pair = MU_SETS[mu_set]
    rows = f["rows"]
    if len(rows) == 1:                       # one state cone: the mixed pair's second coefficient goes to an input cone (its items are whatever
        ic_ = ([f["input_row"]], [3], [pair[1]]) if mu_set == "mixed" else None        # u + yc makes them: no pass of the wave is all-inside then)
        return ([rows[0]], [3], [pair[0]]), ic_, (pair[0],)
    mus = tuple(pair[k % 2] for k in range(len(rows)))
    return (list(rows), [3] * len(rows), list(mus)), None, mus


def config(form, mu_set, max_iter, tol=0.0):
    """oracle/scenarios.py's config dictionary for the family: boxes off, the state cones (and the pair's input cone) on"""
    f = FORMS[form]
    nx, nu, N = f["nx"], f["nu"], f["N"]
    sc_, ic_, _ = cone_setup(form, mu_set)
    return dict(max_iter=int(max_iter), abs_pri_tol=tol, abs_dua_tol=tol, check_termination=1, en_state_bound=0, en_input_bound=0,
                en_state_soc=1, en_input_soc=1 if ic_ else 0, state_cone=sc_, input_cone=ic_,
                x_min=np.full((nx, N), -1e17), x_max=np.full((nx, N), 1e17), u_min=np.full((nu, N - 1), -1e17), u_max=np.full((nu, N - 1), 1e17),
                en_state_linear=0, en_input_linear=0, en_tv_state_linear=0, en_tv_input_linear=0, linear=None, tv_linear=None)


def pack(form, items, fill_value=0.0):
    """items (B, cones, N, 3) -> a state field (B, nx, N) with the items on the cone rows"""
    f = FORMS[form]
    out = np.full((items.shape[0], f["nx"], f["N"]), fill_value)
    for k, r in enumerate(f["rows"]):
        out[:, r:r + 3, :] = items[:, k].transpose(0, 2, 1)
    return out


def unpack(form, field):
    """a state field (B, nx, N) -> its cone rows as items (B, cones, N, 3)"""
    return np.stack([field[:, r:r + 3, :].transpose(0, 2, 1) for r in FORMS[form]["rows"]], axis=1)


def noncone_rows(form):
    f = FORMS[form]
    return np.array([r for r in range(f["nx"]) if not any(c <= r < c + 3 for c in f["rows"])], dtype=int)


def directed_batch(form, mu_set, iters, B=64, seed=0):
    """the directed batch of one (form, coefficient set, iteration count): items (launches, B, cones, N, 3), their labels, the cones'
    coefficients.  As many launches of B instances as it takes for every class to have MIN_PER_CLASS members; instance b of launch l
    shifts the class ladder by b + 7 l, so every (lane, pass) position of the item layout meets every class.  iters = 1 keeps the
    classes whose result is not finite (a_overflow); more iterations keep only items that stay finite."""
    f = FORMS[form]
    _, _, mus = cone_setup(form, mu_set)
    N, K = f["N"], len(mus)
    finite = iters > 1
    most = max(len(classes_for(mu, finite, True)) for mu in mus)
    launches = -(-(MIN_PER_CLASS + 1) * most // (B * N))          # (every cone alone has enough: a class may exist at one coefficient only)
    rng = np.random.default_rng([seed, sorted(FORMS).index(form), sorted(MU_SETS).index(mu_set), iters])
    items = np.zeros((launches, B, K, N, 3))
    labels = np.zeros((launches, B, K, N), dtype=np.int8)
    for k, mu in enumerate(mus):
        cl = classes_for(mu, finite, True)
        shift = (np.arange(B)[None, :, None] + 7 * np.arange(launches)[:, None, None] + 3 * k)
        idx = (np.arange(N)[None, None, :] + shift) % len(cl)
        for c_i, c in enumerate(cl):
            at = idx == c_i
            n = int(at.sum())
            items[:, :, k][at] = draw(rng, c, mu, n, finite)
            labels[:, :, k][at] = CLASSES.index(c)
    return items, labels, mus


def class_counts(labels):
    return {CLASSES[k]: int(n) for k, n in enumerate(np.bincount(np.asarray(labels).ravel(), minlength=len(CLASSES))) if n}


# ---- what the CPU and the GPU test module share
CASES = [(form, mu_set) for form in FORMS for mu_set in ("pow2", "plain", "mixed")] + \
        [(form, mu_set) for form in ("one_row_6_3_10", "wide_20_4_10") for mu_set in ("pow2_60", "pow2_61")]


def oracle_cone_rows(form, mu_set, iters, gc, x0=None, tol=0.0, dynamics=False):
    """one oracle solve per instance of the A = 0 family, warm gc -> (vcnew, gc, iterations), the fields whole"""
    import scenarios as sc                       # (oracle/: on the path of every test module)
    from cpu_solvers import OracleSolver
    prob = family(form, dynamics=dynamics)
    o = sc.make_solver(OracleSolver, prob, config(form, mu_set, iters, tol))
    B = gc.shape[0]
    v, g, it = np.zeros_like(gc), np.zeros_like(gc), np.zeros(B, dtype=int)
    zero = {k: np.zeros(o[k].shape) for k in o.STATE_FIELDS + ("Xref", "Uref")}
    for b in range(B):
        o.restore(zero)
        o["gc"] = gc[b]
        if x0 is not None:
            o["x"][:, 0] = x0[b]
        o.solve()
        v[b], g[b], it[b] = o["vcnew"], o["gc"], int(o.get("sol_iter"))
    o.close()
    return v, g, it
