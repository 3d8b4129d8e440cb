"""TEST INFRASTRUCTURE -- the half-space step of update_slack (src/tinympc/admm.cpp:137-211, project_hyperplane :70-73) restated in
numpy exactly as oracle/tinympc_oracle.c:387 forms it, and seeded generators of the inputs at which a restatement of it can go wrong
without any golden noticing.

One column z (n rows) meets the K half-spaces a_k'z <= b_k of its family one after the other: cv = a_k'z and nn = a_k'a_k are summed
from 0.0 in row order with every product rounded, the test is strict (cv > b), dist = (cv - b) / nn, z_r <- z_r - round(dist a_kr).
numpy evaluates every ufunc on its own, so nothing here is fused.  (The REFERENCE's Eigen reductions pair the terms differently once a
row has more than 3 entries: tests/test_halfspace_ref_cpu.py bounds that difference with summation_bound() below.)

project(z, A, b)               -> (out, facts)       z (..., n), A (..., K, n), b (..., K), broadcast against each other
tables(sets, family, N)        -> (A, b) per column  the static tables, or the time-varying ones indexed as the reference does
step(sets, N, x, u, duals)     -> the eight fields of one update_slack + update_dual of the families that are on
iterate(gl, x, A, b, iters)    -> (vlnew, gl)        a column whose x is given: vlnew = P(x + gl), gl = (gl + x) - vlnew
draw(rng, cls, A, b, x, scale) -> gl (n,)            x + gl is a member of class `cls` (CLASSES), decided on the model's own facts
"""
import functools
import math
from fractions import Fraction

import numpy as np

from soc_ref import same_bits  # noqa: F401  (re-exported: elementwise the same 64 bits, or both NaN)

FAMILIES = (("vlnew", "gl", "x", "sx"), ("zlnew", "yl", "u", "su"), ("vlnew_tv", "gl_tv", "x", "tx"), ("zlnew_tv", "yl_tv", "u", "tu"))
FLAG = {"sx": "en_state_linear", "su": "en_input_linear", "tx": "en_tv_state_linear", "tu": "en_tv_input_linear"}


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def project(z, A, b):
    """sequential projection; facts: viol (..., K) whether half-space k projected, cv (..., K) the a_k'z it tested, cv0 (..., K) a_k'z of
    the column as it came in, nn (..., K)"""
    z = np.asarray(z, dtype=np.float64)
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    K, n = A.shape[-2], A.shape[-1]
    lead = np.broadcast_shapes(z.shape[:-1], A.shape[:-2], b.shape[:-1])
    z = np.array(np.broadcast_to(z, lead + (n,)))
    A = np.broadcast_to(A, lead + (K, n))
    b = np.broadcast_to(b, lead + (K,))
    z0 = z.copy()
    viol, cvs, cv0, nns = (np.zeros(lead + (K,), dtype=t) for t in (bool, float, float, float))
    with np.errstate(all="ignore"):
        for k in range(K):
            cv, c0, nn = np.zeros(lead), np.zeros(lead), np.zeros(lead)
            for r in range(n):
                cv = cv + A[..., k, r] * z[..., r]
                c0 = c0 + A[..., k, r] * z0[..., r]
                nn = nn + A[..., k, r] * A[..., k, r]
            hit = cv > b[..., k]
            dist = (cv - b[..., k]) / nn
            for r in range(n):
                pr = dist * A[..., k, r]
                z[..., r] = np.where(hit, z[..., r] - pr, z[..., r])
            viol[..., k], cvs[..., k], cv0[..., k], nns[..., k] = hit, cv, c0, nn
    return z, dict(viol=viol, cv=cvs, cv0=cv0, nn=nns)


def tv_tables(tA, tb, N, n):
    """the reference's time-varying lookup (admm.cpp:186-211): half-space k of knot i is row nt * i + k of tv_Alin and tv_blin(k, i)
    -> A (N, nt, n), b (N, nt)"""
    tb = np.asarray(tb, dtype=np.float64).reshape(-1, N)
    nt = tb.shape[0]
    tA = np.asarray(tA, dtype=np.float64).reshape(nt * N, n)
    A = np.stack([np.stack([tA[nt * i + k] for k in range(nt)]) if nt else np.zeros((0, n)) for i in range(N)])
    b = np.stack([np.array([tb[k, i] for k in range(nt)]) for i in range(N)]).reshape(N, nt)
    return A, b


def tables(sets, fam, N, nx, nu):
    """(A, b) of one family, broadcastable against its columns (batch, knot): static (K, n) | time-varying (knots, K, n); None: off"""
    if not sets.get(FLAG[fam]):
        return None
    if fam in ("sx", "su"):
        Ax, bx, Au, bu = sets["linear"]
        A, b, n = (Ax, bx, nx) if fam == "sx" else (Au, bu, nu)
        return np.asarray(A, dtype=np.float64).reshape(-1, n), np.asarray(b, dtype=np.float64).ravel()
    tAx, tbx, tAu, tbu = sets["tv_linear"]
    if fam == "tx":
        return tv_tables(tAx, tbx, N, nx)
    return tv_tables(tAu, tbu, N - 1, nu)


def step(sets, x, u, duals):
    """one update_slack + update_dual of the half-space families that are on: x (B, nx, N), u (B, nu, N - 1), duals: gl, yl, gl_tv,
    yl_tv as the solver holds them -> {vlnew, gl, ...} and `viol` per family (B, knots, K)"""
    nx, N, nu = x.shape[1], x.shape[2], u.shape[1]
    out = {}
    for v, g, src, fam in FAMILIES:
        t = tables(sets, fam, N, nx, nu)
        if t is None:
            continue
        col = (x if src == "x" else u).transpose(0, 2, 1)
        with np.errstate(all="ignore"):
            s = col + np.asarray(duals[g], dtype=np.float64).transpose(0, 2, 1)          # :139 / :144 / :177 / :182
            p, f = project(s, t[0], t[1])
            out[v], out[g], out["viol_" + fam] = p.transpose(0, 2, 1), (s - p).transpose(0, 2, 1), f["viol"]   # :239-254
    return out


def iterate(gl, x, A, b, iters):
    """`iters` ADMM iterations of columns whose x is given (gl, x (..., n)) -> (vlnew, gl) after the last one"""
    gl = np.asarray(gl, dtype=np.float64)
    v = np.zeros_like(gl)
    for _ in range(int(iters)):
        with np.errstate(all="ignore"):
            s = x + gl
            v, _ = project(s, A, b)
            gl = s - v
    return v, gl


# ---- exact evaluation and the summation bound (tests/test_halfspace_ref_cpu.py only) ---------------------------------------------------
def exact_column(z, A, b, viol):
    """the sequential projection in rational arithmetic along the branch pattern `viol` (K bools) -> list of Fractions"""
    z = [Fraction(float(v)) for v in z]
    for k in range(len(b)):
        if not viol[k]:
            continue
        a = [Fraction(float(v)) for v in A[k]]
        cv, nn = sum(p * q for p, q in zip(a, z)), sum(p * p for p in a)
        z = [zr - (cv - Fraction(float(b[k]))) / nn * ar for zr, ar in zip(z, a)]
    return z


def summation_bound(z, A, b, viol, with_dcv=False):
    """how far two evaluations of the projection of ONE column may lie apart, per row, when both take the branch pattern `viol`, round
    every product and every operation once and differ only in the ORDER of the two sums: each computed sum of n rounded products lies
    within g |a|'|z| of the exact one, g = gamma_(n+1) (n - 1 additions and one rounding per product; Higham, Accuracy and Stability,
    3.1), so the two sums differ by at most 2 g |a|'|z| (cv) and 2 g nn (nn); dist = (cv - b) / nn adds two roundings to each, the
    product and the subtraction one each.  To first order, with u = 2^-53 and everything evaluated at the values of this column:
        |d cv|   <= 2 g |a|'|z| + |a|'|d z|                             (|d z|: what the column already carries from earlier half-spaces)
        |d dist| <= (|d cv| + 2 u |cv - b|) / nn + |dist| (2 g + 2 u)
        |d z_r|  <= |a_r| |d dist| + u |dist a_r| + u |z_r'|
    A factor 2 covers the second-order terms (g < 2^-48 here).  with_dcv: also the bound on |d cv| at every half-space, projected or
    not -- two evaluations can decide cv > b differently only where the cv of either lies within it of b."""
    u = 2.0 ** -53
    n = len(z)
    g = (n + 1) * u / (1.0 - (n + 1) * u)
    z = np.array(z, dtype=np.float64)
    dz = np.zeros(n)
    dcvs = np.zeros(len(b))
    for k in range(len(b)):
        a = np.asarray(A[k], dtype=np.float64)
        absdot, nn, cv = float(np.abs(a) @ np.abs(z)), float(a @ a), float(a @ z)
        dcv = 2 * g * absdot + float(np.abs(a) @ dz)
        dcvs[k] = 2.0 * dcv
        if not viol[k]:
            continue
        dist = (cv - b[k]) / nn
        ddist = (dcv + 2 * u * abs(cv - b[k])) / nn + abs(dist) * (2 * g + 2 * u)
        znew = z - dist * a
        dz = dz + np.abs(a) * ddist + u * np.abs(dist * a) + u * np.abs(znew)
        z = znew
    return (2.0 * dz, dcvs) if with_dcv else 2.0 * dz


def project_forced(z, A, b, viol):
    """the model's arithmetic along a GIVEN branch pattern -> (column, the a_k'z each half-space saw)"""
    z = [float(v) for v in z]
    cvs = []
    for k in range(len(b)):
        a = [float(v) for v in A[k]]
        cv = nn = 0.0
        for r in range(len(z)):
            cv = cv + a[r] * z[r]
            nn = nn + a[r] * a[r]
        cvs.append(cv)
        if viol[k]:
            dist = (cv - float(b[k])) / nn
            z = [zr - dist * ar for zr, ar in zip(z, a)]
    return np.array(z), np.array(cvs)


# ---- a scalar restatement for the generators (plain Python floats: IEEE doubles, nothing fused) ------------------------------------------
def _facts1(z, A, b):
    z = [float(v) for v in z]
    z0 = list(z)
    viol, cvs, cv0 = [], [], []
    for k in range(len(b)):
        a = [float(v) for v in A[k]]
        cv = c0 = nn = 0.0
        for r in range(len(z)):
            cv = cv + a[r] * z[r]
            c0 = c0 + a[r] * z0[r]
            nn = nn + a[r] * a[r]
        hit = cv > b[k]
        if hit:
            dist = (cv - b[k]) / nn if nn != 0.0 else math.copysign(math.inf, cv - b[k]) if cv != b[k] else math.nan
            z = [zr - dist * ar for zr, ar in zip(z, a)]
        viol.append(hit), cvs.append(cv), cv0.append(c0)
    return z, viol, cvs, cv0


CLASSES = ("slack", "one_violated", "all_violated", "on_plane", "ulp_above", "ulp_below", "chain_on", "chain_off", "repeat", "negzero",
           "nn_overflow", "nn_underflow", "null_row_nan", "nan_in", "inf_in")
NONFINITE = ("nn_overflow", "nn_underflow", "null_row_nan", "nan_in", "inf_in")
# classes that are a property of the half-space set, not of the column: every column under such a set is a member
SET_CLASSES = {"axis": "axis", "sparse": "sparse", "scaled": "scaled", "full4": "pad", "k5": "pad", "sparse_null": "null_row_inert"}


def _rows(A):
    return [k for k in range(len(A)) if np.any(np.asarray(A[k]) != 0.0)]


def _dups(A, b):
    return [(i, j) for i in range(len(b)) for j in range(i + 1, len(b)) if np.array_equal(A[i], A[j]) and b[i] == b[j] and np.any(A[i] != 0)]


def member(cls, s, A, b):
    """the class's defining property of the column s = x + gl, on the model's own intermediate values"""
    s = np.asarray(s, dtype=np.float64)
    _, viol, cv, cv0 = _facts1(s, A, b)
    K = len(b)
    fin = bool(np.all(np.isfinite(s)))
    nn = [float(np.sum(np.asarray(A[k]) * np.asarray(A[k]))) for k in range(K)]
    with np.errstate(all="ignore"):
        if cls == "slack":
            return fin and not any(viol) and all(b[k] - cv[k] > 1e-6 * (abs(b[k]) + abs(cv[k])) or not np.any(A[k]) for k in range(K))
        if cls == "one_violated":
            return fin and sum(viol) == 1
        if cls == "all_violated":
            return fin and K >= 1 and all(viol)
        if cls == "on_plane":
            return fin and any(cv[k] == b[k] and np.any(A[k]) for k in range(K))       # (strict test: this half-space does not move it)
        if cls == "ulp_above":
            return fin and any(b[k] == np.nextafter(cv[k], -np.inf) for k in range(K))
        if cls == "ulp_below":
            return fin and any(b[k] == np.nextafter(cv[k], np.inf) and np.any(A[k]) for k in range(K))
        if cls == "chain_on":
            return fin and any(viol[k] and cv0[k] <= b[k] and any(viol[:k]) for k in range(K))
        if cls == "chain_off":
            return fin and any(not viol[k] and cv0[k] > b[k] and any(viol[:k]) for k in range(K))
        if cls == "repeat":
            return fin and any(viol[i] for i, _ in _dups(A, b))
        if cls == "negzero":                         # (of the DUAL: -0.0 entries where x is zero; the column itself has +0 there)
            return fin and bool(np.any(s == 0))
        if cls == "nn_overflow":
            return fin and any(viol[k] and math.isinf(nn[k]) and math.isfinite(cv[k]) for k in range(K))
        if cls == "nn_underflow":
            return fin and any(viol[k] and nn[k] == 0.0 and np.any(A[k]) and math.isfinite(cv[k]) for k in range(K))
        if cls == "null_row_nan":
            return fin and any(viol[k] and not np.any(A[k]) for k in range(K))
        if cls == "nan_in":
            return bool(np.any(np.isnan(s)))
        if cls == "inf_in":
            return bool(np.any(np.isinf(s))) and not np.any(np.isnan(s))
    raise KeyError(cls)


def feasible(cls, A, b):
    """can a column of this family be a member at all"""
    A = np.asarray(A, dtype=np.float64)
    K, rows, dup = len(b), _rows(A), _dups(A, b)
    with np.errstate(all="ignore"):
        nn = np.sum(A * A, axis=-1) if K else np.zeros(0)
    tame = K > 0 and bool(np.all(np.isfinite(nn))) and bool(np.all(nn[rows] > 1e-200)) if K else False
    if any(b[k] < 0 and k not in rows for k in range(K)):            # 0 > b: such a row projects every column, onto NaN
        return cls == "null_row_nan"
    if cls == "slack":
        return K == 0 or tame or not rows
    if K == 0 or not rows:
        return cls == "null_row_nan" and any(b[k] < 0 for k in range(K)) or (cls in ("negzero", "nan_in", "inf_in"))
    if cls in ("nan_in", "inf_in"):
        return tame
    if cls == "nn_overflow":
        return bool(np.any(np.isinf(nn)))
    if cls == "nn_underflow":
        return bool(np.any(nn[rows] == 0.0))
    if cls == "null_row_nan":
        return any(b[k] < 0 and k not in rows for k in range(K))
    if not tame:
        return False
    if cls == "all_violated":
        return len(rows) == K and not dup and K <= A.shape[1] and np.linalg.matrix_rank(A) == K
    if cls in ("chain_on", "chain_off"):
        sign = -1.0 if cls == "chain_on" else 1.0
        return any(sign * float(A[i] @ A[j]) > 1e-3 * math.sqrt(nn[i] * nn[j]) and not np.array_equal(A[i], A[j]) for i in rows for j in rows if i < j)
    if cls == "repeat":
        return bool(dup)
    return True


def classes_for(A, b, finite=True):
    return tuple(c for c in CLASSES if (c not in NONFINITE or not finite) and feasible(c, A, b))


# ---- candidates
def _interior(rng, A, b, scale, margin=0.2):
    """a column that satisfies every half-space with a margin (cyclic projections onto the shrunken half-spaces)"""
    A = np.asarray(A, dtype=np.float64)
    n = A.shape[1]
    z = rng.normal(0.0, 1.0, n) * scale
    rows = _rows(A)
    for _ in range(200):
        moved = False
        for k in rows:
            a = A[k]
            nn = float(a @ a)
            m = margin * rng.uniform(0.5, 1.5) * (math.sqrt(nn) * scale + abs(b[k]))
            if a @ z > b[k] - m:
                z = z - ((a @ z - (b[k] - 2.0 * m)) / nn) * a
                moved = True
        if not moved:
            return z
    return z


def _cv_at(s, A, b, k):
    return _facts1(s, A, b)[2][k]


def _ordered(v):
    i = np.float64(v).view(np.int64)
    return int(i) if i >= 0 else int(-(i & np.int64(0x7FFFFFFFFFFFFFFF)))


def _from_ordered(i):
    return float(np.int64(i).view(np.float64)) if i >= 0 else -float(np.int64(-i).view(np.float64))


def _boundary(rng, A, b, x, scale, k, target):
    """gl such that the model's a_k'(x + gl) at half-space k is exactly target(b_k): bisection on one entry of gl (cv is a monotone
    step function of it); None when the steps skip the target"""
    A = np.asarray(A, dtype=np.float64)
    a = A[k]
    z = _interior(rng, A, b, scale)
    # the last nonzero row carries the sum: the rows before it are shrunk until their partial sum is below |b| / 4, so the final addition
    # rounds on b's own grid and every double near b is a value the sum can take (a partial sum larger than b would skip half of them)
    r = int(np.flatnonzero(a != 0.0)[-1])
    part = float(a[:r] @ z[:r])
    if part != 0.0:
        z[:r] = z[:r] * min(1.0, abs(b[k]) / (4.0 * abs(part)))
    z[r] = (b[k] - float(a[:r] @ z[:r])) / a[r]
    gl = z - x
    want = target(b[k])
    up = a[r] > 0

    def cv(i):
        g = gl.copy()
        g[r] = _from_ordered(i)
        return _cv_at(x + g, A, b, k)
    c = _ordered(gl[r])
    span = 1 << 40
    lo, hi = c - span, c + span
    if not up:
        f = lambda i: cv(-i)                                          # noqa: E731
        lo, hi = -hi, -lo
    else:
        f = cv
    if not (f(lo) < want <= f(hi)):
        return None
    while hi - lo > 1:                                                # the smallest i with f(i) >= want
        mid = (lo + hi) // 2
        if f(mid) >= want:
            hi = mid
        else:
            lo = mid
    if f(hi) != want:
        return None
    gl[r] = _from_ordered(hi if up else -hi)
    return gl


def _candidate(rng, cls, A, b, x, scale, slot=None):
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    K, n = A.shape
    rows = _rows(A)
    z = _interior(rng, A, b, scale) if K and cls not in ("nn_overflow", "nn_underflow") else rng.normal(0.0, 1.0, n) * scale
    nn = np.sum(A * A, axis=-1) if cls not in ("nn_overflow", "nn_underflow") else None
    if cls == "slack" or cls == "null_row_nan":
        pass
    elif cls in ("one_violated", "repeat"):
        ks = rows if cls == "one_violated" else [i for i, _ in _dups(A, b)]
        k = int(rng.choice(ks)) if slot is None else ks[slot % len(ks)]       # (slot: the violated half-space runs over every slot)
        over = rng.uniform(0.05, 0.5) * (scale * math.sqrt(nn[k]) + abs(b[k]))
        d = np.linalg.pinv(A[rows])[:, rows.index(k)] if cls == "one_violated" else A[k] / nn[k]    # a_k'd = 1, a_j'd = 0 for the other rows
        z = z + (b[k] - A[k] @ z + over) * (d if abs(A[k] @ d - 1.0) < 1e-6 else A[k] / nn[k])
    elif cls == "all_violated":
        over = np.sort(rng.uniform(0.1, 1.0, K))[::-1] * np.arange(1, K + 1) * (np.sqrt(nn) * scale + np.abs(b))
        w = rng.normal(0.0, 1.0, n) * scale
        z = w + np.linalg.lstsq(A, b + over - A @ w, rcond=None)[0]
    elif cls in ("on_plane", "ulp_above", "ulp_below"):
        k = int(rng.choice(rows))
        target = {"on_plane": lambda v: v, "ulp_above": lambda v: float(np.nextafter(v, np.inf)), "ulp_below": lambda v: float(np.nextafter(v, -np.inf))}[cls]
        return _boundary(rng, A, b, x, scale, k, target)
    elif cls in ("chain_on", "chain_off"):
        sign = -1.0 if cls == "chain_on" else 1.0
        pairs = [(i, j) for i in rows for j in rows if i < j and sign * float(A[i] @ A[j]) > 1e-3 * math.sqrt(nn[i] * nn[j]) and not np.array_equal(A[i], A[j])]
        i, j = pairs[int(rng.integers(len(pairs)))]
        m = rng.uniform(0.1, 0.5) * (math.sqrt(nn[i]) * scale + abs(b[i]))
        eps = rng.uniform(0.02, 0.1) * (math.sqrt(nn[j]) * scale + abs(b[j]))
        aij = float(A[i] @ A[j])
        want = np.array([b[i] - m, b[j] - sign * eps - (m / nn[i]) * aij])      # w: inside i by m; after the projection onto i, j is off by -sign eps
        M = np.stack([A[i], A[j]])
        w = z + np.linalg.lstsq(M, want - M @ z, rcond=None)[0]
        s_ = m / nn[i] + 3.0 * eps / abs(aij)
        z = w + s_ * A[i]
    elif cls == "negzero":
        free = np.flatnonzero(x == 0)                                  # x + gl is +0 there whatever the dual's zero: the dual carries the sign
        z[free[rng.random(len(free)) < 0.4]] = 0.0
        z[int(rng.choice(free))] = 0.0
        return np.where((z == 0) & (x == 0), -0.0, z - x)
    elif cls == "nn_overflow":
        z = rng.normal(0.0, 1.0, n) * scale + 0.0
        k = int(rng.integers(K))
        z = z + (abs(b[k]) + 1.0) * scale * np.sign(A[k])
    elif cls == "nn_underflow":
        k = int(rng.integers(K))
        z = z + (abs(b[k]) + 1.0) * scale * np.sign(A[k])
    elif cls in ("nan_in", "inf_in"):
        z[int(rng.integers(n))] = np.nan if cls == "nan_in" else rng.choice([np.inf, -np.inf])
    return z - x


def draw(rng, cls, A, b, x=None, scale=1.0, tries=400, slot=None):
    """gl (n,) with x + gl a member of `cls` for the family (A (K, n), b (K)); x: the column's x (default +0)"""
    A = np.asarray(A, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    x = np.zeros(A.shape[1]) if x is None else np.asarray(x, dtype=np.float64)
    for t in range(tries):
        with np.errstate(all="ignore"):
            gl = _candidate(rng, cls, A, b, x, scale, None if slot is None else slot + t // 50)    # (a slot that cannot be had alone: the next)
            if gl is not None and (member(cls, x + gl, A, b) if cls != "negzero" else bool(np.any((gl == 0) & np.signbit(gl)) and np.all(np.isfinite(gl)))):
                return gl
    raise AssertionError(("class ran dry", cls, A.tolist(), b.tolist()))


BOUNDARY = ("on_plane", "ulp_above", "ulp_below")


def draw_ladder(rng, ladder, at, A, b, x=None, scale=1.0, slot=None):
    """draw() of class ladder[at % len]; a boundary class whose value the sum cannot take for this (a, b) -- fl(1.5 z) skips every third
    double -- hands over to the next class of the ladder -> (gl, the class drawn)"""
    for step in range(len(ladder)):
        c = ladder[(at + step) % len(ladder)]
        if c == "negzero" and x is not None and np.all(np.asarray(x) != 0):
            continue
        try:
            return draw(rng, c, A, b, x, scale, tries=16 if c in BOUNDARY else 400, slot=slot), c
        except AssertionError:
            if c not in BOUNDARY:
                raise
    raise AssertionError(("ladder ran dry", ladder))


# ---- named half-space sets ------------------------------------------------------------------------------------------------------------
def make_sets(name, nx, nu, N, families=("sx", "su", "tx", "tu"), counts=None):
    """the configuration entries (linear, tv_linear, the four switches) of a named set for a shape, and `scale`: the size of a column per
    family.  families: which switches are on; counts: (static state, static input, tv state, tv input) half-spaces per knot, overriding
    the set's own"""
    rng = np.random.default_rng([sum(map(ord, name)), nx, nu, N])
    own = {"plain": (3, 2, 2, 1), "dyadic": (3, 2, 2, 1), "axis": (1, 1, 1, 1), "full4": (4, 1, 1, 4), "k5": (5, 2, 2, 1), "scaled": (3, 2, 2, 1),
           "sparse": (3, 2, 2, 1), "sparse_null": (3, 2, 2, 1), "repeat": (3, 2, 3, 2), "huge": (2, 1, 1, 1), "tiny": (2, 1, 1, 1), "null": (2, 2, 2, 1)}[name]
    ks, ki, kts, kti = counts or own
    scale = dict(sx=1.0, su=1.0, tx=1.0, tu=1.0)

    def fam(rows, n, tag):
        if name == "dyadic":
            A, b = rng.integers(-8, 9, (rows, n)) / 8.0, rng.choice([-6, -5, -4, -3, -2, -1, 1, 2, 3, 4, 5, 6], rows) / 4.0
            A[np.arange(rows), rng.integers(0, n, rows)] = 1.0
        elif name == "axis":
            A = np.zeros((rows, n))
            if tag[1] == "x":
                A[:, min(2, n - 1)] = 1.0
                b = 3.0 - 0.125 * np.arange(rows)
            else:
                A[:] = 1.0
                b = 6.0 + 0.25 * np.arange(rows)
        else:
            A, b = rng.normal(0.0, 1.0, (rows, n)), rng.normal(0.0, 0.3, rows)
        if name in ("sparse", "sparse_null"):
            A = np.where(rng.random((rows, n)) < 0.35, 0.0, A)
            A = np.where((A == 0) & (rng.random((rows, n)) < 0.5), -0.0, A)
            A[np.arange(rows), rng.integers(0, n, rows)] = 1.5
        if name == "scaled":
            e = 60 if tag[0] == "s" else -60
            A = A * 2.0 ** e
            scale[tag] = 2.0 ** -e
        if name == "huge":
            A, scale[tag] = A * 1e160, 1e-160
        if name == "tiny":
            A, scale[tag] = A * 1e-170, 1e170
        return A, b
    per = {}
    for tag, k, n, knots in (("sx", ks, nx, 1), ("su", ki, nu, 1), ("tx", kts, nx, N), ("tu", kti, nu, N - 1)):
        A, b = fam(k * knots, n, tag)
        A, b = A.reshape(knots, k, n), b.reshape(knots, k)
        if name == "repeat" and k >= 3:
            A[:, 2], b[:, 2] = A[:, 0], b[:, 0]
        if name == "sparse_null" and k >= 2:
            A[:, 1], b[:, 1] = 0.0, np.where(np.arange(knots) % 2 == 0, 0.0, 0.25)
        if name == "null" and k >= 2:
            A[:, 0], b[:, 0] = 0.0, 0.5
            A[:, 1], b[:, 1] = 0.0, -0.5
        per[tag] = (A, b)
    sets = dict(linear=(per["sx"][0][0], per["sx"][1][0], per["su"][0][0], per["su"][1][0]),
                tv_linear=(per["tx"][0].reshape(-1, nx), per["tx"][1].T.copy(), per["tu"][0].reshape(-1, nu), per["tu"][1].T.copy()),
                scale=scale, name=name)
    for tag, flag in FLAG.items():
        sets[flag] = int(tag in families)
    return sets


def config(sets, nx, nu, N, max_iter, tol=0.0, **kw):
    """oracle/scenarios.py's config dictionary: boxes and cones off, the set's families on"""
    cfg = dict(max_iter=int(max_iter), abs_pri_tol=tol, abs_dua_tol=tol, check_termination=1, en_state_bound=0, en_input_bound=0,
               en_state_soc=0, en_input_soc=0, state_cone=None, input_cone=None,
               x_min=np.full((nx, N), -1e17), x_max=np.full((nx, N), 1e17), u_min=np.full((nu, N - 1), -1e17), u_max=np.full((nu, N - 1), 1e17),
               linear=sets["linear"] if sets["en_state_linear"] or sets["en_input_linear"] else None,
               tv_linear=sets["tv_linear"] if sets["en_tv_state_linear"] or sets["en_tv_input_linear"] else None)
    for flag in FLAG.values():
        cfg[flag] = sets[flag]
    cfg.update(kw)
    return cfg


def family(nx, nu, N, seed=0):
    """the pure-map family: A = 0, B = 0, f = 0, random diagonal Q, R -- x is x0 at knot 0 and +0 at every later knot in every iteration,
    so the state columns of a solve are iterate(gl, x, ...)"""
    rng = np.random.default_rng(seed + 1000 * nx + 10 * nu + N)
    return dict(nx=nx, nu=nu, N=N, rho=1.0, A=np.zeros((nx, nx)), B=np.zeros((nx, nu)), f=np.zeros(nx), Q=rng.uniform(1.0, 10.0, nx), R=rng.uniform(0.1, 1.0, nu))


@functools.lru_cache(maxsize=None)
def _directed(name, nx, nu, N, families, counts, B, seed, finite, with_x0):
    sets = make_sets(name, nx, nu, N, families, counts)
    rng = np.random.default_rng([seed, sum(map(ord, name)), nx, nu, N, int(finite)])
    unit = all(v == 1.0 for v in sets["scale"].values())
    x0 = np.round(rng.normal(0.0, 0.5, (B, nx)) * 8.0) / 8.0 if (with_x0 and unit) else np.zeros((B, nx))
    x0[::3] = 0.0
    out, labels = {}, {}
    for f_i, (v, g, src, fam) in enumerate(FAMILIES):
        if src != "x":
            continue
        t = tables(sets, fam, N, nx, nu)
        if t is None:
            continue
        A, b = (np.broadcast_to(t[0], (N,) + t[0].shape[-2:]), np.broadcast_to(t[1], (N,) + t[1].shape[-1:]))
        gl, lab = np.zeros((B, nx, N)), np.zeros((B, N), dtype=np.int8)
        ladders = [classes_for(A[i], b[i], finite) for i in range(N)]
        for bi in range(B):
            for i in range(N):
                cl = ladders[i]
                x = x0[bi] if i == 0 else np.zeros(nx)
                gl[bi, :, i], c = draw_ladder(rng, cl, i + bi + 3 * f_i, A[i], b[i], x, sets["scale"][fam], slot=(bi * N + i) // len(cl))
                lab[bi, i] = CLASSES.index(c)
        out[g], labels[g] = gl, lab
    return sets, x0, out, labels


def directed_batch(name, nx, nu, N, families=("sx", "su", "tx", "tu"), counts=None, B=64, seed=0, finite=True, with_x0=True):
    """the directed batch of one (set, shape): warm gl / gl_tv (B, nx, N) whose columns x + gl walk the class ladder of their family
    and knot -- instance b shifts it by b, so every (lane, pass) position of the column layout (lane t takes columns S0 + t, S0 + t +
    LPI, ...) meets every class -- x0 (B, nx) (nonzero: knot 0 is P(x0 + gl); every third instance keeps 0) and the labels.  The
    time-varying sets differ at every knot, so a table shifted by one knot cannot pass.  (Cached: do not write into the arrays.)"""
    return _directed(name, nx, nu, N, tuple(families), None if counts is None else tuple(counts), B, seed, finite, with_x0)


def class_counts(labels):
    return {CLASSES[k]: int(n) for k, n in enumerate(np.bincount(np.asarray(labels).ravel(), minlength=len(CLASSES))) if n}


def pure_map_want(sets, nx, nu, N, x0, duals, iters):
    """the state fields of `iters` iterations of the pure-map family from warm gl / gl_tv: {vlnew, gl, vlnew_tv, gl_tv} (B, nx, N)"""
    B = x0.shape[0]
    x = np.zeros((B, N, nx))
    x[:, 0] = x0
    want = {}
    for v, g, src, fam in FAMILIES:
        t = tables(sets, fam, N, nx, nu)
        if src != "x" or t is None:
            continue
        pv, pg = iterate(np.asarray(duals[g]).transpose(0, 2, 1), x, t[0], t[1], iters)
        want[v], want[g] = pv.transpose(0, 2, 1), pg.transpose(0, 2, 1)
    return want


# ---- the fixture: finite directed items and the real reference's answers (oracle/gen_golden.py --halfspace-edges) -----------------------
FIXTURE_FORMS = (("plain", 12, 4, 10), ("dyadic", 6, 3, 10), ("axis", 12, 4, 10), ("full4", 12, 4, 10), ("k5", 12, 4, 10), ("scaled", 6, 3, 10),
                 ("sparse", 5, 3, 7), ("sparse_null", 6, 3, 10), ("repeat", 6, 3, 10), ("plain", 4, 2, 10), ("plain", 3, 3, 8))


def fixture_items(B=5):
    """[(set name, nx, nu, N, sets, duals {gl, yl, gl_tv, yl_tv} (B, rows, knots), labels)]: every finite class on every knot of both
    state families (the directed batch) and of both input families (the same ladder, drawn here); x = u = 0 in the fixture, so the
    columns are 0 + dual"""
    items = []
    for name, nx, nu, N in FIXTURE_FORMS:
        sets, _, duals, labels = directed_batch(name, nx, nu, N, B=B, seed=5, with_x0=False)
        duals, labels = dict(duals), dict(labels)
        rng = np.random.default_rng([9, sum(map(ord, name)), nx, nu, N])
        for f_i, (v, g, src, fam) in enumerate(FAMILIES):
            if src != "u":
                continue
            A, b = tables(sets, fam, N, nx, nu)
            A, b = np.broadcast_to(A, (N - 1,) + A.shape[-2:]), np.broadcast_to(b, (N - 1,) + b.shape[-1:])
            yl, lab = np.zeros((B, nu, N - 1)), np.zeros((B, N - 1), dtype=np.int8)
            for bi in range(B):
                for i in range(N - 1):
                    cl = classes_for(A[i], b[i])
                    yl[bi, :, i], c = draw_ladder(rng, cl, i + bi * 5 + f_i, A[i], b[i], None, sets["scale"][fam])
                    lab[bi, i] = CLASSES.index(c)
            duals[g], labels[g] = yl, lab
        items.append((name, nx, nu, N, sets, duals, labels))
    return items


# ---- what the CPU and the GPU test module share ---------------------------------------------------------------------------------------
ALL = ("sx", "su", "tx", "tu")
B_DIRECTED = 32
# name: shape, set, families that are on, counts (None: the set's own), options of the launch, kernel_path(), a C++ name prefix that
# tm.jit_used() must list (None: compiled in, or nothing to say), state cone on as well
CASES = {
    "planes_12_4_10_lin3": dict(dims=(12, 4, 10), set="plain", fams=ALL, path="regs"),
    "planes_12_4_10_lin1": dict(dims=(12, 4, 10), set="full4", fams=("sx", "su"), path="regs"),
    "planes_12_4_10_lin2": dict(dims=(12, 4, 10), set="repeat", fams=("tx", "tu"), path="regs"),
    "planes_12_4_10_axis": dict(dims=(12, 4, 10), set="axis", fams=ALL, path="regs"),
    "planes_6_3_10_cone": dict(dims=(6, 3, 10), set="dyadic", fams=ALL, path="regs", cone=True),
    "planes_6_3_10_scaled": dict(dims=(6, 3, 10), set="scaled", fams=ALL, path="regs"),
    "planes_6_3_10_null": dict(dims=(6, 3, 10), set="sparse_null", fams=ALL, path="regs"),
    "planes_12_4_10_k5": dict(dims=(12, 4, 10), set="k5", fams=ALL, path="regs", used="tinympc_amd::admm_solve_kernel<12,4,10,"),
    "jit_5_3_7": dict(dims=(5, 3, 7), set="sparse", fams=ALL, path="jit"),
    "tile_20_4_10": dict(dims=(20, 4, 10), set="plain", fams=ALL, path="tile", used="tinympc_amd::admm_tile_kernel<20,4,10,2,"),
    "tile_8_2_50": dict(dims=(8, 2, 50), set="plain", fams=("sx", "su"), path=("tile", "tile-jit")),
    "tile_jit_16_8_6": dict(dims=(16, 8, 6), set="plain", fams=ALL, path="tile-jit"),
    "tile_20_4_10_sparse": dict(dims=(20, 4, 10), set="sparse_null", fams=ALL, path="tile", used="tinympc_amd::admm_tile_kernel<20,4,10,2,"),
    "tile_20_4_10_scaled": dict(dims=(20, 4, 10), set="scaled", fams=ALL, path="tile", used="tinympc_amd::admm_tile_kernel<20,4,10,2,"),
    "tile_20_4_10_repeat": dict(dims=(20, 4, 10), set="repeat", fams=ALL, path="tile", used="tinympc_amd::admm_tile_kernel<20,4,10,2,"),
    "cover_12_4_10_sparse": dict(dims=(12, 4, 10), set="sparse_null", fams=ALL, path="cover", options={"force_general": 1}),
    "cover_12_4_10_scaled": dict(dims=(12, 4, 10), set="scaled", fams=ALL, path="cover", options={"force_general": 1}),
    "cover_12_4_10_repeat": dict(dims=(12, 4, 10), set="repeat", fams=ALL, path="cover", options={"force_general": 1}),
    "cover_12_4_10_axis": dict(dims=(12, 4, 10), set="axis", fams=ALL, path="cover", options={"force_general": 1}),
    "cover_12_4_10": dict(dims=(12, 4, 10), set="plain", fams=ALL, path="cover", options={"force_general": 1}),
    "cover_20_4_10": dict(dims=(20, 4, 10), set="plain", fams=ALL, path="cover", options={"force_general": 1}),
    # the per-knot register form: by solve_kernel_lin_lds the planes of (4,2,30) with time-varying tables need 67 712 B > 65 024 B (the
    # one-row half-space variants are instantiated without UB; tests/test_halfspace_ref_cpu.py pins the row); the kernel choice (csrc/kernel_path.hpp,
    # tile:planes_do_not_fit_one_row) normally gives the tile kernel the shape, no_tile / debug each rule the tile kernel out
    # ((4,2,30) is a compiled-in shape: kernel_path() says "regs"; its half-space variants are run-time instantiated all the same)
    "perknot_4_2_30_no_tile": dict(dims=(4, 2, 30), set="plain", fams=("tx", "tu"), path="regs", options={"no_tile": 1}, used="tinympc_amd::admm_solve_kernel<4,2,30,"),
    "perknot_4_2_30_sparse": dict(dims=(4, 2, 30), set="sparse_null", fams=("tx", "tu"), path="regs", options={"no_tile": 1}, used="tinympc_amd::admm_solve_kernel<4,2,30,"),
    "perknot_4_2_30_scaled": dict(dims=(4, 2, 30), set="scaled", fams=("tx", "tu"), path="regs", options={"no_tile": 1}, used="tinympc_amd::admm_solve_kernel<4,2,30,"),
    "perknot_4_2_30_repeat": dict(dims=(4, 2, 30), set="repeat", fams=("tx", "tu"), path="regs", options={"no_tile": 1}, used="tinympc_amd::admm_solve_kernel<4,2,30,"),
    "perknot_4_2_30_debug": dict(dims=(4, 2, 30), set="plain", fams=("tx", "tu"), path="regs", options={"debug": 1}, used="tinympc_amd::admm_solve_kernel<4,2,30,"),
}
# (c) families and counts, each on one planes form and on the coverage kernel
for _name, _fams, _counts in (("input_only", ("su", "tu"), None), ("state_only", ("sx", "tx"), None), ("count0", ALL, (2, 0, 0, 1)),
                              ("k4", ("sx", "su"), (4, 4, 0, 0)), ("k8", ("sx", "su"), (8, 2, 0, 0)), ("k9", ("sx", "su"), (9, 3, 0, 0))):
    CASES["planes_12_4_10_" + _name] = dict(dims=(12, 4, 10), set="plain", fams=_fams, counts=_counts, path="regs")
    CASES["cover_12_4_10_" + _name] = dict(dims=(12, 4, 10), set="plain", fams=_fams, counts=_counts, path="cover", options={"force_general": 1})
CONE = ([0], [3], [0.5])


def case_setup(name, max_iter, seed=0):
    """-> (problem, config, sets, x0, warm duals, labels) of a CASES entry: the pure-map family with the case's directed batch"""
    c = CASES[name]
    nx, nu, N = c["dims"]
    sets, x0, duals, labels = directed_batch(c["set"], nx, nu, N, c["fams"], c.get("counts"), B=B_DIRECTED, seed=seed)
    cfg = config(sets, nx, nu, N, max_iter)
    rng = np.random.default_rng([seed, 77, nx, nu, N])
    duals = dict(duals)                          # the input families: random warm duals, checked through the own-output identity
    for v, g, src, fam in FAMILIES:
        if src == "u" and sets[FLAG[fam]]:
            duals[g] = rng.normal(0.0, 2.0, (B_DIRECTED, nu, N - 1)) * sets["scale"][fam]
    if c.get("cone"):
        cfg.update(en_state_soc=1, state_cone=CONE)
    return family(nx, nu, N), cfg, sets, x0, duals, labels


def oracle_solve(prob, cfg, x0, warm, fields):
    """one oracle solve per instance from an otherwise zero workspace -> {field: (B, rows, knots)}, iterations"""
    import scenarios as sc                       # (oracle/: on the path of every test module)
    from cpu_solvers import OracleSolver
    o = sc.make_solver(OracleSolver, prob, cfg)
    B = x0.shape[0]
    zero = {k: np.zeros(o[k].shape) for k in o.STATE_FIELDS + o.LINEAR_FIELDS + ("Xref", "Uref")}
    out = {k: np.zeros((B,) + o[k].shape) for k in fields}
    it = np.zeros(B, dtype=int)
    for b in range(B):
        o.restore(zero)
        for k, v in warm.items():
            o[k] = v[b]
        o["x"][:, 0] = x0[b]
        o.solve()
        for k in fields:
            out[k][b] = o[k]
        it[b] = int(o.get("sol_iter"))
    o.close()
    return out, it


def sets_of(cfg):
    """the half-space entries of a scenarios.py config as a `sets` dictionary"""
    return dict(linear=cfg.get("linear"), tv_linear=cfg.get("tv_linear"), **{flag: int(cfg.get(flag, 0)) for flag in FLAG.values()})


def sweep_linear_suite(nx, nu, N, B=4, tv=True, seed=41, static=True):
    """a sweep problem (random stable dynamics) with static (and time-varying) half-spaces, boxes off, and a random warm workspace whose
    duals push most columns over their half-spaces: the tile forms on real dynamics"""
    import scenarios as sc
    prob, _ = sc.random_problem(nx, nu, N)
    rng = np.random.default_rng(seed)
    kw = dict(max_iter=1, en_state_bound=0, en_input_bound=0)
    if static:
        kw.update(en_state_linear=1, en_input_linear=1,
                  linear=(rng.normal(0, 1, (3, nx)), rng.normal(0, 0.3, 3), rng.normal(0, 1, (2, nu)), rng.normal(0, 0.3, 2)))
    if tv:
        kw.update(en_tv_state_linear=1, en_tv_input_linear=1,
                  tv_linear=(rng.normal(0, 1, (2 * N, nx)), rng.normal(0, 0.3, (2, N)), rng.normal(0, 1, (N - 1, nu)), rng.normal(0, 0.3, (1, N - 1))))
    cases = sc.zero_cases(prob, B)
    for k, v in cases.items():
        cases[k] = rng.normal(0.0, 0.3, v.shape)
    return dict(problem=prob, config=sc.default_config(prob, **kw), cases=cases)


def push_over(suite, amount=1.5):
    """adds to the warm half-space duals of a suite `amount` times the sum of the unit normals of their column's half-spaces, so that
    most columns x + gl lie outside at least one of them (the tests assert on the model that at least half do)"""
    cfg, cases = suite["config"], suite["cases"]
    nx, nu, N = suite["problem"]["nx"], suite["problem"]["nu"], suite["problem"]["N"]
    sets = sets_of(cfg)
    for v, g, src, fam in FAMILIES:
        t = tables(sets, fam, N, nx, nu)
        if t is None or t[0].shape[-2] == 0:
            continue
        A = t[0]
        unit = A / np.sqrt(np.sum(A * A, axis=-1, keepdims=True))
        push = amount * unit.sum(axis=-2)                                   # (n,) | (knots, n)
        cases[g] = cases[g] + (push.T if push.ndim == 2 else push[:, None])[None]
    return suite


def hyperplane(z, a, b):
    """project_hyperplane (admm.cpp:70-73) as the oracle's project_halfspace forms it, without the violation test"""
    z, a = np.asarray(z, dtype=np.float64), np.asarray(a, dtype=np.float64)
    with np.errstate(all="ignore"):
        cv = nn = np.float64(0.0)
        for r in range(len(z)):
            cv = cv + a[r] * z[r]
            nn = nn + a[r] * a[r]
        dist = (cv - b) / nn
        return np.array([z[r] - dist * a[r] for r in range(len(z))])


NONFINITE_SETS = (("plain", 6, 3, 10), ("null", 6, 3, 10), ("huge", 6, 3, 10), ("tiny", 6, 3, 10), ("plain", 12, 4, 10))


@functools.lru_cache(maxsize=None)
def nonfinite_batch(name, nx, nu, N, B=6, seed=3):
    """every class, the non-finite ones included, on every knot of all four families of a set (x = u = 0) -> sets, duals, labels"""
    sets = make_sets(name, nx, nu, N)
    rng = np.random.default_rng([seed, sum(map(ord, name)), nx])
    duals, labels = {}, {}
    for f_i, (v, g, src, fam) in enumerate(FAMILIES):
        A, b = tables(sets, fam, N, nx, nu)
        knots, n = (N, nx) if src == "x" else (N - 1, nu)
        A, b = np.broadcast_to(A, (knots,) + A.shape[-2:]), np.broadcast_to(b, (knots,) + b.shape[-1:])
        d, lab = np.zeros((B, n, knots)), np.zeros((B, knots), dtype=np.int8)
        for bi in range(B):
            for i in range(knots):
                cl = classes_for(A[i], b[i], finite=False)
                d[bi, :, i], c = draw_ladder(rng, cl[::-1], i + 2 * bi + f_i, A[i], b[i], None, sets["scale"][fam])   # (the non-finite classes first)
                lab[bi, i] = CLASSES.index(c)
        duals[g], labels[g] = d, lab
    return sets, duals, labels


# name: (maker, kernel_path() of a plain launch): random_linear_suite-like problems on real dynamics, boxes off, warm duals pushed over their half-spaces
IDENTITY_SUITES = {
    "quad_all": (lambda sc: sc.random_linear_suite("quadrotor_20hz", B=4, seed=31, box=False), "regs"),
    "rocket_soc": (lambda sc: sc.random_linear_suite("rocket_landing_20hz", B=4, seed=32, soc=True, box=False), "regs"),
    "cartpole_tv": (lambda sc: sc.random_linear_suite("cartpole", B=4, seed=33, static=False), None),
    "sweep_5_3_7": (lambda sc: sweep_linear_suite(5, 3, 7), "jit"),
    "sweep_20_4_10": (lambda sc: sweep_linear_suite(20, 4, 10), "tile"),
    "sweep_8_2_50": (lambda sc: sweep_linear_suite(8, 2, 50, tv=False), ("tile", "tile-jit")),
    "sweep_16_8_6": (lambda sc: sweep_linear_suite(16, 8, 6), "tile-jit"),
    "sweep_4_2_30_tv": (lambda sc: sweep_linear_suite(4, 2, 30, static=False), "regs"),
}


def identity_suite(name):
    import scenarios as sc
    suite = push_over(IDENTITY_SUITES[name][0](sc))
    suite["config"]["max_iter"] = 1
    suite["config"]["abs_pri_tol"] = suite["config"]["abs_dua_tol"] = 0.0
    return suite


def fixture_from(edges):
    """the items of tests/golden/halfspace_edges.npz in fixture_items()'s form: the sets are rebuilt (make_sets draws from numpy's
    generators alone), the duals and their labels are the stored ones"""
    return [(name, nx, nu, N, make_sets(name, nx, nu, N), {g: edges["%d.%s" % (n_, g)] for _, g, _, _ in FAMILIES},
             {g: edges["%d.%s.label" % (n_, g)] for _, g, _, _ in FAMILIES}) for n_, (name, nx, nu, N) in enumerate(FIXTURE_FORMS)]
