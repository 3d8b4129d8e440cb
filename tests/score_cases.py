"""The setups, the reference and the oracle-side conditions of tests/test_gpu_score.py and tests/test_score_cpu.py (CPU only; computed
once per case and shared).  The meaning of tiny_batch_set_score, restated in plain Python floats -- every operation below is ONE
correctly rounded IEEE double operation, so no rational arithmetic is needed for the three-rounding form: with z = [xn | u0] of an MPC
step,

    cost:       for c = 0 .. nx+nu-1 ascending:  d = z[c] - target[c];  s = (weight[c] * d) * d;  cost = cost + s
    violation:  e[c] = max(z[c] - hi[c], lo[c] - z[c], 0);  m = max_c e[c];  worst = max(worst, m);
                m > 0:  violated_steps += 1, and first_violation = k where it is still -1

Cases: those of plant_cases -- 4_2_10 with 13 instances, 5_3_7 with 11, 12_4_10 with 2, the edge shapes 15_1_3 and 1_15_3, 6_3_10 and
the tile-kernel shape 20_8_10 -- each under its perturbed plant, T = 5 MPC steps.  Setups are per instance: weights U(0.5, 2) and
targets U(-0.3, 0.3), different in every entry; the limits are drawn around the instance's OWN oracle trajectory.  Instance i with
i % 3 == 0 never violates (every limit 0.05 .. 0.2 outside the trajectory's range).  Every other instance gets two crossings: on a state
row one side's limit in the middle of the widest gap between the row's values over the steps -- the steps beyond it cross --, and on an
input row the OTHER side's limit, placed the same way; every other row is wide.  Of all pairs of rows and both assignments of sides the
first is taken whose first crossing is at step 0 for i % 3 == 1 and later for i % 3 == 2 and, where there is one, at which a step shows
the state row as the worst and another step the input row.  Every limit is asserted
to stay 1e-6 away from every oracle value, so a run within the project's 1e-9 of the oracle crosses the same limits at the same steps.
check_case asserts the visibility conditions of the issue from the reference and the oracle loops alone."""
import functools

import numpy as np

import plant_cases as pc

T = pc.T
ORACLE_CASES = pc.ORACLE_CASES
EDGE_CASES = pc.EDGE_CASES
COMPOSE_CASE = "6_3_10"
COVER_CASE = "20_8_10"
ALL_CASES = ORACLE_CASES + EDGE_CASES + (COMPOSE_CASE, COVER_CASE)
MARGIN = 1e-6                                      # every limit is at least this far from every oracle value
ZERO = (0.0, 0.0, 0, -1)                           # a zeroed record: cost, worst, violated_steps, first_violation


def score_step(rec, z, setup, k, order=None, fused=False):
    """one MPC step into the record (cost, worst, violated_steps, first_violation): z (nz,), setup = (weight, target, lo, hi), each (nz,)
    or None (target: zeros, lo / hi: no limit); k the score step counter.  order / fused: the misreadings check_case tells apart --
    another summation order, the addition contracted with the second product into one fma"""
    w, tg, lo, hi = setup
    cost, worst, steps, first = rec
    nz = len(z)
    m = 0.0
    for c in (range(nz) if order is None else order):
        zc = float(z[c])
        d = zc - (0.0 if tg is None else float(tg[c]))
        wd = float(w[c]) * d
        cost = pc.fma(wd, d, cost) if fused else cost + wd * d
    for c in range(nz):
        zc = float(z[c])
        over = -np.inf if hi is None else zc - float(hi[c])
        under = -np.inf if lo is None else float(lo[c]) - zc
        m = max(m, over, under)
    if m > 0.0:
        worst = max(worst, m)
        steps += 1
        if first < 0:
            first = k
    return (cost, worst, steps, first)


def score_reference(states, u0s, setup, k0=0, rec=ZERO, scored=None, **how):
    """the record of ONE instance after the steps of states (T, nx) -- what the plant step handed on: the state log -- and u0s (T, nu)
    -- the applied controls: the step log --, from `rec`, the counter starting at k0.  scored: per step, whether it took a plant step
    (default: all); a step that did not is not scored, the counter advances all the same"""
    for k in range(len(states)):
        if scored is None or scored[k]:
            rec = score_step(rec, np.concatenate([states[k], u0s[k]]), setup, k0 + k, **how)
    return rec


def score_reference_batch(states, u0s, setups, k0=0, recs=None, scored=None):
    """every instance by its own setup: states (T, B, nx), u0s (T, B, nu), setups = four (B, nz) arrays (or None) -> cost, worst (B,)
    float64, violated_steps, first_violation (B,) int32"""
    B = states.shape[1]
    out = [score_reference(states[:, i], u0s[:, i], tuple(None if a is None else a[i] for a in setups), k0=k0, rec=ZERO if recs is None else tuple(r[i] for r in recs),
                           scored=None if scored is None else scored[:, i]) for i in range(B)]
    return (np.array([r[0] for r in out]), np.array([r[1] for r in out]), np.array([r[2] for r in out], dtype=np.int32), np.array([r[3] for r in out], dtype=np.int32))


def broadcast(setup, B):
    """one setup for all, as four (B, nz) arrays"""
    return tuple(None if a is None else np.repeat(np.asarray(a, dtype=float)[None], B, axis=0) for a in setup)


def trajectories(name):
    """the oracle loops of the case under its plant: z [B, T, nz] = [state handed on | u0 applied]"""
    runs = pc.oracle_case(name)
    return np.array([np.concatenate([r["states"], r["u0"]], axis=1) for r in runs])


def crossing(v, upper):
    """a limit on the values v of one row over the steps, in the middle of their widest gap: the steps above it (upper) or below it cross"""
    v = np.sort(v)
    j = int(np.argmax(np.diff(v)))
    return 0.5 * (v[j] + v[j + 1])


def limits_around(z, nx, nu, seed):
    """lo, hi [B, nz] around the trajectories z [B, T, nz], by the rule of the module's docstring"""
    rng = np.random.default_rng(seed)
    B, steps, nz = z.shape
    lo = z.min(axis=1) - rng.uniform(0.05, 0.2, (B, nz))
    hi = z.max(axis=1) + rng.uniform(0.05, 0.2, (B, nz))
    for i in range(B):
        if i % 3 == 0:
            continue
        best = None
        for upper in (i % 2 == 0, i % 2 != 0):                            # (the state row's side; the input row takes the other)
            for a in range(nx):
                for b in range(nu):
                    ca, cb = (i + a) % nx, nx + (i + b) % nu
                    l, h = lo[i].copy(), hi[i].copy()
                    (h if upper else l)[ca] = crossing(z[i, :, ca], upper)
                    (l if upper else h)[cb] = crossing(z[i, :, cb], not upper)
                    per_step = [worst_of_step(z[i, k], (None, None, l, h)) for k in range(steps)]
                    seen = {(row < nx, up) for e, row, up in per_step if e > 0.0}
                    first = min(k for k in range(steps) if per_step[k][0] > 0.0)
                    rank = (len(seen) == 2) + 2 * ((first > 0) == (i % 3 == 2))
                    if best is None or rank > best[0]:
                        best = (rank, l, h)
        lo[i], hi[i] = best[1], best[2]
    return lo, hi


# the seed of every case's weights, targets and margins: the first from 0 on at which check_case holds (the sums that tell a descending
# order and a contracted addition apart differ in bits on a few percent of the steps only)
SEEDS = {"4_2_10": 0, "5_3_7": 0, "12_4_10": 2, "15_1_3": 0, "1_15_3": 0, "6_3_10": 0, "20_8_10": 0}


@functools.lru_cache(maxsize=None)
def setup(name):
    """weight, target, lo, hi [B, nz] of the case"""
    c = pc.case(name)
    B, nx, nu = c["B"], c["nx"], c["nu"]
    rng = np.random.default_rng(7000 + 31 * nx + nu + 100000 * SEEDS[name])
    w = rng.uniform(0.5, 2.0, (B, nx + nu))
    tg = rng.uniform(-0.3, 0.3, (B, nx + nu))
    lo, hi = limits_around(trajectories(name), nx, nu, 7100 + nx + 100000 * SEEDS[name])
    return w, tg, lo, hi


@functools.lru_cache(maxsize=None)
def oracle_scores(name):
    """the reference applied to every instance's own oracle loop"""
    z, s = trajectories(name), setup(name)
    nx = pc.case(name)["nx"]
    return score_reference_batch(np.swapaxes(z[:, :, :nx], 0, 1), np.swapaxes(z[:, :, nx:], 0, 1), s)


def worst_of_step(z, setup_i):
    """(e, row, the hi side?) of the largest violation of one step, e = 0: none"""
    w, tg, lo, hi = setup_i
    over, under = z - hi, lo - z
    e = np.maximum(over, under)
    c = int(np.argmax(e))
    return float(max(e[c], 0.0)), c, bool(over[c] >= under[c])


def check_case(name):
    """the visibility conditions, from the reference and the oracle loops alone"""
    c = pc.case(name)
    B, nx, nu = c["B"], c["nx"], c["nu"]
    nz = nx + nu
    z, s = trajectories(name), setup(name)
    w, tg, lo, hi = s
    assert z.shape == (B, T, nz) and np.max(np.abs(z)) < 100.0
    for a in s:
        assert a.shape == (B, nz)
    assert all(len(np.unique(w[i])) == nz for i in range(B)) and len(np.unique(w)) == B * nz and len(np.unique(tg)) == B * nz
    # every limit keeps its distance from every oracle value
    assert np.min(np.abs(z - lo[:, None])) >= MARGIN and np.min(np.abs(z - hi[:, None])) >= MARGIN
    cost, worst, steps, first = oracle_scores(name)
    violating = steps > 0
    assert 3 * int(np.sum(violating)) >= B and 3 * int(np.sum(~violating)) >= B, (name, steps)
    assert np.all(first[~violating] == -1) and np.all(worst[~violating] == 0.0) and np.all(first[violating] >= 0) and np.all(worst[violating] > 0.0)
    # (a batch of 2 with a third never violating has ONE violating instance: one value is all it can show)
    assert len(set(first[violating].tolist())) >= min(2, int(np.sum(violating))), (name, first)
    sides, rows = set(), set()
    for i in range(B):
        for k in range(T):
            e, row, upper = worst_of_step(z[i, k], tuple(a[i] for a in s))
            if e > 0.0:
                sides.add(upper)
                rows.add(row < nx)
    assert sides == {True, False} and rows == {True, False}, (name, sides, rows)
    # the misreadings: each moves the cost by more than 1e-6 relative or flips a violation count, on every instance
    mA, mB, mf = c["model"]
    runs = pc.oracle_case(name)
    descending = contracted = 0
    for i in range(B):
        own = tuple(a[i] for a in s)
        xs, us = z[i, :, :nx], z[i, :, nx:]
        before = np.concatenate([c["x0"][i][None], xs[:-1]])
        solver_x1 = np.array([pc.plant_step(mA[i], mB[i], mf[i], before[k], us[k]) for k in range(T)])
        n = (i + 1) % B
        swapped = (np.concatenate([w[i, nx:], w[i, :nx]]),) + own[1:]
        others = {"the setup of instance %d" % n: score_reference(xs, us, tuple(a[n] for a in s)),
                  "weights read in [u | x] order": score_reference(xs, us, swapped),
                  "the state before the plant step": score_reference(before, us, own),
                  "the solver's own x[:,1]": score_reference(solver_x1, us, own)}
        for what, other in others.items():
            moved = abs(other[0] - cost[i]) / abs(cost[i])
            assert moved > 1e-6 or other[2] != steps[i], (name, i, what, moved)
        assert np.array_equal(runs[i]["states"], xs)
        descending += score_reference(xs, us, own, order=range(nz - 1, -1, -1))[0] != cost[i]
        contracted += score_reference(xs, us, own, fused=True)[0] != cost[i]
    assert descending >= 1 and contracted >= 1, (name, descending, contracted)
