"""GPU: the second-order-cone projection at its float-rounding, range and fast-path edges, bit for bit against tests/soc_ref.py (the
numpy model that tests/test_soc_ref_cpu.py pins to the real reference on tests/golden/project_soc_edges.npz).

The project restates project_soc (admm.cpp:39-60) as soc_project3 + soc_all_inside (the transposed step of the one-row and the tile
kernel), soc3_inplace (the coverage kernel) and project_soc_kernel (the exported symbol).  State cones are driven through whole solves
on the A = 0 family of tests/soc_ref.py, on which the cone rows of a solve are the pure map vcnew = P(gc), gc = gc - vcnew: any
difference is a difference of the projection (a contracted sum of squares, a square root or a conversion that rounds differently, a
flushed float denormal, a * (1 / mu) where it is not a / mu, a margin of the all-inside shortcut that a float rounding bridges, a
gc-is-zero flag that outlives its solve).  Every test asserts which kernel ran."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "oracle"))
sys.path.insert(0, HERE)

import scenarios as sc  # noqa: E402
import soc_ref as sr  # noqa: E402
from cpu_solvers import OracleSolver  # noqa: E402

CASES, oracle_cone_rows = sr.CASES, sr.oracle_cone_rows

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(HERE, "golden")
RTOL = 1e-9                # tests/test_gpu_parity.py's bound on every field of a solve

# what the dispatcher gives a cone launch of each form: kernel_path(), and for the tile kernel last_tile_form (-1: the cone variants are
# instantiated at run time, no tile_dims.txt entry) / last_tile_dyn (0: they have no dynamic-slot form).  (4,3,10): the half-row form
# exists for plain box launches only -- a cone launch gets whole rows
EXPECT = {"one_row_6_3_10": "regs", "one_cone_6_3_10": "regs", "one_row_5_3_7": "jit", "half_4_3_10": "jit", "wide_20_4_10": "tile", "long_8_3_50": "tile-jit",
          "tile_jit_16_8_6": "tile-jit"}


def inside_set(form):
    """the coefficient set of the tests that need passes with nothing but state-cone items in them: two state cones, or one without the
    input cone that `mixed` adds (its items u + yc are not inside, and ONE item outside takes the whole pass of the wave off the fast path)"""
    return "mixed" if len(sr.FORMS[form]["rows"]) > 1 else "plain"


def make(form, mu_set, max_iter, B, tol=0.0, dynamics=False, **options):
    from hip_runner import make_batch
    suite = dict(problem=sr.family(form, dynamics=dynamics), config=sr.config(form, mu_set, max_iter, tol), cases=dict(x0=np.zeros((B, sr.FORMS[form]["nx"]))))
    s = make_batch(suite, batch=B)
    for k, v in options.items():
        s.set_option(k, v)
    return s


def assert_kernel(s, form, path=None):
    path = path or EXPECT[form]
    assert s.kernel_path() == path, (form, s.kernel_path(), path)
    if path in ("tile", "tile-jit"):
        assert s.get_option("last_tile_form") == -1 and s.get_option("last_tile_dyn") == 0, (s.get_option("last_tile_form"), s.get_option("last_tile_dyn"))
    elif path in ("regs", "jit"):
        assert s.get_option("last_half_rows") == 0


def assert_instantiated(prefix):
    """no option reports the (W, R) of a run-time instantiated tile form (last_tile_form is -1 for all of them); the list of
    instantiated C++ names does: admm_tile_kernel<nx, nu, N, W, R, SOC, ...>"""
    import tinympc_amd as tm
    assert any(n.replace(" ", "").startswith(prefix.replace(" ", "")) for n in tm.jit_used()), (prefix, tm.jit_used())


def solve_cone_rows(s, form, items, x0=None, noncone_gc=None):
    """warm gc = the items on the cone rows (noncone_gc on the others), everything else zero -> (vcnew, gc) fields, iteration counts"""
    gc = sr.pack(form, items)
    if noncone_gc is not None:
        gc[:, sr.noncone_rows(form), :] = noncone_gc
    s.reset()
    s.set_x0(np.zeros((items.shape[0], sr.FORMS[form]["nx"])) if x0 is None else x0)
    s.set("gc", gc)
    s.solve()
    return s.get("vcnew"), s.get("gc"), s.status()["iter"]


def assert_items(form, got_field, want_items, labels, what):
    same = np.all(sr.same_bits(sr.unpack(form, got_field), want_items), axis=-1)
    if not same.all():
        bad = np.argwhere(~same)
        first = tuple(bad[0])
        raise AssertionError((what, "items that differ", int((~same).sum()), "of", same.size,
                              "classes", sorted({sr.CLASSES[c] for c in np.asarray(labels)[~same]}) if labels is not None else None,
                              "first (instance, cone, knot)", first, "got", sr.unpack(form, got_field)[first].tolist(), "want", want_items[first].tolist()))


# ---- 1. the exported symbol
def test_project_soc_symbol_on_the_directed_set():
    """project_soc(TinyVector, float) with the reference's calling convention on all of project_soc_edges.npz: the reference's recorded
    answer, bit for bit (NaNs where it has NaNs).  (No batch handle, no dispatcher: the symbol always launches project_soc_kernel.)"""
    import pod
    import tinympc_amd as tm
    L = tm.lib()
    kat = np.load(os.path.join(GOLDEN, "project_soc_edges.npz"))
    L.project_soc.argtypes, L.project_soc.restype = [C.POINTER(pod.Vec), C.POINTER(pod.Vec), C.c_float], C.POINTER(pod.Vec)
    libc = C.CDLL(None)
    libc.free.argtypes = [C.c_void_p]
    got = np.zeros_like(kat["out"])
    for i in range(len(kat["s"])):
        v, keep = pod.vec(kat["s"][i])
        out = pod.Vec()
        L.project_soc(C.byref(out), C.byref(v), float(kat["mu"][i]))
        assert out.rows == 3
        got[i] = pod.to_np(out)
        libc.free(C.cast(out.data, C.c_void_p))
    same = np.all(sr.same_bits(got, kat["out"]), axis=1)
    assert same.all(), [(str(kat["names"][kat["label"][i]]), float(kat["mu"][i]), kat["s"][i].tolist(), got[i].tolist(), kat["out"][i].tolist())
                        for i in np.flatnonzero(~same)[:5]]


# ---- 2. the coverage kernel's update_slack, both cone kinds, every coefficient of the fixture (0 and -0.5 included), non-finite items
def test_coverage_kernel_update_slack_on_the_directed_set():
    """phase("update_slack") with x = u = 0: vcnew = P(0 + gc), zcnew = P(0 + yc) with gc / yc = the fixture's items of three coefficients
    at a time (two state cones, one input cone), spread over all knots.  Bit for bit against the REFERENCE's recorded outputs where the
    input survives 0 + s (every item but a -0.0), against the model on all of them.  NaN / inf items sit between
    finite ones of the same instance: nothing but their own three cells may notice.  Which kernel: tiny_batch_phase launches the coverage
    kernel's single-phase form whatever the shape (batch_api.hip: launch_general), kernel_path() describes solves only -- nothing to assert."""
    from hip_runner import make_batch
    kat = np.load(os.path.join(GOLDEN, "project_soc_edges.npz"))
    mus = list(dict.fromkeys(kat["mu"].tolist()))                      # 8 + 2 distinct coefficients
    assert len(mus) == 10
    form, N = "one_row_6_3_10", 10
    prob = sr.family(form)
    rng = np.random.default_rng(8)
    seen = 0
    at_input = []
    for g in range(len(mus)):                                          # every coefficient is the input cone's once, a state cone's twice
        trio = [mus[(g + 1) % len(mus)], mus[(g + 2) % len(mus)], mus[g]]
        at_input.append(trio[2])
        sets = [np.flatnonzero(kat["mu"] == m) for m in trio]
        B = -(-max(len(ix) for ix in sets) // (N - 1))
        items = np.zeros((3, B * N, 3))
        want = np.zeros((3, B * N, 3))
        for k, ix in enumerate(sets):
            at = rng.permutation(B * (N - 1) if k == 2 else B * N)[:len(ix)]      # (an input cone has N - 1 knots)
            items[k, at] = kat["s"][ix]
            want[k] = sr.project(0.0 + items[k], trio[k])[0]
            unchanged = np.all(sr.same_bits(0.0 + kat["s"][ix], kat["s"][ix]), axis=1)
            assert np.all(sr.same_bits(want[k, at][unchanged], kat["out"][ix][unchanged]))     # the model IS the reference here
            seen += len(ix)
        cfg = sr.config(form, "mixed", 1)
        cfg.update(en_input_soc=1, state_cone=([0, 3], [3, 3], trio[:2]), input_cone=([0], [3], trio[2:]))
        s = make_batch(dict(problem=prob, config=cfg, cases=dict(x0=np.zeros((B, 6)))), batch=B)
        gc = sr.pack(form, items[:2].reshape(2, B, N, 3).transpose(1, 0, 2, 3))
        yc = items[2, :B * (N - 1)].reshape(B, N - 1, 3).transpose(0, 2, 1)
        s.set("gc", gc)
        s.set("yc", yc)
        s.phase("update_slack")
        assert_items(form, s.get("vcnew"), want[:2].reshape(2, B, N, 3).transpose(1, 0, 2, 3), None, ("vcnew", trio))
        zc = s.get("zcnew")
        same = np.all(sr.same_bits(zc.transpose(0, 2, 1), want[2, :B * (N - 1)].reshape(B, N - 1, 3)), axis=-1)
        assert same.all(), ("zcnew", trio, np.argwhere(~same)[:5].tolist())
        assert np.all(sr.same_bits(s.get("gc"), gc)) and np.all(sr.same_bits(s.get("yc"), yc))         # (update_slack writes no dual)
        s.close()
    assert sorted(at_input) == sorted(mus) and seen == 3 * len(kat["s"])


def test_non_finite_items_stay_in_their_cone():
    """update_slack on instances of deep-inside items with ONE NaN / inf item each (every non-finite class, head and last component):
    the item itself gives what the model gives (zeros for the NaN classes), every other cell of the instance -- the neighbouring knots
    of the same cone, the other cone, the rows of no cone -- and every other instance comes back bit for bit as it went in.  (The coverage
    kernel projects item by item; the wave-coupled kernels are held to this by the solve test below.  tiny_batch_phase: see above.)"""
    form, N, B = "one_row_6_3_10", 10, 16
    rng = np.random.default_rng(12)
    mus = np.array(sr.cone_setup(form, "mixed")[2])
    items = np.stack([sr.deep_inside(rng, mu, (B, N)) for mu in mus], axis=1)
    bad = np.zeros((B, 2, N), dtype=bool)
    for b in range(0, B, 2):                                           # (odd instances stay clean)
        k, i = (b // 2) % 2, (3 * b) % N
        items[b, k, i] = sr.draw(rng, sr.NONFINITE[(b // 2) % 4], mus[k], 1)[0]
        bad[b, k, i] = True
    s = make(form, "mixed", 1, B)
    gc = sr.pack(form, items)
    s.set("gc", gc)
    s.phase("update_slack")
    got = s.get("vcnew")
    s.close()
    want = sr.project(items, mus[None, :, None])[0]
    assert np.all(want[bad][np.isnan(items[bad]).any(axis=-1)] == 0.0)
    assert_items(form, got, want, None, "vcnew")
    assert np.all(sr.same_bits(sr.unpack(form, got)[~bad], items[~bad]))


@pytest.mark.parametrize("clean", ["inside", "directed"])
@pytest.mark.parametrize("form", ["one_cone_6_3_10", "one_row_6_3_10", "wide_20_4_10"])
def test_a_non_finite_item_does_not_reach_its_wave_neighbours(form, clean):
    """whole solves, 1 and 3 iterations, B = 16: instance 4 m + 1 carries ONE NaN / inf item (all four non-finite classes in turn, at
    varying cones and knots), the others are clean -- on the one-row kernel every wave of four holds one poisoned row, on the W = 2 tile
    form every other wave pairs a poisoned instance with a clean one.  The reference spreads the NaN over the poisoned instance itself
    (0 * NaN in the backward pass), so only its iteration count is asked (the oracle's); every CLEAN instance must still iterate the pure map bit for bit and
    run its iterations.  What is wave-coupled and now sees a non-finite value: soc_all_inside's ballot ("NaNs fail the test and take
    the exact path", `u0 < 1e300` for an infinite last component -- clean = inside: every other item of the wave would take the fast
    path), soc_project3's `outside` ballot and the wave-uniform multiply path (clean = directed: every finite class), the gc-is-zero flag."""
    f = sr.FORMS[form]
    B, N = 16, f["N"]
    mu_set = inside_set(form)
    mus = np.array(sr.cone_setup(form, mu_set)[2])
    K = len(mus)
    poisoned = np.arange(B) % 4 == 1
    for iters in (1, 3):
        rng = np.random.default_rng([51, iters])
        if clean == "inside":
            items = np.stack([sr.deep_inside(rng, mu, (B, N)) for mu in mus], axis=1)
        else:
            items = np.stack([sr.fill(rng, mu, (B, N), finite=True, shift=np.arange(B)[:, None] + 5 * k)[0] for k, mu in enumerate(mus)], axis=1)
        for n, b in enumerate(np.flatnonzero(poisoned)):
            k, i = n % K, (3 * n + 1) % N
            items[b, k, i] = sr.draw(rng, sr.NONFINITE[n % 4], mus[k], 1)[0]
        assert np.all(np.isfinite(items[~poisoned])) and not np.any(np.all(np.isfinite(items[poisoned]), axis=(1, 2, 3)))
        s = make(form, mu_set, iters, B)
        v, g, it = solve_cone_rows(s, form, items)
        assert_kernel(s, form)
        s.close()
        want_v, want_g = sr.iterate(items[~poisoned], mus[None, :, None], iters)
        assert np.all(it[~poisoned] == iters), it
        with np.errstate(all="ignore"):                                # the poisoned instances: nothing but the oracle's iteration count
            _, _, want_it = oracle_cone_rows(form, mu_set, iters, sr.pack(form, items[poisoned]))
        assert np.array_equal(it[poisoned], want_it) and np.all(want_it == iters), (it[poisoned], want_it)
        assert_items(form, v[~poisoned], want_v, None, ("vcnew of the clean instances", iters))
        assert_items(form, g[~poisoned], want_g, None, ("gc of the clean instances", iters))
        rest = g[~poisoned][:, sr.noncone_rows(form), :]
        assert not np.any(rest) and not np.any(np.signbit(rest))


# ---- 3. every register form, state cones at every knot of whole solves
FORM_CASES = [(form, mu_set, {}) for form, mu_set in CASES] + [("one_row_6_3_10", "mixed", {"prefer_tile": 1}), ("one_row_6_3_10", "mixed", {"force_general": 1})]


@pytest.mark.parametrize("form,mu_set,options", FORM_CASES, ids=["-".join([f, m] + sorted(o)) for f, m, o in FORM_CASES])
def test_state_cones_of_a_solve_are_the_models_map(form, mu_set, options):
    """the directed batches of tests/soc_ref.py (every class at every position of the item layout; tests/test_soc_ref_cpu.py shows the
    oracle agreeing with the model on exactly these) after 1 and after 3 iterations: vcnew and gc on the cone rows bit for bit, gc +0 on
    the rows of no cone.  prefer_tile on (6,3,10): the shape has no tile form, the dispatcher keeps it on the one-row kernel."""
    path = "cover" if options.get("force_general") else None
    for iters in (1, 3):
        items, labels, mus = sr.directed_batch(form, mu_set, iters)
        mu_arr = np.asarray(mus)[None, :, None]
        s = make(form, mu_set, iters, items.shape[1], **options)
        for l in range(items.shape[0]):
            v, g, it = solve_cone_rows(s, form, items[l])
            assert_kernel(s, form, path)
            if form == "long_8_3_50":
                assert_instantiated("tinympc_amd::admm_tile_kernel<8,3,50,1,2,2,")       # W = 1, R = 2, state cones
            if form == "wide_20_4_10":
                assert_instantiated("tinympc_amd::admm_tile_kernel<20,4,10,2,1,2,")      # W = 2: rows 14..16 straddle the two DPP rows
            assert np.all(it == iters)
            want_v, want_g = sr.iterate(items[l], mu_arr, iters)
            assert_items(form, v, want_v, labels[l], ("vcnew", iters, l))
            assert_items(form, g, want_g, labels[l], ("gc", iters, l))
            rest = g[:, sr.noncone_rows(form), :]
            assert not np.any(rest) and not np.any(np.signbit(rest))
        s.close()


# ---- 4. the all-inside fast path and its margin
@pytest.mark.parametrize("form", ["one_cone_6_3_10", "wide_20_4_10"])
def test_all_inside_fast_path_and_its_margin(form):
    """every item deep inside its cone (norm <= 0.2 u0), a nonzero warm gc on the cone rows AND on the rows of no cone; one item per
    launch is the exception: just below the fast path's margin q = u0^2 (1 - 2^-20) (the wave may skip the square root), just above it
    (it may not; the reference still says inside), and one whose double norm is below u0 by more than 2^-26 of it while the float norm is
    ABOVE u0 (the reference says outside: a margin as narrow as 2^-26 copies it through).  After 1 iteration vcnew = the input bit for
    bit where the model says inside and gc = +0 everywhere; after 2 the inputs are zero vectors, the model's `below` branch: the
    transition from the fast to the exact path of the gc-is-zero flag."""
    f = sr.FORMS[form]
    B, N = 16, f["N"]
    rng = np.random.default_rng(21)
    mu_set = inside_set(form)
    mus = np.array(sr.cone_setup(form, mu_set)[2])
    rest_rows = sr.noncone_rows(form)
    for which in ("margin_below", "margin_above", "bridged"):
        items = np.stack([sr.deep_inside(rng, mu, (B, N)) for mu in mus], axis=1)
        b, k, i = 5, len(mus) - 1, 3
        items[b, k, i] = sr.bridged(rng, mus[k], 1)[0] if which == "bridged" else sr.draw(rng, which, mus[k], 1)[0]
        fast = sr.fast_path_takes(items, mus[None, :, None])
        assert fast.sum() == fast.size - (which != "margin_below")
        noncone = rng.normal(0.0, 1.0, (B, len(rest_rows), N))
        for iters in (1, 2):
            s = make(form, mu_set, iters, B)
            v, g, it = solve_cone_rows(s, form, items, noncone_gc=noncone)
            assert_kernel(s, form)
            s.close()
            want_v, want_g = sr.iterate(items, mus[None, :, None], iters)
            assert_items(form, v, want_v, None, ("vcnew", which, iters))
            assert_items(form, g, want_g, None, ("gc", which, iters))
            assert not np.any(g[:, rest_rows, :]) and not np.any(np.signbit(g[:, rest_rows, :])), (which, iters)
            if iters == 1 and which != "bridged":
                assert np.all(sr.same_bits(sr.unpack(form, v), items)) and not np.any(g) and not np.any(np.signbit(g))
            if iters == 2 and which != "bridged":
                assert not np.any(sr.unpack(form, v)) and not np.any(sr.unpack(form, g))


# ---- 5. the gc-is-zero flag across the instances of a persistent row
@pytest.mark.parametrize("form,interleaved", [("one_cone_6_3_10", False), ("one_cone_6_3_10", True), ("wide_20_4_10", False), ("wide_20_4_10", True)])
def test_gc_zero_flag_does_not_outlive_its_instance(form, interleaved):
    """grid_waves_per_cu = 1 and B = 3 091 (tests/test_gpu_hetero_adaptive.py's size: more than 12 instances per CU of an MI355X's 256, at
    most four to a wave, odd, so the last tile is partial): every wave serves at least three tiles one after the other, and the
    flag that says "this lane's gc cells are already zero" lives in a lane across them.  All items deep inside with a nonzero warm gc
    everywhere: every instance's gc must come back +0 and its vcnew its input, bit for bit.  interleaved: every third group of four
    instances is all-outside, so a row alternates between the two paths from one instance to the next.  (tile_dyn = 1 is set on
    the tile shape: the cone variants have no dynamic-slot form, the static one runs -- asserted.)"""
    B = 3091
    f = sr.FORMS[form]
    N = f["N"]
    rng = np.random.default_rng(33)
    mu_set = inside_set(form)
    mus = np.array(sr.cone_setup(form, mu_set)[2])
    items = np.stack([sr.deep_inside(rng, mu, (B, N)) for mu in mus], axis=1)
    out = np.zeros(B, dtype=bool)
    if interleaved:
        out = (np.arange(B) // 4) % 3 == 1
        for k, mu in enumerate(mus):
            items[out, k] = sr.draw(rng, "outside", mu, int(out.sum()) * N, finite=True).reshape(-1, N, 3)
    noncone = rng.normal(0.0, 1.0, (B, len(sr.noncone_rows(form)), N))
    opts = {"grid_waves_per_cu": 1}
    if EXPECT[form] == "tile":
        opts["tile_dyn"] = 1
    s = make(form, mu_set, 2, B, **opts)
    v, g, it = solve_cone_rows(s, form, items, noncone_gc=noncone)
    assert_kernel(s, form)
    s.close()
    want_v, want_g = sr.iterate(items, mus[None, :, None], 2)
    assert_items(form, v, want_v, None, "vcnew")
    assert_items(form, g, want_g, None, "gc")
    assert not np.any(g[~out]) and not np.any(np.signbit(g[~out]))
    assert not np.any(g[:, sr.noncone_rows(form), :])
    s = make(form, mu_set, 1, B, **opts)
    v, g, it = solve_cone_rows(s, form, items, noncone_gc=noncone)
    assert_kernel(s, form)
    s.close()
    assert np.all(sr.same_bits(sr.unpack(form, v)[~out], items[~out])) and not np.any(g[~out]) and not np.any(np.signbit(g[~out]))
    assert_items(form, g, sr.iterate(items, mus[None, :, None], 1)[1], None, "gc after 1")


# ---- 6. rows that stop while others go on
@pytest.mark.parametrize("form", ["one_cone_6_3_10", "wide_20_4_10"])
def test_rows_that_stop_while_their_wave_goes_on(form):
    """default tolerances, max_iter = 4: the even instances have a zero x0 and converge at iteration 1, the odd ones carry 1e3 in a row of
    no cone and run to the cap -- in the same waves (the family with dynamics on the rows of no cone: with A = 0 the gain is zero and x0 is
    forgotten after one iteration; the cone rows of A stay zero, which is what keeps x at 0 there).  Cone items at the fast path's margin in both halves (all just below it in one
    launch, all just above in the next).  Iteration counts = the oracle's; vcnew and gc = the model's map iterated that often."""
    f = sr.FORMS[form]
    B, N = 16, f["N"]
    rng = np.random.default_rng(44)
    mu_set = inside_set(form)
    mus = np.array(sr.cone_setup(form, mu_set)[2])
    x0 = np.zeros((B, f["nx"]))
    x0[1::2, sr.noncone_rows(form)[0]] = 1e3
    for which in ("margin_below", "margin_above"):
        items = np.stack([sr.draw(rng, which, mu, B * N).reshape(B, N, 3) for mu in mus], axis=1)
        _, _, want_it = oracle_cone_rows(form, mu_set, 4, sr.pack(form, items), x0, tol=1e-3, dynamics=True)
        assert np.all(want_it[0::2] == 1) and np.all(want_it[1::2] == 4), want_it
        s = make(form, mu_set, 4, B, tol=1e-3, dynamics=True)
        v, g, it = solve_cone_rows(s, form, items, x0=x0)
        assert_kernel(s, form)
        s.close()
        assert np.array_equal(it, want_it), (it, want_it)
        for n in (1, 4):
            at = want_it == n
            want_v, want_g = sr.iterate(items[at], mus[None, :, None], n)
            assert_items(form, v[at], want_v, None, ("vcnew", which, n))
            assert_items(form, g[at], want_g, None, ("gc", which, n))


# ---- 7. input cones through a solve
def test_input_cones_through_a_solve_match_the_oracle():
    """(6,3,10) with an input cone on all three inputs (mu 0.5, R equal on its rows so that the direction of Uref survives) next to the
    two state cones; Uref proportional to a deep-inside, an outside and a below triple at three scales, 40 iterations.  u = -d passes
    through Quu_inv, so this is a comparison with the oracle at tests/test_gpu_parity.py's tolerance, not bit for bit; the projection's
    last input u + yc = zcnew + yc (oracle's) is at least 2^-16 (relative) away from both branch boundaries in every item, so a
    flipped branch is a fault and not a rounding."""
    from hip_runner import make_batch
    form, N, iters = "one_row_6_3_10", 10, 40
    prob = sr.family(form)
    prob["R"] = np.full(3, 0.7)
    prob["B"] = 0.05 * prob["B"]
    triples = np.array([[0.1, 0.1, 1.0], [1.0, 1.0, 0.5], [0.05, 0.05, -1.0]])
    Uref = np.stack([c * np.repeat(t[:, None], N - 1, axis=1) for t in triples for c in (0.1, 1.0, 10.0)])
    B = len(Uref)
    cfg = sr.config(form, "mixed", iters)
    cfg.update(en_input_soc=1, input_cone=([0], [3], [0.5]))
    o = sc.make_solver(OracleSolver, prob, cfg)
    ref = {k: np.zeros((B,) + o[k].shape) for k in ("u", "zcnew", "yc", "vcnew", "gc")}
    zero = {k: np.zeros(o[k].shape) for k in o.STATE_FIELDS + ("Xref",)}
    for b in range(B):
        o.restore(zero)
        o["Uref"] = Uref[b]
        o.solve()
        for k in ref:
            ref[k][b] = o[k]
    o.close()
    f = sr.facts((ref["zcnew"] + ref["yc"]).transpose(0, 2, 1), 0.5)
    gap = np.minimum(np.abs(f["rd"] - f["u0"]), np.abs(f["rd"] + f["u0"])) / np.maximum(f["rd"], np.abs(f["u0"]))
    assert gap.min() >= 2.0 ** -16, gap.min()
    branch = sr.project((ref["zcnew"] + ref["yc"]).transpose(0, 2, 1), 0.5)[1]
    assert set(np.unique(branch)) == {0, 1, 2}
    s = make_batch(dict(problem=prob, config=cfg, cases=dict(x0=np.zeros((B, 6)))), batch=B)
    s.set_u_ref(Uref)
    s.solve()
    assert_kernel(s, form)
    worst = 0.0
    for k in ref:
        got = s.get(k)
        for b in range(B):
            e = float(np.max(np.abs(got[b] - ref[k][b])) / max(np.max(np.abs(ref[k][b])), 1e-300))
            worst = max(worst, e)
            assert e < RTOL, (k, b, e)
    assert np.all(s.status()["iter"] == iters)
    s.close()
    print("input cones through a solve: worst relative deviation from the oracle", worst, "smallest distance from a branch boundary", float(gap.min()))
