"""GPU tests of the disturbance and measurement-noise sequences generated on the device (tiny_batch_generate_disturbance /
..._measurement_noise, tiny_group_generate_*): the fill kernels of batch_instance.hip against the host function tiny_noise_generate and the
restatement tests/noise_ref.py, bit for bit.  Shapes and batches: tests/disturbance_cases.py.
  a. the fill equals the host: every row read back through the getters, on every shape class, an odd nx, one and two instances, a batch
     whose pairs straddle a 256-thread block with a ragged last block, ids that carry into counter word 1; diagonal and factor, one
     scale for all and per instance, host and device arrays;
  b. the closed loop of a handle that generates equals, bit for bit, the one of a handle that is handed tiny_noise_generate's rows through
     the ordinary setter -- fused and single-stepped, on the one-row kernel and the coverage path, under a disturbance, under
     measurement noise with an estimator, and under both from one seed;
  c. a group's rows and closed loop do not depend on the sharding;
  d. the lifecycle: replacing, the read-backs, reset, refused calls, removal, and 50 generate / remove cycles without a leak."""
import ctypes as C
import functools

import numpy as np
import pytest

import disturbance_cases as dc
import noise_ref as nr
import tinympc_amd as tm
from test_gpu_disturbance import assert_same_bits, make, settings, snapshot
from test_gpu_plant import _hip_runtime, advance, fused

pytestmark = pytest.mark.gpu
T = dc.T
BIG_BASE = 2**32 - 3                               # with stride 3: ids 2^32 - 3, 2^32, ...: the carry into counter word 1
_dp = C.POINTER(C.c_double)


def handle(name, B=None):
    """a bare handle of a case's shape (the fill reads nothing of the problem)"""
    c = dc.case(name)
    return tm.TinyBatchSolver.from_problem(c["fams"][0], B or c["B"])


def read_rows(s, stream, n_steps):
    get = s.get_measurement_noise if stream else s.get_disturbance
    return np.array([[get(k, i) for i in range(s.batch)] for k in range(n_steps)])


def noise_arrays(nx, B, factor, per_instance, seed=5):
    """scale and mean as matrices (tinympc_amd.noise_spec): entries of both signs, none zero, every one distinct"""
    rng = np.random.default_rng(100 * nx + 10 * B + 2 * factor + per_instance + seed)
    lead = (B,) if per_instance else ()
    shape = lead + ((nx, nx) if factor else (nx,))
    return rng.uniform(0.25, 2.0, shape) * rng.choice([-1.0, 1.0], shape), rng.uniform(-3.0, 3.0, lead + (nx,))


def on_device(a):
    hip = _hip_runtime()
    flat = np.ascontiguousarray(a, dtype=np.float64).ravel()
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), C.c_size_t(max(flat.nbytes, 8))) == 0
    assert hip.hipMemcpy(p, flat.ctypes.data_as(C.c_void_p), C.c_size_t(flat.nbytes), 1) == 0      # hipMemcpyHostToDevice
    return p


def generate(s, stream, device, seed, n_steps, scale, mean, factor, id_base, id_stride):
    """through the package from host arrays, or through the C ABI from device arrays that are freed right after the call (they are copied)"""
    if not device:
        (s.generate_measurement_noise if stream else s.generate_disturbance)(seed, n_steps, scale, mean, factor, id_base, id_stride)
        return
    spec, (flat, mu) = tm.noise_spec(s.batch, s.nx, seed, n_steps, scale, mean, factor, id_base, id_stride)
    ptrs = [on_device(a) for a in (flat, mu) if a is not None]
    spec.scale, spec.mean, spec.flags = C.cast(ptrs[0], _dp), (C.cast(ptrs[1], _dp) if mu is not None else None), spec.flags | tm.DEVICE
    L = tm.lib()
    rc = (L.tiny_batch_generate_measurement_noise if stream else L.tiny_batch_generate_disturbance)(s._h, C.byref(spec))
    for p in ptrs:
        assert _hip_runtime().hipFree(p) == 0
    assert rc == tm.OK, (rc, L.tiny_batch_last_error(s._h).decode())


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
FILL = [("6_3_10_box", 13, 4, 0), ("5_3_7", 11, 4, 0), ("1_15_3", 11, 4, 0), ("15_1_3", 11, 4, 0), ("20_4_10", 11, 4, 0), ("6_3_10_b2", 1, 4, 0),
        ("6_3_10_b2", 2, 4, 0), ("5_3_7", 300, 3, 0), ("5_3_7", 11, 4, BIG_BASE)]


@pytest.mark.parametrize("name,B,n_steps,id_base", FILL)
def test_the_fill_equals_the_host_function_and_the_restatement_bit_for_bit(name, B, n_steps, id_base):
    s = handle(name, B)
    nx = s.nx
    seed, stride = 0xFFFFFFFF00000001 if id_base else 7, 3 if id_base else 1
    if B == 300:                                                     # three pairs a row: pair 0 of row 85 is thread 255, its others thread 256 and 257
        assert (nx + 1) // 2 == 3 and (n_steps * B * 3) % 256 != 0 and n_steps * B * 3 > 256
    checked = 0
    for factor in (False, True):
        for per_instance in (False, True):
            scale, mean = noise_arrays(nx, B, factor, per_instance)
            for stream in (0, 1):
                with_mean = mean if (stream + per_instance) % 2 == 0 else None      # (both ways under each form and stream)
                host = tm.noise_generate(seed, stream, n_steps, B, nx, scale, with_mean, factor, id_base, stride)
                ref = nr.rows(seed, stream, n_steps, B, nx, scale, with_mean, factor, id_base, stride)
                assert np.array_equal(host, ref), ("tiny_noise_generate against the restatement", factor, per_instance, stream)
                for device in (False, True):
                    generate(s, stream, device, seed, n_steps, scale, with_mean, factor, id_base, stride)
                    opt = "measurement_noise" if stream else "disturbance"
                    assert (s.get_option(opt), s.get_option(opt + "_generated"), s.get_option("measurement_step" if stream else "disturbance_step")) == (n_steps, 1, 0)
                    got = read_rows(s, stream, n_steps)
                    assert np.array_equal(got, host), (factor, per_instance, stream, device, float(np.max(np.abs(got - host))))
                    checked += 1
    assert checked == 16
    s.close()


# ---- b. ------------------------------------------------------------------------------------------------------------------------------
LOOP_CASES = {"6_3_10_box": 3, "6_3_10_cones": 3, "20_4_10": 2, "6_3_10_force_general": 2}      # name: tiny_batch_kernel_path
MODES = ("disturbance", "measurement_and_estimator", "both")
DRIVES = {"fused": fused, "single_stepped": advance}
SEED = 20261021
W_SCALE, V_SCALE = 0.1, 0.05                       # process noise / sensor noise, every entry's standard deviation


def configure(s, c, mode, source):
    """the loop's inputs on handle s: `generated` on the device, or `host`: tiny_noise_generate's rows through the ordinary setters"""
    B, nx, nu = c["B"], c["nx"], c["nu"]
    w_scale, v_scale = np.full(nx, W_SCALE), np.full(nx, V_SCALE)
    if mode in ("disturbance", "both"):
        if source == "generated":
            s.generate_disturbance(SEED, T, w_scale)
        else:
            s.set_disturbance(tm.noise_generate(SEED, 0, T, B, nx, w_scale))
    if mode in ("measurement_and_estimator", "both"):
        if source == "generated":
            s.generate_measurement_noise(SEED, T, v_scale)
        else:
            s.set_measurement_noise(tm.noise_generate(SEED, 1, T, B, nx, v_scale))
        s.set_estimator(0.5 * np.eye(nx))
    if mode != "none":
        s.set_score(np.ones(nx + nu), None, np.full(nx + nu, -0.6), np.full(nx + nu, 0.6))


@functools.lru_cache(maxsize=None)
def undisturbed(name, drive):
    """u0 of every step of the case with nothing installed (computed once and shared; never modified)"""
    c = dc.case(name)
    r = make(c)
    configure(r, c, "none", "host")
    run = DRIVES[drive](r)
    r.close()
    return run["log_u0"]


@pytest.mark.parametrize("name,mode,drive", [(n, m, d) for n in LOOP_CASES for m in MODES for d in DRIVES])
def test_a_generating_handle_runs_the_closed_loop_of_a_handle_given_the_same_rows(name, mode, drive):
    c = dc.case(name)
    keys = dc.keys(c)
    runs = {}
    for source in ("generated", "host"):
        s = make(c)
        configure(s, c, mode, source)
        run = DRIVES[drive](s)
        runs[source] = dict(snapshot(s, keys), **run)
        runs[source].update(zip(("cost", "worst", "violated_steps", "first_violation"), s.get_score()))
        runs[source]["path"] = np.array(tm.lib().tiny_batch_kernel_path(s._h))
        has_w, has_v = mode in ("disturbance", "both"), mode in ("measurement_and_estimator", "both")
        assert (s.get_option("disturbance"), s.get_option("last_disturbance")) == (T * has_w, int(has_w))
        assert (s.get_option("measurement_noise"), s.get_option("last_measurement_noise"), s.get_option("last_estimator")) == (T * has_v, int(has_v), int(has_v))
        assert (s.get_option("disturbance_generated"), s.get_option("measurement_noise_generated")) == ((int(has_w), int(has_v)) if source == "generated" else (0, 0))
        assert s.get_option("last_score") == 1 and s.get_option("last_half_rows") == 0 and s.get_option("last_prefetch") == 0
        if source == "generated" and mode == "both":                 # (the streams differ: the same seed and scale would give v = w / 2 otherwise)
            w, v = read_rows(s, 0, T), read_rows(s, 1, T)
            assert np.all(v != w) and np.all(v * (W_SCALE / V_SCALE) != w)
        s.close()
    assert int(runs["generated"]["path"]) == LOOP_CASES[name], runs["generated"]["path"]
    assert_same_bits(runs["generated"], runs["host"], (name, mode, drive))
    moved = np.max(np.abs(runs["generated"]["log_u0"][1] - undisturbed(name, drive)[1]), axis=1)
    assert np.all(moved > 1e-6), moved                               # (every instance: the noise reaches the next step's u0)
    assert np.max(np.abs(runs["generated"]["x"])) < 100.0 and np.max(np.abs(runs["generated"]["log_iter"])) > 1


# ---- c. ------------------------------------------------------------------------------------------------------------------------------
LAYOUTS = [dict(devices=[0]), dict(devices=[0, 0], interleaved=False), dict(devices=[0, 0], interleaved=True), dict(devices=[0, 0, 0], interleaved=True)]


def prepare(s, c):
    s.set_bound_constraints(*[a[0] for a in c["box"]])
    s.update_settings(**settings(c))
    s.set_x0(c["x0"])
    s.set_x_ref(c["Xref"])
    s.set_u_ref(c["Uref"])


def group_rows(g, stream, n_steps):
    """every shard's rows, gathered to the caller's order"""
    L = tm.lib()
    out = np.full((n_steps, g.batch, g.nx), np.nan)
    get = L.tiny_batch_get_measurement_noise if stream else L.tiny_batch_get_disturbance
    for k in range(g.shards):
        h = L.tiny_group_shard(g._h, k)
        for local, i in enumerate(g.shard_indices(k)):
            for step in range(n_steps):
                row = np.zeros(g.nx)
                assert get(h, step, local, row.ctypes.data_as(_dp)) == tm.OK
                out[step, i] = row
    return out


@functools.lru_cache(maxsize=None)
def single_batch_reference():
    """the rows and the closed loop of ONE batch of 13 (computed once and shared; never modified)"""
    c = dc.case("6_3_10_box")
    B, nx, nu = c["B"], c["nx"], c["nu"]
    assert B == 13
    out = {}
    s = make(c)
    for factor in (False, True):
        scale, mean = noise_arrays(nx, B, factor, True)
        s.generate_disturbance(SEED, 4, scale, mean, factor, BIG_BASE, 3)
        s.generate_measurement_noise(SEED, 4, scale, mean, factor, BIG_BASE, 3)
        out["rows", factor] = (read_rows(s, 0, 4), read_rows(s, 1, 4))
        assert np.array_equal(out["rows", factor][0], tm.noise_generate(SEED, 0, 4, B, nx, scale, mean, factor, BIG_BASE, 3))
    configure(s, c, "both", "generated")
    run = fused(s, 3)
    out["loop"] = dict(snapshot(s, dc.keys(c)), log_x0=run["log_x0"])
    out["loop"].update(zip(("cost", "worst", "violated_steps", "first_violation"), s.get_score()))
    assert tm.lib().tiny_batch_kernel_path(s._h) == 3
    s.close()
    return out


@pytest.mark.parametrize("kw", LAYOUTS)
def test_a_groups_noise_and_closed_loop_do_not_depend_on_the_sharding(kw):
    c = dc.case("6_3_10_box")
    B, nx = c["B"], c["nx"]
    want = single_batch_reference()
    g = tm.TinyGroupSolver.from_problem(c["fams"][0], B, **kw)
    assert g.shards == len(kw["devices"])
    prepare(g, c)
    for factor in (False, True):
        scale, mean = noise_arrays(nx, B, factor, True)              # (per instance: every shard gets its own slice)
        g.generate_disturbance(SEED, 4, scale, mean, factor, BIG_BASE, 3)
        g.generate_measurement_noise(SEED, 4, scale, mean, factor, BIG_BASE, 3)
        for stream in (0, 1):
            assert np.array_equal(group_rows(g, stream, 4), want["rows", factor][stream]), (kw, factor, stream)
    configure(g, c, "both", "generated")
    g.set_option("steps_per_launch", 3)
    g.set_option("state_log", 1)
    g.solve()
    got = {k: g.get(k) for k in dc.keys(c) + ("x0",)}
    st = g.status()
    got.update(iter=st["iter"].copy(), solved=st["solved"].copy(), log_x0=g.state_log(3))
    got.update(zip(("cost", "worst", "violated_steps", "first_violation"), g.get_score()))
    for k in range(g.shards):
        h = tm.lib().tiny_group_shard(g._h, k)
        opt = lambda n: int(tm.lib().tiny_batch_get_option(h, n))
        assert (opt(b"disturbance_generated"), opt(b"measurement_noise_generated"), opt(b"last_disturbance"), opt(b"last_measurement_noise"),
                tm.lib().tiny_batch_kernel_path(h)) == (1, 1, 1, 1, 3)
    g.close()
    assert_same_bits(got, want["loop"], kw)


# ---- d. ------------------------------------------------------------------------------------------------------------------------------
def test_lifecycle_replacing_read_backs_reset_refusals_and_removal():
    s = handle("5_3_7")
    B, nx = s.batch, s.nx
    L = tm.lib()
    scale = np.linspace(0.5, 1.5, nx)
    for stream, name, counter in ((0, "disturbance", "disturbance_step"), (1, "measurement_noise", "measurement_step")):
        gen = s.generate_measurement_noise if stream else s.generate_disturbance
        setter = s.set_measurement_noise if stream else s.set_disturbance
        call = L.tiny_batch_generate_measurement_noise if stream else L.tiny_batch_generate_disturbance
        assert (s.get_option(name), s.get_option(name + "_generated")) == (0, 0)
        # twice with two seeds: the second wins and the counter is rewound
        gen(1, 4, scale)
        s.set_option(counter, 3)
        gen(2, 6, scale)
        second = tm.noise_generate(2, stream, 6, B, nx, scale)
        assert (s.get_option(name), s.get_option(name + "_generated"), s.get_option(counter)) == (6, 1, 0)
        assert np.array_equal(read_rows(s, stream, 6), second) and not np.array_equal(second[:4], tm.noise_generate(1, stream, 4, B, nx, scale))
        # tiny_batch_reset keeps the sequence and its counter
        s.set_option(counter, 2)
        s.reset()
        assert (s.get_option(name), s.get_option(name + "_generated"), s.get_option(counter)) == (6, 1, 2)
        assert np.array_equal(read_rows(s, stream, 6), second)
        # every refused call leaves the installed sequence and its counter, bit for bit
        good, keep = tm.noise_spec(B, nx, 3, 5, scale)
        bad = [dict(scale=None), dict(n_steps=0), dict(n_steps=-2), dict(id_stride=0), dict(id_stride=-1), dict(id_base=-1), dict(flags=16 | tm.BROADCAST)]
        for kw in bad:
            spec, _ = tm.noise_spec(B, nx, 3, 5, scale)
            for k, v in kw.items():
                setattr(spec, k, v)
            assert call(s._h, C.byref(spec)) == tm.ERR_ARG, kw
            assert L.tiny_batch_last_error(s._h).decode().startswith("generated "), kw
        assert call(s._h, None) == tm.ERR_ARG
        assert (s.get_option(name), s.get_option(name + "_generated"), s.get_option(counter)) == (6, 1, 2)
        assert np.array_equal(read_rows(s, stream, 6), second)
        # a caller's sequence through the setter: no longer generated; generating again: generated
        setter(second[:3])
        assert (s.get_option(name), s.get_option(name + "_generated"), s.get_option(counter)) == (3, 0, 0)
        assert call(s._h, C.byref(good)) == tm.OK
        assert (s.get_option(name), s.get_option(name + "_generated")) == (5, 1)
        # removal through the setter frees it
        setter(None)
        assert (s.get_option(name), s.get_option(name + "_generated"), s.get_option(counter)) == (0, 0, 0)
        row = np.zeros(nx)
        assert (L.tiny_batch_get_measurement_noise if stream else L.tiny_batch_get_disturbance)(s._h, 0, 0, row.ctypes.data_as(_dp)) == tm.ERR_ARG
    s.close()


def test_the_example_flies_its_worst_instance_again_alone_to_the_last_bit():
    """examples/seeded_monte_carlo.c (C99, built by __graft_entry__.build()): 4 096 point masses under generated process and sensor noise
    with an estimator and a score, 60 fused steps; then the worst instance as a batch of one with id_base = its index"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "_build", "seeded_monte_carlo")
    if not os.path.exists(exe):
        pytest.fail("examples/_build/seeded_monte_carlo is missing: __graft_entry__.build() produces it")
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(p.stdout)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert "batch mean cost" in p.stdout and "matches the study to the last bit" in p.stdout and "kernel path 3" in p.stdout, p.stdout


def test_fifty_generate_and_remove_cycles_leave_device_memory_where_it_began():
    hip = _hip_runtime()

    def free_bytes():
        free, total = C.c_size_t(), C.c_size_t()
        assert hip.hipDeviceSynchronize() == 0 and hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
        return free.value
    s = handle("6_3_10_box")
    n_steps = 4096                                                   # 13 x 6 doubles a row: 2.4 MiB a sequence, 50 leaked ones would be 122 MiB
    one = n_steps * s.batch * s.nx * 8
    S = np.eye(s.nx)

    def cycle(i):
        s.generate_disturbance(i, n_steps, S if i % 2 else np.ones(s.nx), factor=bool(i % 2))
        s.generate_measurement_noise(i, n_steps, np.ones(s.nx), np.zeros(s.nx))
        assert (s.get_option("disturbance"), s.get_option("measurement_noise")) == (n_steps, n_steps)
        s.set_disturbance(None)
        s.set_measurement_noise(None)
    cycle(0)                                                         # (whatever the runtime keeps after a first use is in place)
    before = free_bytes()
    for i in range(1, 51):
        cycle(i)
    after = free_bytes()
    s.close()
    assert before - after < one, (before, after, one)
