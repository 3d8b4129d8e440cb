"""CPU: the counter-based normal generator (tinympc_amd/csrc/noise_gen.hpp; tiny_noise_generate) without a GPU.  The driver
tests/dropin/noise_gen_driver.cpp includes the header alone and is built with the host compiler.
  a. Philox4x32-10: Random123's three known answers, from the driver and from the restatement (tests/noise_ref.py);
  b. rows bit-equal to the restatement: nx in {1, 2, 5, 12, 15, 32}, both streams, diagonal and factor, with and without a mean, one
     scale for all and per instance, id_base = 2^32 - 3 with 8 instances (the carry into counter word 1), id_stride = 3, rows k = 0 .. 4,
     seeds 0, 1 and 0xFFFFFFFF00000001 -- from noise_fill_host, from the routines a device thread runs (rows32) and from the library's
     tiny_noise_generate;
  c. accuracy against a libm Box-Muller on the same uniforms over the first 2^16 pairs of seed 1 (stream 0, row 0, pair 0, ids 0 ..
     2^16 - 1);
  d. statistics of 2^20 deviates of one fixed seed (deterministic): mean, variance, Kolmogorov-Smirnov, the tail count, the correlation
     between neighbouring entries, rows, ids and between the streams;
  e. the factor form's sample covariance;  f. tiny_noise_generate's error codes, the exported symbols and the header's text."""
import ctypes as C
import functools
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import noise_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tinympc_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
NEW_SYMBOLS = ("tiny_batch_generate_disturbance", "tiny_batch_generate_measurement_noise", "tiny_group_generate_disturbance",
               "tiny_group_generate_measurement_noise", "tiny_noise_generate")
SEEDS = (0, 1, 0xFFFFFFFF00000001)
ID_BASE, ID_STRIDE, BATCH, N_STEPS = 2**32 - 3, 3, 8, 5     # ids 2^32 - 3, 2^32, 2^32 + 3, ...: counter word 1 becomes 1 at the second instance
# the measured maximum of |g - g_libm| / max(1, |g|) over the pairs of c. (profiles/noise_generator.md); the bound is 8 x that and never
# looser than 1e-13: a series cut one term short or a constant typed in single precision shows far above it
MEASURED_ACCURACY = 2.4424906541753444e-15
ACCURACY_BOUND = min(8 * MEASURED_ACCURACY, 1e-13)
# the statistics' seed.  2024 was the first one tried (on the driver's output, which b. shows to be the restatement's bit for bit) and
# lands inside every bound
STAT_SEED = 2024


@functools.lru_cache(maxsize=None)
def driver():
    out = os.path.join(ROOT, "tests", "dropin", "_build")
    os.makedirs(out, exist_ok=True)
    exe = os.path.join(out, "noise_gen_driver")
    src = os.path.join(ROOT, "tests", "dropin", "noise_gen_driver.cpp")
    cxx = shutil.which("g++")
    cmd = [cxx, "-ffp-contract=off"] if cxx else [HIPCC, "-x", "c++"]
    mine = "%s.%d" % (exe, os.getpid())                                # (test processes that run side by side each build their own, then rename: never a half-written file)
    subprocess.run(cmd + ["-std=c++17", "-O2", "-I", CSRC, src, "-o", mine], check=True, capture_output=True, timeout=600)
    os.replace(mine, exe)
    return exe


def driver_rows(mode, seed, stream, n_steps, batch, nx, scale, mean, factor, broadcast, id_base, id_stride):
    """scale / mean as the C ABI takes them (flat; a factor column-major)"""
    data = np.ascontiguousarray(scale, dtype=np.float64).tobytes() + (b"" if mean is None else np.ascontiguousarray(mean, dtype=np.float64).tobytes())
    args = [driver(), mode, str(seed), str(stream), str(n_steps), str(batch), str(nx), str(int(factor)), str(int(broadcast)), str(int(mean is not None)),
            str(id_base), str(id_stride)]
    raw = subprocess.run(args, input=data, capture_output=True, check=True, timeout=600).stdout
    return np.frombuffer(raw, dtype=np.float64).reshape(n_steps, batch, nx)


def library_rows(seed, stream, n_steps, batch, nx, scale, mean, factor, id_base, id_stride):
    """tiny_noise_generate through the package (scale / mean as matrices: tinympc_amd.noise_spec passes a factor on column-major)"""
    import tinympc_amd as tm
    return tm.noise_generate(seed, stream, n_steps, batch, nx, scale, mean, factor=factor, id_base=id_base, id_stride=id_stride)


def arrays(nx, factor, broadcast, with_mean, seed):
    """scale and mean as MATRICES (noise_ref.rows) and flat as the C ABI takes them: entries of both signs, none zero, every one distinct"""
    rng = np.random.default_rng(1000 * nx + 10 * seed % 997 + 2 * factor + broadcast)
    sets = 1 if broadcast else BATCH
    shape = (sets, nx, nx) if factor else (sets, nx)
    scale = rng.uniform(0.25, 2.0, shape) * rng.choice([-1.0, 1.0], shape)
    mean = rng.uniform(-3.0, 3.0, (sets, nx)) if with_mean else None
    flat = np.ascontiguousarray(scale.transpose(0, 2, 1)) if factor else scale
    ref_scale, ref_mean = (scale[0], None if mean is None else mean[0]) if broadcast else (scale, mean)
    return ref_scale, ref_mean, flat.ravel(), None if mean is None else mean.ravel()


# ---- a. ------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    lines = "".join("%x %x %x %x %x %x\n" % (c + k) for c, k, _ in nr.KNOWN_ANSWERS)
    out = subprocess.run([driver(), "philox"], input=lines, capture_output=True, text=True, check=True, timeout=60).stdout.splitlines()
    assert len(out) == 3
    for (c, k, want), line in zip(nr.KNOWN_ANSWERS, out):
        assert tuple(int(x, 16) for x in line.split()) == want, (c, k, line)
        assert nr.philox(c, k) == want
        many = nr.philox_many(*[np.array([v]) for v in c], *k)
        assert tuple(int(v[0]) for v in many) == want


# ---- b. ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 2, 5, 12, 15, 32])
def test_rows_equal_the_restatement_bit_for_bit(nx):
    checked = 0
    for seed in SEEDS:
        for stream in (0, 1):
            for factor in (False, True):
                for with_mean in (False, True):
                    broadcast = (stream + with_mean) % 2 == 0               # (both ways under every seed, form and stream)
                    ref_scale, ref_mean, scale, mean = arrays(nx, factor, broadcast, with_mean, seed)
                    want = nr.rows(seed, stream, N_STEPS, BATCH, nx, ref_scale, ref_mean, factor, ID_BASE, ID_STRIDE)
                    assert np.all(np.isfinite(want)) and np.unique(want).size == want.size
                    for what, got in (("noise_fill_host", driver_rows("rows", seed, stream, N_STEPS, BATCH, nx, scale, mean, factor, broadcast, ID_BASE, ID_STRIDE)),
                                      ("a device thread's routines", driver_rows("rows32", seed, stream, N_STEPS, BATCH, nx, scale, mean, factor, broadcast, ID_BASE, ID_STRIDE)),
                                      ("tiny_noise_generate", library_rows(seed, stream, N_STEPS, BATCH, nx, ref_scale, ref_mean, factor, ID_BASE, ID_STRIDE))):
                        assert np.array_equal(got, want), (what, hex(seed), stream, factor, with_mean, float(np.max(np.abs(got - want))))
                        checked += 1
    assert checked == 3 * 2 * 2 * 2 * 3


def test_ids_rows_streams_and_seeds_all_move_the_deviates():
    """what the counter is made of: the instance with id_base + i * id_stride is the instance with that id whatever the batch"""
    nx, one = 5, np.ones(5)
    base = nr.rows(1, 0, 2, 4, nx, one, id_base=ID_BASE, id_stride=ID_STRIDE)
    for i in range(4):
        alone = nr.rows(1, 0, 2, 1, nx, one, id_base=ID_BASE + i * ID_STRIDE)
        assert np.array_equal(alone[:, 0], base[:, i])
    assert nr.counter(1, 0, ID_BASE, 0, 0)[0][:2] == (2**32 - 3, 0) and nr.counter(1, 0, ID_BASE + ID_STRIDE, 0, 0)[0][:2] == (0, 1)
    others = (nr.rows(2, 0, 2, 4, nx, one, id_base=ID_BASE, id_stride=ID_STRIDE), nr.rows(1, 1, 2, 4, nx, one, id_base=ID_BASE, id_stride=ID_STRIDE),
              nr.rows(1, 0, 2, 4, nx, one, id_base=ID_BASE + 1, id_stride=ID_STRIDE), nr.rows(1 << 32, 0, 2, 4, nx, one, id_base=ID_BASE, id_stride=ID_STRIDE))
    for other in others:
        assert not np.any(other == base)
    assert not np.any(base[0] == base[1])


# ---- c. ------------------------------------------------------------------------------------------------------------------------------
def test_accuracy_against_a_libm_box_muller():
    n = 1 << 16
    raw = subprocess.run([driver(), "pairs", "1", "0", "0", "0", "0", str(n)], capture_output=True, check=True, timeout=600).stdout
    g = np.frombuffer(raw, dtype=np.float64).reshape(n, 2)
    ids = np.arange(n, dtype=np.uint64)
    r = [np.array(v).astype(object) for v in nr.philox_many(ids & np.uint64(nr.MASK), ids >> np.uint64(32), 0, 0, 1, 0)]
    assert tuple(int(v[77]) for v in r) == nr.philox(*nr.counter(1, 0, 77, 0, 0))
    worst = 0.0
    for i in range(n):
        n1, n2 = (int(r[0][i]) << 20) | (int(r[1][i]) >> 12), (int(r[2][i]) << 20) | (int(r[3][i]) >> 12)
        want = nr.pair_libm_from_draws(2 * n1 + 1, n2 >> 49, n2 & ((1 << 49) - 1))
        worst = max(worst, abs(g[i, 0] - want[0]) / max(1.0, abs(g[i, 0])), abs(g[i, 1] - want[1]) / max(1.0, abs(g[i, 1])))
    print("max |g - g_libm| / max(1, |g|) over 2^16 pairs of seed 1: %.17g (bound %.3g)" % (worst, ACCURACY_BOUND))
    assert worst <= ACCURACY_BOUND, worst
    assert np.max(np.abs(g)) <= 8.6


# ---- d. ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stat_blocks():
    """[stream][4 rows k][65 536 ids][4 entries]: 2^20 standard normals per stream (unit scale, no mean: fma(g, 1, 0) = g)"""
    return [driver_rows("rows", STAT_SEED, stream, 4, 1 << 16, 4, np.ones(4), None, False, True, 0, 1) for stream in (0, 1)]


def test_statistics_of_a_million_deviates():
    g = stat_blocks()[0]
    x = g.ravel()
    n = x.size
    assert n == 1 << 20
    mean, var = float(np.mean(x)), float(np.var(x))
    assert abs(mean) < 5 / math.sqrt(n), mean
    assert abs(var - 1.0) < 5 * math.sqrt(2.0 / n), var
    xs = np.sort(x)
    cdf = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in xs])
    steps = np.arange(n, dtype=np.float64)
    ks = float(max(np.max((steps + 1) / n - cdf), np.max(cdf - steps / n)))
    assert ks < 1.95 / math.sqrt(n), ks
    tail = int(np.sum(np.abs(x) > 4.0))
    assert 26 <= tail <= 107, tail                                       # (expected 66.4, +- 5 sigma)
    assert np.max(np.abs(x)) <= 8.6
    print("mean %.3e var-1 %.3e ks %.3e tail %d" % (mean, var - 1.0, ks, tail))


def test_neighbouring_deviates_are_uncorrelated():
    g0, g1 = stat_blocks()
    n = g0.size
    corr = lambda a, b: float(np.corrcoef(a.ravel(), b.ravel())[0, 1])
    pairs = {"entries j and j + 1": (g0[:, :, :-1], g0[:, :, 1:]), "rows k and k + 1": (g0[:-1], g0[1:]), "ids i and i + 1": (g0[:, :-1], g0[:, 1:]),
             "stream 0 and stream 1": (g0, g1)}
    for what, (a, b) in pairs.items():
        c = corr(a, b)
        print("%s: %.3e" % (what, c))
        assert abs(c) < 5 / math.sqrt(n), (what, c)
    assert not np.any(g0 == g1)


# ---- e. ------------------------------------------------------------------------------------------------------------------------------
def test_factor_form_gives_the_covariance_of_its_factor():
    cov = np.array([[4.0, 1.2, -0.6], [1.2, 1.0, 0.1], [-0.6, 0.1, 0.5]])
    S = np.linalg.cholesky(cov)
    mean = np.array([1.0, -2.0, 0.5])
    n = 1 << 18
    rows = driver_rows("rows", STAT_SEED, 0, 4, 1 << 16, 3, np.ascontiguousarray(S.T).ravel(), mean, True, True, 0, 1).reshape(n, 3)
    d = rows - mean
    sample = d.T @ d / n
    err = np.abs(sample - cov) / np.sqrt(np.outer(np.diag(cov), np.diag(cov)))
    print("covariance error, relative:", err.max())
    assert np.all(err < 6 / math.sqrt(n)), err
    assert np.all(np.abs(np.mean(rows, axis=0) - mean) < 5 * np.sqrt(np.diag(cov) / n))


# ---- f. ------------------------------------------------------------------------------------------------------------------------------
def test_error_codes_of_tiny_noise_generate():
    import tinympc_amd as tm
    L = tm.lib()
    nx, B, T = 3, 2, 2
    scale, out = np.ones(nx), np.full((T, B, nx), 7.0)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def spec(**kw):
        f = dict(seed=1, id_base=0, id_stride=1, n_steps=T, flags=tm.HOST | tm.BROADCAST, scale=dp(scale), mean=None)
        f.update(kw)
        return tm.NoiseSpec(**f)
    assert L.tiny_noise_generate(C.byref(spec()), 0, B, nx, dp(out)) == tm.OK and not np.any(out == 7.0)
    out[:] = 7.0
    bad = (dict(scale=None), dict(n_steps=0), dict(n_steps=-1), dict(id_stride=0), dict(id_stride=-1), dict(id_base=-1), dict(flags=tm.DEVICE | tm.BROADCAST),
           dict(flags=8 | tm.BROADCAST))
    for kw in bad:
        assert L.tiny_noise_generate(C.byref(spec(**kw)), 0, B, nx, dp(out)) == tm.ERR_ARG, kw
    for stream, batch, n, o in ((2, B, nx, dp(out)), (-1, B, nx, dp(out)), (0, 0, nx, dp(out)), (0, B, 0, dp(out)), (0, B, 2 * 65536 + 1, dp(out)), (0, B, nx, None)):
        assert L.tiny_noise_generate(C.byref(spec()), stream, batch, n, o) == tm.ERR_ARG, (stream, batch, n)
    assert L.tiny_noise_generate(None, 0, B, nx, dp(out)) == tm.ERR_ARG
    assert np.all(out == 7.0)                                            # (a refused call writes nothing)


def test_new_symbols_are_declared_exported_and_documented():
    import tinympc_amd as tm
    header = open(os.path.join(ROOT, "include", "tinympc_amd.h")).read()
    nm = subprocess.run(["nm", "-D", "--defined-only", tm.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    for name in NEW_SYMBOLS:
        assert "int %s(" % name in header, name
        assert name in exported, name
    L = tm.lib()
    assert L.tiny_batch_generate_disturbance(None, None) == tm.ERR_NULL and L.tiny_batch_generate_measurement_noise(None, None) == tm.ERR_NULL
    assert L.tiny_group_generate_disturbance(None, None) == tm.ERR_NULL and L.tiny_group_generate_measurement_noise(None, None) == tm.ERR_NULL
    for cls in (tm.TinyBatchSolver, tm.TinyGroupSolver):
        for name in ("generate_disturbance", "generate_measurement_noise"):
            assert callable(getattr(cls, name)), (cls, name)
    assert callable(tm.noise_generate) and tm.NOISE_FACTOR == 4
    assert C.sizeof(tm.NoiseSpec) == 48
    for word in ("Philox4x32-10", "0xD2511F53", "0xCD9E8D57", "0x9E3779B9", "0xBB67AE85", "(stream << 16) | p", "(2 n1 + 1) * 2^-53", "n2 >> 49", "(2 m + 1) * 2^-50",
                 "0x6A09E667F3BCD", "0x3FE62E42FEFA39EF", "0x3FE921FB54442D18", "TINY_NOISE_FACTOR", "disturbance_generated", "measurement_noise_generated",
                 "fma(g[j], scale[j], mean[j])", "fma(g[c], S[j + nx*c], acc)", "Out of scope: generating inside the solve kernels"):
        assert word in header, word
    text = open(os.path.join(CSRC, "noise_gen.hpp")).read()
    code = text[text.index("#pragma once"):]
    assert "#include <hip" not in code and "clang fp contract(off)" in code and "FP_CONTRACT OFF" in code
    for call in ("log(", "sin(", "cos(", "exp(", "pow(", "log1p(", "sincos("):
        assert call not in code.replace("noise_log", "").replace("noise_sincos", ""), call
