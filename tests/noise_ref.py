"""An independent restatement of the counter-based normal generator (tinympc_amd/csrc/noise_gen.hpp, tiny_batch_generate_disturbance /
..._measurement_noise / tiny_noise_generate), written from the header's comment alone (CPU only).

  * Philox4x32-10 in Python integers;
  * the two uniforms as exact Fractions: u1 = K / 2^53 with K = 2 n1 + 1, t = (2 m + 1) / 2^50, the octant q;
  * the library's ln / sin / cos chains and the row rules, every fma through the Fraction-based fma of tests/plant_cases.py (the exact
    product and sum, rounded once); a lone * + - / of two doubles and math.sqrt are correctly rounded as Python does them;
  * a libm Box-Muller (math.log, math.cos, math.sin, math.sqrt) on the same uniforms, for the accuracy test.

philox_many is the same Philox on numpy uint64 arrays, for the tests that need many uniforms (checked against the scalar one)."""
import functools
import math
import struct
from fractions import Fraction

import numpy as np

from plant_cases import fma

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF
LN2 = struct.unpack("<d", struct.pack("<Q", 0x3FE62E42FEFA39EF))[0]
PIO4 = struct.unpack("<d", struct.pack("<Q", 0x3FE921FB54442D18))[0]
SQRT2_MANTISSA = 0x6A09E667F3BCD
FACT = [math.factorial(n) for n in range(21)]
assert all(float(f) == f for f in FACT)                      # (every n! up to 20! is a double)

KNOWN_ANSWERS = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                 ((MASK,) * 4, (MASK,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                 ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(counter, key):
    c0, c1, c2, c3 = counter
    k0, k1 = key
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def philox_many(c0, c1, c2, c3, k0, k1):
    """the same on numpy arrays (uint64 holding 32-bit words; broadcast against each other)"""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0), int(k1)
    m = np.uint64(MASK)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def counter(seed, stream, ident, k, p):
    ident &= (1 << 64) - 1
    return (ident & MASK, ident >> 32, k, (stream << 16) | p), (seed & MASK, (seed >> 32) & MASK)


def draws(seed, stream, ident, k, p):
    """(K, q, m): u1 = K / 2^53, theta = (q + (2 m + 1) / 2^50) pi/4"""
    r0, r1, r2, r3 = philox(*counter(seed, stream, ident, k, p))
    n1, n2 = (r0 << 20) | (r1 >> 12), (r2 << 20) | (r3 >> 12)
    return 2 * n1 + 1, n2 >> 49, n2 & ((1 << 49) - 1)


def uniforms(seed, stream, ident, k, p):
    K, q, m = draws(seed, stream, ident, k, p)
    return Fraction(K, 1 << 53), q, Fraction(2 * m + 1, 1 << 50)


def log_u1(K):
    """the library's ln(K / 2^53)"""
    P = K.bit_length() - 1
    e = P - 53
    F = (K << (52 - P)) & ((1 << 52) - 1)
    mr = 1.0 + F / float(1 << 52)                            # (exact: 53 bits)
    if F > SQRT2_MANTISSA:
        mr, e = mr / 2.0, e + 1
    f = mr - 1.0
    d = 2.0 + f
    s = f / d
    z = s * s
    w = 1.0 / 23.0
    for j in range(10, 0, -1):
        w = fma(w, z, 1.0 / (2 * j + 1))
    zw = z * w
    h = fma(s, zw, s)
    return fma(float(e), LN2, h + h)


def sincos_octant(a):
    """the library's (sin, cos) of a * pi/4, a in (0, 1)"""
    x = a * PIO4
    y = x * x
    ws = -(1.0 / FACT[19])
    for n in range(17, 1, -2):
        c = 1.0 / FACT[n]
        ws = fma(ws, y, c if n % 4 == 1 else -c)
    yw = y * ws
    sn = fma(x, yw, x)
    wc = 1.0 / FACT[20]
    for n in range(18, 0, -2):
        c = 1.0 / FACT[n]
        wc = fma(wc, y, c if n % 4 == 0 else -c)
    cs = fma(y, wc, 1.0)
    return sn, cs


def pair_from_draws(K, q, m):
    R = math.sqrt(-2.0 * log_u1(K))
    t = float(Fraction(2 * m + 1, 1 << 50))                  # (exact: 50 bits)
    sn, cs = sincos_octant(1.0 - t if q & 1 else t)
    c, s = (sn, cs) if q in (1, 2, 5, 6) else (cs, sn)
    if q in (2, 3, 4, 5):
        c = -c
    if q >= 4:
        s = -s
    return R * c, R * s


def pair(seed, stream, ident, k, p):
    """the two standard normals g[2p], g[2p+1]"""
    return pair_from_draws(*draws(seed, stream, ident, k, p))


def pair_libm_from_draws(K, q, m):
    u1, t = K / float(1 << 53), (2 * m + 1) / float(1 << 50)
    R, theta = math.sqrt(-2.0 * math.log(u1)), (q + t) * (math.pi / 4)
    return R * math.cos(theta), R * math.sin(theta)


def pair_libm(seed, stream, ident, k, p):
    return pair_libm_from_draws(*draws(seed, stream, ident, k, p))


def normals(seed, stream, ident, k, nx):
    g = []
    for p in range((nx + 1) // 2):
        g.extend(pair(seed, stream, ident, k, p))
    return g[:nx]


@functools.lru_cache(maxsize=64)
def normals_block(seed, stream, n_steps, batch, nx, id_base=0, id_stride=1):
    """g [n_steps, batch, nx]: the standard normals of every row (computed once per argument set and shared; never modified)"""
    out = np.array([[normals(seed, stream, id_base + i * id_stride, k, nx) for i in range(batch)] for k in range(n_steps)], dtype=np.float64)
    out.setflags(write=False)
    return out


def rows(seed, stream, n_steps, batch, nx, scale, mean=None, factor=False, id_base=0, id_stride=1):
    """[n_steps, batch, nx] as the library fills them.  scale: (nx,) / (batch, nx), or with factor (nx, nx) / (batch, nx, nx) as
    MATRICES S[j, c] (the C ABI takes them column-major); mean: None, (nx,) or (batch, nx)"""
    scale = np.asarray(scale, dtype=np.float64)
    per = scale.ndim == (3 if factor else 2)
    mean = None if mean is None else np.asarray(mean, dtype=np.float64)
    out = np.zeros((n_steps, batch, nx))
    block = normals_block(seed, stream, n_steps, batch, nx, id_base, id_stride)
    for k in range(n_steps):
        for i in range(batch):
            g = block[k, i]
            S = scale[i] if per else scale
            mu = np.zeros(nx) if mean is None else (mean[i] if mean.ndim == 2 else mean)
            for j in range(nx):
                if not factor:
                    out[k, i, j] = fma(g[j], S[j], mu[j])
                    continue
                acc = float(mu[j])
                for c in range(nx):
                    acc = fma(g[c], S[j, c], acc)
                out[k, i, j] = acc
    return out
