// noise_gen.hpp -- the counter-based normal generator behind tiny_batch_generate_disturbance / ..._measurement_noise / tiny_noise_generate.
// Plain C++17, no HIP include: the same text is compiled for the host and for gfx950 (TINY_NOISE_HD is `__host__ __device__` under
// hipcc, nothing otherwise) and both give the same bits: integer operations, exact integer -> double conversions, IEEE double + - * /,
// sqrt and fma only -- no libm or ocml call.  Every multiply-add below is spelled __builtin_fma; every other multiply and add stands alone (contraction is off for this file).
//
// WHAT A DEVIATE IS.  g[2p], g[2p+1] -- the two standard normals of pair p of sequence row k of the instance with the 64-bit id `id` on
// stream `stream` (0 disturbance, 1 measurement noise) under `seed` -- are a pure function of (seed, stream, id, k, p):
//   1. bits: (r0, r1, r2, r3) = Philox4x32-10(counter = (id low 32, id high 32, k, (stream << 16) | p), key = (seed low 32, seed high 32)).
//      One round, M0 = 0xD2511F53, M1 = 0xCD9E8D57, the products 32 x 32 -> 64:
//          c' = (hi(M1*c2) ^ c1 ^ k0,  lo(M1*c2),  hi(M0*c0) ^ c3 ^ k1,  lo(M0*c0));   then (k0, k1) += (0x9E3779B9, 0xBB67AE85)
//      ten rounds (the key is bumped between rounds, nine times).  p < 65 536: at most 131 072 normals a row.
//   2. uniforms, both exact: n1 = (r0 << 20) | (r1 >> 12) (52 bits), K = 2 n1 + 1, u1 = K * 2^-53 in (0, 1);
//      n2 = (r2 << 20) | (r3 >> 12), octant q = n2 >> 49, m = n2 & (2^49 - 1), t = (2 m + 1) * 2^-50 in (0, 1).
//   3. L = ln u1.  With P = the index of K's top bit (0 .. 52): e = P - 53 and the 52 mantissa bits F = (K << (52 - P)) & (2^52 - 1).
//      If F > 0x6A09E667F3BCD (sqrt 2's mantissa) the reduced argument is mr = (1 + F 2^-52) / 2 and e += 1, else mr = 1 + F 2^-52
//      (both formed as bit patterns: exponent field 0x3FE or 0x3FF over F).  Then, each line one operation:
//          f = mr - 1;  d = 2 + f;  s = f / d;  z = s * s
//          w = 1/23;  w = fma(w, z, 1/(2j+1)) for j = 10, 9, ..., 1        (the constants: the divisions 1.0 / 23.0 ... 1.0 / 3.0, rounded)
//          zw = z * w;  h = fma(s, zw, s);  L = fma((double)e, LN2, h + h)   (LN2 = 0x3FE62E42FEFA39EF)
//      -- ln(1 + f) = 2 atanh(s), the odd series through s^23.
//   4. radius: R = sqrt(-2 * L)   (-2 * L is exact).
//   5. angle theta = (q + t) pi/4, never formed: a = t for even q, 1 - t (exact) for odd q;  x = a * PIO4 (PIO4 = 0x3FE921FB54442D18);
//      y = x * x;
//          ws = -1/19!;  ws = fma(ws, y, c) for c = +1/17!, -1/15!, +1/13!, -1/11!, +1/9!, -1/7!, +1/5!, -1/3!;  yw = y * ws;  sn = fma(x, yw, x)
//          wc = +1/20!;  wc = fma(wc, y, c) for c = -1/18!, +1/16!, -1/14!, +1/12!, -1/10!, +1/8!, -1/6!, +1/4!, -1/2!;  cs = fma(y, wc, 1)
//      (the constants: 1.0 / n! with n! written out -- every n! up to 20! is a double --, rounded, then negated where the sign says so).
//      cos theta = (q in {1, 2, 5, 6} ? sn : cs), negated for q in {2, 3, 4, 5};  sin theta = (q in {1, 2, 5, 6} ? cs : sn), negated for q >= 4.
//   6. g[2p] = R * cos theta,  g[2p+1] = R * sin theta (one multiplication each).  |g| <= sqrt(2 * 53 ln 2) < 8.6 since u1 >= 2^-53.
//
// FROM NORMALS TO A SEQUENCE ROW.  Instance i of a batch has id = id_base + i * id_stride (64-bit, wrapping).  Row k of that instance:
//   diagonal scale:              row[j] = fma(g[j], scale[j], mean[j])
//   factor scale (nx x nx column-major S, the upper triangle read like any other entry):
//                                acc = mean[j];  acc = fma(g[c], S[j + nx c], acc) for c = 0 .. nx-1 ascending;  row[j] = acc
//   a null mean is zeros.  For odd nx the second deviate of the last pair is not used.
//
// Out of scope: generating inside the solve kernels' PD / PM forms instead of filling a buffer they read (it would save the buffer's
// memory, not time, and costs a MODE bit and registers in forms that sit at 255 VGPRs); distributions other than the normal;
// tiny_codegen, tiny_solve_batch and the drop-in structs.
#pragma once
#include <stddef.h>
#include <stdint.h>

#pragma clang fp contract(off)
#pragma STDC FP_CONTRACT OFF

#if defined(__HIP__) || defined(__HIPCC__)
#define TINY_NOISE_HD __host__ __device__
#else
#define TINY_NOISE_HD
#endif

namespace tinympc_amd {

struct PhiloxBits { uint32_t r[4]; };
TINY_NOISE_HD inline PhiloxBits philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return PhiloxBits{{c0, c1, c2, c3}};
}

TINY_NOISE_HD inline double noise_bits_to_double(uint64_t bits) {
    double d;
    __builtin_memcpy(&d, &bits, sizeof(d));
    return d;
}

// ln u1 of u1 = K * 2^-53, K odd in [1, 2^53)
TINY_NOISE_HD inline double noise_log_u1(uint64_t K) {
#pragma clang fp contract(off)
    const int P = 63 - __builtin_clzll(K);
    int e = P - 53;
    const uint64_t F = (K << (52 - P)) & 0xFFFFFFFFFFFFFull;
    uint64_t top = 0x3FFull;
    if (F > 0x6A09E667F3BCDull) { top = 0x3FEull; e += 1; }
    const double mr = noise_bits_to_double((top << 52) | F);
    const double f = mr - 1.0;
    const double d = 2.0 + f;
    const double s = f / d;
    const double z = s * s;
    double w = 1.0 / 23.0;
    w = __builtin_fma(w, z, 1.0 / 21.0);
    w = __builtin_fma(w, z, 1.0 / 19.0);
    w = __builtin_fma(w, z, 1.0 / 17.0);
    w = __builtin_fma(w, z, 1.0 / 15.0);
    w = __builtin_fma(w, z, 1.0 / 13.0);
    w = __builtin_fma(w, z, 1.0 / 11.0);
    w = __builtin_fma(w, z, 1.0 / 9.0);
    w = __builtin_fma(w, z, 1.0 / 7.0);
    w = __builtin_fma(w, z, 1.0 / 5.0);
    w = __builtin_fma(w, z, 1.0 / 3.0);
    const double zw = z * w;
    const double h = __builtin_fma(s, zw, s);
    return __builtin_fma((double)e, noise_bits_to_double(0x3FE62E42FEFA39EFull), h + h);
}

// sin and cos of x = a * pi/4, a in (0, 1)
struct NoiseSinCos { double sn, cs; };
TINY_NOISE_HD inline NoiseSinCos noise_sincos_octant(double a) {
#pragma clang fp contract(off)
    const double x = a * noise_bits_to_double(0x3FE921FB54442D18ull);
    const double y = x * x;
    double ws = -(1.0 / 121645100408832000.0);
    ws = __builtin_fma(ws, y, 1.0 / 355687428096000.0);
    ws = __builtin_fma(ws, y, -(1.0 / 1307674368000.0));
    ws = __builtin_fma(ws, y, 1.0 / 6227020800.0);
    ws = __builtin_fma(ws, y, -(1.0 / 39916800.0));
    ws = __builtin_fma(ws, y, 1.0 / 362880.0);
    ws = __builtin_fma(ws, y, -(1.0 / 5040.0));
    ws = __builtin_fma(ws, y, 1.0 / 120.0);
    ws = __builtin_fma(ws, y, -(1.0 / 6.0));
    const double yw = y * ws;
    const double sn = __builtin_fma(x, yw, x);
    double wc = 1.0 / 2432902008176640000.0;
    wc = __builtin_fma(wc, y, -(1.0 / 6402373705728000.0));
    wc = __builtin_fma(wc, y, 1.0 / 20922789888000.0);
    wc = __builtin_fma(wc, y, -(1.0 / 87178291200.0));
    wc = __builtin_fma(wc, y, 1.0 / 479001600.0);
    wc = __builtin_fma(wc, y, -(1.0 / 3628800.0));
    wc = __builtin_fma(wc, y, 1.0 / 40320.0);
    wc = __builtin_fma(wc, y, -(1.0 / 720.0));
    wc = __builtin_fma(wc, y, 1.0 / 24.0);
    wc = __builtin_fma(wc, y, -(1.0 / 2.0));
    const double cs = __builtin_fma(y, wc, 1.0);
    return NoiseSinCos{sn, cs};
}

// the two standard normals of pair p of row k of instance `id` on stream `stream` under `seed`
struct NoisePair { double g0, g1; };
TINY_NOISE_HD inline NoisePair noise_pair(uint64_t seed, uint32_t stream, uint64_t id, uint32_t k, uint32_t p) {
#pragma clang fp contract(off)
    const PhiloxBits b = philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), k, (stream << 16) | p, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t n1 = ((uint64_t)b.r[0] << 20) | (b.r[1] >> 12), n2 = ((uint64_t)b.r[2] << 20) | (b.r[3] >> 12);
    const double L = noise_log_u1(2 * n1 + 1);
    const double R = __builtin_sqrt(-2.0 * L);
    const uint32_t q = (uint32_t)(n2 >> 49);
    const uint64_t m = n2 & 0x1FFFFFFFFFFFFull;
    const double t = (double)(int64_t)(2 * m + 1) * noise_bits_to_double(0x3CD0000000000000ull);      // (2 m + 1) * 2^-50: 50 bits, exact
    const NoiseSinCos v = noise_sincos_octant((q & 1) ? 1.0 - t : t);
    const bool swap = ((q + 1) >> 1) & 1;
    double c = swap ? v.sn : v.cs, s = swap ? v.cs : v.sn;
    if (((q + 2) >> 2) & 1) c = -c;
    if (q >> 2) s = -s;
    return NoisePair{R * c, R * s};
}

// what one call describes (TinyNoiseSpec with the stream and the shape, the arrays wherever the caller of these functions can read them)
struct NoiseFill {
    uint64_t seed, id_base, id_stride;
    uint32_t stream;
    int n_steps, batch, nx;
    bool factor, broadcast;                      // scale is S (nx x nx) / scale and mean are one for all
    const double *scale, *mean;                  // mean may be null
};
TINY_NOISE_HD inline int noise_pairs(int nx) { return (nx + 1) / 2; }

// diagonal form: entries 2p and 2p+1 (the second only where 2p+1 < nx) of row k of batch instance i -> out2[0], out2[1]
TINY_NOISE_HD inline void noise_diagonal_pair(const NoiseFill& F, uint32_t k, size_t i, int p, double* out2) {
    const NoisePair g = noise_pair(F.seed, F.stream, F.id_base + (uint64_t)i * F.id_stride, k, (uint32_t)p);
    const size_t at = (F.broadcast ? 0 : i * (size_t)F.nx) + 2 * (size_t)p;
    out2[0] = __builtin_fma(g.g0, F.scale[at], F.mean ? F.mean[at] : 0.0);
    if (2 * p + 1 < F.nx) out2[1] = __builtin_fma(g.g1, F.scale[at + 1], F.mean ? F.mean[at + 1] : 0.0);
}

// factor form, nx <= 32: row k of batch instance i -> row[0 .. nx).  The accumulators are indexed by constants only (the loops over j
// unroll completely), so that the device build keeps them in registers
TINY_NOISE_HD inline void noise_factor_row32(const NoiseFill& F, uint32_t k, size_t i, double* row) {
    const int nx = F.nx;
    const uint64_t id = F.id_base + (uint64_t)i * F.id_stride;
    const double* S = F.scale + (F.broadcast ? 0 : i * (size_t)nx * nx);
    const double* mean = F.mean ? F.mean + (F.broadcast ? 0 : i * (size_t)nx) : nullptr;
    double acc[32];
#pragma unroll
    for (int j = 0; j < 32; ++j) acc[j] = (mean && j < nx) ? mean[j] : 0.0;
    for (int p = 0; 2 * p < nx; ++p) {
        const NoisePair g = noise_pair(F.seed, F.stream, id, k, (uint32_t)p);
        const double* col = S + (size_t)nx * 2 * p;
#pragma unroll
        for (int j = 0; j < 32; ++j) if (j < nx) acc[j] = __builtin_fma(g.g0, col[j], acc[j]);
        if (2 * p + 1 < nx) {
#pragma unroll
            for (int j = 0; j < 32; ++j) if (j < nx) acc[j] = __builtin_fma(g.g1, col[nx + j], acc[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < 32; ++j) if (j < nx) row[j] = acc[j];
}

// factor form, any nx, on the host: the same chain with the normals of the row in g[0 .. 2 * noise_pairs(nx)) (scratch of the caller's)
inline void noise_factor_row_host(const NoiseFill& F, uint32_t k, size_t i, double* g, double* row) {
    const int nx = F.nx;
    const uint64_t id = F.id_base + (uint64_t)i * F.id_stride;
    const double* S = F.scale + (F.broadcast ? 0 : i * (size_t)nx * nx);
    const double* mean = F.mean ? F.mean + (F.broadcast ? 0 : i * (size_t)nx) : nullptr;
    for (int p = 0; 2 * p < nx; ++p) {
        const NoisePair v = noise_pair(F.seed, F.stream, id, k, (uint32_t)p);
        g[2 * p] = v.g0; g[2 * p + 1] = v.g1;
    }
    for (int j = 0; j < nx; ++j) {
        double acc = mean ? mean[j] : 0.0;
        for (int c = 0; c < nx; ++c) acc = __builtin_fma(g[c], S[j + (size_t)nx * c], acc);
        row[j] = acc;
    }
}

// the whole block on the host: out [n_steps][batch][nx], exactly as the device fills it
inline void noise_fill_host(const NoiseFill& F, double* out, double* g_scratch) {
    for (int k = 0; k < F.n_steps; ++k)
        for (size_t i = 0; i < (size_t)F.batch; ++i) {
            double* row = out + ((size_t)k * F.batch + i) * F.nx;
            if (F.factor) { noise_factor_row_host(F, (uint32_t)k, i, g_scratch, row); continue; }
            for (int p = 0; 2 * p < F.nx; ++p) {
                double two[2];
                noise_diagonal_pair(F, (uint32_t)k, i, p, two);
                row[2 * p] = two[0];
                if (2 * p + 1 < F.nx) row[2 * p + 1] = two[1];
            }
        }
}

}  // namespace tinympc_amd
