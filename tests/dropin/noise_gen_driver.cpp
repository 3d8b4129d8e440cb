// noise_gen_driver.cpp -- tinympc_amd/csrc/noise_gen.hpp alone under the host compiler (tests/test_noise_gen_cpu.py).
//   philox                     stdin: lines of "c0 c1 c2 c3 k0 k1" in hex            -> stdout: "r0 r1 r2 r3" in hex, a line each
//   rows | rows32  seed stream n_steps batch nx factor broadcast has_mean id_base id_stride
//                              stdin: scale then mean as raw doubles                  -> stdout: [n_steps][batch][nx] raw doubles
//                              (rows: noise_fill_host; rows32: the device's per-thread routines, nx <= 32)
//   pairs  seed stream k p id0 count                                                  -> stdout: count x (g0, g1) raw doubles, ids id0 ..
#include "noise_gen.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace tinympc_amd;

static std::vector<double> read_doubles(size_t n) {
    std::vector<double> v(n);
    if (n && fread(v.data(), sizeof(double), n, stdin) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "philox")) {
        unsigned c[4], k[2];
        while (scanf("%x %x %x %x %x %x", &c[0], &c[1], &c[2], &c[3], &k[0], &k[1]) == 6) {
            const PhiloxBits b = philox4x32_10(c[0], c[1], c[2], c[3], k[0], k[1]);
            printf("%08x %08x %08x %08x\n", b.r[0], b.r[1], b.r[2], b.r[3]);
        }
        return 0;
    }
    if (!strcmp(argv[1], "pairs") && argc == 8) {
        const uint64_t seed = strtoull(argv[2], nullptr, 0), id0 = strtoull(argv[6], nullptr, 0), count = strtoull(argv[7], nullptr, 0);
        const uint32_t stream = (uint32_t)atoi(argv[3]), k = (uint32_t)strtoul(argv[4], nullptr, 0), p = (uint32_t)strtoul(argv[5], nullptr, 0);
        std::vector<double> out(2 * count);
        for (uint64_t i = 0; i < count; ++i) {
            const NoisePair g = noise_pair(seed, stream, id0 + i, k, p);
            out[2 * i] = g.g0; out[2 * i + 1] = g.g1;
        }
        fwrite(out.data(), sizeof(double), out.size(), stdout);
        return 0;
    }
    if ((!strcmp(argv[1], "rows") || !strcmp(argv[1], "rows32")) && argc == 12) {
        NoiseFill F = {};
        F.seed = strtoull(argv[2], nullptr, 0); F.stream = (uint32_t)atoi(argv[3]); F.n_steps = atoi(argv[4]); F.batch = atoi(argv[5]); F.nx = atoi(argv[6]);
        F.factor = atoi(argv[7]) != 0; F.broadcast = atoi(argv[8]) != 0;
        const bool has_mean = atoi(argv[9]) != 0;
        F.id_base = strtoull(argv[10], nullptr, 0); F.id_stride = strtoull(argv[11], nullptr, 0);
        const size_t sets = F.broadcast ? 1 : (size_t)F.batch;
        const std::vector<double> scale = read_doubles(sets * F.nx * (F.factor ? F.nx : 1)), mean = read_doubles(has_mean ? sets * F.nx : 0);
        F.scale = scale.data(); F.mean = has_mean ? mean.data() : nullptr;
        std::vector<double> out((size_t)F.n_steps * F.batch * F.nx), g((size_t)2 * noise_pairs(F.nx));
        if (!strcmp(argv[1], "rows")) noise_fill_host(F, out.data(), g.data());
        else {
            if (F.nx > 32) return 2;
            for (int k = 0; k < F.n_steps; ++k)
                for (size_t i = 0; i < (size_t)F.batch; ++i) {
                    double* row = out.data() + ((size_t)k * F.batch + i) * F.nx;
                    if (F.factor) { noise_factor_row32(F, (uint32_t)k, i, row); continue; }
                    for (int p = 0; p < noise_pairs(F.nx); ++p) {
                        double two[2];
                        noise_diagonal_pair(F, (uint32_t)k, i, p, two);
                        row[2 * p] = two[0];
                        if (2 * p + 1 < F.nx) row[2 * p + 1] = two[1];
                    }
                }
        }
        fwrite(out.data(), sizeof(double), out.size(), stdout);
        return 0;
    }
    return 2;
}
