// lane_tables_dump.cpp -- the host-built lane tables as raw bytes, without a GPU: fills a TinyBatch by hand (no HIP call), runs
// build_tables / build_tile_tables / build_general_tables (and build_adaptive_table) of csrc/batch_tables.hip and writes what they
// left.  Stand-alone, one command:
//     hipcc --offload-arch=gfx950 -std=c++17 -I tinympc_amd/csrc -x hip tests/dropin/lane_tables_dump.cpp tinympc_amd/csrc/batch_tables.hip -o dump
//     dump case OUT nx nu N [key=value ...]     one problem: a record of tables AND inputs (tests/test_lane_tables_cpu.py reads it)
//     dump sweep HASHES                         every combination of profiles/lane_tables.md: the tables' bytes on stdout, one line
//                                               per combination (its key and the FNV-1a hash of its bytes) in HASHES
// Two builds whose sweeps write the same bytes build the same tables.  -DLANE_TABLES_DUMP_BEFORE builds against a tree from before
// the builders shared one mapping (it had no build_adaptive_table, two uniform flags, and box_is_uniform in another unit): that mode
// served the one comparison profiles/lane_tables.md records and can be deleted with the next change to this file.
// keys: bounds=none|same|xdiff|udiff|nan|unan  cone=none|state|input|both|two|shared  lin=K tlin=K (half-spaces per knot, all four families)
//       sb ib ssoc isoc sl il tsl til = 0|1 (the enable switches)  prime=1 (A, B and the sensitivity tables are distinct primes)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <string>

#include "batch_impl.hpp"
#include "batch_dispatch.hpp"

namespace tinympc_amd {
int fail(TinyBatch*, int code, const char*, ...) { return code; }
#ifdef LANE_TABLES_DUMP_BEFORE
bool box_is_uniform(const TinyBatch*) { return true; }     // (AND-ed to the tile table's own scan there)
#endif
}  // namespace tinympc_amd
using namespace tinympc_amd;

#ifdef LANE_TABLES_DUMP_BEFORE
#define TILE_UNIFORM tile_bounds_uniform
#else
#define TILE_UNIFORM bounds_uniform
#endif

typedef std::map<std::string, std::string> Keys;
static int geti(const Keys& k, const char* name, int dflt) { auto it = k.find(name); return it == k.end() ? dflt : atoi(it->second.c_str()); }
static std::string gets(const Keys& k, const char* name, const char* dflt) { auto it = k.find(name); return it == k.end() ? dflt : it->second; }

static int next_prime(int& p) {
    for (++p;; ++p) {
        bool ok = p > 1;
        for (int d = 2; d * d <= p && ok; ++d) ok = p % d != 0;
        if (ok) return p;
    }
}

// dynamics and cost of a shape: non-symmetric stable A, full B, f != 0, distinct Q and R diagonals; the cache from them
static void set_shape(TinyBatch& b, int nx, int nu, int N, bool prime) {
    b.nx = nx; b.nu = nu; b.N = N;
    b.A = Mat(nx, nx); b.B = Mat(nx, nu); b.f = Mat(nx, 1);
    b.Qw.assign(nx, 0.0); b.Rw.assign(nu, 0.0);
    const double rho = 1.5;
    for (int i = 0; i < nx; ++i) {
        for (int j = 0; j < nx; ++j) b.A(i, j) = (i == j ? 0.8 : 0.0) + 0.01 * ((3 * i + 7 * j) % 11 - 4) / (1.0 + 0.1 * nx);
        for (int m = 0; m < nu; ++m) b.B(i, m) = 0.05 * ((5 * i + 2 * m) % 9 + 1);
        b.f(i, 0) = 0.001 * (i + 1);
        b.Qw[i] = 10.0 + i + rho;
    }
    for (int m = 0; m < nu; ++m) b.Rw[m] = 2.0 + 0.5 * m + rho;
    if (!precompute_cache(b.A, b.B, b.f, Mat::diag(b.Qw), Mat::diag(b.Rw), rho, &b.cache)) { fprintf(stderr, "singular cache\n"); exit(2); }
    b.dKinf.clear(); b.dPinf.clear(); b.dC1.clear(); b.dC2.clear();
    if (prime) {        // only the ATAB tables read these: a transposed index cannot land on an equal number
        int p = 1;
        for (double& v : b.A.a) v = next_prime(p);
        for (double& v : b.B.a) v = next_prime(p);
        b.dKinf.resize((size_t)nu * nx); b.dPinf.resize((size_t)nx * nx); b.dC1.resize((size_t)nu * nu); b.dC2.resize((size_t)nx * nx);
        for (auto* t : {&b.dKinf, &b.dPinf, &b.dC1, &b.dC2})
            for (double& v : *t) v = next_prime(p);
    }
}

static void set_case(TinyBatch& b, const Keys& k) {
    const int nx = b.nx, nu = b.nu, N = b.N;
    b.set = Settings();
    b.set.en_state_bound = geti(k, "sb", 1); b.set.en_input_bound = geti(k, "ib", 1);
    const std::string bounds = gets(k, "bounds", "none");
    b.have_bounds = bounds != "none";
    b.x_min.assign((size_t)N * nx, 0.0); b.x_max = b.x_min; b.u_min.assign((size_t)(N - 1) * nu, 0.0); b.u_max = b.u_min;
    if (b.have_bounds) {
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < nx; ++j) { b.x_min[(size_t)i * nx + j] = -5.0 - j; b.x_max[(size_t)i * nx + j] = 6.0 + 2 * j; }
        for (int i = 0; i < N - 1; ++i)
            for (int a = 0; a < nu; ++a) { b.u_min[(size_t)i * nu + a] = -0.5 - a; b.u_max[(size_t)i * nu + a] = 0.75 + a; }
        // (the last knot that has the bound: a difference at knot 0 would move the value every other knot is compared with)
        if (bounds == "xdiff") b.x_max[(size_t)(N - 1) * nx + nx - 1] += 1.0;
        if (bounds == "udiff") b.u_min[(size_t)(N - 2) * nu + nu - 1] -= 1.0;
        if (bounds == "unan") b.u_max[0] = std::numeric_limits<double>::quiet_NaN();     // (N = 2: the only input knot)
        if (bounds == "nan") b.x_min[(size_t)(N - 1) * nx] = std::numeric_limits<double>::quiet_NaN();
    } else {
        b.x_min.clear(); b.x_max.clear(); b.u_min.clear(); b.u_max.clear();
    }
    const std::string cone = gets(k, "cone", "none");
    b.set.en_state_soc = geti(k, "ssoc", 0); b.set.en_input_soc = geti(k, "isoc", 0);
    b.Acx.clear(); b.cx.clear(); b.Acu.clear(); b.cu.clear();
    if (cone == "state" || cone == "both") { b.Acx = {nx - 3}; b.cx = {0.25}; }
    if (cone == "input" || cone == "both") { b.Acu = {nu - 3}; b.cu = {0.7}; }
    if (cone == "two") { b.Acx = {0, 3}; b.cx = {0.25, 0.5}; }
    if (cone == "shared") { b.Acx = {0, 1}; b.cx = {0.25, 0.5}; }
    const int lin = geti(k, "lin", 0), tlin = geti(k, "tlin", 0);
    b.set.en_state_linear = geti(k, "sl", 0); b.set.en_input_linear = geti(k, "il", 0);
    b.set.en_tv_state_linear = geti(k, "tsl", 0); b.set.en_tv_input_linear = geti(k, "til", 0);
    b.nsl = lin; b.nil = lin ? (lin == 2 ? 1 : lin) : 0;              // (2: nsl = 2, nil = 1)
    b.ntsl = tlin; b.ntil = tlin ? (tlin == 2 ? 1 : tlin) : 0;
    auto coef = [](std::vector<double>& A, std::vector<double>& bv, int rows, int n, double seed) {
        A.resize((size_t)rows * n); bv.resize(rows);
        for (int r = 0; r < rows; ++r) {
            for (int c = 0; c < n; ++c) A[(size_t)r * n + c] = seed + 0.125 * ((r * 5 + c * 3) % 13) - 0.5;
            bv[r] = 2.0 + seed + 0.25 * r;
        }
    };
    coef(b.Alin_x, b.blin_x, b.nsl, nx, 0.1); coef(b.Alin_u, b.blin_u, b.nil, nu, 0.2);
    coef(b.tvA_x, b.tvb_x, N * b.ntsl, nx, 0.3); coef(b.tvA_u, b.tvb_u, (N - 1) * b.ntil, nu, 0.4);
}

struct Out {
    FILE* f;
    uint64_t hash = 1469598103934665603ull;
    void bytes(const void* p, size_t n) {
        if (f) fwrite(p, 1, n, f);
        for (size_t i = 0; i < n; ++i) hash = (hash ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
    }
    void i32(int v) { bytes(&v, sizeof(v)); }
    void vec(const std::vector<double>& v) { i32((int)v.size()); bytes(v.data(), v.size() * sizeof(double)); }
};

// the record of one case: [count, doubles] for h_tab, h_ttab, h_gtab, then the 19 offsets of gargs, then the two uniform flags.  A table
// that is not built for the shape (one-row layout: nx + nu <= 16) has count 0
static void dump_tables(TinyBatch& b, int W, bool general_only, Out& o) {
    b.tile_dyn = TileEntry{b.nx, b.nu, b.N, W, 1, 0, nullptr, nullptr, nullptr, nullptr};
    b.tile = &b.tile_dyn;
    b.h_tab.clear(); b.h_ttab.clear();
    int flag_row = -1, flag_tile = -1;
    if (!general_only) {
        if (b.nx + b.nu <= 16) { build_tables(&b); flag_row = b.bounds_uniform; }
        build_tile_tables(&b); flag_tile = b.TILE_UNIFORM;
    }
    build_general_tables(&b);
    o.vec(b.h_tab); o.vec(b.h_ttab); o.vec(b.h_gtab);
    const GeneralArgs& g = b.gargs;
    for (int v : {g.o_mb, g.o_mf1, g.o_mf2, g.o_pt, g.o_cb, g.o_cf, g.o_qr, g.o_lo, g.o_hi, g.o_sc, g.o_ic, g.o_ax, g.o_bx, g.o_au, g.o_bu, g.o_tax,
                  g.o_tbx, g.o_tau, g.o_tbu}) o.i32(v);
    o.i32(flag_row); o.i32(flag_tile);
}

static int sweep(const char* hashes_path) {
    FILE* hf = fopen(hashes_path, "w");
    if (!hf) return 2;
    const int shapes[][3] = {{1, 1, 2}, {2, 2, 3}, {12, 4, 10}, {6, 3, 10}, {8, 8, 4}, {15, 1, 4}, {20, 8, 10}, {16, 16, 4}, {31, 1, 4}};
    const char* bounds[] = {"bounds=none", "bounds=same", "bounds=xdiff", "bounds=udiff", "bounds=nan", "bounds=unan", "bounds=same sb=0", "bounds=same ib=0"};
    const char* cones[] = {"cone=none", "cone=state ssoc=1", "cone=state ssoc=0", "cone=input isoc=1", "cone=input isoc=0",
                           "cone=both ssoc=1 isoc=1", "cone=both ssoc=0 isoc=0", "cone=two ssoc=1", "cone=shared ssoc=1"};
    const char* lins[] = {"lin=0", "lin=2 sl=1 il=1", "lin=5 sl=1 il=1", "lin=33 sl=1 il=1", "tlin=2 tsl=1 til=1", "tlin=5 tsl=1 til=1",
                          "tlin=33 tsl=1 til=1", "lin=2 sl=0 il=1", "lin=2 sl=1 il=0", "tlin=2 tsl=0 til=1", "tlin=2 tsl=1 til=0"};
    Out all{stdout};
    int count = 0;
    for (auto& s : shapes) {
        TinyBatch b;
        set_shape(b, s[0], s[1], s[2], false);
        const int W = s[0] + s[1] <= 16 ? 1 : 2;
        for (const char* bd : bounds)
            for (const char* cn : cones)
                for (const char* ln : lins) {
                    const std::string spec = std::string(bd) + " " + cn + " " + ln;
                    Keys k;
                    char buf[256];
                    snprintf(buf, sizeof(buf), "%s", spec.c_str());
                    for (char* tok = strtok(buf, " "); tok; tok = strtok(nullptr, " ")) { char* eq = strchr(tok, '='); k[std::string(tok, eq - tok)] = eq + 1; }
                    const std::string cone = gets(k, "cone", "none");
                    // cones need three rows (two cones: six; a shared row: four) in their family
                    if ((cone == "state" || cone == "both") && s[0] < 3) continue;
                    if ((cone == "input" || cone == "both") && s[1] < 3) continue;
                    if ((cone == "two" && s[0] < 6) || (cone == "shared" && s[0] < 4)) continue;
                    set_case(b, k);
                    Out one{nullptr};
                    dump_tables(b, W, cone == "shared", one);
                    dump_tables(b, W, cone == "shared", all);
                    fprintf(hf, "%d %d %d W=%d %s  %016llx\n", s[0], s[1], s[2], W, spec.c_str(), (unsigned long long)one.hash);
                    ++count;
                }
    }
    fprintf(hf, "%d combinations, all bytes %016llx\n", count, (unsigned long long)all.hash);
    fclose(hf);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 3 && !strcmp(argv[1], "sweep")) return sweep(argv[2]);
    if (argc < 6 || strcmp(argv[1], "case")) { fprintf(stderr, "usage: %s case OUT nx nu N [key=value ...] | sweep HASHES\n", argv[0]); return 2; }
    Keys k;
    for (int i = 6; i < argc; ++i) { const char* eq = strchr(argv[i], '='); if (eq) k[std::string(argv[i], eq - argv[i])] = eq + 1; }
    TinyBatch b;
    set_shape(b, atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), geti(k, "prime", 0) != 0);
    set_case(b, k);
    Out o{fopen(argv[2], "wb")};
    if (!o.f) return 2;
    dump_tables(b, b.nx + b.nu <= 16 ? 1 : 2, false, o);
    // the inputs the tables were built from (matrices column-major): A, B, f, Qw, Rw, Kinf, Pinf, Quu_inv, AmBKt, APf, BPf; the sensitivity
    // tables dK, dP, dC1, dC2 (prime=1; empty otherwise); the bounds, the cones (first rows, coefficients), the half-spaces; then the
    // ATAB table of the sensitivity tables (prime=1)
    const TinyBatch& cb = b;
    const Cache& c = cb.cache;
    const std::vector<double> acx(cb.Acx.begin(), cb.Acx.end()), acu(cb.Acu.begin(), cb.Acu.end());
    for (const std::vector<double>* v : {&cb.A.a, &cb.B.a, &cb.f.a, &cb.Qw, &cb.Rw, &c.Kinf.a, &c.Pinf.a, &c.Quu_inv.a, &c.AmBKt.a, &c.APf.a, &c.BPf.a,
                                         &cb.dKinf, &cb.dPinf, &cb.dC1, &cb.dC2, &cb.x_min, &cb.x_max, &cb.u_min, &cb.u_max, &acx, &cb.cx, &acu, &cb.cu,
                                         &cb.Alin_x, &cb.blin_x, &cb.Alin_u, &cb.blin_u, &cb.tvA_x, &cb.tvb_x, &cb.tvA_u, &cb.tvb_u}) o.vec(*v);
#ifndef LANE_TABLES_DUMP_BEFORE
    o.vec(b.dKinf.empty() ? std::vector<double>() : build_adaptive_table(&b));
#endif
    fclose(o.f);
    return 0;
}
