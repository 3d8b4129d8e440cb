// instance_halfspaces_dump.cpp -- what the fill rule of a half-space block (csrc/lane_tables.hpp halfspace_entry: the one statement the
// helper kernel behind tiny_batch_set_instance_linear_constraints / ..._tv_... calls) puts in every (constraint k, lane), without a GPU.
// Stand-alone, one command:
//     hipcc --offload-arch=gfx950 -std=c++17 -I tinympc_amd/csrc -x hip tests/dropin/instance_halfspaces_dump.cpp tinympc_amd/csrc/batch_tables.hip -o dump
//     dump nx nu N n_state n_input n_tv_state n_tv_input en_state en_input en_tv_state en_tv_input km input.bin
// input.bin: one instance's eight arrays as doubles in the setters' own (column-major) layout, one after the other -- Alin_x
// (n_state x nx), blin_x, Alin_u (n_input x nu), blin_u, tv_Alin_x ((n_tv_state * N) x nx), tv_blin_x (n_tv_state x N), tv_Alin_u
// ((n_tv_input * (N - 1)) x nu), tv_blin_u (n_tv_input x (N - 1)).  Output, one line per entry of a block [3][km][lw]:
//     R set slot k lane coefficient offset norm      the rule on the caller's arrays at stride km (set 0 static: slot 0; set 1: slots 0 .. N-1)
//     T set slot k lane coefficient offset norm      the blocks fill_lane_tables writes when the same numbers are the SHARED sets: the
//                                                    one-row table (nx + nu <= 16) or the tile table (lw = 32), at the table's own
//                                                    stride (first line: "KM <that stride>")
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"

namespace tinympc_amd {
int fail(TinyBatch*, int code, const char*, ...) { return code; }
}  // namespace tinympc_amd
using namespace tinympc_amd;

// column-major (n x cols) -> row-major [k][cols], as the shared setters keep their host copies
static std::vector<double> rows_of(const double* colmajor, int n, int cols) {
    std::vector<double> out((size_t)n * cols);
    for (int k = 0; k < n; ++k)
        for (int c = 0; c < cols; ++c) out[(size_t)k * cols + c] = colmajor[(size_t)c * n + k];
    return out;
}

static void print_block(const char* tag, int set, int slot, int km, int lw, const double* blk) {
    for (int k = 0; k < km; ++k)
        for (int j = 0; j < lw; ++j) printf("%s %d %d %d %d %.17g %.17g %.17g\n", tag, set, slot, k, j, blk[k * lw + j], blk[km * lw + k * lw + j], blk[2 * km * lw + k * lw + j]);
}

int main(int argc, char** argv) {
    if (argc != 14) { fprintf(stderr, "usage: %s nx nu N ns ni nts nti en_s en_i en_ts en_ti km input.bin\n", argv[0]); return 2; }
    const int nx = atoi(argv[1]), nu = atoi(argv[2]), N = atoi(argv[3]);
    const int ns = atoi(argv[4]), ni = atoi(argv[5]), nts = atoi(argv[6]), nti = atoi(argv[7]);
    const bool on[4] = {atoi(argv[8]) != 0, atoi(argv[9]) != 0, atoi(argv[10]) != 0, atoi(argv[11]) != 0};
    const int km = atoi(argv[12]);
    const size_t len[8] = {(size_t)ns * nx, (size_t)ns, (size_t)ni * nu, (size_t)ni, (size_t)nts * N * nx, (size_t)nts * N, (size_t)nti * (N - 1) * nu, (size_t)nti * (N - 1)};
    std::vector<double> in[8];
    FILE* f = fopen(argv[13], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[13]); return 2; }
    for (int i = 0; i < 8; ++i) {
        in[i].resize(len[i] + 1);
        if (fread(in[i].data(), sizeof(double), len[i], f) != len[i]) { fprintf(stderr, "short input\n"); return 2; }
    }
    fclose(f);
    const int lw = box_lanes(nx, nu);
    // the rule, on the caller's arrays
    const HalfspaceRows sx = halfspace_caller_rows(in[0].data(), in[1].data(), ns, nx, 1, on[0]), su = halfspace_caller_rows(in[2].data(), in[3].data(), ni, nu, 1, on[1]);
    const HalfspaceRows tx = halfspace_caller_rows(in[4].data(), in[5].data(), nts, nx, N, on[2]), tu = halfspace_caller_rows(in[6].data(), in[7].data(), nti, nu, N - 1, on[3]);
    std::vector<double> blk((size_t)3 * km * lw);
    auto rule = [&](int set, int slot, const HalfspaceRows& st, const HalfspaceRows& inp) {
        for (int k = 0; k < km; ++k)
            for (int j = 0; j < lw; ++j) {
                const HalfspaceEntry e = halfspace_entry(st, inp, nx, nu, k, j, km);
                blk[k * lw + j] = e.a; blk[km * lw + k * lw + j] = e.b; blk[2 * km * lw + k * lw + j] = e.nn;
                if (halfspace_offset(st, inp, nx, nu, k, j, km) != e.b && e.b == e.b) { fprintf(stderr, "halfspace_offset disagrees\n"); exit(2); }
            }
        print_block("R", set, slot, km, lw, blk.data());
    };
    rule(0, 0, sx, su);
    for (int s = 0; s < N; ++s) rule(1, s, tx.knot(s), tu.knot(s - 1));
    // the shared table of the same numbers
    TinyBatch b;
    b.nx = nx; b.nu = nu; b.N = N;
    b.A = Mat(nx, nx); b.B = Mat(nx, nu); b.f = Mat(nx, 1);
    b.Qw.assign(nx, 0.0); b.Rw.assign(nu, 0.0);
    const double rho = 1.5;
    for (int i = 0; i < nx; ++i) {
        for (int j = 0; j < nx; ++j) b.A(i, j) = (i == j ? 0.8 : 0.0) + 0.01 * ((3 * i + 7 * j) % 11 - 4) / (1.0 + 0.1 * nx);
        for (int m = 0; m < nu; ++m) b.B(i, m) = 0.05 * ((5 * i + 2 * m) % 9 + 1);
        b.Qw[i] = 10.0 + i + rho;
    }
    for (int m = 0; m < nu; ++m) b.Rw[m] = 2.0 + 0.5 * m + rho;
    if (!precompute_cache(b.A, b.B, b.f, Mat::diag(b.Qw), Mat::diag(b.Rw), rho, &b.cache)) { fprintf(stderr, "singular cache\n"); return 2; }
    b.set = Settings();
    b.set.en_state_linear = on[0]; b.set.en_input_linear = on[1]; b.set.en_tv_state_linear = on[2]; b.set.en_tv_input_linear = on[3];
    b.nsl = ns; b.nil = ni; b.ntsl = nts; b.ntil = nti;
    b.Alin_x = rows_of(in[0].data(), ns, nx); b.blin_x.assign(in[1].begin(), in[1].begin() + len[1]);
    b.Alin_u = rows_of(in[2].data(), ni, nu); b.blin_u.assign(in[3].begin(), in[3].begin() + len[3]);
    b.tvA_x = rows_of(in[4].data(), nts * N, nx); b.tvb_x.assign(in[5].begin(), in[5].begin() + len[5]);
    b.tvA_u = rows_of(in[6].data(), nti * (N - 1), nu); b.tvb_u.assign(in[7].begin(), in[7].begin() + len[7]);
    LaneTab T = ROW_TAB;
    const std::vector<double>* t = &b.h_tab;
    if (nx + nu <= 16) build_tables(&b);
    else {
        b.tile_dyn = TileEntry{nx, nu, N, 2, 1, 0, nullptr, nullptr, nullptr, nullptr};
        b.tile = &b.tile_dyn;
        build_tile_tables(&b);
        T = LaneTab{32, 32};
        t = &b.h_ttab;
    }
    if (T.lw != lw) { fprintf(stderr, "the table's lanes (%d) are not the block's (%d)\n", T.lw, lw); return 2; }
    const int tkm = lin_kmax(&b) > (int)LIN_KMAX ? lin_kmax(&b) : (int)LIN_KMAX;
    printf("KM %d\n", tkm);
    print_block("T", 0, 0, tkm, lw, t->data() + T.lin_offset(N));
    for (int s = 0; s < N; ++s) print_block("T", 1, s, tkm, lw, t->data() + T.tlin_offset(N, tkm) + (size_t)s * 3 * tkm * lw);
    return 0;
}
