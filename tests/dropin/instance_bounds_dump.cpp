// instance_bounds_dump.cpp -- what the fill rule of a bounds block (csrc/lane_tables.hpp box_entry: the one statement the helper kernel
// behind tiny_batch_set_instance_bounds calls) puts in every (slot, lane), without a GPU.  Stand-alone, one command:
//     hipcc --offload-arch=gfx950 -std=c++17 -I tinympc_amd/csrc -x hip tests/dropin/instance_bounds_dump.cpp tinympc_amd/csrc/batch_tables.hip -o dump
//     dump nx nu N en_state_bound en_input_bound
// One instance whose every source element is a distinct number: x_min[e] = 1 + e, x_max[e] = 10001 + e (e = knot * nx + row),
// u_min[e] = 20001 + e, u_max[e] = 30001 + e (e = knot * nu + row).  Output, one line per (slot, lane) of the block [N][lw]:
//     R slot lane lo hi      the rule (lw = box_lanes(nx, nu))
//     T slot lane lo hi      the bounds block fill_lane_tables writes for the same box as a SHARED one: the one-row table (nx + nu <= 16)
//                            or the tile table (lw = 32)
#include <cstdio>
#include <cstdlib>

#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"

namespace tinympc_amd {
int fail(TinyBatch*, int code, const char*, ...) { return code; }
}  // namespace tinympc_amd
using namespace tinympc_amd;

int main(int argc, char** argv) {
    if (argc != 6) { fprintf(stderr, "usage: %s nx nu N en_state_bound en_input_bound\n", argv[0]); return 2; }
    const int nx = atoi(argv[1]), nu = atoi(argv[2]), N = atoi(argv[3]);
    const bool sb = atoi(argv[4]) != 0, ib = atoi(argv[5]) != 0;
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
    b.set.en_state_bound = sb; b.set.en_input_bound = ib;
    b.have_bounds = true;
    for (int e = 0; e < N * nx; ++e) { b.x_min.push_back(1 + e); b.x_max.push_back(10001 + e); }
    for (int e = 0; e < (N - 1) * nu; ++e) { b.u_min.push_back(20001 + e); b.u_max.push_back(30001 + e); }
    const int lw = box_lanes(nx, nu);
    for (int s = 0; s < N; ++s)
        for (int j = 0; j < lw; ++j) {
            const BoxEntry e = box_entry(b.x_min.data(), b.x_max.data(), b.u_min.data(), b.u_max.data(), nx, nu, s, j, sb, ib);
            printf("R %d %d %.17g %.17g\n", s, j, e.lo, e.hi);
        }
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
    for (int s = 0; s < N; ++s)
        for (int j = 0; j < lw; ++j) printf("T %d %d %.17g %.17g\n", s, j, (*t)[T.BOUNDS() + s * lw + j], (*t)[T.BOUNDS() + N * lw + s * lw + j]);
    return 0;
}
