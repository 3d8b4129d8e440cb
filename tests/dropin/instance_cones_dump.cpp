// instance_cones_dump.cpp -- what the fill rule of a cone-coefficient block (csrc/lane_tables.hpp cone_entry: the one statement the helper
// kernel behind tiny_batch_set_instance_cone_coefficients calls) puts in every lane, without a GPU.  Stand-alone, one command:
//     hipcc --offload-arch=gfx950 -std=c++17 -I tinympc_amd/csrc -x hip tests/dropin/instance_cones_dump.cpp tinympc_amd/csrc/batch_tables.hip -o dump
//     dump nx nu N en_state_soc en_input_soc Acx Acu         (Acx / Acu: the cones' first rows, comma separated; "-": none)
// One instance whose every coefficient is a distinct number: cx[k] = 101 + k, cu[k] = 201 + k.  Output, one line per lane of the block [lw]:
//     R lane mu            the rule as the helper kernel calls it: every family counted, whatever the switches say (lw = box_lanes(nx, nu))
//     T lane mu base       VEC_CONE_MU and VEC_CONE_BASE fill_lane_tables writes for the same cones as a SHARED set under the switches
//                          given: the one-row table (nx + nu <= 16) or the tile table (lw = 32)
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "batch_impl.hpp"
#include "batch_dispatch.hpp"
#include "lane_tables.hpp"

namespace tinympc_amd {
int fail(TinyBatch*, int code, const char*, ...) { return code; }
}  // namespace tinympc_amd
using namespace tinympc_amd;

static std::vector<int> rows_of_list(const char* s) {
    std::vector<int> out;
    if (!strcmp(s, "-")) return out;
    for (const char* p = s; *p;) {
        out.push_back(atoi(p));
        p = strchr(p, ',');
        if (!p) break;
        ++p;
    }
    return out;
}

int main(int argc, char** argv) {
    if (argc != 8) { fprintf(stderr, "usage: %s nx nu N en_state_soc en_input_soc Acx Acu\n", argv[0]); return 2; }
    const int nx = atoi(argv[1]), nu = atoi(argv[2]), N = atoi(argv[3]);
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
    b.set.en_state_soc = atoi(argv[4]) != 0; b.set.en_input_soc = atoi(argv[5]) != 0;
    b.Acx = rows_of_list(argv[6]); b.Acu = rows_of_list(argv[7]);
    for (size_t k = 0; k < b.Acx.size(); ++k) { b.qcx.push_back(3); b.cx.push_back(101.0 + k); }
    for (size_t k = 0; k < b.Acu.size(); ++k) { b.qcu.push_back(3); b.cu.push_back(201.0 + k); }
    const int lw = box_lanes(nx, nu);
    for (int j = 0; j < lw; ++j)
        printf("R %d %.17g\n", j, cone_entry(b.cx.data(), b.cu.data(), b.Acx.data(), (int)b.Acx.size(), b.Acu.data(), (int)b.Acu.size(), nx, nu, j));
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
    for (int j = 0; j < lw; ++j) printf("T %d %.17g %.17g\n", j, (*t)[T.VEC() + VEC_CONE_MU * lw + j], (*t)[T.VEC() + VEC_CONE_BASE * lw + j]);
    return 0;
}
