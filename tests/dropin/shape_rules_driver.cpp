// shape_rules_driver.cpp -- the two shape formulas of csrc/jit.hpp (jit_shape_fits, jit_tile_shape) and the kernel a shape ends on
// (csrc/kernel_path.hpp decide_path, fed the way tiny_batch_setup and path_facts feed it), asked without a GPU.
// Stand-alone, one command:
//     hipcc -x c++ -std=c++17 -D__HIP_PLATFORM_AMD__ -I /opt/rocm/include -I tinympc_amd/csrc tests/dropin/shape_rules_driver.cpp -o driver
//     driver rules                 every nx, nu in 1..32 with nx+nu <= 33 and every N in 2..170, one line each:
//                                  nx nu N fits_box fits_soc tile W R          (W = R = 0 where the tile rule refuses)
//     driver path < QUERIES        one line of `name=value ...` per query: nx, nu, N, has_entry (kernel_dims.txt holds the shape),
//                                  entry_plain, tile_entry (tile_dims.txt holds it), and any fact of PathFacts that is a setting or an
//                                  option (a name that is absent is 0).  The shape facts -- fits_box, fits, has_tile, tile_is_jit --
//                                  are computed here as tiny_batch_setup (batch_api.hip) and path_facts (batch_dispatch.hip) compute them
// A path query prints: kernel rule code fits_box fits has_tile tile_is_jit W R consistent.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>

#include "jit.hpp"
#include "kernel_path.hpp"

using namespace tinympc_amd;

static const char* KERNEL_NAME[] = {"ONE_ROW", "TILE", "COVERAGE"};

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rules") {
        for (int nx = 1; nx <= 32; ++nx)
            for (int nu = 1; nu <= 32 && nx + nu <= 33; ++nu)
                for (int N = 2; N <= 170; ++N) {
                    int W = 0, R = 0;
                    const bool tile = jit_tile_shape(nx, nu, N, &W, &R);
                    printf("%d %d %d %d %d %d %d %d\n", nx, nu, N, jit_shape_fits(nx, nu, N, false) ? 1 : 0, jit_shape_fits(nx, nu, N, true) ? 1 : 0, tile ? 1 : 0,
                           tile ? W : 0, tile ? R : 0);
                }
        return 0;
    }
    if (mode != "path") { fprintf(stderr, "usage: %s rules | path < QUERIES\n", argv[0]); return 2; }
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::map<std::string, int> q;
        std::string word;
        while (in >> word) {
            const size_t eq = word.find('=');
            if (eq == std::string::npos) { fprintf(stderr, "not name=value: %s\n", word.c_str()); return 2; }
            q[word.substr(0, eq)] = atoi(word.c_str() + eq + 1);
        }
        auto take = [&](const char* name) { const int v = q.count(name) ? q[name] : 0; q.erase(name); return v; };
        const int nx = take("nx"), nu = take("nu"), N = take("N");
        PathFacts f;
        f.has_entry = take("has_entry"); f.entry_plain = take("entry_plain"); f.entry_klin = take("entry_klin");
        f.soc = take("soc"); f.lin_families = take("lin_families"); f.lin_kmax = take("lin_kmax");
        f.tile_lin = take("tile_lin"); f.planes_fit = take("planes_fit"); f.pl_planes_fit = take("pl_planes_fit");
        f.cones_overlap = take("cones_overlap"); f.hetero = take("hetero"); f.tile_ext = take("tile_ext"); f.adaptive = take("adaptive"); f.debug = take("debug");
        f.inst_bounds = take("inst_bounds"); f.inst_lin = take("inst_lin"); f.inst_cones = take("inst_cones");
        f.force_general = take("force_general"); f.no_jit = take("no_jit"); f.no_tile = take("no_tile"); f.prefer_tile = take("prefer_tile");
        f.jit_failed = take("jit_failed"); f.variant_jit_failed = take("variant_jit_failed"); f.tile_soc_failed = take("tile_soc_failed");
        f.disturbance = take("disturbance"); f.plant = take("plant"); f.state_log = take("state_log");
        // tiny_batch_setup: a tile entry of tile_dims.txt, else a shape chosen at run time -- (W,R) = (1,1) is the one-row kernel's job where that fits
        const bool tile_entry = take("tile_entry");
        int W = 0, R = 0;
        f.has_tile = tile_entry;
        if (!tile_entry && jit_tile_shape(nx, nu, N, &W, &R) && (W * R > 1 || !jit_shape_fits(nx, nu, N, false))) f.has_tile = f.tile_is_jit = true;
        else W = R = 0;
        // path_facts
        f.fits_box = jit_shape_fits(nx, nu, N, false);
        f.fits = f.soc ? jit_shape_fits(nx, nu, N, true) : f.fits_box;
        if (!q.empty()) { fprintf(stderr, "unknown name %s\n", q.begin()->first.c_str()); return 2; }
        const PathDecision d = decide_path(f);
        printf("kernel=%s rule=%s code=%d fits_box=%d fits=%d has_tile=%d tile_is_jit=%d W=%d R=%d consistent=%d\n", KERNEL_NAME[d.kernel], d.rule, kernel_path_code(d, f),
               f.fits_box ? 1 : 0, f.fits ? 1 : 0, f.has_tile ? 1 : 0, f.tile_is_jit ? 1 : 0, W, R, facts_consistent(f) ? 1 : 0);
    }
    return 0;
}
