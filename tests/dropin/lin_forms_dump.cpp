// lin_forms_dump.cpp -- which form a half-space variant of the one-row kernel takes, without a GPU: prints solve_kernel_lin_planes,
// solve_kernel_lin_waves and solve_kernel_lin_lds (csrc/admm_kernel.hip.h) for a list of shapes.  No option of the library reports
// "slack planes in LDS" versus "per-knot register form"; these three functions decide it at compile time.  Stand-alone, no HIP call:
//     hipcc --offload-arch=gfx950 -std=c++17 -I tinympc_amd/csrc -x hip tests/dropin/lin_forms_dump.cpp -o dump
//     dump nx,nu,N,soc,lin,kmax,ub [...]      one line per argument: nx nu N soc lin kmax ub planes waves lds_bytes
#include <cstdio>

#include "admm_kernel.hip.h"

int main(int argc, char** argv) {
    using namespace tinympc_amd;
    for (int i = 1; i < argc; ++i) {
        int nx, nu, n, soc, lin, kmax, ub;
        if (sscanf(argv[i], "%d,%d,%d,%d,%d,%d,%d", &nx, &nu, &n, &soc, &lin, &kmax, &ub) != 7) { fprintf(stderr, "usage: %s nx,nu,N,soc,lin,kmax,ub ...\n", argv[0]); return 2; }
        printf("%d %d %d %d %d %d %d %d %d %ld\n", nx, nu, n, soc, lin, kmax, ub, (int)solve_kernel_lin_planes(nx, nu, n, soc != 0, lin, kmax, ub != 0),
               solve_kernel_lin_waves(nx, nu, n, soc != 0, lin, kmax, ub != 0), solve_kernel_lin_lds(nx, nu, n, soc != 0, lin, kmax, ub != 0));
    }
    return 0;
}
