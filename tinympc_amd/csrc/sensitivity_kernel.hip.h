// sensitivity_kernel.hip.h -- the adaptive-rho sensitivity tables d(cache)/d(rho), computed on the GPU for `batch` instances at once.
//
// The reference declares compute_sensitivity_matrices (tiny_api.hpp:29-31) and defines it nowhere; its only tables are the quadrotor
// literals of tiny_initialize_sensitivity_matrices.  This kernel evaluates the derivative of the cache tiny_setup computes, where rho
// enters Q and R twice (cache.hpp:6-7, riccati_kernel.hip.h:106-107), at the cache as it stands.  With K = Kinf, C1 = Quu_inv,
// Acl = A - B K:
//     dP   solves  dP = Acl' dP Acl + 2 (I + K' K)              (discrete Lyapunov equation)
//     dK   = C1 (B' dP Acl - 2 K)
//     dC1  = -C1 (2 I + B' dP B) C1
//     dC2  = -(B dK)'                                            (C2 = AmBKt)
// (Pinf itself does not enter: the right-hand side of the Lyapunov equation is the explicit rho-dependence of Q and R alone.)
//
// sensitivity_kernel : one wavefront per instance, grid stride over the batch, all matrices in LDS (as riccati_kernel).  The Lyapunov
//                  equation is solved by squaring -- X <- X + M' X M, M <- M M, starting from X = 2 (I + K' K), M = Acl: after s
//                  steps X holds 2^s terms of the series -- until the increment falls below 1e-15 of X (max norms, reduced over the
//                  wave: every lane takes the same branch) or 64 squarings have run.  No FMA contraction; there is no host path.
//                  Its epilogue writes the instance's ATAB_* lane tables (admm_kernel.hip.h) through the mapping the host uses for a
//                  shared family (lane_tables.hpp), ATAB_AT from the instance's own A and B (shapes of the one-row kernel only).
// LDS: five nx x nx matrices (Acl, M, X and two temporaries), five nx x nu ones (B, K, B' dP, its product, dK) and three nu x nu
//                  ones.  At nx = 31, nu = 1: 5 * 7688 + 5 * 248 + 24 = 39 704 bytes, four blocks per CU of 160 KB; at the
//                  quadrotor's (12,4): 8 064 bytes, LDS is not the limit.
#pragma once
#include <hip/hip_runtime.h>

#include "lane_tables.hpp"
#include "riccati_kernel.hip.h"

namespace tinympc_amd {

struct SensitivityArgs {
    const double *A, *B, *Kinf, *Quu_inv;            // [batch][nx*nx], [batch][nx*nu], [batch][nu*nx], [batch][nu*nu], column-major
    const int* riccati_iters;                        // optional [batch]: -1 marks an instance whose cache is not valid
    double *dKinf, *dPinf, *dC1, *dC2;               // [batch][nu*nx], [batch][nx*nx], [batch][nu*nu], [batch][nx*nx], column-major
    int* steps;                                      // [batch]: squarings taken, -1: not converged / no valid cache
    double* atabs;                                   // optional [batch][ATAB_DOUBLES] (nx + nu <= 16 only)
    int nx, nu, batch;
};
constexpr int SENS_MAX_STEPS = 64;
constexpr size_t sensitivity_lds_bytes(int nx, int nu) { return (size_t)(5 * nx * nx + 5 * nx * nu + 3 * nu * nu) * sizeof(double); }

#ifdef TINYMPC_GENERAL_KERNEL_IMPL   // compiled into batch_dispatch.hip only

#pragma clang fp contract(off)

// C(m x n) = X'(m x k) * Y(k x n) with X stored k x m, column-major, sequential k
__device__ __forceinline__ void w_mm_tn(int m, int k, int n, const double* X, const double* Y, double* C, int lane) {
    for (int e = lane; e < m * n; e += 64) {
        const int i = e % m, j = e / m;
        double s = 0.0;
        for (int l = 0; l < k; ++l) s = __dadd_rn(s, __dmul_rn(X[l + k * i], Y[l + k * j]));
        C[e] = s;
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void sensitivity_kernel(const SensitivityArgs P) {
    extern __shared__ double sm[];
    const int lane = threadIdx.x, nx = P.nx, nu = P.nu;
    const int xx = nx * nx, xu = nx * nu, uu = nu * nu;
    double* Acl = sm;          double* M = Acl + xx;    double* X = M + xx;      double* T = X + xx;      double* T2 = T + xx;
    double* B = T2 + xx;       double* K = B + xu;      double* BtX = K + xu;    double* T1 = BtX + xu;   double* dK = T1 + xu;
    double* C1 = dK + xu;      double* G = C1 + uu;     double* GC = G + uu;
    for (int b = blockIdx.x; b < P.batch; b += gridDim.x) {
        const double* Ag = P.A + (size_t)b * xx;
        for (int e = lane; e < xu; e += 64) { B[e] = P.B[(size_t)b * xu + e]; K[e] = P.Kinf[(size_t)b * xu + e]; }
        for (int e = lane; e < uu; e += 64) C1[e] = P.Quu_inv[(size_t)b * uu + e];
        __syncthreads();
        w_mm(nx, nu, nx, B, K, T, lane);                                       // B K
        w_mm_tn(nx, nu, nx, K, K, X, lane);                                    // K' K
        for (int e = lane; e < xx; e += 64) {
            const double acl = Ag[e] - T[e];
            Acl[e] = acl; M[e] = acl;
            X[e] = 2.0 * (((e % nx == e / nx) ? 1.0 : 0.0) + X[e]);            // W = 2 (I + K' K)
        }
        __syncthreads();
        int steps = -1;
        for (int s = 0; s < SENS_MAX_STEPS; ++s) {
            w_mm(nx, nx, nx, X, M, T, lane);
            w_mm_tn(nx, nx, nx, M, T, T2, lane);                               // M' X M
            double inc = 0.0, top = 0.0;
            bool bad = false;
            for (int e = lane; e < xx; e += 64) {
                const double d = T2[e], x = X[e] + d;
                X[e] = x;
                inc = fmax(inc, fabs(d)); top = fmax(top, fabs(x));
                bad = bad || !(fabs(x) <= 1.79e308);                           // (fmax drops a NaN: keep it in sight)
            }
            for (int off = 32; off >= 1; off >>= 1) { inc = fmax(inc, __shfl_xor(inc, off)); top = fmax(top, __shfl_xor(top, off)); }
            const bool any_bad = __any(bad);                                   // wave-uniform from here on
            __syncthreads();
            if (any_bad) break;                                                // Acl is not a contraction: no derivative
            if (inc < 1e-15 * top) { steps = s + 1; break; }
            w_mm(nx, nx, nx, M, M, T, lane);
            for (int e = lane; e < xx; e += 64) M[e] = T[e];
            __syncthreads();
        }
        if (P.riccati_iters && P.riccati_iters[b] < 0) steps = -1;
        w_mm_tn(nu, nx, nx, B, X, BtX, lane);                                  // B' dP                (nu x nx)
        w_mm(nu, nx, nx, BtX, Acl, T1, lane);
        for (int e = lane; e < xu; e += 64) T1[e] = T1[e] - 2.0 * K[e];        // B' dP Acl - 2 K
        __syncthreads();
        w_mm(nu, nu, nx, C1, T1, dK, lane);                                    // dK
        w_mm(nu, nx, nu, BtX, B, G, lane);
        for (int e = lane; e < uu; e += 64) if (e % nu == e / nu) G[e] = 2.0 + G[e];   // 2 I + B' dP B
        __syncthreads();
        w_mm(nu, nu, nu, G, C1, GC, lane);
        w_mm(nu, nu, nu, C1, GC, G, lane);                                     // C1 (2 I + B' dP B) C1   (dC1 = its negative)
        w_mm(nx, nu, nx, B, dK, T, lane);                                      // B dK                    (dC2 = its negative transpose)
        for (int e = lane; e < xu; e += 64) P.dKinf[(size_t)b * xu + e] = dK[e];
        for (int e = lane; e < xx; e += 64) {
            const int i = e % nx, j = e / nx;
            P.dPinf[(size_t)b * xx + e] = X[e];
            P.dC2[(size_t)b * xx + e] = -T[j + nx * i];
        }
        for (int e = lane; e < uu; e += 64) P.dC1[(size_t)b * uu + e] = -G[e];
        if (lane == 0) P.steps[b] = steps;
        if (P.atabs) {                                                         // (the host passes it for nx + nu <= 16 only)
            double* tab = P.atabs + (size_t)b * ATAB_DOUBLES;
            const struct {                                                     // dC1 = -G, dC2 = -(B dK)': B dK is in T
                ColMajor A, B, dK, dP;
                const double *G, *T;
                int nx, nu;
                __device__ double dC1(int k, int j) const { return -G[k + nu * j]; }
                __device__ double dC2(int k, int j) const { return -T[j + nx * k]; }
            } view = {{Ag, nx}, {B, nx}, {dK, nu}, {X, nx}, G, T, nx, nu};
            for (int e = lane; e < 256; e += 64) {
                const AtabEntries a = atab_entries(view, nx, nu, e % 16, e / 16);   // lane j = e % 16, column k = e / 16
                tab[ATAB_AT + e] = a.at; tab[ATAB_DK + e] = a.dk; tab[ATAB_DP + e] = a.dp; tab[ATAB_DC1 + e] = a.dc1; tab[ATAB_DC2 + e] = a.dc2;
            }
        }
        __syncthreads();
    }
}

#pragma clang fp contract(fast)
#endif  // TINYMPC_GENERAL_KERNEL_IMPL

}  // namespace tinympc_amd
