"""numpy reference of the adaptive-rho sensitivity tables (csrc/sensitivity_kernel.hip.h): d(cache)/d(rho) of the cache tiny_setup
computes, where rho enters Q and R twice (Q + 2 rho I, R + 2 rho I in the Riccati recursion), evaluated at a given cache.

With K = Kinf, C1 = Quu_inv, Acl = A - B K:
    dP   solves  dP = Acl' dP Acl + 2 (I + K' K)
    dK   = C1 (B' dP Acl - 2 K)
    dC1  = -C1 (2 I + B' dP B) C1
    dC2  = -(B dK)'
test_sensitivity_ref_cpu.py pins these against central differences of a converged Riccati recursion; the GPU tests compare the
device's tables with them."""
import numpy as np

NAMES = ("dKinf_drho", "dPinf_drho", "dC1_drho", "dC2_drho")


def lyapunov(Acl, W, tol=1e-15, max_steps=64):
    """X = sum_k Acl'^k W Acl^k by squaring (X <- X + M' X M, M <- M M); -> (X, steps)"""
    X, M = W.copy(), Acl.copy()
    for n in range(1, max_steps + 1):
        inc = M.T @ X @ M
        X = X + inc
        if np.max(np.abs(inc)) < tol * np.max(np.abs(X)):
            return X, n
        M = M @ M
    raise RuntimeError("Lyapunov series did not converge: A - B K is not a contraction")


def tables(A, B, K, C1):
    """the four tables at the cache (K, C1) of the system (A, B) -> dict name -> array, plus 'steps'"""
    A, B, K, C1 = (np.asarray(m, dtype=np.float64) for m in (A, B, K, C1))
    nx, nu = B.shape
    Acl = A - B @ K
    dP, steps = lyapunov(Acl, 2.0 * (np.eye(nx) + K.T @ K))
    dK = C1 @ (B.T @ dP @ Acl - 2.0 * K)
    dC1 = -C1 @ (2.0 * np.eye(nu) + B.T @ dP @ B) @ C1
    dC2 = -(B @ dK).T
    return {"dKinf_drho": dK, "dPinf_drho": dP, "dC1_drho": dC1, "dC2_drho": dC2, "steps": steps}


def dare_cache(A, B, Qdiag, Rdiag, rho, tol=1e-14, max_iter=200000):
    """tiny_setup's cache with the recursion run to convergence: (Kinf, Pinf, Quu_inv, AmBKt) for Q + 2 rho I, R + 2 rho I"""
    nx, nu = B.shape
    Q1 = np.diag(Qdiag) + 2.0 * rho * np.eye(nx)
    R1 = np.diag(Rdiag) + 2.0 * rho * np.eye(nu)
    P = rho * np.eye(nx)
    for _ in range(max_iter):
        K = np.linalg.solve(R1 + B.T @ P @ B, B.T @ P @ A)
        Pn = Q1 + A.T @ P @ (A - B @ K)
        done = np.max(np.abs(Pn - P)) < tol * max(1.0, np.max(np.abs(P)))
        P = Pn
        if done:
            break
    K = np.linalg.solve(R1 + B.T @ P @ B, B.T @ P @ A)
    return K, P, np.linalg.inv(R1 + B.T @ P @ B), (A - B @ K).T


def random_system(rng, nx, nu):
    """a random stable-ish system in the style of tools/fuzz_parity.py: (A, B, Qdiag, Rdiag, rho)"""
    M = rng.standard_normal((nx, nx))
    A = M * rng.uniform(0.5, 1.0) / np.max(np.abs(np.linalg.eigvals(M)))
    return (A, rng.standard_normal((nx, nu)) / np.sqrt(nx), rng.uniform(0.5, 10, nx), rng.uniform(0.1, 2, nu),
            float(rng.choice([1.0, 5.0, 17.3])))


def rel_max(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))
