"""LOBPCG with hard locking by part (measurement script, not a test): python -m tests.perf_eig_many [m]

Poisson, laplacian3D(m) (default 128: 126^3 interior rows, the benchmark's operator) on the product's own hierarchy, K = 8, in one
process, after warm-up:
  * the locked set: the first 56 eigenvectors from one sgpu_eigs_LOBPCG_many (its time, iterations and sweeps are printed);
  * the two lock kernels as back-to-back runs inside the library (sgpu_debug_time_lock, device events) at L = 8, 24, 56 next to
    sgpu_debug_stream_ceiling for the bytes each moves -- the Gram 8 n (ceil(L / 8) K + L) (Y once per pass, every column once), the
    projection 8 n (L + 2 K).  Alternated three times; the second-best time is printed next to the best: the run's own spread;
  * per iteration of sgpu_eigs_LOBPCG_locked at L = 0, 8, 24, 56 locked columns: wall clock of runs of 8 and of 16 iterations
    (tolerance 0) from the same start, the difference divided by 8 -- the start-up (two projections of X, two Gram blocks, the
    Rayleigh-Ritz of X) cancels --, next to the two kernels' sum for that L;
  * the time to 24 pairs at sweeps of 4, twice.
Nothing is claimed in the documents until this script's log is in profiles/eig_many_128.log.
"""
import ctypes as C
import sys
import time

import numpy as np

from saena_amd import capi, host
from tests.perf_eig import timed

K = 8
LS = (0, 8, 24, 56)


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    capi.init(0)
    print(capi.device_info(), flush=True)
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    t0 = time.time()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    n = A.num_local_rows
    ld = n + (n & 1)
    print(f"--- Poisson, laplacian3D({m}): {n} rows, setup + upload + autotune {time.time() - t0:.1f} s, {S.num_levels} levels", flush=True)
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), lambda: None                                  # owned by the solver
    sync = lambda: capi.check(capi.lib().sgpu_device_sync())      # noqa: E731

    nmax = max(LS)
    sync(); t0 = time.perf_counter()
    lam, res, Q, it, sweeps, conv = G.lobpcg_many(n, nmax, K, 4, max_iter=2000, tol=1e-8, ld=ld)
    print(f"--- the locked set: {len(lam)} pairs in {it} iterations, {sweeps} sweeps, {time.perf_counter() - t0:.2f} s with the download "
          f"({'converged' if conv else 'NOT converged'}); lambda_0 = {lam[0]:.12e}, lambda_{len(lam) - 1} = {lam[-1]:.12e}, "
          f"max |Q^T Q - I| = {np.max(np.abs(Q.T @ Q - np.eye(Q.shape[1]))):.2e}", flush=True)
    if len(lam) < nmax:
        raise SystemExit("the locked set is incomplete")
    cols = np.zeros((nmax, ld))
    cols[:, :n] = Q.T
    dQ = capi.DeviceVector(nmax * ld, cols.ravel())
    del cols, Q

    rng = np.random.default_rng(5)
    X0 = rng.standard_normal((n, K))
    Y = capi.BlockVector(n, K, X0)
    kernels = {0: 0.0}
    for Lc in LS[1:]:
        passes = -(-Lc // 8)
        total = 0.0
        for name, kind, rd, wr in (("lock_gram", 0, 8 * n * (passes * K + Lc), 0), ("lock_project", 1, 8 * n * (Lc + K), 8 * n * K)):
            cwr = max(wr, 8 * n)                                   # (the ceiling kernel writes at least a double per row: scaled by the bytes below)
            t, (us_c, mode, mv_c) = timed(lambda r: G.time_lock(kind, dQ, ld, Lc, Y, n, K, r), lambda r: capi.stream_ceiling(rd, cwr, r), 20)
            moved = rd + wr
            print(f"L = {Lc:2d} {name:12s}: {t[0]:8.1f} us (again {t[1]:8.1f})  {moved / 1e6:7.1f} MB  {moved / t[0] / 1e3:6.0f} GB/s  "
                  f"ceiling {us_c:8.1f} us ({mode}, {mv_c / 1e6:7.1f} MB)  ceiling / kernel {us_c * moved / mv_c / t[0]:5.2f}", flush=True)
            total += t[0]
        kernels[Lc] = total

    X = capi.BlockVector(n, K, X0)
    for Lc in LS:
        wall = {}
        for iters in (8, 16):
            best = []
            for rep in range(4):
                X.upload(X0)
                sync(); t0 = time.perf_counter()
                done = G.lobpcg_locked(X, K, dQ, ld, Lc, max_iter=iters, tol=0.0)[2]
                sync()
                if rep:
                    best.append(1e6 * (time.perf_counter() - t0))
                if done != iters:
                    raise SystemExit(f"L = {Lc}: {done} iterations of {iters}")
            wall[iters] = sorted(best)
        per = [(wall[16][i] - wall[8][i]) / 8 for i in (0, 1)]
        print(f"L = {Lc:2d}: {per[0]:8.1f} us per iteration (again {per[1]:8.1f}); runs of 8 / 16 iterations {wall[8][0] / 1e3:.2f} / {wall[16][0] / 1e3:.2f} ms; "
              f"the two lock kernels {kernels[Lc]:8.1f} us of it", flush=True)

    for rep in range(2):
        sync(); t0 = time.perf_counter()
        lam, res, Q, it, sweeps, conv = G.lobpcg_many(n, 24, K, 4, max_iter=2000, tol=1e-8, ld=ld)
        print(f"to 1e-8, 24 pairs at sweeps of 4: {it} iterations, {sweeps} sweeps, {1e3 * (time.perf_counter() - t0):9.1f} ms with the download of Q "
              f"({'converged' if conv else 'not converged'}), lambda_23 = {lam[-1]:.12e}", flush=True)


if __name__ == "__main__":
    main()
