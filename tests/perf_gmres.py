"""The orthogonalisation of FGMRES against the streaming ceiling, and an FGMRES iteration against a pCG iteration (measurement
script, not a test): python -m tests.perf_gmres [m]

In one process, after warm-up, with device events:
  * the Gram-Schmidt dots and the update (with its fused norm) over 1, 8 and 30 basis vectors of n = 2 000 376 rows, as back-to-back
    runs inside the library (sgpu_debug_time_gs), each next to sgpu_debug_stream_ceiling for the same bytes: per pass of up to 8
    columns w is read once and every column once, 8 n bytes each; the update also writes w once per pass.  The ceiling kernel
    needs an output stream to spread its lanes over: for the dots, which write next to nothing, it writes one vector (8 n bytes),
    and the two sides are compared per byte moved (ceiling / kernel = the kernel's GB/s over the ceiling's).  Alternated three
    times; the second-best time is printed next to the best: the run's own spread;
  * Poisson m^3 (default 128) on the product's own hierarchy: wall clock per inner iteration of sgpu_solve_FGMRES (restart 30) and
    per iteration of sgpu_solve_pCG, both run for a fixed number of iterations (tolerance 0), uploads excluded.
"""
import ctypes as C
import sys
import time

import numpy as np

from saena_amd import capi, host

N = 2_000_376          # 126^3, even: the leading dimension is n
COLS = (1, 8, 30)


def gs_bytes(kind, ncols, n):
    passes = -(-ncols // 8)
    return 8 * n * (ncols + passes), (8 * n * passes if kind == 1 else 0)


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    capi.init(0)
    print(capi.device_info(), flush=True)
    rng = np.random.default_rng(3)
    V = capi.DeviceVector(N * max(COLS))
    col = rng.standard_normal(N)
    for c in range(max(COLS)):
        capi.check(capi.lib().sgpu_vec_upload(C.c_void_p(V.ptr.value + 8 * N * c), np.roll(col, 1009 * c).ctypes.data, N))
    w = capi.DeviceVector(N, rng.standard_normal(N))
    print(f"--- Gram-Schmidt kernels, n = {N}", flush=True)
    for kind, name in ((0, "dots"), (1, "update + norm")):
        for ncols in COLS:
            rd, wr = gs_bytes(kind, ncols, N)
            reps = 50 if ncols < 30 else 20
            cwr = max(wr, 8 * N)
            capi.time_gs(kind, V, N, ncols, w, N, 3); capi.stream_ceiling(rd, cwr, 3)         # warm-up
            t, c = [], []
            for _ in range(3):
                t.append(1e3 * capi.time_gs(kind, V, N, ncols, w, N, reps))
                c.append(capi.stream_ceiling(rd, cwr, reps))
            t.sort()
            us_c, mode, moved = min(c)
            print(f"{name:14s} {ncols:2d} columns: {t[0]:8.1f} us (again {t[1]:8.1f})  {(rd + wr) / 1e6:7.1f} MB  {(rd + wr) / t[0] / 1e3:6.0f} GB/s  "
                  f"ceiling {us_c:8.1f} us ({mode}, {moved / 1e6:7.1f} MB)  ceiling / kernel {us_c * (rd + wr) / moved / t[0]:5.2f}", flush=True)
    del V, w

    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    t0 = time.time()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    n = A.num_local_rows
    print(f"--- Poisson {m}^3: {n} rows, setup + upload + autotune {time.time() - t0:.1f} s, {S.num_levels} levels", flush=True)
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), lambda: None                                  # owned by the solver
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, A.laplacian3D_rhs())
    it, hist, ok, _ = G.solve_fgmres(du, dr, restart=30)
    itp, histp, okp = G.solve_pCG(du, dr)
    print(f"to 1e-8: FGMRES(30) {it} iterations ({'converged' if ok else 'not converged'}), pCG {itp} iterations ({'converged' if okp else 'not converged'})", flush=True)
    for iters in (8, 16):
        G.set_solve_params(iters, 0.0, "jacobi", 3, 3)
        row = []
        for name, run in (("FGMRES(30)", lambda: G.solve_fgmres(du, dr, restart=30)), ("pCG", lambda: G.solve_pCG(du, dr))):
            run()
            best = []
            for _ in range(3):
                capi.check(capi.lib().sgpu_device_sync())
                t0 = time.perf_counter()
                done = run()[0]
                capi.check(capi.lib().sgpu_device_sync())
                best.append(1e6 * (time.perf_counter() - t0) / done)
            best.sort()
            row.append(best[0])
            print(f"{iters:2d} iterations of {name:10s}: {best[0]:8.1f} us per iteration (again {best[1]:8.1f})", flush=True)
        print(f"{iters:2d} iterations: FGMRES / pCG per iteration {row[0] / row[1]:5.2f}", flush=True)


if __name__ == "__main__":
    main()
