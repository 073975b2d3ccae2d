"""LOBPCG by part, its kernels against the streaming ceiling, and the V-cycle against no preconditioner (measurement script, not a
test): python -m tests.perf_eig [m]

Poisson m^3 (default 128) on the product's own hierarchy, K = 2, 4, 8, in one process, after warm-up, with device events:
  * each new kernel as back-to-back runs inside the library (sgpu_debug_time_eig) next to sgpu_debug_stream_ceiling for the bytes it
    moves -- a Gram block of two distinct block vectors reads 16 n K bytes (the ceiling kernel needs an output stream to spread its
    lanes over: it writes one column, 8 n bytes, and the two sides are compared per byte moved), a mix of NS sources and one output
    8 n K (NS + 1), the residual 24 n K.  Alternated three times; the second-best time is printed next to the best: the run's own spread;
  * the block V-cycle and the block SpMV, the same way (sgpu_debug_time_vcycle / _time_block);
  * per iteration of sgpu_eigs_LOBPCG run for a fixed number of iterations (tolerance 0): wall clock, the sum of its parts from the
    figures above (one V-cycle, one SpMV, 3 + 12 Gram blocks and their reductions, 4 + 4 mixes, one residual) and the remainder --
    the host: three synchronisations, the dense problems, launch gaps.  The sum is a model and overstates the kernels a little: the
    solver reduces its Gram blocks in 3 launches per iteration where 15 stand-alone timings carry 15, and it understates them where
    3 of the 6 one-source mixes also read an Add vector that the timed variant does not; read the remainder with that in mind;
  * time to tolerance 1e-8 (nev = 1, 4, 7: at a gap of the spectrum) with the V-cycle and without, alternated.
"""
import ctypes as C
import sys
import time

import numpy as np

from saena_amd import capi, host
from tests import eig_ref as er


def timed(fn, ceiling, reps):
    fn(3); ceiling(3)
    t, c = [], []
    for _ in range(3):
        t.append(1e3 * fn(reps))
        c.append(ceiling(reps))
    t.sort()
    return t, min(c)


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    capi.init(0)
    print(capi.device_info(), flush=True)
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    t0 = time.time()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    n = A.num_local_rows
    print(f"--- Poisson {m}^3: {n} rows, setup + upload + autotune {time.time() - t0:.1f} s, {S.num_levels} levels", flush=True)
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), lambda: None                                  # owned by the solver
    A0 = S.device_op(0)
    rng = np.random.default_rng(5)
    for K in (2, 4, 8):
        X, Y, Out = (capi.BlockVector(n, K, rng.standard_normal((n, K))) for _ in range(3))
        print(f"--- K = {K}", flush=True)
        part = {}
        cases = [("gram", 0, 1, 16 * n * K, 0)] + [(f"mix NS={ns}", 1, ns, 8 * n * K * ns, 8 * n * K) for ns in (1, 2, 3)] + [("residual", 2, 1, 16 * n * K, 8 * n * K)]
        for name, kind, ns, rd, wr in cases:
            cwr = max(wr, 8 * n)
            t, (us_c, mode, moved) = timed(lambda r: G.time_eig(kind, ns, X, Y, Out, n, K, r), lambda r: capi.stream_ceiling(rd, cwr, r), 50)
            part[name] = t[0]
            print(f"{name:10s}: {t[0]:8.1f} us (again {t[1]:8.1f})  {(rd + wr) / 1e6:7.1f} MB  {(rd + wr) / t[0] / 1e3:6.0f} GB/s  "
                  f"ceiling {us_c:8.1f} us ({mode}, {moved / 1e6:7.1f} MB)  ceiling / kernel {us_c * (rd + wr) / moved / t[0]:5.2f}", flush=True)
        G.time_vcycle(Out, X, 3)
        vc = sorted(1e3 * G.time_vcycle(Out, X, 20) for _ in range(3))
        A0.time_block(0, X, None, Out, 3)
        mv = sorted(1e3 * A0.time_block(0, X, None, Out, 50) for _ in range(3))
        print(f"block V-cycle: {vc[0]:8.1f} us (again {vc[1]:8.1f});  block SpMV: {mv[0]:8.1f} us (again {mv[1]:8.1f})", flush=True)
        parts = vc[0] + mv[0] + 15 * part["gram"] + 6 * part["mix NS=1"] + 2 * part["mix NS=2"] + part["residual"]
        X0 = er.start_vectors(n, K)
        for iters in (8, 16):
            X.upload(X0)
            G.lobpcg(X, K, max_iter=iters, tol=0.0)
            best = []
            for _ in range(3):
                X.upload(X0)
                capi.check(capi.lib().sgpu_device_sync())
                t0 = time.perf_counter()
                done = G.lobpcg(X, K, max_iter=iters, tol=0.0)[2]
                capi.check(capi.lib().sgpu_device_sync())
                best.append(1e6 * (time.perf_counter() - t0) / max(done, 1))
            best.sort()
            print(f"{iters:2d} iterations of LOBPCG: {best[0]:8.1f} us per iteration (again {best[1]:8.1f}); its kernels {parts:8.1f} us "
                  f"(V-cycle {vc[0]:.1f}, SpMV {mv[0]:.1f}, Gram {15 * part['gram']:.1f}, mix {6 * part['mix NS=1'] + 2 * part['mix NS=2']:.1f}, "
                  f"residual {part['residual']:.1f}), host and gaps {best[0] - parts:8.1f} us", flush=True)
        nev = {2: 1, 4: 4, 8: 7}[K]                                   # ends at a gap of the spectrum (clusters of 1, 3, 3)
        for rep in range(2):
            for precond in (True, False):
                X.upload(X0)
                capi.check(capi.lib().sgpu_device_sync())
                t0 = time.perf_counter()
                lam, res, it, _, conv = G.lobpcg(X, nev, max_iter=2000, tol=1e-8, precond=precond)
                capi.check(capi.lib().sgpu_device_sync())
                print(f"to 1e-8, nev = {nev}, {'V-cycle' if precond else 'plain  '}: {it:4d} iterations, {1e3 * (time.perf_counter() - t0):9.1f} ms "
                      f"({'converged' if conv else 'not converged'}), lambda_0 = {lam[0]:.12e}", flush=True)
        del X, Y, Out


if __name__ == "__main__":
    main()
