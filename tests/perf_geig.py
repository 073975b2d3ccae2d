"""The generalised LOBPCG (A x = lambda B x) by part, and k_geig_residual against the streaming ceiling (measurement script, not a
test): python -m tests.perf_geig [m]

Poisson, laplacian3D(m) (default 128: 126^3 interior rows, the benchmark's operator) on the product's own hierarchy, K = 2, 4, 8,
both mass matrices of tests/geig_ref.py for the interior grid (the 27-point consistent one and the lumped one), in one process, after
warm-up, with device events:
  * k_geig_residual with its two reductions as back-to-back runs inside the library (sgpu_debug_time_geig) next to
    sgpu_debug_stream_ceiling for the 24 n K bytes it moves (two block vectors read, one written), and next to k_eig_residual
    (sgpu_debug_time_eig, kind 2), which moves the same bytes and forms one set of norms.  Alternated three times; the second-best
    time is printed next to the best: the run's own spread;
  * the Gram block and the mixes (sgpu_debug_time_eig), the block V-cycle and the block SpMV with A and with B, the same way;
  * per iteration of sgpu_eigs_LOBPCG_gen run for a fixed number of iterations (tolerance 0): wall clock, the sum of its parts from
    the figures above (one V-cycle, one SpMV with A and one with B, 3 + 12 Gram blocks, 9 one-source mixes -- the projection, W, BW,
    P, AP, BP, then X, AX, BX -- and 3 two-source mixes, one residual) and the remainder -- the host: three synchronisations, the
    dense problems, launch gaps.  The sum is a model, with the caveats tests/perf_eig.py states;
  * the standard solve's iteration next to it, and the time to tolerance 1e-8 of both.
Nothing is claimed in the documents until this script's log is in profiles/geig_128.log.
"""
import ctypes as C
import sys
import time

import numpy as np

from saena_amd import capi, host
from tests import eig_ref as er, geig_ref as gg
from tests.perf_eig import timed


def device_mass(comm, name, mi, n):
    """-> (host Matrix, device operator) of geig_ref.mass27(mi) / lumped(mi), mi^3 = n the rows of the hierarchy.  Assembled without
    boundary removal: it would take every row of the diagonal `lumped` for a boundary node.  The size is checked here, before any
    launch: sgpu_debug_time_block takes bare pointers and checks none"""
    Bs = gg.mass(name, mi).tocoo()
    B = host.Matrix(comm)
    B.set_remove_boundary(False)
    B.set_many(Bs.row.astype(np.int32), Bs.col.astype(np.int32), Bs.data)
    B.assemble()
    op = host.device_operator(B)
    if B.num_local_rows != n or op.M != n or op.N_local != n:
        raise SystemExit(f"{name}: B is {op.M} x {op.N_local}, the hierarchy has {n} rows")
    return B, op


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    capi.init(0)
    print(capi.device_info(), flush=True)
    L = host.load("gpu")
    comm = host.Comm("gpu", "rccl")
    A = host.Matrix(comm).laplacian3D(m).assemble()
    t0 = time.time()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    n = A.num_local_rows
    print(f"--- Poisson, laplacian3D({m}): {n} = {m - 2}^3 rows, setup + upload + autotune {time.time() - t0:.1f} s, {S.num_levels} levels", flush=True)
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), lambda: None                                  # owned by the solver
    A0 = S.device_op(0)
    mi = m - 2                                                    # laplacian3D(m) removes its boundary rows: (m - 2)^3 interior rows
    if mi ** 3 != n:
        raise SystemExit(f"laplacian3D({m}) has {n} rows, not {mi}^3")
    masses = {name: device_mass(comm, name, mi, n) for name in gg.MASSES}
    rng = np.random.default_rng(5)
    for K in (2, 4, 8):
        X, Y, Out = (capi.BlockVector(n, K, rng.standard_normal((n, K))) for _ in range(3))
        print(f"--- K = {K}", flush=True)
        moved = 24 * n * K
        ceiling = lambda r: capi.stream_ceiling(16 * n * K, 8 * n * K, r)      # noqa: E731
        for name, fn in (("geig_residual", lambda r: G.time_geig(X, Y, Out, n, K, r)), ("eig_residual", lambda r: G.time_eig(2, 1, X, Y, Out, n, K, r))):
            t, (us_c, mode, mv_c) = timed(fn, ceiling, 50)
            print(f"{name:14s}: {t[0]:8.1f} us (again {t[1]:8.1f})  {moved / 1e6:7.1f} MB  {moved / t[0] / 1e3:6.0f} GB/s  "
                  f"ceiling {us_c:8.1f} us ({mode}, {mv_c / 1e6:7.1f} MB)  ceiling / kernel {us_c * moved / mv_c / t[0]:5.2f}", flush=True)
            if name == "geig_residual":
                residual = t[0]
        part = {}
        for name, kind, ns in (("gram", 0, 1), ("mix NS=1", 1, 1), ("mix NS=2", 1, 2)):
            G.time_eig(kind, ns, X, Y, Out, n, K, 3)
            part[name] = sorted(1e3 * G.time_eig(kind, ns, X, Y, Out, n, K, 50) for _ in range(3))[0]
        G.time_vcycle(Out, X, 3)
        vc = sorted(1e3 * G.time_vcycle(Out, X, 20) for _ in range(3))
        A0.time_block(0, X, None, Out, 3)
        mv = sorted(1e3 * A0.time_block(0, X, None, Out, 50) for _ in range(3))
        print(f"gram {part['gram']:8.1f} us, mix NS=1 {part['mix NS=1']:8.1f} us, mix NS=2 {part['mix NS=2']:8.1f} us, block V-cycle {vc[0]:8.1f} us "
              f"(again {vc[1]:8.1f}), block SpMV with A {mv[0]:8.1f} us (again {mv[1]:8.1f})", flush=True)
        X0 = er.start_vectors(n, K)
        nev = {2: 1, 4: 4, 8: 7}[K]                                   # ends at a gap of the spectrum (clusters of 1, 3, 3)
        for mass, (_, Bop) in masses.items():
            Bop.time_block(0, X, None, Out, 3)
            mb = sorted(1e3 * Bop.time_block(0, X, None, Out, 50) for _ in range(3))
            parts = vc[0] + mv[0] + mb[0] + 15 * part["gram"] + 9 * part["mix NS=1"] + 3 * part["mix NS=2"] + residual
            for iters in (8, 16):
                best = []
                for rep in range(4):
                    X.upload(X0)
                    capi.check(capi.lib().sgpu_device_sync())
                    t0 = time.perf_counter()
                    done = G.lobpcg(X, K, max_iter=iters, tol=0.0, B=Bop)[2]
                    capi.check(capi.lib().sgpu_device_sync())
                    if rep:
                        best.append(1e6 * (time.perf_counter() - t0) / max(done, 1))
                best.sort()
                print(f"{mass}: {iters:2d} iterations of the generalised LOBPCG: {best[0]:8.1f} us per iteration (again {best[1]:8.1f}); its kernels "
                      f"{parts:8.1f} us (V-cycle {vc[0]:.1f}, SpMV A {mv[0]:.1f}, SpMV B {mb[0]:.1f}, Gram {15 * part['gram']:.1f}, "
                      f"mix {9 * part['mix NS=1'] + 3 * part['mix NS=2']:.1f}, residual {residual:.1f}), host and gaps {best[0] - parts:8.1f} us", flush=True)
            for rep in range(2):
                for Bq in (Bop, None):
                    X.upload(X0)
                    capi.check(capi.lib().sgpu_device_sync())
                    t0 = time.perf_counter()
                    lam, res, it, _, conv = G.lobpcg(X, nev, max_iter=2000, tol=1e-8, B=Bq)
                    capi.check(capi.lib().sgpu_device_sync())
                    print(f"to 1e-8, nev = {nev}, {mass if Bq is not None else 'standard'}: {it:4d} iterations, {1e3 * (time.perf_counter() - t0):9.1f} ms "
                          f"({'converged' if conv else 'not converged'}), lambda_0 = {lam[0]:.12e}", flush=True)
        del X, Y, Out


if __name__ == "__main__":
    main()
