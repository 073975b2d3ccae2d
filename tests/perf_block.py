"""Block right-hand sides against the scalar path (measurement script, not a test): python -m tests.perf_block [m]

Poisson m^3 on the product's own hierarchy (autotuned scalar forms).  In one process, after warm-up, with device events, BOTH sides
as back-to-back launches inside the library (sgpu_time_kernel / sgpu_debug_time_block / sgpu_debug_time_vcycle), so no host call
rate enters either figure:
  * per level, for A (one Jacobi sweep), R and P: K scalar applies of the autotuned form against ONE block apply, K = 2, 4, 8,
    alternated; the scalar side's second-best time is printed next to its best: the run's own spread;
  * the whole V-cycle: K replays of the scalar graph against one replay of the block graph;
  * pCG to the reference tolerance: K scalar solves against one block solve (wall clock, uploads excluded).
Each row carries the algorithmic bytes of both sides from the shapes: scalar K * sgpu_algorithmic_bytes; block
12 nnz + 4 (M + 1) + 8 K (N + M v) (+ 8 M for the shared inverse diagonal of a sweep), v the epilogue's block vectors besides x
(1 for a product, 2 for a Jacobi sweep)."""
import sys
import time

import numpy as np

from saena_amd import capi, host

KS = (2, 4, 8)


def compare(name, scalar_us, block, K, reps, bytes_scalar, bytes_block):
    """scalar_us() / block(): us of ONE scalar / ONE block apply.  Alternated: scalar, block, scalar, block, ..."""
    s, b = [], []
    for _ in range(3):
        s.append(K * scalar_us())
        b.append(block())
    s_lo, s_hi, b_lo = min(s), sorted(s)[1], min(b)
    print(f"{name:28s} K={K}: scalar {s_lo:9.1f} us (again {s_hi:9.1f}, spread {100 * (s_hi / s_lo - 1):4.1f} %)  block {b_lo:9.1f} us  "
          f"block/scalar {b_lo / s_lo:5.2f}  bytes {bytes_block / 1e6:9.1f} / {bytes_scalar / 1e6:9.1f} MB = {bytes_block / bytes_scalar:4.2f}  "
          f"block {bytes_block / b_lo / 1e3:6.0f} GB/s", flush=True)
    return s_lo, s_hi, b_lo


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    capi.init(0)
    print(capi.device_info(), flush=True)
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    t0 = time.time()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    print(f"Poisson {m}^3: setup + upload + autotune {time.time() - t0:.1f} s, {S.num_levels} levels", flush=True)
    for l in range(S.num_levels - 1):
        opA, opP, opR = S.device_op(l, 0), S.device_op(l, 1), S.device_op(l, 2)
        M, Mc = opA.M, opR.M
        ia, ip, ir = opA.info(), opP.info(), opR.info()
        reps = 20 if ia["nnz_local"] > 5e6 else 100
        print(f"--- level {l}: A {M} rows, {ia['nnz_local']} nnz ({ia['nnz_local'] / M:.1f} per row, scalar form {opA.variant()[1]}, block lanes {opA.block_lanes()}); "
              f"R {ir['nnz_local'] / max(Mc, 1):.1f} per row ({opR.variant()[1]}, block lanes {opR.block_lanes()}); "
              f"P {ip['nnz_local'] / M:.1f} per row ({opP.variant()[1]}, block lanes {opP.block_lanes()})", flush=True)
        x, y, rhs = capi.DeviceVector(M, np.ones(M)), capi.DeviceVector(M), capi.DeviceVector(M, np.ones(M))
        xc, yc = capi.DeviceVector(Mc, np.ones(Mc)), capi.DeviceVector(Mc)
        for K in KS:
            X, Y, B = capi.BlockVector(M, K, np.ones((M, K))), capi.BlockVector(M, K), capi.BlockVector(M, K, np.ones((M, K)))
            Xc, Yc = capi.BlockVector(Mc, K, np.ones((Mc, K))), capi.BlockVector(Mc, K)
            for _ in range(2):                                   # warm-up: code objects, buffers
                opA.time_block(1, X, B, Y, 2); opR.time_block(0, X, None, Yc, 2); opP.time_block(0, Xc, None, Y, 2)
                opA.time_kernel(1, x, rhs, y, 2); opR.time_kernel(0, x, None, yc, 2); opP.time_kernel(0, xc, None, y, 2)
            nA, nR, nP = ia["nnz_local"], ir["nnz_local"], ip["nnz_local"]
            compare(f"L{l} A Jacobi sweep", lambda: opA.time_kernel(1, x, rhs, y, reps) * 1e3, lambda: opA.time_block(1, X, B, Y, reps) * 1e3, K, reps,
                    K * opA.algorithmic_bytes(1), 12 * nA + 4 * (M + 1) + 8 * K * (M + 2 * M) + 8 * M)
            compare(f"L{l} R", lambda: opR.time_kernel(0, x, None, yc, reps) * 1e3, lambda: opR.time_block(0, X, None, Yc, reps) * 1e3, K, reps,
                    K * opR.algorithmic_bytes(0), 12 * nR + 4 * (Mc + 1) + 8 * K * (M + Mc))
            compare(f"L{l} P", lambda: opP.time_kernel(0, xc, None, y, reps) * 1e3, lambda: opP.time_block(0, Xc, None, Y, reps) * 1e3, K, reps,
                    K * opP.algorithmic_bytes(0), 12 * nP + 4 * (M + 1) + 8 * K * (Mc + M))
            for v in (X, Y, B, Xc, Yc):
                v.free()
    # ---- whole V-cycle and pCG
    G = capi.Amg.__new__(capi.Amg)
    G.h = capi._VP(S.device_handle())
    G.destroy = lambda: None                                     # owned by the solver
    n = A.num_local_rows
    rhs_h = A.laplacian3D_rhs()
    u, r = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, rhs_h)
    for K in KS:
        RH = np.stack([rhs_h * (1.0 + 0.25 * j) for j in range(K)], axis=1)
        U, R = capi.BlockVector(n, K, np.zeros((n, K))), capi.BlockVector(n, K, RH)
        sv, bv = [], []
        for _ in range(3):
            sv.append(K * G.time_vcycle(u, r, 10) * 1e3)
            bv.append(G.time_vcycle(U, R, 10) * 1e3)
        s_lo, s_hi, b_lo = min(sv), sorted(sv)[1], min(bv)
        print(f"V-cycle K={K}: {K} scalar replays {s_lo:9.1f} us (again {s_hi:9.1f}, spread {100 * (s_hi / s_lo - 1):4.1f} %)  one block replay {b_lo:9.1f} us  "
              f"block/scalar {b_lo / s_lo:5.2f}  per right-hand side {b_lo / K:9.1f} against {s_lo / K:9.1f} us", flush=True)
        capi.check(capi.lib().sgpu_device_sync())
        ts = []
        for _ in range(2):
            t0 = time.perf_counter()
            for j in range(K):
                it_s = G.solve_pCG(u, r)[0]
            capi.check(capi.lib().sgpu_device_sync())
            ts.append(time.perf_counter() - t0)
        tb = []
        for _ in range(2):
            t0 = time.perf_counter()
            its, _, conv = G.solve_pCG_block(U, R)
            capi.check(capi.lib().sgpu_device_sync())
            tb.append(time.perf_counter() - t0)
        print(f"pCG K={K}: {K} scalar solves ({it_s} iterations each) {1e3 * min(ts):8.2f} ms (again {1e3 * max(ts):8.2f})  one block solve (iterations {its}, "
              f"converged {conv}) {1e3 * min(tb):8.2f} ms  block/scalar {min(tb) / min(ts):5.2f}", flush=True)
        U.free(); R.free()


if __name__ == "__main__":
    main()
