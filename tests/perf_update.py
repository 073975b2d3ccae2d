"""update2 and update1 against the full setup of the same operator (measurement script, not a test): python -m tests.perf_update [m] [steps]

Poisson m^3 (default 128) plus c_k times a fixed positive diagonal field (c_k = 0.01 k, as examples/poisson_update.cpp; the field between 0.5 and 1.5), k = 1 .. steps
(default 3), in one process, on the product's own options (Chebyshev 3 + 3, the reference's options001 otherwise).  For every k:

  fresh    a new AmgSolver on operator k: saena_amg_set_matrix (the whole host setup), then saena_amg_to_device;
  update2  ONE solver built on operator 0: saena_amg_update(A_k, 2) -- R A P over the kept aggregates, P and R, the filter, the eigenvalue
           estimates, then new device operators for every A;
  update1  ONE solver built on operator 0: saena_amg_update(A_k, 1) -- only the finest operator follows.

Printed per k: wall-clock seconds of each (host part and device part apart for the fresh setup), and the pCG iterations of the three
solvers on the same right-hand side.  The baseline is existing code (set_matrix of the same operator in the same process), not the code
under test.  SAENA_SETUP_TIMING=1 is set: the phase lines of every setup ("[setup L<l>] ...") and update ("[update L<l>] ...") go to
stderr."""
import os
import sys
import time

import numpy as np

os.environ.setdefault("SAENA_SETUP_TIMING", "1")

from saena_amd import capi, host          # noqa: E402


def operator(m, c):
    """the assembled Laplacian m^3 (boundary rows removed) with c * field added to its diagonal, as a new Matrix"""
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    if c == 0.0:
        return A
    d = A.layout()
    n = int(d["M"])
    r = np.repeat(np.arange(n, dtype=np.int32), d["nnzPerRow_local"])
    col, val = d["col_local"], d["val_local"].copy()
    on = r == col
    val[on] += c * (1.0 + 0.5 * np.sin(0.01 * np.arange(n)))[r[on]]
    B = host.Matrix(host.Comm("gpu", "rccl"))
    B.set_remove_boundary(False)
    B.set_many(r, col, val)
    B.assemble()
    A.free()
    return B


def main():
    m = int(sys.argv[1]) if len(sys.argv) > 1 else 128
    steps = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    capi.init(0)
    L = host.load("gpu")
    print(capi.device_info(), flush=True)
    opts = dict(host.OPTIONS001, smoother="chebyshev")

    def fresh(A):
        t0 = time.perf_counter()
        S = host.AmgSolver(A, host.options(L, **opts))
        t1 = time.perf_counter()
        S.to_device()
        return S, t1 - t0, time.perf_counter() - t1

    A0a, A0b = operator(m, 0.0), operator(m, 0.0)
    n = A0a.num_local_rows
    rhs = np.sin(0.37 * np.arange(n) + 0.1) + 0.05
    S2, h, d = fresh(A0a)
    print(f"operator 0: {n} rows, {S2.num_levels} levels; set_matrix {h:.3f} s + to_device {d:.3f} s", flush=True)
    S1, _, _ = fresh(A0b)
    keep2, keep1 = A0a, A0b
    for k in range(1, steps + 1):
        c = 0.01 * k
        Af, B2, B1 = operator(m, c), operator(m, c), operator(m, c)
        print(f"--- step {k}: fresh set_matrix", file=sys.stderr, flush=True)
        Sf, t_host, t_dev = fresh(Af)
        print(f"--- step {k}: update2", file=sys.stderr, flush=True)
        t0 = time.perf_counter(); S2.update(B2, 2); t_u2 = time.perf_counter() - t0
        keep2.free(); keep2 = B2
        print(f"--- step {k}: update1", file=sys.stderr, flush=True)
        t0 = time.perf_counter(); S1.update(B1, 1); t_u1 = time.perf_counter() - t0
        keep1.free(); keep1 = B1
        its = []
        for S in (Sf, S2, S1):
            _, it, hist, conv = S.solve_pCG(rhs)
            its.append(f"{it}{'' if conv else ' (not converged)'}")
        print(f"step {k} (c = {c:.3f}): set_matrix + to_device {t_host + t_dev:.3f} s ({t_host:.3f} + {t_dev:.3f}), update2 {t_u2:.3f} s, "
              f"update1 {t_u1:.3f} s; update2 / setup = {t_u2 / (t_host + t_dev):.3f}; pCG iterations fresh {its[0]}, update2 {its[1]}, "
              f"update1 {its[2]}", flush=True)
        Sf.free(); Af.free()


if __name__ == "__main__":
    main()
