"""The device coarsest CG against the host-driven loop on a coarsest level past 1 024 rows (measurement script, not a test):
python -m tests.perf_coarse_cg <mode> [max_level] [m]

Poisson m^3 (default 128) on the product's own options (Chebyshev 3 + 3, the reference's options001 otherwise) with the hierarchy cut at
`max_level` (default 3; at 128^3, 3 and 4 leave coarsest levels of 13 633 and 2 569 rows).  The host setup runs once; its device
operators then serve two hierarchies made with sgpu_amg_create, one with use_graph = 0 and one with use_graph = 1, under

  mode host        coarse_solver "CG": past 1 024 rows the host-driven loop (three allocations per V-cycle, two round trips per CG
                   iteration, no graph capture whatever use_graph says) -- what "direct" runs there too;
  mode device_cg   coarse_solver "device_cg": the fixed launch sequence of saena_amd/csrc/kernels_coarse_cg.hip.h, inside the graph.

Printed: ms per V-cycle (sgpu_debug_time_vcycle, 20 cycles back to back after one that captures) eager and captured, pCG iterations and
wall-clock ms (the second of two solves) eager and captured, the coarsest CG's iteration count on the V-cycle's own coarse right-hand
side stand-in (a smooth vector), and under device_cg one launch of the product kernel against sgpu_time_kernel of the coarsest
operator's tuned form.

`mode host` uses nothing this feature adds, so it runs on the parent commit's library too: put that commit's saena_amd/ package first
on sys.path (python -m puts the working directory first, so: python -c "import sys, runpy; sys.path.insert(0, PARENT); sys.argv =
['perf_coarse_cg', 'host', '3']; runpy.run_module('tests.perf_coarse_cg', run_name='__main__')"); the first line printed names the
library that was loaded.  For a comparison alternate the two modes in fresh processes on one box; profiles/device_cg_128.log is such a log."""
import sys
import time

import numpy as np

from saena_amd import capi, host


def main():
    mode = sys.argv[1] if len(sys.argv) > 1 else "device_cg"
    max_level = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    m = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    assert mode in ("host", "device_cg"), mode
    capi.init(0)
    L = host.load("gpu")
    print(f"mode {mode}, max_level {max_level}, Poisson {m}^3, library {capi.__file__}", flush=True)
    print(capi.device_info(), flush=True)
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(m).assemble()
    S = host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, smoother="chebyshev", dynamic_levels=0, max_level=max_level))).to_device()
    nl = S.num_levels
    rows = [S.level_info(l)["rows"] for l in range(nl)]
    eig = [S.level_info(l)["eig_max"] for l in range(nl)]
    print(f"{nl} levels, rows {rows}", flush=True)
    GA = [S.device_op(l, 0) for l in range(nl)]
    GP = [S.device_op(l, 1) for l in range(nl - 1)]
    GR = [S.device_op(l, 2) for l in range(nl - 1)]
    n, nc = rows[0], rows[-1]
    rhs = A.laplacian3D_rhs()
    du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, rhs)
    name = "CG" if mode == "host" else "device_cg"
    for use_graph in (False, True):
        G = capi.Amg(GA, GP, GR, eig_max=eig, pre=3, post=3, smoother="chebyshev", max_iter=100, tol=1e-8, use_graph=use_graph, coarse_solver=name)
        what = "captured" if use_graph else "eager"
        du.upload(np.zeros(n))
        G.vcycle(du, dr)                                     # (captures, where it can)
        l0 = capi.launch_count()
        ms = G.time_vcycle(du, dr, 20)
        per = (capi.launch_count() - l0) / 20.0
        print(f"{mode} {what}: V-cycle {ms:.4f} ms, {per:.1f} enqueues per cycle", flush=True)
        for rep in range(2):
            t0 = time.perf_counter()
            it, hist, conv = G.solve_pCG(du, dr)
            capi.check(capi.lib().sgpu_device_sync())
            t = (time.perf_counter() - t0) * 1e3
        print(f"{mode} {what}: pCG {it} iterations{'' if conv else ' (not converged)'}, {t:.3f} ms, ||r|| {hist[0]:.3e} -> {hist[-1]:.3e}", flush=True)
        if use_graph:
            bc = np.cos(0.05 * np.arange(nc)) - 0.3
            dcu, dcb = capi.DeviceVector(nc, np.zeros(nc)), capi.DeviceVector(nc, bc)
            t0 = time.perf_counter()
            itc = G.coarsest_solve(dcu, dcb)
            t = (time.perf_counter() - t0) * 1e3
            print(f"{mode}: coarsest CG on {nc} rows: {itc} iterations, {t:.3f} ms with the count read back", flush=True)
            if mode == "device_cg":
                dx, dy = capi.DeviceVector(nc, bc), capi.DeviceVector(nc)
                GA[-1].time_kernel(0, dx, None, dy, 5)
                tuned = GA[-1].time_kernel(0, dx, None, dy, 200) * 1e3
                own = G.time_dcg_matvec(dx, dy, 200) * 1e3
                print(f"device_cg: product kernel {own:.2f} us per launch, the operator's tuned form {tuned:.2f} us "
                      f"({GA[-1].variant()}), {GA[-1].info()['nnz_local']} entries", flush=True)
        G.destroy()


if __name__ == "__main__":
    main()
