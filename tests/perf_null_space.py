"""What knowing the constant null space costs per V-cycle and per pCG iteration (not collected by pytest):

    python -m tests.perf_null_space <n> [repeats = 3] [only]   the whole measurement, every figure from a fresh process; only: one
                                                               configuration, as direct:5
    python -m tests.perf_null_space one <n> <kind> <coarse> <max_level>

The pure-Neumann Laplacian of an n^3 box (tests/null_space_ref.neumann3d), Jacobi 3 + 3, a CONSISTENT right-hand side, so that kind 0
(the hierarchy as sgpu_amg_create makes it, which converges there only by luck) can serve as the baseline.  Kinds 1 and 0 alternate,
under "direct" (the whole hierarchy) and under "cg" and "device_cg" with the hierarchy cut at level 3.  Prints, per configuration, the
range over the repeats of the V-cycle time (sgpu_debug_time_vcycle) and of the pCG time per iteration -- both on the solver's own
hierarchy, with its captured graphs where it captures -- and the launches of one V-cycle and of one pCG solve counted on a second
hierarchy over the same device operators with use_graph = 0 (a captured V-cycle is one launch whatever it holds).
"""
import ctypes as C
import json
import subprocess
import sys
import time

import numpy as np

# (coarsest solver, max_level).  "direct" on the whole hierarchy, and cut at level 5 (a few hundred coarsest rows): past some depth the
# setup's coarsest operator no longer annihilates constants to 1e-10 and kind 1 is refused -- the line then says so
CONFIGS = (("direct", 20), ("direct", 5), ("cg", 3), ("device_cg", 3))


def one(n, kind, coarse, max_level):
    from saena_amd import capi, host
    from tests import null_space_ref as ns
    capi.init(0)
    L = host.load("gpu")
    A0 = ns.neumann3d(n).tocoo()
    M = host.Matrix(host.Comm("gpu", "rccl"))
    M.set_remove_boundary(False)
    M.set_many(A0.row.astype(np.int32), A0.col.astype(np.int32), A0.data)
    M.assemble()
    o = dict(host.OPTIONS001, max_level=max_level, dynamic_levels=1 if max_level >= 20 else 0)
    S = host.AmgSolver(M, host.options(L, **o), coarse_solver=coarse, null_space="constant" if kind else "none")
    try:
        S.to_device()
    except capi.SgpuError as e:                              # (kind 0 on a singular operator: the factorisation may refuse it)
        print("RESULT " + json.dumps(dict(kind=kind, coarse=coarse, refused=str(e))), flush=True)
        return
    G = capi.Amg.__new__(capi.Amg)
    G.h, G.destroy = C.c_void_p(S.device_handle()), (lambda: None)
    nl = S.num_levels
    E = capi.Amg([S.device_op(l, 0) for l in range(nl)], [S.device_op(l, 1) for l in range(nl - 1)], [S.device_op(l, 2) for l in range(nl - 1)],
                 smoother="jacobi", max_iter=o["solver_max_iter"], tol=o["relative_tol"], use_graph=False, coarse_solver=coarse,
                 null_space="constant" if kind else None)
    N = n ** 3
    rhs = ns.center(ns.rhs_for(N))[0]
    du, drhs = capi.DeviceVector(N), capi.DeviceVector(N, rhs)
    E.vcycle(du, drhs)
    l0 = capi.launch_count()
    E.vcycle(du, drhs)
    l1 = capi.launch_count()
    eit, _, _ = E.solve_pCG(du, drhs)
    launches, pcg_launches = l1 - l0, capi.launch_count() - l1
    G.vcycle(du, drhs)
    vc = [G.time_vcycle(du, drhs, 20) for _ in range(3)]
    G.solve_pCG(du, drhs)
    per = []
    for _ in range(3):
        capi.check(capi.lib().sgpu_device_sync())
        t0 = time.perf_counter()
        it, hist, conv = G.solve_pCG(du, drhs)
        capi.check(capi.lib().sgpu_device_sync())
        per.append(1e3 * (time.perf_counter() - t0) / max(1, it))
    print("RESULT " + json.dumps(dict(kind=kind, coarse=coarse, levels=S.num_levels, vcycle_ms=min(vc), pcg_ms_per_it=min(per), iters=it,
                                      converged=bool(conv), launches_per_vcycle=launches, launches_per_pcg=pcg_launches, eager_iters=eit)), flush=True)


def main():
    if sys.argv[1] == "one":
        return one(int(sys.argv[2]), int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    n, reps = int(sys.argv[1]), int(sys.argv[2]) if len(sys.argv) > 2 else 3
    only = sys.argv[3] if len(sys.argv) > 3 else None
    rows = {}
    for coarse, max_level in CONFIGS:
        if only and only != f"{coarse}:{max_level}":
            continue
        for _ in range(reps):
            for kind in (1, 0):
                out = subprocess.run([sys.executable, "-m", "tests.perf_null_space", "one", str(n), str(kind), coarse, str(max_level)],
                                     capture_output=True, text=True, timeout=900)
                if out.returncode != 0:                       # a failed child ends the measurement: nothing more is started on the card
                    print(out.stdout[-2000:], out.stderr[-3000:])
                    return out.returncode
                r = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
                if "refused" in r:
                    print(f"neumann3d({n}) {coarse} max_level {max_level} kind {kind}: refused: {r['refused']}", flush=True)
                    continue
                rows.setdefault((coarse, max_level, kind), []).append(r)
    for (coarse, max_level, kind), rs in rows.items():
        v, p = [r["vcycle_ms"] for r in rs], [r["pcg_ms_per_it"] for r in rs]
        print(f"neumann3d({n}) {coarse:9s} max_level {max_level:2d} kind {kind}: {rs[0]['levels']} levels, V-cycle {min(v):.3f}-{max(v):.3f} ms, pCG {min(p):.3f}-{max(p):.3f} ms per "
              f"iteration ({sorted({r['iters'] for r in rs})} iterations, converged {all(r['converged'] for r in rs)}), "
              f"eager launches: {rs[0]['launches_per_vcycle']} per V-cycle, {rs[0]['launches_per_pcg']} per pCG solve of {rs[0]['eager_iters']} iterations", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
