"""Block solves across ranks: several processes on this one card, halos and reductions routed through gloo
(sgpu_debug_init_host_transport; RCCL needs one device per rank) -- the pattern of tests/test_gpu_vcycle.py's multi-rank solve.

Poisson 32^3, options001, the row-distributed hierarchy.  Every worker runs solve_pCG_block with K = 4 -- the Poisson right-hand
side, a scaled and shifted copy, an exactly zero column, inputs.rhs2 -- then the scalar solve_pCG on each non-zero column, one block
V-cycle from zero against the scalar sgpu_vcycle per column, and asks for LOBPCG and FGMRES, which stay on one rank.
Asserted: every rank reports the same iteration counts and histories; the zero column has 0 iterations and u = 0; per column the
iteration count is the scalar solve's, every history entry within 1e-9 h0 + 1e-6 h of it (the bound the scalar multi-rank test
uses between rank counts) and the solution within rel-l2 1e-9 -- after checking that no scalar history entry lies within a
factor 1 +- 1e-3 of its threshold, where a last-bit difference could move the count.  With fp32 halos (float_level = 0):
convergence and the same-on-every-rank property, as the scalar fp32-halo solve test."""
import numpy as np
import pytest

from tests.test_gpu_vcycle import POLICIES, TOL_VCYCLE

pytestmark = pytest.mark.gpu
K = 4
NONZERO = (0, 1, 3)


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def _worker(rank, world, port, smoother, float_level, policy, ret):
    import os
    import sys
    import torch.distributed as dist                      # torch first (its HIP runtime), like bench.py --gpus N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(POLICIES[policy])
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from saena_amd import capi as c, host
        from tests import inputs
        c.init_host_transport(0, dist)
        L = host.load("gpu")
        A = host.Matrix(host.Comm("gpu", "dist", dist)).laplacian3D(32).assemble()
        S = host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, smoother=smoother, float_level=float_level))).to_device()
        split = [int(x) for x in A.split]
        n = A.num_local_rows
        b0 = A.laplacian3D_rhs()
        B = np.stack([b0, 0.5 * b0 + 3.0, np.zeros(n), inputs.rhs2(split[-1])[split[rank]:split[rank + 1]]], axis=1)
        U, its, hists, ok = S.solve_pCG_block(B)
        scalar = {}
        for j in NONZERO:
            u, it, hist, okj = S.solve_pCG(B[:, j])
            scalar[j] = (it, [float(h) for h in hist], bool(okj), float(np.sum((U[:, j] - u) ** 2)), float(np.sum(u ** 2)))
        # one block V-cycle from zero against the scalar V-cycle per column (this rank's rows; the norms are summed by the parent)
        dU, dB = c.BlockVector(n, K, np.zeros((n, K))), c.BlockVector(n, K, B)
        c.check(c.lib().sgpu_vcycle_block(S.device_handle(), dU.ptr, dB.ptr, K))
        VU = dU.download()
        vc = {}
        for j in range(K):
            du, dr = c.DeviceVector(n, np.zeros(n)), c.DeviceVector(n, B[:, j])
            c.check(c.lib().sgpu_vcycle(S.device_handle(), du.ptr, dr.ptr))
            v = du.download()
            vc[j] = (float(np.sum((VU[:, j] - v) ** 2)), float(np.sum(v ** 2)))
        refused = []
        for what, call in (("lobpcg", lambda: S.eigs(2, 1)), ("fgmres", lambda: S.solve_pFGMRES(b0))):
            try:
                call()
                refused.append(f"{what}: not refused")
            except Exception as e:      # noqa
                refused.append(str(e))
        ret[rank] = ("ok", its, [[float(h) for h in hj] for hj in hists], bool(ok), float(np.abs(U[:, 2]).max()) if n else 0.0, scalar, vc, refused,
                     float(host.OPTIONS001["relative_tol"]))
    except BaseException as e:      # noqa
        import traceback
        ret[rank] = ("".join(traceback.format_exception(type(e), e, e.__traceback__)),)
    finally:
        dist.destroy_process_group()


def _run(world, smoother, float_level, policy):
    import multiprocessing as mp      # not torch's: this process already runs the system HIP runtime
    import socket
    assert world <= 4
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, world, port, smoother, float_level, policy, ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
        alive = [p.is_alive() for p in procs]
        for p in procs:
            if p.is_alive():
                p.terminate()
        res = dict(ret)
    assert not any(alive), f"workers still running at the time limit: {alive} (a rank that skipped a collective?)"
    for r in range(world):
        assert res.get(r) and res[r][0] == "ok", f"rank {r}: {res.get(r)}"
    return res


@pytest.mark.parametrize("world,smoother,float_level,policy", [(3, "jacobi", 3, "rows4096"), (4, "chebyshev", 3, "stride"), (3, "jacobi", 0, "rows4096")],
                         ids=["3-jacobi", "4-chebyshev-stride", "3-jacobi-fp32-halos"])
def test_block_pcg_and_vcycle_across_ranks(capi, world, smoother, float_level, policy):
    res = _run(world, smoother, float_level, policy)
    _, its, hists, ok, zero_max, scalar, vc, refused, tol = res[0]
    for r in range(1, world):
        assert res[r][1] == its and res[r][2] == hists and res[r][3] == ok, "every rank must report the same iteration counts and histories"
        for j in NONZERO:
            assert res[r][5][j][:3] == scalar[j][:3]
    for r in range(world):
        assert all("one rank" in m for m in res[r][7]), res[r][7]
    assert ok, (its, [h[-1] for h in hists])
    assert its[2] == 0 and len(hists[2]) == 1 and hists[2][0] == 0.0 and all(res[r][4] == 0.0 for r in range(world)), "the zero column: 0 iterations, u = 0"
    assert all(its[j] > 0 and hists[j][-1] < tol * hists[j][0] for j in NONZERO), (its, hists)
    if float_level == 0:
        return
    for j in NONZERO:
        it1, h1, ok1 = scalar[j][:3]
        h1 = np.array(h1)
        thr = tol * h1[0]
        assert ok1 and not np.any((h1 > thr * (1 - 1e-3)) & (h1 < thr * (1 + 1e-3))), f"column {j}: a scalar history entry sits at its threshold: {h1}, {thr}"
        assert its[j] == it1, (j, its[j], it1)
        hb = np.array(hists[j])
        assert hb.shape == h1.shape and np.all(np.abs(hb - h1) <= 1e-9 * h1[0] + 1e-6 * h1), (j, hb, h1)
        err = np.sqrt(sum(res[r][5][j][3] for r in range(world)) / sum(res[r][5][j][4] for r in range(world)))
        assert err <= 1e-9, (j, err)
    for j in range(K):
        num, den = sum(res[r][6][j][0] for r in range(world)), sum(res[r][6][j][1] for r in range(world))
        if j == 2:
            assert num == 0.0 and den == 0.0
            continue
        assert np.sqrt(num / den) <= TOL_VCYCLE, (j, np.sqrt(num / den))
