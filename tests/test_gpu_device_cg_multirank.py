"""The large coarsest level across ranks: a coarsest level of more than CG_MAXN = 1 024 rows in a three-rank world, under every value
of coarse_solver -- the device-resident CG (2, "device_cg") on the one rank that owns the level, inside and outside the multi-rank
tail graph, and the collective host-driven CG (0 "cg", 1 "direct") with two ranks of zero rows.

Several processes on this one card, halos and reductions routed through gloo (sgpu_debug_init_host_transport; RCCL needs one device
per rank) -- the pattern of tests/test_gpu_block_multirank.py.  The worlds are those of tests/device_cg_world.py (Poisson 32^3 cut at
max_level = 2: rows 27 000 / 13 500 / 1 420), whose rows and owners tests/test_device_cg_multirank_cases.py holds on the CPU.  Every
worker runs with SAENA_NO_AUTOTUNE=1: bits are compared between processes, and the plan-time autotune picks kernels by timing.

Every comparison is against a run that shares none of the code in question -- the eager form (SAENA_NO_TAIL_GRAPH=1), the one-rank
solve in this process, the host-driven CG -- or against numpy in high precision (solver_ref.residual_hp on the scipy matrix, with u
assembled from the ranks' slices).  Bounds: bit identity; exact launch counts derived from the code; between rank counts and between
coarsest solvers the iteration count and 1e-9 h0 + 1e-6 h per history entry (tests/test_gpu_vcycle.py's bound between rank counts),
after checking that no reference entry lies within a factor 1 +- 1e-3 of the threshold (tests/test_gpu_block_multirank.py's guard).

Every worker also calls sgpu_coarsest_solve on its own and asks which rank holds the device CG's work space: under "device_cg" the
owner enqueues 449 launches and the other ranks none, and the work space exists on the owner alone.

Each test makes its own spawns: a worker that fails or hangs fails its own test only."""
import numpy as np
import pytest

from tests import device_cg_ref as dr, device_cg_world as dw, solver_ref as sr
from tests.test_gpu_vcycle import TOL_VCYCLE

pytestmark = pytest.mark.gpu
FULL = dr.launches(sr.CG_MAX_ITER)      # 449: the device CG's sequence, which a tail graph absorbs
K = 4
NONZERO = (0, 1, 3)
TOL = 1e-8                              # host.OPTIONS001["relative_tol"]


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def problem():
    """-> (scipy matrix, rhs) of Poisson 32^3, from the oracle's entries"""
    import scipy.sparse as sp
    from oracle import oracle as orc
    e, M = orc.laplacian3d(dw.M)
    return sp.csr_matrix((e["val"], (e["row"], e["col"])), shape=(M, M)), orc.laplacian3d_rhs(dw.M)


@pytest.fixture(scope="module")
def one_rank(capi):
    """the same cut hierarchy with "device_cg" on one rank, in this process -> (iterations, history)"""
    from saena_amd import host
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "self")).laplacian3D(dw.M).assemble()
    S = host.AmgSolver(A, dw.options(host, L), coarse_solver="device_cg").to_device()
    assert [S.level_info(l)["rows"] for l in range(S.num_levels)] == dw.ROWS
    _, it, hist, ok = S.solve_pCG(A.laplacian3D_rhs())
    assert ok
    return it, np.array(hist)


def _worker(rank, world, port, config, solver, env, what, ret):
    import os
    import sys
    import torch.distributed as dist                      # torch first (its HIP runtime), like bench.py --gpus N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(dw.CONFIGS[config]["env"])
    os.environ["SAENA_NO_AUTOTUNE"] = "1"
    os.environ.update(env or {})
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from saena_amd import capi as c, host
        from tests import inputs
        c.init_host_transport(0, dist)
        L = host.load("gpu")
        A = host.Matrix(host.Comm("gpu", "dist", dist)).laplacian3D(dw.M).assemble()
        S = host.AmgSolver(A, dw.options(host, L), coarse_solver=solver).to_device()
        split = [int(x) for x in A.split]
        n = A.num_local_rows
        b0 = A.laplacian3D_rhs()
        out = dict(rows=[S.level_info(l)["rows"] for l in range(S.num_levels)], owners=dw.owners_of(S, world), split=split)

        def refusal(call):
            try:
                call()
                return "not refused"
            except Exception as e:      # noqa
                return str(e)

        if what == "solve":
            u, it, hist, ok = S.solve_pCG(b0)
            du, drhs = c.DeviceVector(n, np.zeros(n)), c.DeviceVector(n, b0)
            c.check(c.lib().sgpu_vcycle(S.device_handle(), du.ptr, drhs.ptr))
            l0 = c.launch_count()
            c.check(c.lib().sgpu_vcycle(S.device_handle(), du.ptr, drhs.ptr))
            out.update(it=it, hist=[float(h) for h in hist], ok=bool(ok), launches=c.launch_count() - l0, u=u.tobytes(),
                       v=du.download().tobytes(), rhs=b0.tobytes())
            # sgpu_coarsest_solve on its own (collective where the coarsest CG is host-driven: every rank calls it): count and launches
            import ctypes as C
            from tests import solver_ref
            sc = [int(x) for x in S.level_split(S.num_levels - 1)]
            nc = sc[rank + 1] - sc[rank]
            dcu = c.DeviceVector(max(nc, 1), np.zeros(max(nc, 1)))
            dcr = c.DeviceVector(max(nc, 1), solver_ref.rhs_for(sc[-1])[sc[rank]:sc[rank + 1]] if nc else np.zeros(1))
            itc = C.c_int(-1)
            l0 = c.launch_count()
            c.check(c.lib().sgpu_coarsest_solve(S.device_handle(), dcu.ptr, dcr.ptr, C.byref(itc)))
            out.update(coarse_it=itc.value, coarse_launches=c.launch_count() - l0)
            # which ranks hold the device CG's work space: the debug timer of its product kernel refuses a hierarchy without one
            ms = C.c_float()
            out["work_space"] = refusal(lambda: c.check(c.lib().sgpu_debug_dcg_matvec_time(S.device_handle(), dcr.ptr, dcu.ptr, 1, C.byref(ms))))
            if config == "rows300":      # refused before any collective, on every rank alike
                out["block"] = refusal(lambda: S.solve_pCG_block(np.stack([b0, 0.5 * b0], axis=1)))
        else:
            B = np.stack([b0, 0.5 * b0 + 3.0, np.zeros(n), inputs.rhs2(split[-1])[split[rank]:split[rank + 1]]], axis=1)
            if solver != "device_cg":
                out["block"] = refusal(lambda: S.solve_pCG_block(B))
            else:
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
                    du, drhs = c.DeviceVector(n, np.zeros(n)), c.DeviceVector(n, B[:, j])
                    c.check(c.lib().sgpu_vcycle(S.device_handle(), du.ptr, drhs.ptr))
                    v = du.download()
                    vc[j] = (float(np.sum((VU[:, j] - v) ** 2)), float(np.sum(v ** 2)))
                out.update(its=its, hists=[[float(h) for h in hj] for hj in hists], ok=bool(ok), zero_max=float(np.abs(U[:, 2]).max()) if n else 0.0,
                           scalar=scalar, vc=vc, refused=[refusal(lambda: S.eigs(2, 1)), refusal(lambda: S.solve_pFGMRES(b0))])
        ret[rank] = ("ok", out)
    except BaseException as e:      # noqa
        import traceback
        ret[rank] = ("".join(traceback.format_exception(type(e), e, e.__traceback__)),)
    finally:
        dist.destroy_process_group()


def _run(config, solver, env=None, what="solve"):
    """one spawn of three workers -> [the dict of rank r]"""
    import multiprocessing as mp      # not torch's: this process already runs the system HIP runtime
    import socket
    world = dw.WORLD
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, world, port, config, solver, env, what, ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
        alive = [p.is_alive() for p in procs]
        for p in procs:
            if p.is_alive():
                p.terminate()
        res = dict(ret)
    assert not any(alive), f"{config} {solver}: workers still running at the time limit: {alive} (a rank that skipped a collective?)"
    for r in range(world):
        assert res.get(r) and res[r][0] == "ok", f"{config} {solver} rank {r}: {res.get(r)}"
    out = [res[r][1] for r in range(world)]
    for r in range(world):
        assert out[r]["rows"] == dw.ROWS and out[r]["owners"] == dw.CONFIGS[config]["owners"], (config, r, out[r]["rows"], out[r]["owners"])
    return out


def same_on_every_rank(res, what):
    for r in range(1, len(res)):
        assert (res[r]["it"], res[r]["hist"], res[r]["ok"]) == (res[0]["it"], res[0]["hist"], res[0]["ok"]), f"{what}: rank {r} reports another history than rank 0"


def bit_identical(a, b, what):
    """two spawns: histories, u and the V-cycle output of every rank"""
    for r in range(len(a)):
        assert a[r]["it"] == b[r]["it"] and a[r]["hist"] == b[r]["hist"], f"{what}: rank {r}: the histories differ: {a[r]['hist']} {b[r]['hist']}"
        assert a[r]["u"] == b[r]["u"], f"{what}: rank {r}: u differs"
        assert a[r]["v"] == b[r]["v"], f"{what}: rank {r}: the V-cycle output differs"


def guard(it1, h1, what):
    """no entry of the reference history within a factor 1 +- 1e-3 of the threshold, where a last-bit difference could move the count"""
    thr = TOL * h1[0]
    assert not np.any((h1 > thr * (1 - 1e-3)) & (h1 < thr * (1 + 1e-3))), f"{what}: a reference history entry sits at its threshold: {h1}, {thr}"


def close_histories(it, hist, it1, h1, what):
    """the count, and every entry within 1e-9 h0 + 1e-6 h of the reference history"""
    guard(it1, h1, what)
    hist = np.array(hist)
    worst = float(np.max(np.abs(hist - h1) / (1e-9 * h1[0] + 1e-6 * h1))) if hist.shape == h1.shape else float("nan")
    print(f"{what}: {it} iterations (reference {it1}), worst history deviation {worst:.3g} of its bound")
    assert it == it1, (what, it, it1)
    assert hist.shape == h1.shape and np.all(np.abs(hist - h1) <= 1e-9 * h1[0] + 1e-6 * h1), (what, hist, h1)


def residual_check(problem, res, what):
    """u assembled from the ranks' slices, on the scipy matrix, in np.longdouble"""
    A, rhs = problem
    split = res[0]["split"]
    u = np.concatenate([np.frombuffer(res[r]["u"], np.float64) for r in range(len(res))])
    b = np.concatenate([np.frombuffer(res[r]["rhs"], np.float64) for r in range(len(res))])
    assert len(u) == split[-1] == A.shape[0] and [len(res[r]["u"]) // 8 for r in range(len(res))] == list(np.diff(split))
    assert np.array_equal(b, rhs), "the ranks' right-hand side is not the Poisson right-hand side"
    got, bound = sr.residual_hp(A, u, rhs), TOL * np.linalg.norm(rhs) * (1 + 1e-6)
    print(f"{what}: high-precision residual {got:.6e} of {bound:.6e}")
    assert got <= bound


def device_cg_runs_on_the_owner_alone(res, what):
    """sgpu_coarsest_solve under "device_cg": the owner enqueues the whole sequence, a rank without a coarsest row returns at once --
    not one launch (a k_coarse_cg on zero rows would be one), count 0"""
    print(f"{what}: sgpu_coarsest_solve launches per rank {[x['coarse_launches'] for x in res]}, counts {[x['coarse_it'] for x in res]}")
    assert [x["coarse_launches"] for x in res] == [FULL, 0, 0]
    held = ["no device CG on this rank" not in x["work_space"] for x in res]
    assert held == [True, False, False] and res[0]["work_space"] == "not refused", [x["work_space"] for x in res]      # the work space: on the owner alone
    assert 1 < res[0]["coarse_it"] <= sr.CG_MAX_ITER - 1 and [x["coarse_it"] for x in res[1:]] == [0, 0]      # (1 420 rows may take the whole cap)


def graph_against_eager(config, more_on_rank0, problem, one_rank):
    a = _run(config, "device_cg")
    b = _run(config, "device_cg", env={"SAENA_NO_TAIL_GRAPH": "1"})
    la, lb = [x["launches"] for x in a], [x["launches"] for x in b]
    print(f"{config}: owners {a[0]['owners']}, {a[0]['it']} iterations; launches of a V-cycle per rank: graph {la}, eager {lb}; "
          f"rank 0 difference {lb[0] - la[0]} (at least {more_on_rank0})")
    same_on_every_rank(a, f"{config} graph")
    same_on_every_rank(b, f"{config} eager")
    bit_identical(a, b, f"{config}: tail graph against eager")
    assert a[0]["ok"]
    assert lb[0] - la[0] >= more_on_rank0, (la, lb)
    assert lb[0] > FULL                                                    # (rank 0 does run the sequence)
    device_cg_runs_on_the_owner_alone(a, f"{config} graph")
    device_cg_runs_on_the_owner_alone(b, f"{config} eager")
    for r in (1, 2):
        assert la[r] == lb[r] < FULL, f"rank {r} owns no coarsest row: it runs no coarsest sequence, graph or not ({la}, {lb})"
    # against one rank, and against high precision
    it1, h1 = one_rank
    close_histories(a[0]["it"], a[0]["hist"], it1, h1, f"{config} device_cg at 3 ranks against one rank")
    residual_check(problem, a, f"{config} device_cg")


def test_model_the_tail_graph_holds_the_device_cg(capi, problem, one_rank):
    """levels 1 and 2 on rank 0: the tail graph holds level 1 and the 449 launches of the coarsest solve.  Eagerly rank 0 pays
    FULL - 1 more for the sequence (the graph is one launch) and at least 6 more for the other tail level (tests/test_gpu_vcycle.py's
    figure); ranks 1 and 2 launch the same number either way"""
    graph_against_eager("model", FULL - 1 + 6, problem, one_rank)


def test_rows4096_the_tail_is_the_coarsest_solve_alone(capi, problem, one_rank):
    """level 1 exchanges halos on all three ranks around a tail that is the device CG alone"""
    graph_against_eager("rows4096", FULL - 1, problem, one_rank)


@pytest.mark.parametrize("config", ["model", "rows4096"])
def test_the_host_driven_cg_with_ranks_of_zero_rows(capi, problem, config):
    """coarse_solver 0 and 1 on the same hierarchies: the collective host-driven CG, in which ranks 1 and 2 hold no row and still take
    part in every dot.  Against the device CG's run at 3 ranks (a spawn of this test's own): the count, the history bound.  "direct"
    has "cg"'s history bit for bit: past 1 024 rows it is ignored"""
    dev = _run(config, "device_cg")
    cg = _run(config, "cg")
    direct = _run(config, "direct")
    for res, name in ((dev, "device_cg"), (cg, "cg"), (direct, "direct")):
        same_on_every_rank(res, f"{config} {name}")
        print(f"{config} {name}: {res[0]['it']} iterations, launches per rank {[x['launches'] for x in res]}, last entry {res[0]['hist'][-1]:.6e}")
        assert res[0]["ok"] and res[0]["hist"][-1] < TOL * res[0]["hist"][0]
    device_cg_runs_on_the_owner_alone(dev, f"{config} device_cg")
    for res, name in ((cg, "cg"), (direct, "direct")):      # collective: every rank reports the one count, and no rank sits it out
        its, ls = [x["coarse_it"] for x in res], [x["coarse_launches"] for x in res]
        print(f"{config} {name}: sgpu_coarsest_solve counts {its}, launches {ls}")
        assert len(set(its)) == 1 and 1 < its[0] <= sr.CG_MAX_ITER - 1 and all(l > 0 for l in ls)
        assert all("no device CG on this rank" in x["work_space"] for x in res), [x["work_space"] for x in res]
    assert [x["coarse_it"] for x in cg] == [x["coarse_it"] for x in direct]
    it1, h1 = dev[0]["it"], np.array(dev[0]["hist"])
    close_histories(cg[0]["it"], cg[0]["hist"], it1, h1, f"{config} cg against device_cg")
    residual_check(problem, cg, f"{config} cg")
    residual_check(problem, direct, f"{config} direct")
    bit_identical(cg, direct, f"{config}: direct against cg")


def test_rows300_a_row_partitioned_coarsest_level_ignores_value_2(capi, problem):
    """the coarsest level on all three ranks: the distributed CG whatever coarse_solver says, so "device_cg" has "cg"'s bits; the
    block solve is refused on every rank alike"""
    dev = _run("rows300", "device_cg")
    cg = _run("rows300", "cg")
    same_on_every_rank(dev, "rows300 device_cg")
    same_on_every_rank(cg, "rows300 cg")
    print(f"rows300: {dev[0]['it']} iterations, launches per rank {[x['launches'] for x in dev]}, block solve: {dev[0]['block'][:60]}...")
    bit_identical(dev, cg, "rows300: device_cg against cg")
    for k in ("coarse_it", "coarse_launches", "launches"):      # the same code ran: the distributed CG, one count on every rank
        print(f"rows300 {k}: device_cg {[x[k] for x in dev]}, cg {[x[k] for x in cg]}")
        assert [x[k] for x in dev] == [x[k] for x in cg]
    assert len({x["coarse_it"] for x in dev}) == 1
    assert all("no device CG on this rank" in x["work_space"] for x in dev + cg), "value 2 made a work space for a row-partitioned level"
    assert dev[0]["ok"] and dev[0]["hist"][-1] < TOL * dev[0]["hist"][0]
    residual_check(problem, dev, "rows300 device_cg")
    for res in (dev, cg):
        for r in range(dw.WORLD):
            assert "row-partitioned" in res[r]["block"], (r, res[r]["block"])


def test_block_solves_on_model_with_the_device_cg(capi):
    """tests/test_gpu_block_multirank.py's body at K = 4 on the cut hierarchy: rank 0 runs the device CG column by column inside the
    block V-cycle, ranks 1 and 2 return at once.  Under "cg" the block solve is refused on every rank, those without a coarsest row
    included"""
    res = _run("model", "device_cg", what="block")
    world = dw.WORLD
    its, hists, ok, scalar, vc = (res[0][k] for k in ("its", "hists", "ok", "scalar", "vc"))
    print(f"block: iterations {its}, scalar {[scalar[j][0] for j in NONZERO]}")
    for r in range(1, world):
        assert res[r]["its"] == its and res[r]["hists"] == hists and res[r]["ok"] == ok, "every rank must report the same iteration counts and histories"
        for j in NONZERO:
            assert res[r]["scalar"][j][:3] == scalar[j][:3]
    for r in range(world):
        assert all("one rank" in m for m in res[r]["refused"]), res[r]["refused"]
    assert ok, (its, [h[-1] for h in hists])
    assert its[2] == 0 and len(hists[2]) == 1 and hists[2][0] == 0.0 and all(res[r]["zero_max"] == 0.0 for r in range(world)), "the zero column: 0 iterations, u = 0"
    assert all(its[j] > 0 and hists[j][-1] < TOL * hists[j][0] for j in NONZERO), (its, hists)
    for j in NONZERO:
        it1, h1, ok1 = scalar[j][:3]
        assert ok1
        close_histories(its[j], hists[j], it1, np.array(h1), f"block column {j} against its scalar solve")
        err = np.sqrt(sum(res[r]["scalar"][j][3] for r in range(world)) / sum(res[r]["scalar"][j][4] for r in range(world)))
        print(f"block column {j}: rel-l2 to the scalar solution {err:.3g}")
        assert err <= 1e-9, (j, err)
    for j in range(K):
        num, den = sum(res[r]["vc"][j][0] for r in range(world)), sum(res[r]["vc"][j][1] for r in range(world))
        if j == 2:
            assert num == 0.0 and den == 0.0
            continue
        print(f"block V-cycle column {j}: rel-l2 to the scalar V-cycle {np.sqrt(num / den):.3g}")
        assert np.sqrt(num / den) <= TOL_VCYCLE, (j, np.sqrt(num / den))
    cg = _run("model", "cg", what="block")
    for r in range(world):
        assert "host-driven CG" in cg[r]["block"], (r, cg[r]["block"])
