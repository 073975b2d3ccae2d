"""The premises of tests/test_gpu_device_cg_multirank.py, checked where no GPU is needed: the host setup at 3 ranks over gloo builds,
under each environment of tests/device_cg_world.py, the three levels and the ownership that module's GPU tests are written for.  The
coarsest level must exceed the 1 024 rows of the LDS-resident solvers, or none of those tests reaches the code it is about."""
import pytest

from tests import device_cg_world as dw, solver_ref as sr


def _worker(rank, world, port, name, ret):
    import os
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    os.environ.update(dw.CONFIGS[name]["env"])
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from saena_amd import host
        L = host.load("host")
        A = host.Matrix(host.Comm("host", "dist", dist)).laplacian3D(dw.M).assemble()
        S = host.AmgSolver(A, dw.options(host, L))
        ret[rank] = ("ok", [S.level_info(l)["rows"] for l in range(S.num_levels)], dw.owners_of(S, world))
    except BaseException as e:      # noqa
        import traceback
        ret[rank] = ("".join(traceback.format_exception(type(e), e, e.__traceback__)),)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("name", list(dw.CONFIGS))
def test_rows_and_owners(name, monkeypatch):
    import torch.multiprocessing as mp
    from tests.test_host_layout import _free_port
    monkeypatch.setenv("SAENA_SETUP_THREADS", "2")
    for k in ("SAENA_SHRINK_CHAIN_US", "SAENA_SHRINK_ROWS"):      # the children inherit this environment: only the table's may hold
        monkeypatch.delenv(k, raising=False)
    port = _free_port()
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, dw.WORLD, port, name, ret)) for r in range(dw.WORLD)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(300)
        alive = [p.is_alive() for p in procs]
        for p in procs:
            if p.is_alive():
                p.terminate()
        res = dict(ret)
    assert not any(alive), f"workers still running at the time limit: {alive}"
    want = dw.CONFIGS[name]["owners"]
    for r in range(dw.WORLD):
        assert res.get(r) and res[r][0] == "ok", f"rank {r}: {res.get(r)}"
        _, rows, owners = res[r]
        print(f"{name} rank {r}: rows {rows}, owners {owners}")
        assert rows == dw.ROWS, f"{name}: the cut hierarchy has rows {rows}, tests/device_cg_world.py says {dw.ROWS}"
        assert owners == want, (f"{name}: the shrink policy gives owners {owners}, tests/device_cg_world.py says {want}: the cases of "
                                "tests/test_gpu_device_cg_multirank.py no longer reach the paths they are written for")
    assert dw.ROWS[-1] > sr.CG_MAXN
