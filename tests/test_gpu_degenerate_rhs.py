"""include/saena_gpu.h, "Degenerate right-hand sides", on the GPU: what the outer loops do with a right-hand side that gives them
nothing to iterate on -- zero, constant under null_space 1, non-finite -- and with a history buffer shorter than the solve.

The rules are stated in numpy in tests/degenerate_ref.py; tests/test_degenerate_ref.py shows on the CPU that the inputs used here reach
every branch (the centred vector of c 1 is exactly zero on neumann8 for c = 1.0 and 0.1, and d 1 with d != 0 on neumann12x8x5 for
c = pi) and that the restatement solves the perturbed constants to the four checks.  Histories are read through lib() into buffers
filled with a sentinel that is not a NaN, so that a NaN entry is seen and an entry never written is told from one that was.
Hierarchies: hierarchy.poisson_hierarchy(10, 2) (Dirichlet, sgpu_amg_create: all six entry points), neumann8 and neumann12x8x5
(null_space 1: all but FGMRES, which refuses them), neumann16cut once (the host-driven and the device coarsest CG).
"""
import ctypes as C

import numpy as np
import pytest

from tests import degenerate_ref as dg, hierarchy, null_space_ref as ns, solver_ref as sr
from tests import test_gpu_null_space as gn
from tests.test_gpu_solver_layer import Padded, bits

pytestmark = pytest.mark.gpu

SMOOTHERS = ("jacobi", "chebyshev")
SCALAR = ("solve", "solve_smoother", "solve_CG", "solve_pCG")
CAP, TAIL = 64, 4
SENT = -7.25                              # a history entry nobody wrote
OK, NOCONV = 0, -6
K = 4
_PD = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


_dirichlet = {}


def hier(name):
    if name != "dirichlet":
        return ns.hierarchy(name)
    if not _dirichlet:
        As, Ps, Rs = hierarchy.poisson_hierarchy(10, 2)
        _dirichlet.update(A=As, P=Ps, R=Rs, eig=hierarchy.eig_estimates(As), name="dirichlet")
    return _dirichlet


def kind(name):
    return None if name == "dirichlet" else "constant"


def solvers_of(name):
    return SCALAR + (("solve_FGMRES",) if name == "dirichlet" else ())


def takes_block(H, coarse):
    """the block solve refuses a hierarchy whose coarsest level needs the host-driven CG"""
    return H["A"][-1].shape[0] <= sr.CG_MAXN or coarse == "device_cg"


def raw(capi, G, solver, u, rhs, cap=CAP, want_iters=True, want_hist=True):
    """one scalar entry point through lib() -> (status, iters, the whole buffer of cap + TAIL entries, sgpu_last_error, launches)"""
    L = capi.lib()
    it = C.c_int(-99)
    hist = np.full(cap + TAIL, SENT)
    pit = C.byref(it) if want_iters else None
    ph = hist.ctypes.data_as(_PD) if want_hist else None
    l0 = capi.launch_count()
    if solver == "solve_FGMRES":
        st = L.sgpu_solve_FGMRES(G.h, u.ptr, rhs.ptr, 30, 1, pit, ph, cap, None)
    else:
        st = getattr(L, "sgpu_" + solver)(G.h, u.ptr, rhs.ptr, pit, ph, cap)
    launches = capi.launch_count() - l0
    return st, it.value, hist, L.sgpu_last_error().decode(errors="replace"), launches


def raw_block(capi, G, U, RHS, cap=CAP):
    L = capi.lib()
    it = (C.c_int * K)(*([-99] * K))
    hist = np.full(K * cap + TAIL, SENT)
    l0 = capi.launch_count()
    st = L.sgpu_solve_pCG_block(G.h, U.ptr, RHS.ptr, K, it, hist.ctypes.data_as(_PD), cap)
    launches = capi.launch_count() - l0
    assert np.all(hist[K * cap:] == SENT), "wrote behind the history buffer"
    return st, [int(v) for v in it], hist[:K * cap].reshape(K, cap), L.sgpu_last_error().decode(errors="replace"), launches


def scalar(capi, G, solver, rhs, cap=CAP):
    """a solve into a NaN-filled Padded u -> dict(st, it, hist, msg, launches, u)"""
    du, dr = Padded(capi, np.full(len(rhs), np.nan)), capi.DeviceVector(len(rhs), rhs)
    st, it, hist, msg, launches = raw(capi, G, solver, du, dr, cap)
    assert np.all(hist[cap:] == SENT), "wrote behind the history buffer"
    return dict(st=st, it=it, hist=hist[:cap], msg=msg, launches=launches, u=du.head())


def assert_rule1(r, what):
    """u = 0 (every entry +0), 0 iterations, res_hist[0] = +0.0 and nothing behind it, SGPU_OK"""
    assert r["st"] == OK and r["it"] == 0, (what, r["st"], r["it"], r["msg"])
    assert bits(r["hist"][:1])[0] == 0 and np.all(r["hist"][1:] == SENT), (what, r["hist"][:4])
    assert not np.any(bits(r["u"])), (what, "u is not +0 everywhere")


def set_max_iter(G, smoother, max_iter):
    G.set_solve_params(max_iter, ns.TOL, smoother, 3, 3)


# ---------------------------------------------------------------------------
# rule 1
ZERO_CASES = [(h, s, e) for h in ("dirichlet", "neumann8", "neumann12x8x5") for s in SMOOTHERS for e in solvers_of(h) + ("solve_pCG_block",)]
ZERO_CASES += [("neumann16cut", "jacobi", e) for e in SCALAR + ("solve_pCG_block",)]


@pytest.mark.parametrize("name,smoother,entry", ZERO_CASES)
def test_zero_rhs(capi, name, smoother, entry):
    """rhs = +0 and rhs = -0 through one entry point, under every coarsest solver the hierarchy takes, into a NaN-filled u: rule 1; the
    launch count of the call is the same at solver_max_iter 1 and 50 and below that of a one-iteration solve of rhs_for(n) (which also
    takes the first use of the operators out of the counts).
    On the parent commit: sgpu_solve and sgpu_solve_smoother return SGPU_ERR_NOCONV after solver_max_iter iterations, sgpu_solve_pCG
    and sgpu_solve_CG a NaN u; sgpu_solve_pCG_block and sgpu_solve_FGMRES pass"""
    H = hier(name)
    n = H["A"][0].shape[0]
    for coarse in gn.coarse_kinds(H):
        if entry == "solve_pCG_block" and not takes_block(H, coarse):
            continue
        G = gn.amg(capi, H, smoother, coarse, null_space=kind(name), max_iter=1)
        if entry != "solve_pCG_block":
            one = scalar(capi, G, entry, ns.rhs_for(n))
            assert one["it"] == 1 and np.isfinite(one["hist"][1]) and one["hist"][0] > 0, (entry, one["it"], one["hist"][:3])
            for zero in (np.zeros(n), np.full(n, -0.0)):
                counts = []
                for max_iter in (1, 50):
                    set_max_iter(G, smoother, max_iter)
                    r = scalar(capi, G, entry, zero)
                    assert_rule1(r, (name, smoother, coarse, entry, max_iter))
                    counts.append(r["launches"])
                print(f"{name} {smoother} {coarse} {entry}: {counts[0]} launches on a zero right-hand side, {one['launches']} for one iteration")
                assert counts[0] == counts[1] < one["launches"], (entry, counts, one["launches"])
        else:
            dU, dR = capi.BlockVector(n, K), capi.BlockVector(n, K, np.stack(sr.block_columns(n, K), axis=1))
            one = raw_block(capi, G, dU, dR)[4]
            counts = []
            for max_iter in (1, 50):
                set_max_iter(G, smoother, max_iter)
                for z in (0.0, -0.0):
                    dU, dR = capi.BlockVector(n, K, np.full((n, K), np.nan)), capi.BlockVector(n, K, np.full((n, K), z))
                    st, its, hists, msg, launches = raw_block(capi, G, dU, dR)
                    assert st == OK and its == [0] * K, (st, its, msg)
                    assert not np.any(bits(hists[:, 0])) and np.all(hists[:, 1:] == SENT)
                    assert not np.any(bits(dU.download()))
                    counts.append(launches)
            assert len(set(counts)) == 1 and counts[0] < one, (counts, one)
        G.destroy()


@pytest.mark.parametrize("name,smoother,coarse", [("dirichlet", "jacobi", "direct"), ("dirichlet", "chebyshev", "cg"), ("neumann8", "jacobi", "direct"),
                                                  ("neumann8", "chebyshev", "cg"), ("neumann12x8x5", "jacobi", "direct"),
                                                  ("neumann16cut", "jacobi", "device_cg")])
def test_a_block_column_is_its_scalar_solve(capi, name, smoother, coarse):
    """K = 4 with column 1 zero and, under null_space 1, column 2 a constant (exactly zero after centring on neumann8, dust d 1 on
    neumann12x8x5): the scalar solve of EVERY column has the block column's iters, history and u bit for bit.  One lane per row on
    both sides, as test_pcg_block_has_the_bits_of_scalar_solves"""
    H = hier(name)
    n = H["A"][0].shape[0]
    GA, GP, GR = [gn.gpu_op(capi, A) for A in H["A"]], [gn.gpu_op(capi, P, False) for P in H["P"]], [gn.gpu_op(capi, R, False) for R in H["R"]]
    for o in GA + GP + GR:
        o.set_lanes_per_row(1)
        o.set_block_lanes(1)
    G = capi.Amg(GA, GP, GR, eig_max=H["eig"], smoother=smoother, coarse_solver=coarse, max_iter=ns.MAX_ITER, tol=ns.TOL, null_space=kind(name))
    cols = sr.block_columns(n, K)
    cols[1] = np.zeros(n)
    if kind(name):
        cols[2] = dg.constant(n, np.pi if name == "neumann12x8x5" else 0.1)
    RHS = np.stack(cols, axis=1)
    dU, dR = capi.BlockVector(n, K, np.full((n, K), np.nan)), capi.BlockVector(n, K, RHS)
    st, its, hists, msg, _ = raw_block(capi, G, dU, dR)
    Ub = dU.download()
    assert st == OK, msg
    assert its[1] == 0 and (not kind(name) or its[2] == 0) and its[0] > 0 and its[3] > 0, its
    for j in range(K):
        r = scalar(capi, G, "solve_pCG", RHS[:, j])
        assert r["st"] == OK and r["it"] == its[j], (j, r["it"], its[j], r["msg"])
        assert np.array_equal(bits(r["hist"]), bits(hists[j])), j            # the unwritten entries too: the sentinel on both sides
        assert np.array_equal(bits(r["u"]), bits(Ub[:, j])), j
        if its[j] == 0:
            assert_rule1(r, (name, j))


# ---------------------------------------------------------------------------
# rule 2
@pytest.mark.parametrize("name,c,smoother", [("neumann8", 1.0, "jacobi"), ("neumann8", 0.1, "chebyshev"), ("neumann12x8x5", np.pi, "jacobi"),
                                             ("neumann12x8x5", np.pi, "chebyshev"), ("neumann16cut", 0.1, "jacobi")])
def test_constant_rhs_under_null_space(capi, name, c, smoother):
    """rhs = c 1 on a hierarchy that knows the constant null space: every solver it admits, and a block with such a column, returns
    rule 1's result with a launch count that does not depend on solver_max_iter -- where the centred vector is exactly zero (neumann8)
    and where it is d 1, d != 0 (neumann12x8x5, c = pi), which rule 1 alone does not catch"""
    H = hier(name)
    n = H["A"][0].shape[0]
    y = ns.center(dg.constant(n, c))[0]
    print(f"{name}, c = {c!r}: the centred vector is {'exactly zero' if not np.any(y) else f'd 1 with d / c = {y[0] / c:.3e}'}")
    if name == "neumann12x8x5":
        assert y[0] != 0.0
    for coarse in gn.coarse_kinds(H):
        G = gn.amg(capi, H, smoother, coarse, max_iter=1)
        for solver in SCALAR:
            counts = []
            for max_iter in (1, 1, 50):                                         # (the first call: the operators' first use, outside the counts)
                set_max_iter(G, smoother, max_iter)
                r = scalar(capi, G, solver, dg.constant(n, c))
                assert_rule1(r, (name, c, smoother, coarse, solver, max_iter))
                counts.append(r["launches"])
            assert counts[1] == counts[2], (solver, counts)
        if takes_block(H, coarse):
            set_max_iter(G, smoother, ns.MAX_ITER)
            cols = sr.block_columns(n, K)
            cols[1], cols[3] = dg.constant(n, c), dg.constant(n, -c)
            dU, dR = capi.BlockVector(n, K, np.full((n, K), np.nan)), capi.BlockVector(n, K, np.stack(cols, axis=1))
            st, its, hists, msg, _ = raw_block(capi, G, dU, dR)
            Ub = dU.download()
            assert st == OK and its[1] == 0 and its[3] == 0 and its[0] > 0 and its[2] > 0, (st, its, msg)
            for j in (1, 3):
                assert bits(hists[j][:1])[0] == 0 and np.all(hists[j][1:] == SENT) and not np.any(bits(Ub[:, j])), j
        G.destroy()


@pytest.mark.parametrize("name,c", [("neumann8", 0.1), ("neumann12x8x5", np.pi)])
def test_a_perturbed_constant_is_still_solved(capi, name, c):
    """the other side of the criterion: rhs = c + a |c| v, v the centred rhs_for(n) at unit RMS, a = 1e-3 (the value at which
    tests/test_degenerate_ref.py shows the restatement passing; the criterion sits 3.7e11 below this input's centred norm, at least
    1e6 is asserted).  sgpu_solve_pCG and sgpu_solve solve it to check_solution's four checks against ns.solve_plus"""
    H = hier(name)
    n = H["A"][0].shape[0]
    rhs = dg.perturbed(n, c)
    y, m = ns.center(rhs)
    assert np.linalg.norm(y) >= 1e6 * np.sqrt(dg.criterion(n, m))
    for solver, want in (("solve_pCG", ns.pcg(H, rhs)), ("solve", ns.stationary(H, rhs))):
        G = gn.amg(capi, H)
        r = scalar(capi, G, solver, rhs)
        assert r["st"] == OK, r["msg"]
        dg.four_checks(H, r["u"], r["hist"][:r["it"] + 1], True, rhs, want, f"{name} {solver}, c = {c!r}, a = {dg.A_PERTURB}")
        G.destroy()


# ---------------------------------------------------------------------------
# rule 3
def assert_rule3_at_start(r, solver, what):
    assert r["st"] == NOCONV and r["it"] == 0, (what, r["st"], r["it"], r["msg"])
    assert "non-finite residual at iteration 0" in r["msg"], (what, r["msg"])
    assert not np.isfinite(r["hist"][0]) and np.all(r["hist"][1:] == SENT), (what, r["hist"][:4])
    assert not np.any(bits(r["u"])), (what, "u is not zero")


@pytest.mark.parametrize("name,smoother", [("dirichlet", "jacobi"), ("dirichlet", "chebyshev"), ("neumann8", "jacobi"), ("neumann16cut", "jacobi")])
def test_nonfinite_rhs(capi, name, smoother):
    """one NaN, one -inf in the right-hand side: rule 3 at iteration 0 for every entry point, with a launch count that does not depend
    on solver_max_iter (3 and 50)"""
    H = hier(name)
    n = H["A"][0].shape[0]
    for coarse in gn.coarse_kinds(H):
        G = gn.amg(capi, H, smoother, coarse, null_space=kind(name), max_iter=3)
        for solver in solvers_of(name):
            for bad in (np.nan, -np.inf):
                rhs = ns.rhs_for(n)
                rhs[n // 3] = bad
                counts = []
                for max_iter in (3, 3, 50):                                     # (the first call: the operators' first use, outside the counts)
                    set_max_iter(G, smoother, max_iter)
                    r = scalar(capi, G, solver, rhs)
                    assert_rule3_at_start(r, solver, (name, smoother, coarse, solver, bad, max_iter))
                    counts.append(r["launches"])
                assert counts[1] == counts[2], (solver, bad, counts)
        G.destroy()


def test_breakdown_with_finite_input(capi):
    """sgpu_solve_CG on the one-level operator diag(+1 x 32, -1 x 32) with rhs = 1: ||r_0|| = 8, the first p . A p is exactly 0 and the
    dot after the first update is not finite: the solve stops there with iters = 1, whatever solver_max_iter is"""
    A = dg.indefinite_diag()
    want = dg.cg(A, np.ones(64))
    assert want["iters"] == 1 and want["stopped"] == "nonfinite"
    G = capi.Amg([gn.gpu_op(capi, A)], [], [], max_iter=3, tol=1e-8)
    counts = []
    for max_iter in (3, 3, 50):                                                 # (the first call: the operator's first use, outside the counts)
        set_max_iter(G, "jacobi", max_iter)
        r = scalar(capi, G, "solve_CG", np.ones(64))
        assert r["st"] == NOCONV and r["it"] == 1, (r["st"], r["it"], r["msg"])
        assert "non-finite residual at iteration 1" in r["msg"], r["msg"]
        assert r["hist"][0] == 8.0 and not np.isfinite(r["hist"][1]) and np.all(r["hist"][2:] == SENT), r["hist"][:4]
        counts.append(r["launches"])
    assert counts[1] == counts[2], counts


@pytest.mark.parametrize("name,smoother", [("dirichlet", "jacobi"), ("neumann8", "chebyshev")])
def test_a_poisoned_block_column(capi, name, smoother):
    """K = 4, one NaN in column 2: SGPU_ERR_NOCONV, that column has 0 iterations, a non-finite res_hist[0] and u = 0; columns 0, 1 and 3
    have the bits (u, history, count) of the same block with a clean column 2 -- a copy of column 0, so that the clean block runs as
    many iterations -- and the call launches what the clean solve launches, not the cap's worth"""
    H = hier(name)
    n = H["A"][0].shape[0]
    G = gn.amg(capi, H, smoother, "direct", null_space=kind(name), max_iter=ns.MAX_ITER)
    cols = sr.block_columns(n, K)
    cols[2] = cols[0].copy()
    clean = np.stack(cols, axis=1)
    dirty = clean.copy()
    dirty[n // 3, 2] = np.nan
    dU, dR = capi.BlockVector(n, K, np.full((n, K), np.nan)), capi.BlockVector(n, K, clean)
    raw_block(capi, G, dU, dR)                                               # (the capture: outside the counts)
    st0, its0, hists0, msg0, l0 = raw_block(capi, G, dU, dR)
    U0 = dU.download()
    assert st0 == OK and max(its0) < ns.MAX_ITER and its0[2] == its0[0], (st0, its0, msg0)
    dU.upload(np.full((n, K), np.nan)); dR.upload(dirty)
    st1, its1, hists1, msg1, l1 = raw_block(capi, G, dU, dR)
    U1 = dU.download()
    assert st1 == NOCONV and "non-finite residual at iteration 0 (column 2)" in msg1, (st1, msg1)
    assert its1[2] == 0 and not np.isfinite(hists1[2][0]) and np.all(hists1[2][1:] == SENT) and not np.any(bits(U1[:, 2]))
    for j in (0, 1, 3):
        assert its1[j] == its0[j], (j, its1, its0)
        assert np.array_equal(bits(hists1[j]), bits(hists0[j])) and np.all(np.isfinite(hists1[j][:its1[j] + 1])), j
        assert np.array_equal(bits(U1[:, j]), bits(U0[:, j])), j
    assert l1 == l0, (l1, l0)


# ---------------------------------------------------------------------------
# history capacity
@pytest.mark.parametrize("name", ["dirichlet", "neumann8"])
def test_history_capacity(capi, name):
    """hist_cap = 3 on solves of more than 3 iterations: entries 0 to 2 are those of the same solve with room for all, what lies
    behind the buffer is untouched, iters and u are unchanged; iters = NULL and res_hist = NULL are accepted"""
    H = hier(name)
    n = H["A"][0].shape[0]
    rhs = ns.rhs_for(n)
    G = gn.amg(capi, H, null_space=kind(name), max_iter=ns.MAX_ITER)
    for solver in solvers_of(name):
        full = scalar(capi, G, solver, rhs)
        assert full["it"] > 3, (solver, full["it"])
        short = scalar(capi, G, solver, rhs, cap=3)                            # (scalar() checks the TAIL entries behind cap)
        assert short["st"] == full["st"] and short["it"] == full["it"], (solver, short["it"], full["it"])
        assert np.array_equal(bits(short["hist"]), bits(full["hist"][:3])) and np.array_equal(bits(short["u"]), bits(full["u"])), solver
        du, dr = Padded(capi, np.full(n, np.nan)), capi.DeviceVector(n, rhs)
        st = raw(capi, G, solver, du, dr, cap=0, want_iters=False, want_hist=False)[0]
        assert st == full["st"] and np.array_equal(bits(du.head()), bits(full["u"])), solver
    RHS = np.stack(sr.block_columns(n, K), axis=1)
    dU, dR = capi.BlockVector(n, K, np.full((n, K), np.nan)), capi.BlockVector(n, K, RHS)
    st0, its0, hists0, _, _ = raw_block(capi, G, dU, dR)
    U0 = dU.download()
    assert st0 == OK and min(its0) > 3, its0
    st1, its1, hists1, _, _ = raw_block(capi, G, dU, dR, cap=3)                # (raw_block checks the entries behind K * cap)
    assert st1 == OK and its1 == its0 and np.array_equal(bits(hists1), bits(hists0[:, :3])) and np.array_equal(bits(dU.download()), bits(U0))
    assert capi.lib().sgpu_solve_pCG_block(G.h, dU.ptr, dR.ptr, K, None, None, 0) == OK
    assert np.array_equal(bits(dU.download()), bits(U0))


# ---------------------------------------------------------------------------
# the host layer
def test_host_layer_on_a_zero_rhs(capi):
    """host.AmgSolver.solve_pCG on laplacian3D(8) with rhs = 0: converged, 0 iterations, u == 0"""
    from saena_amd import host
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(8).assemble()
    S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
    n = A.num_local_rows
    u, it, hist, ok = S.solve_pCG(np.zeros(n))
    assert ok and it == 0 and not np.any(u) and list(hist) == [0.0]
    u, it, hist, ok = S.solve(np.zeros(n))
    assert ok and it == 0 and not np.any(u) and list(hist) == [0.0]


# ---------------------------------------------------------------------------
# across ranks
def _worker(rank, world, port, ret):
    import os
    import sys
    import torch.distributed as dist                      # torch first (its HIP runtime), like bench.py --gpus N
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from tests.test_gpu_vcycle import POLICIES
    os.environ.update(POLICIES["rows4096"])
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        from saena_amd import capi as c, host
        c.init_host_transport(0, dist)
        L = host.load("gpu")
        A = host.Matrix(host.Comm("gpu", "dist", dist)).laplacian3D(32).assemble()
        S = host.AmgSolver(A, host.options(L, **host.OPTIONS001)).to_device()
        n = A.num_local_rows
        b0 = A.laplacian3D_rhs()
        bad = b0.copy()
        if rank == 1:
            bad[n // 2] = np.nan                          # the only NaN of the whole right-hand side lies in rank 1's rows
        G = type("G", (), {"h": S.device_handle()})()
        out = {}
        for what, rhs in (("zero", np.zeros(n)), ("nan", bad)):
            du, dr = c.DeviceVector(n, np.full(n, np.nan)), c.DeviceVector(n, rhs)
            st, it, hist, msg, _ = raw(c, G, "solve_pCG", du, dr)
            u = du.download()
            out[what] = (st, it, [int(v) for v in bits(hist)], msg, bool(np.any(bits(u))) if n else False)
            cols = np.stack([b0, 0.5 * b0 + 3.0, rhs, b0], axis=1)
            dU, dR = c.BlockVector(n, K, np.full((n, K), np.nan)), c.BlockVector(n, K, cols)
            st, its, hists, msg, _ = raw_block(c, G, dU, dR)
            U = dU.download()
            out[what + "_block"] = (st, its, [int(v) for v in bits(hists.ravel())], msg, bool(np.any(bits(U[:, 2]))) if n else False)
        ret[rank] = ("ok", out)
    except BaseException as e:      # noqa
        import traceback
        ret[rank] = ("".join(traceback.format_exception(type(e), e, e.__traceback__)),)
    finally:
        dist.destroy_process_group()


def test_across_ranks(capi):
    """three host-transport ranks on Poisson 32^3 (the size tests/test_gpu_block_multirank.py builds its row-distributed hierarchy at):
    sgpu_solve_pCG and sgpu_solve_pCG_block on a zero right-hand side (column 2 of the block), then on one whose only NaN lies in rank
    1's rows.  The decision is taken on the rank-summed dot: every rank returns the same status, iters and history bits, rule 1
    resp. rule 3 at iteration 0, and no rank is still running at the join"""
    import multiprocessing as mp      # not torch's: this process already runs the system HIP runtime
    import socket
    world = 3
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, world, port, ret)) for r in range(world)]
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
    out = res[0][1]
    for r in range(1, world):
        for key in out:
            assert res[r][1][key][:3] == out[key][:3], f"rank {r} and rank 0 differ on {key}: {res[r][1][key][:2]}, {out[key][:2]}"
    sent = int(bits([SENT])[0])
    for r in range(world):
        o = res[r][1]
        st, it, hist, msg, u_any = o["zero"]
        assert st == OK and it == 0 and hist[0] == 0 and all(h == sent for h in hist[1:]) and not u_any, (r, st, it, msg)
        st, it, hist, msg, u_any = o["nan"]
        assert st == NOCONV and it == 0 and "non-finite residual at iteration 0" in msg and not u_any, (r, st, it, msg)
        h = np.array(hist, np.uint64).view(np.float64)
        assert not np.isfinite(h[0]) and all(v == sent for v in hist[1:CAP]), (r, h[:3])
        st, its, hists, msg, u_any = o["zero_block"]
        hb = np.array(hists, np.uint64).view(np.float64).reshape(K, CAP)
        assert st == OK and its[2] == 0 and min(its[0], its[1], its[3]) > 0 and hists[2 * CAP] == 0 and not u_any, (r, st, its, msg)
        assert np.all(hb[2][1:] == SENT)
        st, its, hists, msg, u_any = o["nan_block"]
        hb = np.array(hists, np.uint64).view(np.float64).reshape(K, CAP)
        assert st == NOCONV and its[2] == 0 and "non-finite residual at iteration 0 (column 2)" in msg and not u_any, (r, st, its, msg)
        assert not np.isfinite(hb[2][0]) and np.all(hb[2][1:] == SENT)
        for j in (0, 1, 3):                                                     # the other columns went on to their own thresholds
            assert its[j] == o["zero_block"][1][j] and np.all(np.isfinite(hb[j][:its[j] + 1])), (r, j, its)
