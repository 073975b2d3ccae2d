"""update1 / update2 on the device: sgpu_amg_set_operator and the device half of saena_amg_update.

What is held, every comparison bit for bit unless a bound is named:
  * an operator made again from the same descriptor and installed with sgpu_amg_set_operator changes no result, and the first call
    after it captures again (it launches more than the one graph launch of a replay);
  * after saena_amg_update(A', 2) on a hierarchy that is on the device, and after the same update driven from here through
    sgpu_amg_set_operator, V-cycle and pCG history are those of a second device hierarchy built by hand from the updated host levels
    (level_layout -> sgpu_op_create -> sgpu_amg_create) -- both smoothers, both coarsest solvers; the refreshed dense inverse solves
    the NEW coarsest operator within tests/solver_ref.py's bound for the direct solve;
  * the same through a hierarchy whose coarsest level takes the device-resident CG (coarse_solver = "device_cg", 5 324 rows): the
    kept work space, a V-cycle captured again, the coarsest-CG contract on the new coarsest operator;
  * no captured graph survives an update: scalar V-cycle, block V-cycle, FGMRES and LOBPCG, each captured before the update, give the
    hand-built hierarchy's results after it -- compared while the old operators are still alive, so that a stale graph is a failed
    comparison and not a read of freed memory -- and the same again once the old operators are destroyed;
  * P and R keep their device handles through saena_amg_update, the refreshed A get new ones;
  * a singular coarsest operator and every malformed call are refused and change nothing;
  * the products of an update on the device kernel build the levels the host kernel builds.

Both sides of a comparison hold every operator in the same form -- pinned (variant 0, one lane per row) where this file makes the
operators, the form sgpu_op_create gives (SAENA_NO_AUTOTUNE) where saena_amg_update makes them: the plan-time autotune picks by
timing, and two operators of the same entries may then sum their rows in different orders.

Cases: Poisson 12^3 and 16^3 cut at three coarsening steps (four levels: 1000 / 2744 rows down to 18 / 42), wgrid16 of
tests/setup_cases.py (irregular, five levels).  A' is update_ref.variant(A, "shift") unless said otherwise."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import setup_cases, setup_ref, update_ref
from tests import solver_ref as sr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def host():
    from saena_amd import host as h
    return h


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(a, b, what):
    assert np.array_equal(bits(a), bits(b)), f"{what}: {int((bits(a) != bits(b)).sum())} of {np.size(a)} values differ"


def solver_on(host, name, smoother, **kw):
    """-> (A, AmgSolver) on the GPU library's host code (products below the setup's threshold: on the host kernel)"""
    L = host.load("gpu")
    if name.startswith("poisson"):
        A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(int(name[7:])).assemble()
        o = dict(host.OPTIONS001, dynamic_levels=0, max_level=3, smoother=smoother, **kw)
    else:
        A = setup_cases.assemble(name, which="gpu", kind="rccl")
        o = setup_cases.options(name, smoother=smoother, **kw)
    return A, host.AmgSolver(A, host.options(L, **o))


def pin(op):
    op.set_variant(0)
    op.set_lanes_per_row(1)
    return op


def level_ops(capi, S, levels=None):
    """pinned device operators A[l] (for `levels`, default all) made from the host levels of S"""
    return [pin(capi.Operator(**S.level_layout(l, 0))) for l in (range(S.num_levels) if levels is None else levels)]


def hand_built(capi, S, smoother, coarse_solver, max_iter=50, pinned=True):
    n = S.num_levels
    form = pin if pinned else (lambda op: op)               # (not pinned: the form sgpu_op_create gives every operator, no autotune)
    GA = [form(capi.Operator(**S.level_layout(l, 0))) for l in range(n)]
    GP = [form(capi.Operator(**S.level_layout(l, 1))) for l in range(n - 1)]
    GR = [form(capi.Operator(**S.level_layout(l, 2))) for l in range(n - 1)]
    eig = [S.level_info(l)["eig_max"] for l in range(n)]
    G = capi.Amg(GA, GP, GR, eig_max=eig, pre=3, post=3, smoother=smoother, max_iter=max_iter, tol=1e-8, coarse_solver=coarse_solver)
    return G, GA, GP, GR


def device_view(capi, S):
    """the device hierarchy of an AmgSolver behind capi.Amg's methods (owned by the solver).  No operator is touched: setting a form
    would by itself make every captured graph stale, which is the update's job here"""
    G = capi.Amg.__new__(capi.Amg)
    G.h = C.c_void_p(S.device_handle())
    G.destroy = lambda: None
    n = S.num_levels
    G.A = [S.device_op(l, 0) for l in range(n)]
    G.P = [S.device_op(l, 1) for l in range(n - 1)]
    G.R = [S.device_op(l, 2) for l in range(n - 1)]
    return G


def run_scalar(capi, G, rhs):
    """-> (V-cycle output from a fixed iterate, pCG solution, pCG history, iterations)"""
    n = len(rhs)
    du, dr = capi.DeviceVector(n, np.cos(0.11 * np.arange(n))), capi.DeviceVector(n, rhs)
    G.vcycle(du, dr)
    v = du.download()
    it, hist, conv = G.solve_pCG(du, dr)
    assert conv, hist
    return v, du.download(), hist, it


def rhs_of(n):
    return np.sin(0.37 * np.arange(n) + 0.1) + 0.05


# ---- an operator of the same descriptor ---------------------------------------------------------------------------------
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_set_operator_with_the_same_entries_changes_nothing_and_recaptures(capi, host, smoother):
    A, S = solver_on(host, "poisson12", smoother)
    G, GA, GP, GR = hand_built(capi, S, smoother, "direct")
    n = GA[0].M
    du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, rhs_of(n))
    G.vcycle(du, dr)                                        # captured
    first = du.download()
    du.upload(np.zeros(n))
    l0 = capi.launch_count(); G.vcycle(du, dr); replay = capi.launch_count() - l0
    assert replay == 1
    same(du.download(), first, "replay")
    it0, hist0, conv0 = G.solve_pCG(capi.DeviceVector(n), dr)
    eig = [S.level_info(l)["eig_max"] for l in range(S.num_levels)]
    for l, op in enumerate(level_ops(capi, S)):             # every level in turn, the coarsest (its dense inverse) included
        old = G.set_operator(l, op, eig[l])
        du.upload(np.zeros(n))
        l0 = capi.launch_count(); G.vcycle(du, dr); after = capi.launch_count() - l0
        assert after > replay, f"level {l}: the first V-cycle after the swap launched {after} times: it replayed a graph"
        same(du.download(), first, f"V-cycle after set_operator({l})")
        old.destroy()
        du.upload(np.zeros(n))
        l0 = capi.launch_count(); G.vcycle(du, dr)
        assert capi.launch_count() - l0 == 1
        same(du.download(), first, f"replay after set_operator({l})")
    it1, hist1, conv1 = G.solve_pCG(capi.DeviceVector(n), dr)
    assert (it1, conv1) == (it0, conv0)
    same(hist1, hist0, "pCG history")


# ---- updated against hand-built -----------------------------------------------------------------------------------------
def check_coarsest(capi, G, S, direct):
    l = S.num_levels - 1
    Ac = setup_ref.from_layout(S.level_layout(l, 0))
    n = Ac.nrows
    D = np.zeros((n, n))
    D[setup_ref.rows_of(Ac), Ac.col] = Ac.val
    rhs = rhs_of(n)
    x, res = sr.solve_hp(D, rhs)
    assert res <= 1e-15
    # (the direct solve ignores the iterate; the CG is the V-cycle's, which starts every coarse level from zero)
    du, dr = capi.DeviceVector(n, np.ones(n) if direct else np.zeros(n)), capi.DeviceVector(n, rhs)
    G.coarsest_solve(du, dr)
    cond = float(np.linalg.cond(D))
    err = sr.rel(du.download(), x)
    bound = sr.direct_bound(n, cond) if direct else 2 * cond * sr.CG_TOL      # the two contracts of tests/test_gpu_solver_layer.py
    print(f"coarsest level: {n} rows, cond {cond:.3g}, error {err:.3g} of {bound:.3g}")
    assert err <= bound


@pytest.mark.parametrize("name", ["poisson16", "wgrid16"])
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_saena_amg_update_on_the_device_equals_a_hand_built_hierarchy(capi, host, name, smoother, monkeypatch):
    """coarsest solver: direct (what saena_amg_to_device builds).  SAENA_NO_AUTOTUNE: both sides keep the form sgpu_op_create gives an
    operator, a function of its entries alone -- checked level by level below"""
    monkeypatch.setenv("SAENA_NO_AUTOTUNE", "1")
    A, S = solver_on(host, name, smoother)
    S.to_device()
    n = A.num_local_rows
    rhs = rhs_of(n)
    before = run_scalar(capi, device_view(capi, S), rhs)    # also: graphs captured before the update
    A2 = update_ref.matrix_from(*update_ref.variant(A, "shift"), which="gpu", kind="rccl")
    S.update(A2, 2)
    G = device_view(capi, S)
    G2, *_keep = hand_built(capi, S, smoother, "direct", pinned=False)
    for mine, theirs in zip(G.A + G.P + G.R, G2.A + G2.P + G2.R):
        assert (mine.variant(), mine.info()["lanes_per_row"]) == (theirs.variant(), theirs.info()["lanes_per_row"])
    got, want = run_scalar(capi, G, rhs), run_scalar(capi, G2, rhs)
    for a, b, what in zip(got, want, ("V-cycle", "pCG solution", "pCG history")):
        same(a, b, f"{name} {smoother}: {what}")
    assert got[3] == want[3]
    assert not np.array_equal(got[0], before[0]), "the update changed nothing"
    check_coarsest(capi, G, S, direct=True)
    u, it, hist, conv = S.solve_pCG(rhs)                    # and through the solver's own entry point
    assert conv and it == want[3]
    same(hist, want[2], "saena_amg_solve_pCG history")


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("mode", [1, 2])
def test_an_update_through_set_operator_with_the_cg_coarsest_solver(capi, host, smoother, mode):
    """the host hierarchy updated on the host, its refreshed levels installed from here: coarse_solver = 0"""
    A, S = solver_on(host, "poisson12", smoother)
    G, GA, GP, GR = hand_built(capi, S, smoother, "CG")
    n = GA[0].M
    rhs = rhs_of(n)
    before = run_scalar(capi, G, rhs)
    S.update(update_ref.matrix_from(*update_ref.variant(A, "perturb"), which="gpu", kind="rccl"), mode)
    levels = [0] if mode == 1 else list(range(S.num_levels))
    for l, op in zip(levels, level_ops(capi, S, levels)):
        G.set_operator(l, op, S.level_info(l)["eig_max"]).destroy()
    G2, *_keep = hand_built(capi, S, smoother, "CG")
    got, want = run_scalar(capi, G, rhs), run_scalar(capi, G2, rhs)
    for a, b, what in zip(got, want, ("V-cycle", "pCG solution", "pCG history")):
        same(a, b, f"mode {mode} {smoother}: {what}")
    assert got[3] == want[3] and not np.array_equal(got[0], before[0])
    check_coarsest(capi, G, S, direct=False)


@pytest.mark.parametrize("mode", [1, 2])
def test_saena_amg_update_under_the_device_cg(capi, host, mode, monkeypatch):
    """coarse_solver = "device_cg" through saena_amg_update: Poisson 24^3 cut at max_level = 1, 5 324 coarse rows.  The update keeps
    the device CG's work space, drops the captured V-cycles and captures again over the new coarsest operator.  Held: V-cycle, pCG
    solution, history and count are those of a hand-built hierarchy over the refreshed levels under "device_cg", bit for bit (the
    standard of the test above; SAENA_NO_AUTOTUNE for the same reason); they differ from the ones before the update; the second
    V-cycle after the update is one launch; sgpu_coarsest_solve on the updated handle meets the four contracts of
    tests/device_cg_ref.py on the coarsest operator the host now holds.  (update_ref.variant(A, "perturb") of this operator has one
    negative eigenvalue, and so has its Galerkin product under mode 2: the condition number of the contracts is
    max |lambda| / min |lambda|, and the numpy CG -- the oracle here -- converges on it as the kernels must.)"""
    import scipy.sparse as sp
    from tests import device_cg_ref as dr
    from tests.test_gpu_solver_layer import Padded
    monkeypatch.setenv("SAENA_NO_AUTOTUNE", "1")
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(24).assemble()
    S = host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, dynamic_levels=0, max_level=1)), coarse_solver="device_cg").to_device()
    assert S.num_levels == 2 and S.level_info(1)["rows"] == 5324 > sr.CG_MAXN
    n = A.num_local_rows
    rhs = rhs_of(n)
    G = device_view(capi, S)
    before = run_scalar(capi, G, rhs)                       # one V-cycle, one pCG solve: their graphs are captured
    du, drhs = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, rhs)
    G.vcycle(du, drhs)
    l0 = capi.launch_count(); G.vcycle(du, drhs); replay = capi.launch_count() - l0
    assert replay == 1
    S.update(update_ref.matrix_from(*update_ref.variant(A, "perturb"), which="gpu", kind="rccl"), mode)
    G = device_view(capi, S)
    # recaptured: the first V-cycle on the vectors of the old graph launches the whole sequence, the second is one launch
    du.upload(np.zeros(n))
    l0 = capi.launch_count(); G.vcycle(du, drhs); first = capi.launch_count() - l0
    v1 = du.download()
    du.upload(np.zeros(n))
    l0 = capi.launch_count(); G.vcycle(du, drhs); second = capi.launch_count() - l0
    print(f"mode {mode}: first V-cycle after the update {first} launches, second {second}")
    assert first > dr.launches(sr.CG_MAX_ITER), f"the first V-cycle after the update launched {first} times: it replayed a graph"
    assert second == 1
    same(du.download(), v1, f"mode {mode}: replay of the recaptured V-cycle")
    G2, *_keep = hand_built(capi, S, "jacobi", "device_cg", pinned=False)
    for mine, theirs in zip(G.A + G.P + G.R, G2.A + G2.P + G2.R):
        assert (mine.variant(), mine.info()["lanes_per_row"]) == (theirs.variant(), theirs.info()["lanes_per_row"])
    got, want = run_scalar(capi, G, rhs), run_scalar(capi, G2, rhs)
    for a, b, what in zip(got, want, ("V-cycle", "pCG solution", "pCG history")):
        same(a, b, f"mode {mode}: {what}")
    print(f"mode {mode}: {got[3]} iterations (hand-built {want[3]}, before the update {before[3]})")
    assert got[3] == want[3]
    for a, b, what in zip(got, before, ("V-cycle", "pCG solution", "pCG history")):
        assert not np.array_equal(a, b), f"mode {mode}: the update did not change the {what}"
    # the coarsest solve of the updated handle, on the coarsest operator the host holds now, stored order kept
    d = S.level_layout(1, 0)
    nc = d["M"]
    Ac = sp.csr_matrix((d["val_local"], d["col_local"], np.concatenate([[0], np.cumsum(d["nnzPerRow_local"])])), shape=(nc, nc))
    c = dr.sparse_case(Ac, sr.rhs_for(nc))
    assert c["resid"] <= 1e-15
    u_o, it_o = sr.coarsest_cg(Ac, c["rhs"])
    dcu, dcr = Padded(capi, np.zeros(nc)), capi.DeviceVector(nc, c["rhs"])
    l0 = capi.launch_count(); it = G.coarsest_solve(dcu, dcr); launches = capi.launch_count() - l0
    print(f"mode {mode}: coarsest operator cond {c['cond']:.4g}, eigenvalues {c['eig_ends']}, {launches} launches")
    dr.check_contracts(c, dcu.head(), it, u_o, it_o)
    assert launches == dr.launches(sr.CG_MAX_ITER)


# ---- stale graphs -------------------------------------------------------------------------------------------------------
class FourWays:
    """scalar V-cycle, block V-cycle at K = 2, FGMRES and LOBPCG on ONE set of device vectors: a captured graph is found again by its
    (u, rhs) pointers, so the second run on the same vectors replays whatever graph is still there"""

    def __init__(self, capi, n):
        self.capi, self.n = capi, n
        i = np.arange(n)
        self.u0, self.rhs = np.cos(0.11 * i), rhs_of(n)
        self.U0 = np.stack([np.cos(0.07 * i), np.sin(0.05 * i + 1.0)], axis=1)
        self.RHS = np.stack([self.rhs, np.cos(0.21 * i) + 0.3], axis=1)
        self.X0 = np.stack([np.sin(0.013 * i + 0.3), np.cos(0.029 * i)], axis=1) + 0.5
        self.du, self.dr = capi.DeviceVector(n), capi.DeviceVector(n, self.rhs)
        self.dg = capi.DeviceVector(n)
        self.DU, self.DR = capi.BlockVector(n, 2), capi.BlockVector(n, 2, self.RHS)
        self.DX = capi.BlockVector(n, 2)

    def run(self, G):
        out = {}
        self.du.upload(self.u0)
        G.vcycle(self.du, self.dr)
        out["vcycle"] = self.du.download()
        self.DU.upload(self.U0)
        G.vcycle_block(self.DU, self.DR)
        out["vcycle_block"] = self.DU.download()
        G.set_solve_params(6, 1e-14, G._smoother, 3, 3)     # six iterations of each solver, no convergence asked
        it, hist, _, _ = G.solve_fgmres(self.dg, self.dr, restart=4)
        out["fgmres"], out["fgmres_hist"] = self.dg.download(), hist
        self.DX.upload(self.X0)
        lam, res, it, _, _ = G.lobpcg(self.DX, 1, max_iter=6, tol=1e-14)
        out["lobpcg"], out["lobpcg_lambda"] = self.DX.download(), lam
        return out


def assert_same_runs(got, want, what):
    for k in want:
        same(got[k], want[k], f"{what}: {k}")


@pytest.mark.parametrize("smoother", ["chebyshev", "jacobi"])
def test_no_captured_graph_survives_an_update(capi, host, smoother):
    A, S = solver_on(host, "poisson12", smoother)
    G, GA, GP, GR = hand_built(capi, S, smoother, "direct")
    G._smoother = smoother
    n = GA[0].M
    ways = FourWays(capi, n)
    old_runs = ways.run(G)                                  # 1. every one of the four has captured its graph
    assert_same_runs(ways.run(G), old_runs, "replay before the update")
    S.update(update_ref.matrix_from(*update_ref.variant(A, "shift"), which="gpu", kind="rccl"), 2)
    G2, *_keep = hand_built(capi, S, smoother, "direct")
    G2._smoother = smoother
    want = FourWays(capi, n).run(G2)
    assert any(not np.array_equal(want[k], old_runs[k]) for k in ("vcycle", "vcycle_block", "fgmres", "lobpcg"))
    old = [G.set_operator(l, op, S.level_info(l)["eig_max"]) for l, op in enumerate(level_ops(capi, S))]     # 2. the old operators stay alive
    assert_same_runs(ways.run(G), want, "after the update, old operators alive")                             # 3.
    for op in old:                                          # 4.
        op.destroy()
    assert_same_runs(ways.run(G), want, "after the old operators are destroyed")


# ---- handles ------------------------------------------------------------------------------------------------------------
def test_p_and_r_keep_their_handles_and_a_gets_new_ones(capi, host, monkeypatch):
    monkeypatch.setenv("SAENA_NO_AUTOTUNE", "1")
    A, S = solver_on(host, "poisson12", "chebyshev")
    S.to_device()
    L = host.load("gpu")
    n = S.num_levels

    def handles():
        return {(l, w): L.saena_amg_device_op(S.h, l, w) for l in range(n) for w in (0, 1, 2) if w == 0 or l < n - 1}
    h0, amg0 = handles(), S.device_handle()
    keepA = A
    A1 = update_ref.matrix_from(*update_ref.variant(A, "shift"), which="gpu", kind="rccl")
    S.update(A1, 1)
    h1 = handles()
    assert S.device_handle() == amg0
    assert h1[(0, 0)] != h0[(0, 0)]
    assert {k: v for k, v in h1.items() if k != (0, 0)} == {k: v for k, v in h0.items() if k != (0, 0)}
    A2 = update_ref.matrix_from(*update_ref.variant(keepA, "perturb"), which="gpu", kind="rccl")
    S.update(A2, 2)
    h2 = handles()
    assert S.device_handle() == amg0
    for (l, w), v in h2.items():
        assert v and ((v == h1[(l, w)]) == (w != 0)), (l, w)
    u, it, hist, conv = S.solve_pCG(rhs_of(A.num_local_rows))
    assert conv


# ---- refusals -----------------------------------------------------------------------------------------------------------
def test_a_singular_coarsest_operator_is_refused_and_the_old_hierarchy_solves_as_before(capi, host):
    A, S = solver_on(host, "poisson12", "chebyshev")
    G, GA, GP, GR = hand_built(capi, S, "chebyshev", "direct")
    n = GA[0].M
    rhs = rhs_of(n)
    before = run_scalar(capi, G, rhs)
    l = S.num_levels - 1
    d = S.level_layout(l, 0)
    r = np.repeat(np.arange(d["M"]), d["nnzPerRow_local"])
    d["val_local"] = np.where((r == 0) | (d["col_local"] == 0), 0.0, d["val_local"])       # row 0 and column 0 are zero
    bad = pin(capi.Operator(**d))
    nc = d["M"]
    dcu, dcr = capi.DeviceVector(nc), capi.DeviceVector(nc, rhs_of(nc))
    G.coarsest_solve(dcu, dcr)
    coarse_before = dcu.download()
    with pytest.raises(capi.SgpuError, match="singular"):
        G.set_operator(l, bad, 0.0)
    assert G.A[l] is GA[l]
    after = run_scalar(capi, G, rhs)
    for a, b, what in zip(after, before, ("V-cycle", "pCG solution", "pCG history")):
        same(a, b, f"after the refusal: {what}")
    G.coarsest_solve(dcu, dcr)
    same(dcu.download(), coarse_before, "coarsest solve after the refusal")


def test_set_operator_refuses_malformed_calls(capi, host):
    A, S = solver_on(host, "poisson12", "chebyshev")
    G, GA, GP, GR = hand_built(capi, S, "chebyshev", "direct")
    n = GA[0].M
    rhs = rhs_of(n)
    before = run_scalar(capi, G, rhs)
    ops = level_ops(capi, S)
    eig = [S.level_info(l)["eig_max"] for l in range(S.num_levels)]
    d = S.level_layout(1, 0)
    d["inv_diag"] = None
    bare = pin(capi.Operator(**d))
    for level, op, e, msg in ((-1, ops[0], eig[0], "level"), (S.num_levels, ops[0], eig[0], "level"), (1, ops[2], eig[1], "rows"),
                              (0, ops[1], eig[0], "rows"), (1, bare, eig[1], "inv_diag"), (1, ops[1], 0.0, "eig_max"), (0, ops[0], -1.0, "eig_max")):
        with pytest.raises(capi.SgpuError, match=msg):
            G.set_operator(level, op, e)
    assert all(a is b for a, b in zip(G.A, GA))
    after = run_scalar(capi, G, rhs)
    for a, b, what in zip(after, before, ("V-cycle", "pCG solution", "pCG history")):
        same(a, b, f"after the refusals: {what}")
    G.set_solve_params(50, 1e-8, "jacobi", 3, 3)            # under Jacobi eig_max is not read: 0 is accepted
    G.set_operator(1, ops[1], 0.0).destroy()


# ---- the products of an update on the device --------------------------------------------------------------------------------
WORKER = r"""
import sys, json
sys.path.insert(0, %(root)r)
from saena_amd import capi, host
from tests import setup_cases, update_ref
capi.init(0)
L = host.load("gpu")
A, S = setup_cases.solver("wgrid16", which="gpu", kind="rccl", smoother="chebyshev")
out = {}
for kind in ("shift", "pattern"):
    B = update_ref.matrix_from(*update_ref.variant(A, kind), which="gpu", kind="rccl")
    host.spgemm_stats_reset(L)
    S.update(B, 2)
    out[kind] = update_ref.state(S)
    out[kind + " stats"] = host.spgemm_stats(L, total=True)
print("RESULT " + json.dumps(out))
"""


def _child(host_spgemm):
    env = dict(os.environ, SAENA_SPGEMM_HOOK_MIN="1")
    env.pop("SAENA_HOST_SPGEMM", None)
    if host_spgemm:
        env["SAENA_HOST_SPGEMM"] = "1"
    out = subprocess.run([sys.executable, "-c", WORKER % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    return json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])


def test_the_device_products_update_to_the_host_s_levels():
    """SAENA_SPGEMM_HOOK_MIN=1 (read once per process: two children): every product of the update on the device kernel, against the
    same update with the host kernel"""
    gpu = _child(False)                                     # (a child that fails ends the test: nothing runs after it)
    ref = _child(True)
    for kind in ("shift", "pattern"):
        sg, sh = gpu.pop(kind + " stats"), ref.pop(kind + " stats")
        assert sg["on_device"] > 0 and sg["declined"] == 0, sg
        assert sh["on_device"] == 0 and sh["host_hash"] + sh["host_dense"] > 0, sh
        assert gpu[kind] == ref[kind], [k for k in gpu[kind] if gpu[kind][k] != ref[kind].get(k)]
