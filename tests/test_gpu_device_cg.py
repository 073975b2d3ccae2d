"""The device-resident coarsest CG (sgpu_amg_params.coarse_solver = 2, capi.Amg(coarse_solver="device_cg")) on the GPU, held to the
coarsest-CG contract of tests/test_gpu_solver_layer.py and to what the flag promises: a coarsest level past 1 024 rows no longer sends
the solve phase to the host, so the V-cycle is one captured graph and the block, FGMRES and LOBPCG solves take the hierarchy.

Cases, the numpy restatement and the restated bounds come from tests/device_cg_ref.py; tests/test_device_cg_ref.py shows on the CPU that
the restatement stays inside every bound asserted here.  Shapes are the smallest at which the kernels can go wrong: 1 025 rows (the
first size on the new path, a last workgroup that is not full) with 3, 17, 49 and 1 025 entries in a row (1, 4 and 16 lanes per row),
1 100 dense rows (a wave per row), 262 401 rows (the partial sums' second grid-stride trip).  Caps: 150, 6, and 1, 2, 3, 7 -- the
setup kernel's own branch, the cap rule at its first iteration, odd caps; sgpu_amg_create refuses no cap.
"""
import numpy as np
import pytest

from tests import device_cg_ref as dr, eig_ref as er, gmres_ref as gr, hierarchy, inputs, solver_ref as sr, util
from tests.test_gpu_gmres import check_against
from tests.test_gpu_solver_layer import Padded, bits, one_level
from tests.test_gpu_vcycle import TOL_HIST, build

pytestmark = pytest.mark.gpu

IDS = lambda c: f"{c[0]}{c[1]}"      # noqa: E731
FULL = dr.launches(sr.CG_MAX_ITER)   # 449 launches at the default cap of 150


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def two_level():
    return sr.tri_two_level(*dr.TWO_LEVEL)


def coarsest(capi, G, n, u0, rhs):
    """-> (u, iterations, launches) of one sgpu_coarsest_solve; nothing may be written behind u"""
    du, drhs = Padded(capi, u0), capi.DeviceVector(n, rhs)
    l0 = capi.launch_count()
    it = G.coarsest_solve(du, drhs)
    return du.head(), it, capi.launch_count() - l0


# ---------------------------------------------------------------------------
# the contract, on one-level hierarchies
@pytest.mark.parametrize("case", dr.CONTRACT_CASES + dr.EXTRA_CASES, ids=IDS)
def test_the_four_contracts(capi, case):
    c = dr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], "device_cg")
    u_o, it_o = O.coarsest_cg(c["rhs"])
    u, it, launches = coarsest(capi, G, n, np.zeros(n), c["rhs"])
    dr.check_contracts(c, u, it, u_o, it_o)
    assert launches == FULL                                    # the fixed sequence, whatever the data
    u2, it2, _ = coarsest(capi, G, n, np.zeros(n), c["rhs"])   # no atomics: the same bits
    assert it2 == it and np.array_equal(bits(u2), bits(u))
    # it starts from the iterate it is given: the recurrence adds its updates to u
    u3, it3, _ = coarsest(capi, G, n, np.ones(n), c["rhs"])
    assert it3 == it and sr.rel(u3 - 1.0, u) <= 1e-13


def test_the_partial_sums_second_trip(capi):
    """262 401 rows: 1 024 workgroups of 256 take the rows in two trips.  Too large for solver_ref.case: against coarsest_cg and the
    high-precision residual only"""
    n = dr.BIG_TRI
    A, rhs = sr.tri(n), sr.rhs_for(n)
    _, G, _ = one_level(capi, A, "device_cg")
    u_o, it_o = sr.coarsest_cg(A, rhs)
    u, it, _ = coarsest(capi, G, n, np.zeros(n), rhs)
    res = sr.residual_hp(A, u, rhs) / np.linalg.norm(rhs)
    print(f"it {it} (coarsest_cg {it_o}), rel {sr.rel(u, u_o):.2e}, residual {res:.2e}")
    assert abs(it - it_o) <= dr.IT_SLACK
    assert sr.rel(u, u_o) <= dr.REL_ORACLE
    assert res <= dr.RESID_FACTOR * sr.CG_TOL


@pytest.mark.parametrize("case", dr.EARLY_OUT_CASES, ids=IDS)
def test_early_outs(capi, case):
    """rhs = 0, and ||rhs|| = 1e-13 so that rhs . rhs < tol^2: no update, u keeps its bits (a -0.0 included), the oracle's count"""
    c = dr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], "device_cg")
    u0 = inputs.v2(n)
    u0[0] = -0.0
    tiny = c["rhs"] * (1e-13 / np.linalg.norm(c["rhs"]))
    for rhs in (np.zeros(n), tiny):
        _, it_o = O.coarsest_cg(rhs)
        u, it, launches = coarsest(capi, G, n, u0, rhs)
        assert it == it_o and launches == FULL
        assert np.array_equal(bits(u), bits(u0))
    # and the flags of an early out do not outlive it: the next solve on the same handle runs
    u, it, _ = coarsest(capi, G, n, np.zeros(n), c["rhs"])
    u_o, it_o = O.coarsest_cg(c["rhs"])
    dr.check_contracts(c, u, it, u_o, it_o)


@pytest.mark.parametrize("case", dr.CAPPED_CASES, ids=IDS)
def test_the_cap(capi, case):
    """CG_coarsest_max_iter = 6: five updates on both sides, the same unconverged iterate, 2 + 3 * 5 launches"""
    c = dr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], "device_cg", cg_max_iter=dr.CAP)
    u_o, it_o = O.coarsest_cg(c["rhs"])
    u, it, launches = coarsest(capi, G, n, np.zeros(n), c["rhs"])
    assert it == 5 and it_o == 5 and launches == dr.launches(dr.CAP) == 17
    assert sr.rel(u, u_o) <= dr.REL_ORACLE
    assert sr.rel(u_o, c["x"]) > 1e-6                           # (the cap ended it, not the tolerance)


@pytest.mark.parametrize("cap", dr.CAPS)
@pytest.mark.parametrize("case", dr.CAPS_CASES, ids=IDS)
def test_the_smallest_and_the_odd_caps(capi, case, cap):
    """CG_coarsest_max_iter = 1, 2, 3, 7 (sgpu_amg_create refuses none of them): the oracle's count 0, 1, 2, 6 and its iterate,
    2, 5, 8, 20 launches.  At cap 1 no kernel touches u: a non-zero start keeps its bits.  A second solve on the same handle has the
    first one's bits: no flag of a capped run outlives it"""
    c = dr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], "device_cg", cg_max_iter=cap)
    u_o, it_o = O.coarsest_cg(c["rhs"])
    u, it, launches = coarsest(capi, G, n, np.zeros(n), c["rhs"])
    print(f"cap {cap}: it {it} (oracle {it_o}), {launches} launches, rel oracle {sr.rel(u, u_o) if cap > 1 else 0.0:.2e}")
    assert it == it_o == dr.CAPS_COUNT[cap]
    assert launches == dr.launches(cap) == 2 + 3 * (cap - 1)
    if cap == 1:
        assert not np.any(u) and not np.any(u_o)
        u0 = inputs.v2(n)
        u0[0] = -0.0
        u1, it1, l1 = coarsest(capi, G, n, u0, c["rhs"])
        assert it1 == 0 and l1 == 2
        assert np.array_equal(bits(u1), bits(u0))
    else:
        assert sr.rel(u, u_o) <= dr.REL_ORACLE
        assert sr.rel(u_o, c["x"]) > 1e-6                       # (the cap ended it, not the tolerance)
    u2, it2, l2 = coarsest(capi, G, n, np.zeros(n), c["rhs"])
    assert it2 == it and l2 == launches and np.array_equal(bits(u2), bits(u))


@pytest.mark.parametrize("n", dr.SMALL_SIZES)
@pytest.mark.parametrize("family", ["tri", "band17"])
def test_a_small_coarsest_level_takes_the_lds_solver(capi, family, n):
    """at most 1 024 rows: value 2 is value 0, bit for bit, in one launch"""
    c = dr.case(family, n)
    _, G0, _ = one_level(capi, c["A"], "CG")
    _, G2, _ = one_level(capi, c["A"], "device_cg")
    u0, it0, l0 = coarsest(capi, G0, n, np.zeros(n), c["rhs"])
    u2, it2, l2 = coarsest(capi, G2, n, np.zeros(n), c["rhs"])
    assert it2 == it0 and l2 == l0 == 1
    assert np.array_equal(bits(u2), bits(u0))


# ---------------------------------------------------------------------------
# inside the V-cycle
def test_graph_and_eager_vcycles_agree_and_a_replay_is_one_launch(capi, two_level):
    _, Gg, (OA, _, _), _ = build(capi, two_level, "jacobi", use_graph=True, coarse_solver="device_cg")
    _, Ge, _, _ = build(capi, two_level, "jacobi", use_graph=False, coarse_solver="device_cg")
    n = OA[0].Mbig
    rhs = sr.rhs_for(n)
    dug, due, drhs = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, rhs)
    for call in range(3):
        l0 = capi.launch_count()
        Gg.vcycle(dug, drhs)
        lg = capi.launch_count() - l0
        Ge.vcycle(due, drhs)
        le = capi.launch_count() - l0 - lg
        assert np.array_equal(bits(dug.download()), bits(due.download())), call
        assert le > FULL
        assert call == 0 or lg == 1, (call, lg)                 # after the capturing call a V-cycle is one launch


def test_the_lifted_refusals_block(capi, two_level):
    """1 300 coarse rows.  "CG" and "direct" still send them to the host-driven loop, which the block solves refuse; under
    "device_cg" a block column has the bits of the scalar solve of that column, and the scalar results are those of "CG" to 1e-9"""
    n = two_level[0][0].shape[0]
    cols8 = sr.block_columns(n, 8)
    for name in ("CG", "direct"):
        _, G, _, _ = build(capi, two_level, "jacobi", coarse_solver=name)
        with pytest.raises(capi.SgpuError, match="host-driven CG"):
            G.vcycle_block(capi.BlockVector(n, 2), capi.BlockVector(n, 2, np.stack(cols8[:2], axis=1)))
    _, Gc, _, _ = build(capi, two_level, "jacobi", coarse_solver="CG")
    _, G, _, _ = build(capi, two_level, "jacobi", coarse_solver="device_cg")
    scalar_v, scalar_s = [], []
    for j, b in enumerate(cols8):
        du, dc, db = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, b)
        G.vcycle(du, db); Gc.vcycle(dc, db)
        scalar_v.append(du.download())
        e = sr.rel(scalar_v[-1], dc.download())
        it, hist, conv = G.solve_pCG(du, db)
        it_c, hist_c, conv_c = Gc.solve_pCG(dc, db)
        scalar_s.append((du.download(), it, hist))
        print(f"column {j}: V-cycle rel to CG {e:.2e}; pCG {it} iterations (CG {it_c}), rel {sr.rel(scalar_s[-1][0], dc.download()):.2e}")
        assert e <= 1e-9
        assert conv and conv_c and it == it_c and sr.rel(scalar_s[-1][0], dc.download()) <= 1e-9
    for K in (2, 8):
        B = np.stack(cols8[:K], axis=1)
        dU, dB = capi.BlockVector(n, K, np.zeros((n, K))), capi.BlockVector(n, K, B)
        G.vcycle_block(dU, dB)
        got = dU.download()
        for j in range(K):
            assert np.array_equal(bits(got[:, j]), bits(scalar_v[j])), (K, j, sr.rel(got[:, j], scalar_v[j]))
        its, hists, conv = G.solve_pCG_block(dU, dB)
        got = dU.download()
        assert conv
        for j in range(K):
            u_s, it_s, hist_s = scalar_s[j]
            assert its[j] == it_s, (K, j)
            assert np.array_equal(bits(hists[j]), bits(hist_s)), (K, j)
            assert np.array_equal(bits(got[:, j]), bits(u_s)), (K, j, sr.rel(got[:, j], u_s))


def test_the_lifted_refusals_fgmres(capi, two_level):
    """tests/test_gpu_gmres.py's contract on this hierarchy: the numpy reference preconditioned by the GPU's own V-cycle"""
    A = two_level[0][0]
    n = A.shape[0]
    rhs = sr.rhs_for(n)
    _, Gc, _, _ = build(capi, two_level, "jacobi", coarse_solver="CG")
    with pytest.raises(capi.SgpuError, match="host-driven CG"):
        Gc.solve_fgmres(capi.DeviceVector(n), capi.DeviceVector(n, rhs), restart=30)
    _, G, _, _ = build(capi, two_level, "jacobi", coarse_solver="device_cg")
    dz, dv = capi.DeviceVector(n), capi.DeviceVector(n)

    def M(v):
        dv.upload(v); dz.fill(0.0)
        G.vcycle(dz, dv)
        return dz.download()

    du, drhs = Padded(capi, np.ones(n)), capi.DeviceVector(n, rhs)
    it, hist, conv, true_res = G.solve_fgmres(du, drhs, restart=30)
    u = du.head()
    ref = gr.fgmres(A, rhs, 30, tol=1e-8, precond=M, dot=gr.gs_dot_blocked)
    assert conv and ref["converged"]
    check_against(ref, it, hist, u, "tri_two_level FGMRES(30)")
    res = sr.residual_hp(A, u, rhs)
    assert res <= 1e-8 * hist[0] * (1 + 1e-6)
    assert abs(res - true_res) <= 1e-6 * res


def test_the_lifted_refusals_lobpcg(capi, two_level):
    """On tri_two_level the refusal is lifted: under "CG" sgpu_eigs_LOBPCG refuses the hierarchy, under "device_cg" it runs.  It
    cannot CONVERGE there under any coarsest solver, so tests/test_gpu_eig.py's bounds are asserted on the Poisson operator they were
    written for: the smallest eigenvalues of tri(2600) are 0.5 + 1.46e-6 k^2, a relative gap of 1e-5 between neighbours, and LOBPCG's
    rate (1 - sqrt(gap)) / (1 + sqrt(gap)) needs hundreds of iterations for eight digits.  Poisson 24^3 in two levels has 1 728 coarse
    rows, and eig_ref.check_pairs knows its spectrum in closed form: assertions 1 and 2 of test_lobpcg, convergence within 100
    iterations, the reported residuals below tol lambda, a second run with the same bits."""
    n = two_level[0][0].shape[0]
    X0 = er.start_vectors(n, 2)
    _, Gc, _, _ = build(capi, two_level, "jacobi", coarse_solver="CG")
    with pytest.raises(capi.SgpuError, match="host-driven CG"):
        Gc.lobpcg(capi.BlockVector(n, 2, X0), 1, max_iter=2)
    _, Gt, _, _ = build(capi, two_level, "jacobi", coarse_solver="device_cg")
    dXt = capi.BlockVector(n, 2, X0)
    lam_t, _, it_t, _, _ = Gt.lobpcg(dXt, 1, max_iter=3, tol=er.TOL)
    exact = 2.5 - 2.0 * np.cos(np.pi / (n + 1))
    print(f"tri_two_level: {it_t} iterations, lambda_0 {lam_t[0]:.12e} (closed form {exact:.12e})")
    assert it_t == 3 and np.all(np.isfinite(lam_t)) and exact <= lam_t[0] * (1 + 1e-12) and lam_t[0] < 4.5     # a Ritz value of tri(n)

    m, K, nev = 24, 4, 4
    hier = hierarchy.poisson_hierarchy(m + 2, 2)
    assert hier[0][1].shape[0] == 1728 > sr.CG_MAXN
    _, G, _, _ = build(capi, hier, "jacobi", coarse_solver="device_cg")
    A = hier[0][0].tocsr()
    X0 = er.start_vectors(m ** 3, K)
    dX = capi.BlockVector(m ** 3, K, X0)
    lam, res, it, hist, conv = G.lobpcg(dX, nev, max_iter=100, tol=er.TOL)
    X = dX.download().copy()
    print(f"Poisson {m}^3, K = {K}: {it} iterations")
    assert conv
    er.check_pairs(A, X, lam, nev, m, what=f"({m}, {K}, {nev})")
    assert np.all(np.diff(lam) >= 0.0) and np.all(np.isfinite(X))
    assert all(res[j] < er.TOL * lam[j] for j in range(nev))
    dX.upload(X0)
    lam2, res2, it2, _, conv2 = G.lobpcg(dX, nev, max_iter=100, tol=er.TOL)
    assert conv2 and it2 == it and np.array_equal(bits(lam2), bits(lam)) and np.array_equal(bits(dX.download()), bits(X))


# ---------------------------------------------------------------------------
# through the setup, and through sgpu_amg_set_operator
def test_through_the_setup(capi):
    """tests/test_gpu_vcycle.py's large-coarsest-level case with coarse_solver="device_cg": Poisson 24^3 cut at max_level = 1
    (5 324 coarse rows); pCG with the oracle's iteration count, its history and its solution"""
    from saena_amd import host
    from tests.test_amg_setup import oracle_amg_from_host
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(24).assemble()
    S = host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, dynamic_levels=0, max_level=1)), coarse_solver="device_cg").to_device()
    assert S.num_levels == 2 and S.level_info(1)["rows"] > sr.CG_MAXN
    rhs = A.laplacian3D_rhs()
    u1, it1, hist1, _ = S.solve_pCG(rhs)                       # captures the V-cycle (every captured launch counts as an enqueue)
    l0 = capi.launch_count()
    u, it, hist, conv = S.solve_pCG(rhs)
    launches = capi.launch_count() - l0
    assert conv and it == it1 and np.array_equal(bits(hist), bits(hist1)) and np.array_equal(bits(u), bits(u1))
    amg, OA = oracle_amg_from_host(S, "jacobi", pre=3, post=3, max_iter=50, tol=1e-8)
    u_o, it_o, hist_o = amg.solve_pCG(rhs)
    print(f"{it} iterations (oracle {it_o}), {launches} launches, rel {np.linalg.norm(u - u_o) / np.linalg.norm(u_o):.2e}")
    assert it_o == it and np.all(np.abs(hist - hist_o) <= TOL_HIST * hist_o[0])
    assert np.linalg.norm(u - u_o) <= 1e-9 * np.linalg.norm(u_o)
    assert launches < FULL                                     # the V-cycles were graph launches: one eager coarsest solve alone is 449
    with pytest.raises(host.SgpuError, match="none of direct, cg, device_cg"):
        S.set_coarse_solver("lu")


def test_the_environment_reaches_a_driver_compiled_unchanged(capi, monkeypatch):
    """SAENA_COARSE_SOLVER, read by to_device: the block solve refuses the cut hierarchy under the default, and takes it with
    device_cg in the environment; a name that is none of the three leaves the setter's value"""
    from saena_amd import host
    L = host.load("gpu")
    A = host.Matrix(host.Comm("gpu", "rccl")).laplacian3D(24).assemble()
    S = host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, dynamic_levels=0, max_level=1)))
    rhs = A.laplacian3D_rhs()
    B = np.stack([rhs, 0.5 * rhs[::-1]], axis=1)
    monkeypatch.setenv("SAENA_COARSE_SOLVER", "lu")
    S.to_device()
    with pytest.raises(host.SgpuError, match="host-driven CG"):
        S.solve_pCG_block(B)
    monkeypatch.setenv("SAENA_COARSE_SOLVER", "device_cg")
    S.to_device()
    U, its, hists, conv = S.solve_pCG_block(B)
    u, it, hist, conv1 = S.solve_pCG(rhs)
    # (no bit contract here: the scalar V-cycle applies every level's tuned form, the block V-cycle k_csr_block)
    print(f"block column 0: {its[0]} iterations (scalar {it}), rel {np.linalg.norm(U[:, 0] - u) / np.linalg.norm(u):.2e}")
    assert conv and conv1 and its[0] == it
    assert np.linalg.norm(U[:, 0] - u) <= 1e-9 * np.linalg.norm(u)


def test_set_operator_on_the_coarsest_level(capi):
    """tri(1300) swapped for band17(1300): the contracts on the new operator, through the kept work space"""
    (f0, n), (f1, _) = dr.SET_OPERATOR
    c0, c1 = dr.case(f0, n), dr.case(f1, n)
    O0, G, op0 = one_level(capi, c0["A"], "device_cg")
    u, it, _ = coarsest(capi, G, n, np.zeros(n), c0["rhs"])
    dr.check_contracts(c0, u, it, *O0.coarsest_cg(c0["rhs"]))
    O1, OA1 = hierarchy.single_level_oracle(c1["A"], cg_max_iter=sr.CG_MAX_ITER, cg_tol=sr.CG_TOL)
    op1 = util.gpu_operator(OA1)
    old = G.set_operator(0, op1)
    assert old is op0
    u, it, launches = coarsest(capi, G, n, np.zeros(n), c1["rhs"])
    dr.check_contracts(c1, u, it, *O1.coarsest_cg(c1["rhs"]))
    assert launches == FULL
    du, drhs = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, c1["rhs"])
    G.vcycle(du, drhs)                                         # captured again, over the new operator
    assert np.array_equal(bits(du.download()), bits(u))
