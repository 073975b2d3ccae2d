"""sgpu_eigs_LOBPCG on the GPU, held to a written contract.

Hierarchies come from tests/hierarchy.poisson_hierarchy through tests/test_gpu_vcycle.build (Jacobi 3 + 3, direct coarsest solve):
8^3 rows in two levels and 16^3 in three, the smallest with those depths and with complete clusters of 1 + 3 + 3 eigenvalues.  Start
vectors, the closed-form spectrum, the numpy reference's iteration counts and orthonormality and every bound come from
tests/eig_ref.py; tests/test_eig_ref.py shows on the CPU that a correct implementation stays inside each of them.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import eig_ref as er, hierarchy, solver_ref as sr
from tests.test_gpu_block_solver_layer import Blk, same_bits
from tests.test_gpu_solver_layer import bits, one_level
from tests.test_gpu_vcycle import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


_HIER = {}


def hier(m):
    if m not in _HIER:
        _HIER[m] = hierarchy.poisson_hierarchy(m + 2, 2 if m == 8 else 3)
    return _HIER[m]


def gpu(capi, m, **kw):
    """-> (GPU hierarchy, scipy A) of the m^3 Poisson operator"""
    _, G, _, _ = build(capi, hier(m), "jacobi", pre=3, post=3, **kw)
    return G, hier(m)[0][0].tocsr()


def test_the_hierarchy_is_the_reference_s():
    """what the GPU solves is eig_ref.poisson(m), whose spectrum eig_ref.analytic states"""
    for m in (8, 16):
        A, B = hier(m)[0][0].tocsr(), er.poisson(m)
        assert A.shape == B.shape and abs(A - B).max() <= 1e-12 * abs(B).max()
        assert [a.shape[0] for a in hier(m)[0]] == [a.shape[0] for a in er.case(m)["As"]]


@pytest.mark.parametrize("shape", er.SHAPES, ids=str)
def test_lobpcg(capi, shape):
    """1. rho_j = ||A x_j - lambda_j x_j|| / ||x_j||, recomputed here in longdouble from the downloaded X, is at most tol lambda_j
    plus the rounding of recomputing a residual; 2. |lambda_j - closed form_j| <= rho_j (a missed or repeated pair fails this);
    3. max |X^T X - I| <= 16 x the reference's; 4. iterations <= ceil(1.25 x the reference's) + 2.  Also: lambda ascending, the
    reported residuals are the recomputed ones, and a second run reproduces every bit"""
    m, K, nev = shape
    G, A = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    lam, res, it, hist, conv = G.lobpcg(dX, nev, max_iter=100, tol=er.TOL)
    X = dX.get().copy()
    defect = er.ortho_defect(X)
    print(f"{shape}: {it} iterations (reference {er.ITERS[shape]}, bound {er.iteration_bound(shape)}), max |X^T X - I| = {defect:.3e} "
          f"(reference {er.ORTHO[shape]:.1e}, bound {er.ORTHO_MARGIN * er.ORTHO[shape]:.1e})")
    assert conv
    rhos = er.check_pairs(A, X, lam, nev, m, what=str(shape))                    # 1 and 2
    assert defect <= er.ORTHO_MARGIN * er.ORTHO[shape]                           # 3
    assert it <= er.iteration_bound(shape)                                        # 4
    assert np.all(np.diff(lam) >= 0.0) and np.all(np.isfinite(lam)) and np.all(np.isfinite(X))
    for j in range(nev):
        assert res[j] < er.TOL * lam[j]
        assert abs(res[j] - rhos[j] * np.linalg.norm(X[:, j])) <= 1e-3 * res[j] + 1e-12 * lam[j]
    assert all(len(h) == it + 1 for h in hist)
    dX.upload(X0)
    lam2, res2, it2, hist2, conv2 = G.lobpcg(dX, nev, max_iter=100, tol=er.TOL)
    assert conv2 and it2 == it
    same_bits(lam2, lam); same_bits(res2, res); same_bits(dX.get(), X)
    for a, b in zip(hist, hist2):
        same_bits(a, b)


def test_the_vcycle_buys_iterations(capi):
    """5. precond = 0 on 8^3 needs at least 3 x the iterations of precond = 1 (the reference: about 4 x here, 7 x on 16^3), and finds
    the same eigenvalues"""
    shape = er.SHAPES[0]
    m, K, nev = shape
    G, A = gpu(capi, m)
    X0 = er.start_vectors(m ** 3, K)
    dX = Blk(capi, X0)
    lam, _, it, _, conv = G.lobpcg(dX, nev, tol=er.TOL)
    dX.upload(X0)
    lam_p, _, it_p, _, conv_p = G.lobpcg(dX, nev, max_iter=400, tol=er.TOL, precond=False)
    print(f"{shape}: {it} iterations with the V-cycle, {it_p} without (reference {er.ITERS[shape]} and {er.ITERS_PLAIN[shape]})")
    assert conv and conv_p
    assert it_p >= er.PLAIN_RATIO_MIN * it
    er.check_pairs(A, dX.get(), lam_p, nev, m, what="plain")


def test_second_solve_from_the_result(capi):
    """0 iterations, and the same lambda to the bound of assertion 1"""
    m, K, nev = er.SHAPES[0]
    G, A = gpu(capi, m)
    dX = Blk(capi, er.start_vectors(m ** 3, K))
    lam, _, it, _, conv = G.lobpcg(dX, nev, tol=er.TOL)
    lam2, res2, it2, hist2, conv2 = G.lobpcg(dX, nev, tol=er.TOL)
    assert conv and conv2 and it > 0 and it2 == 0 and all(len(h) == 1 for h in hist2)
    for j in range(nev):
        _, rounding = er.residual_hp(A, dX.get()[:, j], lam2[j])
        assert abs(lam2[j] - lam[j]) <= er.TOL * lam[j] + rounding
    er.check_pairs(A, dX.get(), lam2, nev, m, what="second solve")


def test_replay_and_zero_filled_inactive_columns(capi):
    """from the second iteration on every iteration costs the same number of launches (the V-cycle's graph is captured once; the
    active set changes coefficients, not launches).  And the columns outside the active set are zero-filled, not skipped: stopped
    right after its orthonormalisation step, an iteration that began with some columns converged has exact zeros in those columns
    of the solver's own W, AW, P and AP, and in no other column"""
    shape = er.SHAPES[1]
    m, K, nev = shape
    G, _ = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    launches = []
    for k in range(1, 7):
        dX.upload(X0)
        l0 = capi.launch_count()
        _, _, it, _, conv = G.lobpcg(dX, nev, max_iter=k, tol=1e-14)
        launches.append(capi.launch_count() - l0)
        assert it == k and not conv
    per_iteration = np.diff(launches)
    print(f"launches of a solve of 1..6 iterations: {launches}")
    assert np.all(per_iteration[1:] == per_iteration[1]) and 0 < per_iteration[1] <= 40, launches
    assert per_iteration[0] <= per_iteration[1]                              # (the first iteration has no P)
    # a run to convergence, then the same run stopped inside an earlier iteration (sgpu_debug_eig_stop: right after the
    # orthonormalisation, before the Rayleigh-Ritz update overwrites P and AP): columns converge at different iterations
    dX.upload(X0)
    lam, _, it_full, hist, conv = G.lobpcg(dX, nev, tol=er.TOL)
    assert conv
    seen = False
    for k in range(it_full - 1, 1, -1):                                        # the iteration with index k
        dX.upload(X0)
        lam_before = G.lobpcg(dX, nev, max_iter=k, tol=er.TOL)[0]              # lambda at the start of that iteration
        dX.upload(X0)
        G.debug_eig_stop(K, k)
        _, _, it, hist_k, conv = G.lobpcg(dX, nev, tol=er.TOL)
        msg = capi.lib().sgpu_last_error().decode()
        assert not conv and it == k and "stopped for inspection" in msg and "with P" in msg, msg
        inactive = [j for j in range(K) if hist_k[j][k] < er.TOL * lam_before[j]]
        for which, name in ((2, "W"), (3, "AW"), (4, "P"), (5, "AP")):
            dV = Blk(capi, np.full((n, K), np.nan))
            G.debug_eig_vector(K, which, dV)
            V = dV.get()
            for j in range(K):
                if j in inactive:
                    assert np.all(bits(V[:, j]) == bits(0.0)), (k, name, j)
                else:
                    assert np.linalg.norm(V[:, j]) > 0.0 and np.all(np.isfinite(V[:, j])), (k, name, j)
        if 0 < len(inactive) < K:
            seen = True
            break
    assert seen, "no iteration with some, not all, columns converged"
    dX.upload(X0)                                                              # the stop was for one solve only
    lam2, _, it2, _, conv2 = G.lobpcg(dX, nev, tol=er.TOL)
    assert conv2 and it2 == it_full
    same_bits(lam2, lam)


@pytest.fixture(scope="module")
def poisson():
    return hierarchy.poisson_hierarchy(18, 4)      # the hierarchy of tests/test_gpu_vcycle.py: 4096 -> 512 -> 64 -> 8 rows


def test_lobpcg_leaves_block_pcg_and_the_scalar_solve_alone(capi, poisson):
    """the block cache of eight captured V-cycles -- sgpu_solve_pCG_block's own pair and seven more -- survives a LOBPCG solve with the
    same K: each still replays as one launch and returns the same bits, block pCG costs the launches it cost before (its graph was
    not evicted) and returns the same bits, and so does the scalar sgpu_solve_pCG"""
    K = 4
    _, G, (OA, _, _), _ = build(capi, poisson, "jacobi")
    n = OA[0].Mbig
    rhs = orc.laplacian3d_rhs(18)
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, rhs)
    it0, hist0, _ = G.solve_pCG(du, dr)
    u0 = du.download()
    B = np.stack([rhs * (1 + j) for j in range(K)], axis=1)
    dU, dB = Blk(capi, np.zeros((n, K))), Blk(capi, B)
    G.solve_pCG_block(dU, dB)                                                 # captures its (rho, r) pair
    l0 = capi.launch_count()
    itb, histb, _ = G.solve_pCG_block(dU, dB)
    launches_b = capi.launch_count() - l0
    ub = dU.get().copy()
    pairs = [(Blk(capi, np.zeros((n, K))), Blk(capi, B * (2 + i))) for i in range(7)]
    for u, r in pairs:
        G.vcycle_block(u, r)                                                  # captured: eight in the cache

    def replay():
        out = []
        for u, r in pairs:
            u.upload(np.zeros((n, K)))
            l0 = capi.launch_count()
            G.vcycle_block(u, r)
            assert capi.launch_count() - l0 == 1
            out.append(u.get().copy())
        return out
    before = replay()
    dX = Blk(capi, er.start_vectors(n, K))
    lam, _, it, _, conv = G.lobpcg(dX, K, tol=er.TOL)
    assert conv and it > 0
    for a, b in zip(before, replay()):
        same_bits(a, b)
    l0 = capi.launch_count()
    itb2, histb2, _ = G.solve_pCG_block(dU, dB)
    assert capi.launch_count() - l0 == launches_b and itb2 == itb
    same_bits(dU.get(), ub)
    for a, b in zip(histb, histb2):
        same_bits(a, b)
    it1, hist1, _ = G.solve_pCG(du, dr)
    assert it1 == it0 and np.array_equal(bits(hist1), bits(hist0)) and np.array_equal(bits(du.download()), bits(u0))


class _K3:
    """something with .ptr and .K = 3"""

    def __init__(self, v):
        self.ptr, self.K = v.ptr, 3


def test_lobpcg_refusals(capi):
    """every refused input is refused with a message before anything is launched or written; max_iter = 2 returns SGPU_ERR_NOCONV
    with finite lambda, X and res"""
    m, K, nev = er.SHAPES[0]
    G, _ = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    with pytest.raises(capi.SgpuError, match="2, 4 or 8"):
        G.lobpcg(_K3(dX), 1)
    for bad in (0, K + 1):
        with pytest.raises(capi.SgpuError, match="nev must be in 1..K"):
            G.lobpcg(dX, bad)
    with pytest.raises(capi.SgpuError, match="precond is 0"):
        capi.check(capi.lib().sgpu_eigs_LOBPCG(G.h, dX.ptr, K, nev, 10, 1e-8, 2, np.zeros(K).ctypes.data_as(capi._PD), None, None, None, 0))
    same_bits(dX.get(), X0)
    dep = X0.copy()
    dep[:, 2] = 2.0 * dep[:, 0] - dep[:, 1]
    dX.upload(dep)
    with pytest.raises(capi.SgpuError, match="linearly dependent"):
        G.lobpcg(dX, nev)
    same_bits(dX.get(), dep)
    _, Gs, _ = one_level(capi, sr.tri(9), "direct")                          # 9 rows < 3 K
    with pytest.raises(capi.SgpuError, match="needs at least as many"):
        Gs.lobpcg(Blk(capi, er.start_vectors(9, K)), nev)
    big = sr.case("tri", 1025)
    _, Gb, _ = one_level(capi, big["A"], "CG")                               # one more row than the LDS-resident coarsest solvers hold
    with pytest.raises(capi.SgpuError, match="host-driven CG"):
        Gb.lobpcg(Blk(capi, er.start_vectors(1025, K)), nev)
    with pytest.raises(capi.SgpuError, match="chebyshev needs eig_max"):     # no eig_max was given: handled as elsewhere
        OA, OP, OR = hierarchy.oracle_hierarchy(*hier(m))
        from tests import util
        ops = [[util.gpu_operator(o) for o in L] for L in (OA, OP, OR)]
        capi.Amg(*ops, eig_max=None, smoother="chebyshev")
    dX.upload(X0)
    lam, res, it, hist, conv = G.lobpcg(dX, nev, max_iter=2, tol=er.TOL)
    assert not conv and it == 2
    assert np.all(np.isfinite(lam)) and np.all(np.isfinite(res)) and np.all(np.isfinite(dX.get())) and np.all(lam > 0)
    assert "above the tolerance" in capi.lib().sgpu_last_error().decode()


def test_lobpcg_with_the_chebyshev_smoother_and_the_cg_coarsest_solver(capi, poisson):
    """a V-cycle that is no fixed linear map is still a preconditioner: the pairs meet assertions 1 and 2"""
    _, G, (OA, _, _), _ = build(capi, poisson, "chebyshev", coarse_solver="CG")
    m, K, nev = 16, 4, 4
    dX = Blk(capi, er.start_vectors(m ** 3, K))
    lam, _, it, _, conv = G.lobpcg(dX, nev, tol=er.TOL)
    print(f"chebyshev / CG coarsest: {it} iterations")
    assert conv
    er.check_pairs(poisson[0][0].tocsr(), dX.get(), lam, nev, m, what="chebyshev")
