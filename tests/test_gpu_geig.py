"""sgpu_eigs_LOBPCG_gen on the GPU -- A x = lambda B x with a second SPD operator -- held to a written contract.

Hierarchies are those of tests/test_gpu_eig.py (8^3 rows in two levels, 16^3 in three; Jacobi 3 + 3, direct coarsest solve).  The mass
matrices (the 27-point consistent one with its closed-form spectrum, a lumped one with a jump), the start vectors, the numpy
reference's iteration counts and B-orthonormality and every bound come from tests/geig_ref.py; tests/test_geig_ref.py shows on the CPU
that a correct implementation stays inside each of them.
"""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import oracle as orc
from tests import eig_ref as er, geig_ref as gg, hierarchy, solver_ref as sr, util
from tests.test_gpu_block_solver_layer import Blk, same_bits
from tests.test_gpu_eig import _K3, gpu
from tests.test_gpu_solver_layer import bits, one_level
from tests.test_gpu_vcycle import build

pytestmark = pytest.mark.gpu

CASES = [(shape, mass) for mass in gg.MASSES for shape in gg.SHAPES]


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def op_of(M, nprocs=1, r=0):
    """a device operator over the scipy matrix M (rank r of an even row partition over nprocs)"""
    n = M.shape[0]
    return util.gpu_operator(orc.OracleOp(hierarchy.scipy_to_coo(M.tocsr()), n, n, orc.split_even(n, nprocs)), r)


def solve(G, dX, nev, B, **kw):
    return G.lobpcg(dX, nev, B=B, **kw)


def check_result(shape, mass, A, Bs, X, lam, res, it, conv, what=""):
    """assertions 1 to 3 on a generalised result; -> the rho_j"""
    m, K, nev = shape
    key = (shape, mass)
    defect = gg.ortho_defect(X, Bs)
    print(f"{what}{shape} {mass}: {it} iterations (reference {gg.ITERS_GEN[key]}, bound {gg.iteration_bound(shape, mass)}), "
          f"max |X^T B X - I| = {defect:.3e} (reference {gg.ORTHO_GEN[key]:.1e}, bound {gg.ORTHO_MARGIN * gg.ORTHO_GEN[key]:.1e})")
    assert conv
    rhos = gg.check_pairs(A, Bs, X, lam, nev, gg.exact(mass, m, nev), gg.LAMBDA_MIN_B[mass], what=f"{what}{shape} {mass}")      # 1 and 2
    assert defect <= gg.ORTHO_MARGIN * gg.ORTHO_GEN[key]                         # 3
    assert it <= gg.iteration_bound(shape, mass)
    assert np.all(np.diff(lam) >= 0.0) and np.all(np.isfinite(lam)) and np.all(np.isfinite(X))
    for j in range(nev):                                                         # the reported residuals are the recomputed ones
        nbx = np.linalg.norm(Bs @ X[:, j])
        assert res[j] < gg.TOL * lam[j] * nbx
        assert abs(res[j] - rhos[j] * nbx) <= 1e-3 * res[j] + 1e-12 * lam[j]
    return rhos


@pytest.mark.parametrize("shape,mass", CASES, ids=str)
def test_lobpcg_gen(capi, shape, mass):
    """1. rho_j = ||A x_j - lambda_j B x_j|| / ||B x_j||, recomputed here in longdouble from the downloaded X, is at most tol lambda_j
    plus the rounding of recomputing a residual; 2. |lambda_j - exact_j| <= rho_j ||B x_j|| / sqrt(lambda_min(B)) (the closed form
    for mass27, a dense eigh or eigsh for lumped); 3. max |X^T B X - I| <= 16 x the reference's, iterations <= ceil(1.25 x the
    reference's) + 2.  Also: lambda ascending, the reported residuals are the recomputed ones, a second run reproduces every bit"""
    m, K, nev = shape
    G, A = gpu(capi, m)
    Bs = gg.mass(mass, m)
    B = op_of(Bs)
    X0 = er.start_vectors(m ** 3, K)
    dX = Blk(capi, X0)
    lam, res, it, hist, conv = solve(G, dX, nev, B, max_iter=100, tol=gg.TOL)
    X = dX.get().copy()
    check_result(shape, mass, A, Bs, X, lam, res, it, conv)
    assert all(len(h) == it + 1 for h in hist)
    dX.upload(X0)
    lam2, res2, it2, hist2, conv2 = solve(G, dX, nev, B, max_iter=100, tol=gg.TOL)
    assert conv2 and it2 == it
    same_bits(lam2, lam); same_bits(res2, res); same_bits(dX.get(), X)
    for a, b in zip(hist, hist2):
        same_bits(a, b)


@pytest.mark.parametrize("shape,mass", [c for c in CASES if c[0][0] == 16], ids=str)
def test_the_vcycle_buys_iterations(capi, shape, mass):
    """3. on 16^3, precond = 0 needs at least 3 x the iterations of precond = 1 (the reference: at least 5 x), and finds the same pairs"""
    m, K, nev = shape
    G, A = gpu(capi, m)
    Bs = gg.mass(mass, m)
    B = op_of(Bs)
    X0 = er.start_vectors(m ** 3, K)
    dX = Blk(capi, X0)
    lam, _, it, _, conv = solve(G, dX, nev, B, tol=gg.TOL)
    dX.upload(X0)
    lam_p, _, it_p, _, conv_p = solve(G, dX, nev, B, max_iter=600, tol=gg.TOL, precond=False, cap=700)
    print(f"{shape} {mass}: {it} iterations with the V-cycle, {it_p} without (reference {gg.ITERS_GEN[(shape, mass)]} and {gg.ITERS_GEN_PLAIN[(shape, mass)]})")
    assert conv and conv_p
    assert it_p >= gg.PLAIN_RATIO_MIN * it
    gg.check_pairs(A, Bs, dX.get(), lam_p, nev, gg.exact(mass, m, nev), gg.LAMBDA_MIN_B[mass], what="plain")


@pytest.mark.parametrize("mass", gg.STOP_MASSES)
def test_stopped_after_the_orthonormalisation(capi, mass):
    """4. stopped at iteration 0 and 1 (sgpu_debug_eig_stop), the solver's own W, BW, P and BP (sgpu_debug_eig_vector 2, 7, 4, 8):
    W^T B W = I on the active columns and X^T B W = 0, each to 16 x the reference's figure; BW = B W by a host product within
    geig_ref.bw_bound; inactive columns are exact zeros and no other column is (with mass27 column 0 starts as an exact eigenvector,
    so it is inactive from iteration 0 on); iteration 0 runs without P.  The active set is the reference's"""
    m, K, nev = gg.SHAPES[0]
    G, A = gpu(capi, m)
    n = m ** 3
    Bs = gg.mass(mass, m)
    B = op_of(Bs)
    X0 = gg.stop_start(mass, m, K)
    c = er.case(m)
    dX = Blk(capi, X0)
    for k in (0, 1):
        ref = gg.lobpcg_gen(c["A"], Bs, X0, nev, precond=er.vcycle_block(c), stop=k)
        act = ref["act"]
        dX.upload(X0)
        G.debug_eig_stop(K, k)
        _, _, it, _, conv = solve(G, dX, nev, B, tol=gg.TOL)
        msg = capi.lib().sgpu_last_error().decode()
        assert not conv and it == k and "stopped for inspection" in msg and ("with P" if k else "without P") in msg, msg
        V = {}
        for which, name in ((2, "W"), (7, "BW"), (3, "AW")) + (((4, "P"), (8, "BP"), (5, "AP")) if k else ()):
            dV = Blk(capi, np.full((n, K), np.nan))
            G.debug_eig_vector(K, which, dV)
            V[name] = dV.get().copy()
            for j in range(K):
                if j in act:
                    assert np.linalg.norm(V[name][:, j]) > 0.0 and np.all(np.isfinite(V[name][:, j])), (k, name, j)
                else:
                    assert np.all(bits(V[name][:, j]) == bits(0.0)), (k, name, j)
        X = dX.get().copy()
        wbw, xbw = gg.stop_defects(dict(X=X, W=V["W"], act=act), Bs)
        print(f"{mass}, iteration {k}: active {act}, max |W^T B W - I| = {wbw:.2e} (reference {gg.STOP_GEN[(mass, k)][0]:.1e}), "
              f"max |X^T B W| = {xbw:.2e} (reference {gg.STOP_GEN[(mass, k)][1]:.1e})")
        assert wbw <= gg.ORTHO_MARGIN * gg.STOP_GEN[(mass, k)][0]
        assert xbw <= gg.ORTHO_MARGIN * gg.STOP_GEN[(mass, k)][1]
        assert np.all(np.abs(V["BW"] - Bs @ V["W"]) <= gg.bw_bound(Bs, V["W"], ref["Tw"], K)), (mass, k)
    dX.upload(X0)                                                              # the stop was for one solve only
    _, _, it2, _, conv2 = solve(G, dX, nev, B, tol=gg.TOL)
    assert conv2 and it2 > 1


@pytest.mark.parametrize("mass", gg.MASSES)
def test_b_scaled_by_four(capi, mass):
    """5. the criterion's scale invariance: with 4 B, lambda' 4 = lambda to 1e-12 relative, X' = X / 2 to 1e-10 relative per entry (up
    to sign), iteration counts within 1.  A criterion without ||B x_j|| fails this: it would stop the scaled solve at another
    iteration"""
    shape = gg.SHAPES[1]
    m, K, nev = shape
    G, _ = gpu(capi, m)
    Bs = gg.mass(mass, m)
    B1, B4 = op_of(Bs), op_of(4.0 * Bs)
    X0 = er.start_vectors(m ** 3, K)
    dX = Blk(capi, X0)
    lam, _, it, _, conv = solve(G, dX, nev, B1, tol=gg.TOL)
    X = dX.get().copy()
    dX.upload(X0)
    lam4, _, it4, _, conv4 = solve(G, dX, nev, B4, tol=gg.TOL)
    X4 = dX.get().copy()
    print(f"{shape} {mass}: {it} iterations with B, {it4} with 4 B; max |4 lambda' - lambda| / lambda = {np.max(np.abs(4 * lam4 - lam) / lam):.2e}")
    assert conv and conv4 and abs(it - it4) <= 1
    assert np.all(np.abs(4.0 * lam4 - lam) <= 1e-12 * lam)
    for j in range(K):
        s = 1.0 if float(X4[:, j] @ X[:, j]) >= 0.0 else -1.0
        assert np.all(np.abs(2.0 * s * X4[:, j] - X[:, j]) <= 1e-10 * np.abs(X[:, j])), (mass, j)


def test_b_lifetime_and_the_shared_graph(capi):
    """6. nothing keeps a pointer to B: solve with B1 = mass27, destroy B1, create B2 = lumped, solve again on the same hierarchy --
    the second result meets assertions 1 to 3 for B2.  From the second iteration of the first solve on every iteration costs the same
    number of launches, and no recapture happens between the solves: a solve of 3 iterations with B2 costs the launches it cost
    with B1 (a captured V-cycle counts each of its kernels, a replay counts one)"""
    shape = gg.SHAPES[1]
    m, K, nev = shape
    G, A = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    B1 = op_of(gg.mass("mass27", m))
    launches = []
    for k in range(1, 7):
        dX.upload(X0)
        l0 = capi.launch_count()
        _, _, it, _, conv = solve(G, dX, nev, B1, max_iter=k, tol=1e-14)
        launches.append(capi.launch_count() - l0)
        assert it == k and not conv
    per_iteration = np.diff(launches)
    print(f"launches of a generalised solve of 1..6 iterations: {launches}")
    assert np.all(per_iteration[1:] == per_iteration[1]) and 0 < per_iteration[1] <= 60, launches      # (the first solve also captured)
    dX.upload(X0)
    l0 = capi.launch_count()
    solve(G, dX, nev, B1, max_iter=3, tol=1e-14)
    three = capi.launch_count() - l0
    assert three == launches[2]
    dX.upload(X0)
    lam1, res1, it1, _, conv1 = solve(G, dX, nev, B1, tol=gg.TOL)
    check_result(shape, "mass27", A, gg.mass("mass27", m), dX.get().copy(), lam1, res1, it1, conv1, what="B1 ")
    B1.destroy()
    del B1
    Bs2 = gg.mass("lumped", m)
    B2 = op_of(Bs2)
    dX.upload(X0)
    l0 = capi.launch_count()
    solve(G, dX, nev, B2, max_iter=3, tol=1e-14)
    assert capi.launch_count() - l0 == three, "the V-cycle was captured again"
    dX.upload(X0)
    lam2, res2, it2, _, conv2 = solve(G, dX, nev, B2, tol=gg.TOL)
    check_result(shape, "lumped", A, Bs2, dX.get().copy(), lam2, res2, it2, conv2, what="B2 ")


def test_the_standard_solve_is_untouched(capi):
    """7. sgpu_eigs_LOBPCG, then a generalised solve, then sgpu_eigs_LOBPCG from the same start: the two standard results are equal bit
    for bit (X, lambda, res, iterations, history), and the second costs one V-cycle capture less in launches at most (no recapture)"""
    shape = gg.SHAPES[1]
    m, K, nev = shape
    G, _ = gpu(capi, m)
    X0 = er.start_vectors(m ** 3, K)
    dX = Blk(capi, X0)
    lam, res, it, hist, conv = G.lobpcg(dX, nev, tol=er.TOL)
    X = dX.get().copy()
    dX.upload(X0)
    l0 = capi.launch_count()
    G.lobpcg(dX, nev, tol=er.TOL)
    replayed = capi.launch_count() - l0
    B = op_of(gg.mass("lumped", m))
    dX.upload(X0)
    _, _, _, _, conv_g = solve(G, dX, nev, B, tol=gg.TOL)
    assert conv and conv_g
    dX.upload(X0)
    l0 = capi.launch_count()
    lam2, res2, it2, hist2, conv2 = G.lobpcg(dX, nev, tol=er.TOL)
    assert capi.launch_count() - l0 == replayed
    assert conv2 and it2 == it
    same_bits(lam2, lam); same_bits(res2, res); same_bits(dX.get(), X)
    for a, b in zip(hist, hist2):
        same_bits(a, b)
    with pytest.raises(capi.SgpuError, match="which is 0 .. 8"):
        G.debug_eig_vector(K, 9, dX)


def test_a_standard_only_hierarchy_has_no_b_vectors(capi):
    """the three extra block vectors are made at the first generalised call: before it sgpu_debug_eig_vector refuses 6, 7 and 8"""
    m, K, nev = gg.SHAPES[0]
    G, _ = gpu(capi, m)
    dX = Blk(capi, er.start_vectors(m ** 3, K))
    G.lobpcg(dX, nev, tol=er.TOL)
    for which in (6, 7, 8):
        with pytest.raises(capi.SgpuError, match="no sgpu_eigs_LOBPCG_gen has run"):
            G.debug_eig_vector(K, which, dX)
    G.debug_eig_vector(K, 5, dX)


def test_the_extra_state_is_allocated_by_the_first_generalised_call_alone(capi):
    """the bytes the library holds (device and pinned arrays, sgpu_debug_op_storage): a second standard solve allocates nothing; the
    first generalised solve with this K adds exactly three block vectors, the partial sums of ||(Bx)_j||^2, their K sums and the
    pinned mirror of those -- so the standard solve before it held none of them; later solves of either kind add nothing"""
    m, K, nev = gg.SHAPES[0]
    G, _ = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    B = op_of(gg.mass("lumped", m))
    G.lobpcg(dX, nev, tol=er.TOL)
    b0 = capi.live_bytes()
    dX.upload(X0)
    G.lobpcg(dX, nev, tol=er.TOL)
    assert capi.live_bytes() == b0
    dX.upload(X0)
    solve(G, dX, nev, B, tol=gg.TOL)
    b1 = capi.live_bytes()
    print(f"the first generalised solve added {b1 - b0} bytes")
    assert b1 - b0 == 8 * (3 * n * K + sr.N_PARTIALS * K + K + K)
    for with_b in (True, False):
        dX.upload(X0)
        G.lobpcg(dX, nev, tol=gg.TOL, B=B if with_b else None)
        assert capi.live_bytes() == b1


def test_block_pcg_and_its_cache_survive_a_generalised_solve(capi):
    """7. eight captured block V-cycles of sgpu_solve_pCG_block still replay as one launch each after a generalised solve with the same
    K and return the same bits, and block pCG costs the launches it cost before and returns the same bits"""
    K = 4
    poisson = hierarchy.poisson_hierarchy(18, 4)                                 # tests/test_gpu_vcycle.py's: 4096 -> 512 -> 64 -> 8 rows
    _, G, (OA, _, _), _ = build(capi, poisson, "jacobi")
    n = OA[0].Mbig
    rhs = orc.laplacian3d_rhs(18)
    Bm = np.stack([rhs * (1 + j) for j in range(K)], axis=1)
    dU, dB = Blk(capi, np.zeros((n, K))), Blk(capi, Bm)
    G.solve_pCG_block(dU, dB)                                                   # captures its (rho, r) pair
    l0 = capi.launch_count()
    itb, histb, _ = G.solve_pCG_block(dU, dB)
    launches_b = capi.launch_count() - l0
    ub = dU.get().copy()
    pairs = [(Blk(capi, np.zeros((n, K))), Blk(capi, Bm * (2 + i))) for i in range(7)]
    for u, r in pairs:
        G.vcycle_block(u, r)                                                    # captured: eight in the cache

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
    lam, _, it, _, conv = solve(G, dX, K, op_of(gg.mass("mass27", 16)), tol=gg.TOL)
    assert conv and it > 0
    for a, b in zip(before, replay()):
        same_bits(a, b)
    l0 = capi.launch_count()
    itb2, histb2, _ = G.solve_pCG_block(dU, dB)
    assert capi.launch_count() - l0 == launches_b and itb2 == itb
    same_bits(dU.get(), ub)
    for a, b in zip(histb, histb2):
        same_bits(a, b)


def test_refusals(capi):
    """8. every refused input is refused with its status and a message that names the cause, before X is written"""
    m, K, nev = gg.SHAPES[0]
    G, _ = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    B = op_of(gg.mass("lumped", m))
    lib, PD = capi.lib(), capi._PD
    lam = np.zeros(K)

    def raw(Bh, X=dX, K=K, nev=nev):
        return lib.sgpu_eigs_LOBPCG_gen(G.h, Bh, X.ptr, K, nev, 10, 1e-8, 1, lam.ctypes.data_as(PD), None, None, None, 0)
    assert raw(None) == -1 and "B is null" in lib.sgpu_last_error().decode()
    with pytest.raises(capi.SgpuError, match="both must have the same size"):
        solve(G, dX, nev, op_of(gg.mass("lumped", 16)))
    half = sp.identity(n, format="csr")
    coupled = sp.bmat([[2.0 * half, 0.1 * half], [0.1 * half, 2.0 * half]]).tocsr()
    Bh = op_of(coupled, nprocs=2, r=0)                                           # n rows, n local columns, and a halo plan
    assert raw(Bh.h) == -1 and "remote part or a halo plan" in lib.sgpu_last_error().decode()
    with pytest.raises(capi.SgpuError, match="B is not positive definite"):
        solve(G, dX, nev, op_of(-1.0 * half))
    assert raw(op_of(-1.0 * half).h) == -1                                       # SGPU_ERR_ARG
    with pytest.raises(capi.SgpuError, match="2, 4 or 8"):
        solve(G, _K3(dX), 1, B)
    for bad in (0, K + 1):
        with pytest.raises(capi.SgpuError, match="nev must be in 1..K"):
            solve(G, dX, bad, B)
    same_bits(dX.get(), X0)
    dep = X0.copy()
    dep[:, 2] = 2.0 * dep[:, 0] - dep[:, 1]
    dX.upload(dep)
    with pytest.raises(capi.SgpuError, match="linearly dependent"):
        solve(G, dX, nev, B)
    same_bits(dX.get(), dep)
    _, Gs, _ = one_level(capi, sr.tri(9), "direct")                              # 9 rows < 3 K
    with pytest.raises(capi.SgpuError, match="needs at least as many"):
        solve(Gs, Blk(capi, er.start_vectors(9, K)), nev, op_of(sp.identity(9, format="csr")))
    big = sr.case("tri", 1025)
    I_big = op_of(sp.identity(1025, format="csr"))
    _, Gb, _ = one_level(capi, big["A"], "CG")                                   # one more row than the LDS-resident coarsest solvers hold
    with pytest.raises(capi.SgpuError, match="host-driven CG"):
        solve(Gb, Blk(capi, er.start_vectors(1025, K)), nev, I_big)
    _, Gd, _ = one_level(capi, big["A"], "device_cg")                            # ... while coarse_solver = 2 is accepted
    lam_d, _, it_d, _, _ = solve(Gd, Blk(capi, er.start_vectors(1025, K)), nev, I_big, max_iter=2)
    assert it_d == 2 and np.all(np.isfinite(lam_d)) and np.all(lam_d > 0)
    dX.upload(X0)
    lam2, res2, it2, _, conv2 = solve(G, dX, nev, B, max_iter=2, tol=gg.TOL)
    assert not conv2 and it2 == 2
    assert np.all(np.isfinite(lam2)) and np.all(np.isfinite(res2)) and np.all(np.isfinite(dX.get())) and np.all(lam2 > 0)
    assert "above the tolerance" in lib.sgpu_last_error().decode()


@pytest.mark.parametrize("precond", (True, False), ids=("vcycle", "plain"))
def test_identity_mass_reproduces_the_standard_solve(capi, precond):
    """the standard and the generalised solve are one loop with a metric, so with B = I (the n x n identity as an operator) the
    generalised solve must reproduce the standard one bit for bit: after three iterations from the same start (tol = 0, so every
    column stays active in both and the factor ||(Bx)_j||^2 of the generalised test decides nothing; P is in use for two of the
    three) lambda, res, every column of the residual history, X and the solver's own AX, R, W, AW, P, AP are equal, and BX, BW, BP
    have the bits of X, W, P.  This rests on I v = v exactly, which fails only for an entry -0.0 (0 + 1 * -0.0 = +0.0): the start
    vectors hold none (np.signbit of their zeros, checked here on the host).

    Which W: a solve that ends at max_iter has formed W = M R of the next iteration before the norms came down (the loop's first
    step), while BW is still B times the W of the last completed iteration -- so at the return BX and BP are compared with X and P,
    and BW with the W a second pair of solves shows when stopped after the orthonormalisation of that last iteration
    (sgpu_debug_eig_stop, index 2), where all nine vectors are compared as well"""
    m, K, nev = er.SHAPES[0]
    G, _ = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    assert not np.any(np.signbit(X0) & (X0 == 0.0))
    B = op_of(sp.identity(n))
    names = ("AX", "R", "W", "AW", "P", "AP", "BX", "BW", "BP")

    def own(which):
        dV = Blk(capi, np.full((n, K), np.nan))
        G.debug_eig_vector(K, which, dV)
        return dV.get().copy()

    def run(Bh, stop):
        dX = Blk(capi, X0)
        if stop is not None:
            G.debug_eig_stop(K, stop)
        lam, res, it, hist, conv = G.lobpcg(dX, nev, max_iter=3, tol=0.0, precond=precond, B=Bh)
        msg = capi.lib().sgpu_last_error().decode()
        if stop is None:
            assert not conv and it == 3 and "above the tolerance after 3 iterations" in msg, msg
            assert all(len(h) == 4 for h in hist)
        else:
            assert not conv and it == stop and "stopped for inspection" in msg and "with P" in msg, msg
        return lam, res, hist, dX.get().copy(), [own(w) for w in range(6 if Bh is None else 9)]

    def compare(std, gen, what):
        (lam, res, hist, X, V), (lam_g, res_g, hist_g, X_g, V_g) = std, gen
        same_bits(lam_g, lam, what + "lambda"); same_bits(res_g, res, what + "res"); same_bits(X_g, X, what + "X")
        for j in range(K):
            same_bits(hist_g[j], hist[j], f"{what}history of column {j}")
        for w in range(6):
            same_bits(V_g[w], V[w], what + names[w])
    full, full_g = run(None, None), run(B, None)
    compare(full, full_g, "")
    stopped, stopped_g = run(None, 2), run(B, 2)
    compare(stopped, stopped_g, "stopped: ")
    X_g, V_g = full_g[3], full_g[4]
    Xs_g, Vs_g = stopped_g[3], stopped_g[4]
    same_bits(V_g[6], X_g, "BX"); same_bits(V_g[8], V_g[4], "BP")
    same_bits(V_g[7], Vs_g[2], "BW at the return, W of the last completed iteration")
    same_bits(Vs_g[6], Xs_g, "stopped: BX"); same_bits(Vs_g[7], Vs_g[2], "stopped: BW"); same_bits(Vs_g[8], Vs_g[4], "stopped: BP")
