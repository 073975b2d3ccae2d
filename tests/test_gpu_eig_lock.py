"""sgpu_eigs_LOBPCG_locked and sgpu_eigs_LOBPCG_many on the GPU -- more than K eigenpairs by locking converged vectors -- held to a
written contract.

Hierarchies are those of tests/test_gpu_eig.py (8^3 rows in two levels, 16^3 in three; Jacobi 3 + 3, direct coarsest solve), the mass
matrices those of tests/geig_ref.py.  The shapes, the numpy reference's total iterations, sweeps and B-orthonormality and every bound
come from tests/eig_lock_ref.py; tests/test_eig_lock_ref.py shows on the CPU that a correct implementation stays inside each of them.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import eig_lock_ref as lr, eig_ref as er, geig_ref as gg, hierarchy, solver_ref as sr
from tests.test_gpu_block_solver_layer import Blk, same_bits
from tests.test_gpu_eig import gpu
from tests.test_gpu_geig import op_of
from tests.test_gpu_solver_layer import bits, one_level
from tests.test_gpu_vcycle import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def mass_op(shape):
    """-> (scipy B or None, device operator or None)"""
    (m, K, nev, sweep_nev), mass = shape
    if not mass:
        return None, None
    Bs = gg.mass(mass, m)
    return Bs, op_of(Bs)


def columns(capi, Q, ld):
    """an (n, L) host array as L column-major device columns of leading dimension ld, NaN in the padding rows"""
    n, L = Q.shape
    a = np.full((max(1, L), ld), np.nan)
    a[:L, :n] = Q.T
    return capi.DeviceVector(a.size, a.ravel())


@pytest.mark.parametrize("shape", lr.SHAPES, ids=str)
def test_many(capi, shape):
    """1. and 2. both assertions of check_pairs on ALL nev pairs, the residual recomputed here in longdouble from the returned Q (a
    missed or repeated eigenvalue fails 2); lambda ascending; 3. max |Q^T B Q - I| <= 16 x the reference's; 4. total iterations <=
    ceil(1.25 x the reference's total) + 2 per sweep of the reference.  Also: the reported residuals are the recomputed ones, the
    padding rows of Q are not written, a second run reproduces every bit"""
    (m, K, nev, sweep_nev), mass = shape
    G, A = gpu(capi, m)
    Bs, B = mass_op(shape)
    n = m ** 3
    lam, res, Q, it, sweeps, conv = G.lobpcg_many(n, nev, K, sweep_nev, B=B, max_iter=lr.MAX_ITER, tol=lr.TOL, ld=n + 6, nan_padding=True)
    defect = lr.ortho_defect(shape, Q)
    print(f"{shape}: {it} iterations in {sweeps} sweeps (reference {lr.ITERS[shape]} in {lr.SWEEPS[shape]}, bound {lr.iteration_bound(shape)}), "
          f"max |Q^T B Q - I| = {defect:.3e} (reference {lr.ORTHO[shape]:.1e}, bound {lr.ORTHO_MARGIN * lr.ORTHO[shape]:.1e})")
    assert conv and Q.shape == (n, nev) and len(lam) == nev
    rhos = lr.check_pairs(shape, Q, lam, A=A)                                       # 1 and 2
    assert np.all(np.diff(lam) >= 0.0) and np.all(np.isfinite(lam)) and np.all(np.isfinite(Q))
    assert defect <= lr.ORTHO_MARGIN * lr.ORTHO[shape]                            # 3
    assert it <= lr.iteration_bound(shape)                                        # 4
    for j in range(nev):
        x = Q[:, j]
        scale = np.linalg.norm(Bs @ x) if mass else np.linalg.norm(x)
        assert res[j] < lr.TOL * lam[j] * scale
        assert abs(res[j] - rhos[j] * scale) <= 1e-3 * res[j] + 1e-12 * lam[j]
    lam2, res2, Q2, it2, sweeps2, conv2 = G.lobpcg_many(n, nev, K, sweep_nev, B=B, max_iter=lr.MAX_ITER, tol=lr.TOL)
    assert conv2 and (it2, sweeps2) == (it, sweeps)
    same_bits(lam2, lam); same_bits(res2, res); same_bits(Q2, Q)


def test_many_padding_rows_and_start_vectors(capi):
    """the rows n .. ld-1 of every column of Q are the caller's: what they held stays; start vectors given by the caller are used
    (another start, the same pairs) and left as they were; sweep_nev = 0 is K / 2"""
    shape = lr.SHAPES[1]
    (m, K, nev, sweep_nev), _ = shape
    G, A = gpu(capi, m)
    n, ld = m ** 3, m ** 3 + 6
    dQ = capi.DeviceVector(nev * ld)
    dQ.fill(-7.5)
    import ctypes as C
    X0 = er.start_vectors(n, K)
    dX0 = Blk(capi, X0)
    lam, res = np.zeros(nev), np.zeros(nev)
    it, nl, sw = C.c_int(), C.c_int(), C.c_int()
    capi.check(capi.lib().sgpu_eigs_LOBPCG_many(G.h, None, dQ.ptr, ld, nev, K, 0, dX0.ptr, lr.MAX_ITER, lr.TOL, 1, lam.ctypes.data_as(capi._PD),
                                                res.ctypes.data_as(capi._PD), C.byref(it), C.byref(nl), C.byref(sw)))
    got = dQ.download().reshape(nev, ld)
    assert nl.value == nev and np.all(got[:, n:] == -7.5)
    same_bits(dX0.get(), X0)
    lr.check_pairs(shape, got[:, :n].T.copy(), lam, A=A, what="start vectors given")
    lam_d, _, _, it_d, sw_d, conv_d = G.lobpcg_many(n, nev, K, K // 2, X0=dX0, max_iter=lr.MAX_ITER, tol=lr.TOL)
    assert conv_d and (it_d, sw_d) == (it.value, sw.value)
    same_bits(lam_d, lam)


@pytest.mark.parametrize("mass", (None,) + gg.MASSES)
def test_nlocked_0_gives_the_bits_of_the_unconstrained_solves(capi, mass):
    """sgpu_eigs_LOBPCG_locked with nlocked = 0: X, lambda, res, iters and the history have the bits of sgpu_eigs_LOBPCG (B = NULL) and
    sgpu_eigs_LOBPCG_gen; it costs the same number of launches -- neither lock kernel is launched --, and `leading` counts the
    converged leading columns"""
    shape = er.SHAPES[0]
    m, K, nev = shape
    G, A = gpu(capi, m)
    n = m ** 3
    B = op_of(gg.mass(mass, m)) if mass else None
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    G.lobpcg(dX, nev, tol=er.TOL, B=B)                                             # (captures the V-cycle: both counted runs replay it)
    dX.upload(X0)
    l0 = capi.launch_count()
    lam, res, it, hist, conv = G.lobpcg(dX, nev, tol=er.TOL, B=B)
    launches = capi.launch_count() - l0
    X = dX.get().copy()
    dX.upload(X0)
    l0 = capi.launch_count()
    lam2, res2, it2, hist2, conv2, lead = G.lobpcg_locked(dX, nev, None, n, 0, B=B, tol=er.TOL)
    launches2 = capi.launch_count() - l0
    assert conv and conv2 and it2 == it and lead >= nev
    same_bits(lam2, lam); same_bits(res2, res); same_bits(dX.get(), X)
    for a, b in zip(hist, hist2):
        same_bits(a, b)
    assert launches2 == launches, (launches, launches2)
    # with one locked column the same solve costs more launches: per projection one Gram pass, the reduce and the projection
    x0 = X[:, :1].copy()
    dQ = columns(capi, x0, n)
    dBQ = columns(capi, gg.mass(mass, m) @ x0, n) if mass else None
    dX.upload(X0)
    l0 = capi.launch_count()
    _, _, it3, _, conv3, _ = G.lobpcg_locked(dX, nev, dQ, n, 1, BQ=dBQ, B=B, tol=er.TOL, max_iter=3)
    dX.upload(X0)
    l1 = capi.launch_count()
    G.lobpcg_locked(dX, nev, None, n, 0, B=B, tol=er.TOL, max_iter=3)
    l2 = capi.launch_count()
    # 2 projections of X, then one of W per pass of the loop: iterations 0, 1, 2 and the pass that finds max_iter reached (W = M R is
    # formed before the norms come down); each is one Gram pass, the reduce and the projection
    assert it3 == 3 and not conv3 and (l1 - l0) - (l2 - l1) == 3 * (2 + 4), (l1 - l0, l2 - l1)


@pytest.mark.parametrize("mass", (None, "mass27"))
def test_locked_exact_vectors_give_the_next_pairs(capi, mass):
    """with the exact eigenvectors of the 4 smallest eigenvalues locked (the cluster 1 + 3: products of sines, B-normalised), a
    constrained solve for 4 pairs returns pairs 5 to 8, B-orthogonal to the locked set"""
    m, K, nev = 8, 8, 4
    shape = ((m, K, 8, 4), mass)
    G, A = gpu(capi, m)
    n = m ** 3
    Bs, B = mass_op(shape)
    s = [np.sin(np.pi * k * np.arange(1, m + 1) / (m + 1.0)) for k in (1, 2)]
    Q = np.stack([np.kron(np.kron(s[a], s[b]), s[c]) for a, b, c in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))], axis=1)
    BQ = Bs @ Q if mass else Q
    Q = Q / np.sqrt(np.sum(Q * BQ, axis=0))[None, :]
    BQ = Bs @ Q if mass else Q
    assert np.max(np.abs(Q.T @ BQ - np.eye(4))) <= 1e-14
    ld = n + 6
    dQ, dBQ = columns(capi, Q, ld), (columns(capi, BQ, ld) if mass else None)
    dX = Blk(capi, er.start_vectors(n, K))
    lam, res, it, hist, conv, lead = G.lobpcg_locked(dX, nev, dQ, ld, 4, BQ=dBQ, B=B, tol=lr.TOL)
    X = dX.get()
    want = lr.exact(shape)
    print(f"{mass}: {it} iterations, lambda {lam[:nev]}, want {want[4:8]}, max |Q^T B X| = {np.max(np.abs(BQ.T @ X)):.2e}")
    assert conv and lead >= nev
    assert np.max(np.abs(BQ.T @ X)) <= 1e-13
    for j in range(nev):
        if mass:
            rho, rounding, nbx = gg.residual_hp(A, Bs, X[:, j], lam[j])
            bound = rho * nbx / np.sqrt(gg.LAMBDA_MIN_B[mass])
        else:
            rho, rounding = er.residual_hp(A, X[:, j], lam[j])
            bound = rho
        assert rho <= lr.TOL * lam[j] + rounding
        assert abs(lam[j] - want[4 + j]) <= bound, (j, lam[j], want[4 + j])


@pytest.fixture(scope="module")
def poisson():
    return hierarchy.poisson_hierarchy(18, 4)      # the hierarchy of tests/test_gpu_vcycle.py: 4096 -> 512 -> 64 -> 8 rows


def test_many_leaves_block_pcg_the_scalar_solve_and_lobpcg_alone(capi, poisson):
    """block pCG's cached graphs (its own pair and seven more captured V-cycles), the scalar sgpu_solve_pCG and a following
    sgpu_eigs_LOBPCG are bit-identical before and after a `many` call with the same K: each cached V-cycle still replays as one
    launch, block pCG and LOBPCG cost the launches they cost before (no graph was evicted or recaptured)"""
    K = 4
    _, G, (OA, _, _), _ = build(capi, poisson, "jacobi")
    n = OA[0].Mbig
    rhs = orc.laplacian3d_rhs(18)
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, rhs)
    it0, hist0, _ = G.solve_pCG(du, dr)
    u0 = du.download()
    Bm = np.stack([rhs * (1 + j) for j in range(K)], axis=1)
    dU, dB = Blk(capi, np.zeros((n, K))), Blk(capi, Bm)
    G.solve_pCG_block(dU, dB)
    l0 = capi.launch_count()
    itb, histb, _ = G.solve_pCG_block(dU, dB)
    launches_b = capi.launch_count() - l0
    ub = dU.get().copy()
    pairs = [(Blk(capi, np.zeros((n, K))), Blk(capi, Bm * (2 + i))) for i in range(7)]
    for u, r in pairs:
        G.vcycle_block(u, r)

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
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    G.lobpcg(dX, K, tol=er.TOL)                                                # captures LOBPCG's V-cycle
    dX.upload(X0)
    l0 = capi.launch_count()
    lam, res, it, hist, conv = G.lobpcg(dX, K, tol=er.TOL)
    launches_e = capi.launch_count() - l0
    Xe = dX.get().copy()
    lam_m, _, Q, it_m, sweeps, conv_m = G.lobpcg_many(n, 10, K, 2, max_iter=lr.MAX_ITER, tol=er.TOL)
    assert conv and conv_m and sweeps >= 3 and Q.shape == (n, 10)
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
    dX.upload(X0)
    l0 = capi.launch_count()
    lam2, res2, it2, hist2, conv2 = G.lobpcg(dX, K, tol=er.TOL)
    assert capi.launch_count() - l0 == launches_e and it2 == it and conv2
    same_bits(lam2, lam); same_bits(res2, res); same_bits(dX.get(), Xe)


def test_a_small_max_iter_returns_the_pairs_locked_so_far(capi):
    """max_iter bounds the TOTAL over the sweeps: SGPU_ERR_NOCONV with 0 < nlocked < nev, the locked pairs valid (both assertions of
    check_pairs) and ascending, iters <= max_iter"""
    shape = lr.SHAPES[0]
    (m, K, nev, sweep_nev), _ = shape
    G, A = gpu(capi, m)
    n = m ** 3
    budget = lr.ITERS[shape] // 2
    lam, res, Q, it, sweeps, conv = G.lobpcg_many(n, nev, K, sweep_nev, max_iter=budget, tol=lr.TOL)
    msg = capi.lib().sgpu_last_error().decode()
    print(f"max_iter {budget}: {len(lam)} of {nev} pairs in {it} iterations, {sweeps} sweeps: {msg}")
    assert not conv and 0 < len(lam) < nev and Q.shape == (n, len(lam)) and it <= budget
    assert "above the tolerance" in msg
    assert np.all(np.diff(lam) >= 0.0)
    lr.check_pairs(shape, Q, lam, nev=len(lam), A=A, what="locked so far")
    assert er.ortho_defect(Q) <= lr.ORTHO_MARGIN * lr.ORTHO[shape]


def test_refusals(capi):
    """every refused input is refused with a message before anything is launched or written"""
    import ctypes as C
    m, K, nev = er.SHAPES[0]
    G, _ = gpu(capi, m)
    n = m ** 3
    X0 = er.start_vectors(n, K)
    dX = Blk(capi, X0)
    q = capi.DeviceVector(64 * (n + 2))
    Bop = op_of(gg.mass("lumped", m))
    _, Gs, _ = one_level(capi, sr.tri(40), "direct")                          # 40 rows: 3 K = 12 fit, 29 locked + 12 do not
    qs, dXs = capi.DeviceVector(64 * 40), Blk(capi, er.start_vectors(40, K))
    l0 = capi.launch_count()
    for kw, msg in ((dict(Q=q, ld=n, nlocked=-1), "nlocked must be in 0..64"), (dict(Q=q, ld=n, nlocked=65), "nlocked must be in 0..64"),
                    (dict(Q=q, ld=n - 2, nlocked=1), "ld must be even"), (dict(Q=q, ld=n + 1, nlocked=1), "ld must be even"),
                    (dict(Q=None, ld=n, nlocked=1), "Q is null"), (dict(Q=q, ld=n, nlocked=1, B=Bop), "BQ is null"),
                    (dict(Q=q, ld=n, nlocked=0, nev=K + 1), "nev must be in 1..K")):
        kw = dict(kw)
        want_nev = kw.pop("nev", nev)
        with pytest.raises(capi.SgpuError, match=msg):
            G.lobpcg_locked(dX, want_nev, **kw)
    with pytest.raises(capi.SgpuError, match="need at least 41"):
        Gs.lobpcg_locked(dXs, nev, Q=qs, ld=40, nlocked=29)
    for args, msg in (((n, 0, K), "nev must be in 1..64"), ((n, 65, K), "nev must be in 1..64"), ((n, 4, 3), "2, 4 or 8")):
        with pytest.raises(capi.SgpuError, match=msg):
            G.lobpcg_many(*args)
    with pytest.raises(capi.SgpuError, match="sweep_nev must be in 1..K"):
        G.lobpcg_many(n, 4, K, K + 1)
    with pytest.raises(capi.SgpuError, match="ld must be even"):
        G.lobpcg_many(n, 4, K, ld=n + 1)
    with pytest.raises(capi.SgpuError, match="need at least"):
        Gs.lobpcg_many(40, 29, K)
    lam = np.zeros(4)
    with pytest.raises(capi.SgpuError, match="null argument"):
        capi.check(capi.lib().sgpu_eigs_LOBPCG_many(G.h, None, None, n, 4, K, 0, None, 10, 1e-8, 1, lam.ctypes.data_as(capi._PD), None, None, None, None))
    assert capi.launch_count() == l0
    same_bits(dX.get(), X0)
