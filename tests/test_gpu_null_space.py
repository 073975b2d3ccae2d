"""Hierarchies that know the constant null space (sgpu_amg_create_null_space, sgpu_vec_center, sgpu_block_center) on the GPU.

Operators, references, restatements and bounds come from tests/null_space_ref.py; tests/test_null_space_ref.py shows on the CPU that
the restatements stay inside every bound asserted here.  The hierarchies are the product's own host setup on neumann3d(8) (512 rows,
3 levels), neumann3d(16) (4 levels), wgrid(40, 5) (1 600 rows, 4 levels) and neumann3d(16) cut at one coarsening step ([4 096, 2 048]:
the smallest coarsest level past 1 024 rows, for the host-driven and the device CG).  Every test that uses a new entry point fails on
a library without it.
"""
import ctypes as C

import numpy as np
import pytest

from tests import eig_lock_ref as lr, hierarchy, null_space_ref as ns, solver_ref as sr
from tests.test_gpu_solver_layer import Padded, bits

pytestmark = pytest.mark.gpu

SMOOTHERS = ("jacobi", "chebyshev")


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def gpu_op(capi, A, diag=True):
    """an sgpu_op of a scipy matrix on one rank"""
    A = A.tocsr()
    A.sort_indices()
    return capi.Operator(M=A.shape[0], N_local=A.shape[1], col_offset=0, nnzPerRow_local=np.diff(A.indptr), col_local=A.indices,
                         val_local=A.data, inv_diag=1.0 / A.diagonal() if diag else None)


_ops = {}


def ops_of(capi, H):
    """the device operators of a hierarchy of null_space_ref, made once (the hierarchies that share them never change them)"""
    if id(H) not in _ops:
        _ops[id(H)] = (H, [gpu_op(capi, A) for A in H["A"]], [gpu_op(capi, P, False) for P in H["P"]], [gpu_op(capi, R, False) for R in H["R"]])
    return _ops[id(H)][1:]


def amg(capi, H, smoother="jacobi", coarse="direct", null_space="constant", A0=None, **kw):
    GA, GP, GR = ops_of(capi, H)
    if A0 is not None:
        GA = [A0] + GA[1:]
    kw.setdefault("max_iter", ns.MAX_ITER)
    return capi.Amg(GA, GP, GR, eig_max=H["eig"], smoother=smoother, coarse_solver=coarse, tol=ns.TOL, null_space=null_space, **kw)


def coarse_kinds(H):
    return ("direct", "cg", "device_cg") if H["A"][-1].shape[0] > sr.CG_MAXN else ("direct", "cg")


def check_solution(H, u, hist, conv, rhs, want, what):
    """the issue's four checks of a solve of A u = rhs - mean(rhs) against the restatement `want`"""
    A = H["A"][0]
    n = A.shape[0]
    bt = ns.center(rhs)[0]
    nb = np.linalg.norm(bt)
    res = sr.residual_hp(A, u, bt)
    x = solve_plus(H)
    err, mean = sr.rel(u, x * 1.0), abs(float(np.sum(u.astype(np.longdouble)) / n))
    print(f"{what}: {len(hist) - 1} iterations (restatement {want['iters']}), residual {res / nb:.2e} of {1.01 * ns.TOL:.2e}, error {err:.2e} of "
          f"{ns.error_bound(A):.2e}, |mean u| {mean:.1e} of {sr.dot_bound(u, np.ones(n)) / n:.1e}")
    assert conv and want["converged"]
    assert abs((len(hist) - 1) - want["iters"]) <= 1
    assert abs(hist[0] - nb) <= 1e-13 * nb                                  # res_hist[0] = ||rhs - mean(rhs)||
    assert res <= 1.01 * ns.TOL * nb
    assert err <= ns.error_bound(A)
    assert mean <= sr.dot_bound(u, np.ones(n)) / n


_plus = {}


def solve_plus(H):
    """A^+ rhs_for(n) of level 0, once per operator: rhs and rhs + 0.5 have the same centred right-hand side, so the same solution"""
    import hashlib
    key = hashlib.sha256(H["A"][0].indptr.tobytes() + H["A"][0].indices.tobytes() + H["A"][0].data.tobytes()).hexdigest()
    if key not in _plus:
        _plus[key] = ns.solve_plus(H["A"][0], ns.center(ns.rhs_for(H["A"][0].shape[0]))[0])[0]
    return _plus[key]


# ---------------------------------------------------------------------------
# kernels
def center_input(n, seed=0):
    return sr.dot_inputs(n, "normal", seed)[0] + (0.75 - 0.5 * seed)       # a mean of the entries' own size


@pytest.mark.parametrize("n", ns.CENTER_SIZES)
def test_vec_center(capi, n):
    """the restatement's bits, out of place and in place, twice; mean_host = S / n; nothing written behind n; x untouched"""
    x = center_input(n)
    want, mean = ns.center(x)
    dx, dy = Padded(capi, x), Padded(capi, np.full(n, np.nan))
    assert capi.vec_center(dx, dy) is None
    got = dy.head()
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(dx.head()), bits(x))
    m = capi.vec_center(dx, dy.upload(np.full(n, np.nan)), want_mean=True)
    assert np.array_equal(bits(dy.head()), bits(want)) and bits([m])[0] == bits([mean])[0]
    capi.vec_center(dx)                                                        # in place
    assert np.array_equal(bits(dx.head()), bits(want))


@pytest.mark.parametrize("K", (2, 4, 8))
@pytest.mark.parametrize("n", ns.CENTER_SIZES)
def test_block_center(capi, n, K):
    """column j has the bits of the scalar call on that column alone: the restatement per column; in place and out of place, twice"""
    X = np.stack([center_input(n, j) for j in range(K)], axis=1)
    want = np.stack([ns.center(X[:, j])[0] for j in range(K)], axis=1)
    dX, dY = capi.BlockVector(n, K, X), capi.BlockVector(n, K, np.full((n, K), np.nan))
    for _ in range(2):
        capi.block_center(dX, dY)
        assert np.array_equal(bits(dY.download()), bits(want))
    assert np.array_equal(bits(dX.download()), bits(X))
    dx = capi.DeviceVector(n, X[:, K - 1])
    capi.vec_center(dx)
    assert np.array_equal(bits(dx.download()), bits(want[:, K - 1]))            # the scalar call itself, on the card
    capi.block_center(dX)
    assert np.array_equal(bits(dX.download()), bits(want))


def test_center_refusals(capi):
    x = capi.DeviceVector(8, np.ones(8))
    for K in (1, 3, 16):
        with pytest.raises(capi.SgpuError, match="2, 4 or 8"):
            capi.check(capi.lib().sgpu_block_center(x.ptr, x.ptr, 1, K))
    with pytest.raises(capi.SgpuError, match="null argument"):
        capi.check(capi.lib().sgpu_vec_center(None, x.ptr, 8, None))
    off = C.c_void_p(x.ptr.value + 8)                                          # one double into the allocation: the block kernels move pairs
    for X, Y in ((off, x.ptr), (x.ptr, off)):
        with pytest.raises(capi.SgpuError, match="16-byte aligned"):
            capi.check(capi.lib().sgpu_block_center(X, Y, 2, 2))


# ---------------------------------------------------------------------------
# coarsest solves
@pytest.mark.parametrize("n", (65, 1024))
def test_path_one_level_direct(capi, n):
    """path(n) as a one-level hierarchy: sgpu_amg_create meets its exact zero pivot and refuses; with the null space known the stored
    pseudo-inverse solves it within the bound, for one column and for a block of 8"""
    A = ns.path(n)
    op = gpu_op(capi, A)
    with pytest.raises(capi.SgpuError, match="coarsest operator is singular"):
        capi.Amg([op], [], [], coarse_solver="direct")
    G = capi.Amg([op], [], [], coarse_solver="direct", null_space="constant")
    assert G.null_space == 1
    D = A.toarray()
    cond = float(np.linalg.cond(ns.shifted(D)[0]))
    bound = ns.pinv_bound(n, cond)
    rhs = ns.rhs_for(n)
    x, resid = ns.solve_plus(A, rhs)
    du, drhs = Padded(capi, np.full(n, np.nan)), capi.DeviceVector(n, rhs)
    l0 = capi.launch_count()
    assert G.coarsest_solve(du, drhs) == 0
    assert capi.launch_count() - l0 == 1                                        # k_dense_solve alone: no centring launch
    u = du.head()
    print(f"path({n}): cond of the shifted matrix {cond:.3e}, rel {sr.rel(u, x):.2e} of {bound:.2e} (reference residual {resid:.1e}), mean {np.mean(u):.1e}")
    assert sr.rel(u, x) <= bound
    K = 8
    RHS = np.stack([sr._COL_SCALE[j] * rhs + (0.1 * j if j != 1 else 0.0) for j in range(K)], axis=1)
    dU, dR = capi.BlockVector(n, K, np.full((n, K), np.nan)), capi.BlockVector(n, K, RHS)
    G.vcycle_block(dU, dR)
    Ub = dU.download()
    for j in range(K):
        if j == 1:
            assert not np.any(Ub[:, j])
            continue
        xj = ns.solve_plus(A, RHS[:, j])[0]
        assert sr.rel(Ub[:, j], xj) <= bound, j
    G.vcycle(du, capi.DeviceVector(n, RHS[:, 0]))
    assert np.array_equal(bits(Ub[:, 0]), bits(du.head()))                      # a block column has the bits of the scalar solve


@pytest.mark.parametrize("name,coarse", [("neumann8", "cg"), ("wgrid40", "cg"), ("neumann16cut", "cg"), ("neumann16cut", "device_cg"),
                                         ("neumann16cut", "direct")])
def test_coarsest_cg_on_an_uncentred_rhs(capi, name, coarse):
    """the coarsest operator of a hierarchy as a one-level hierarchy, its right-hand side with a mean: the CG solvers (LDS-resident,
    host-driven, device; the direct solver's fallback past 1 024 rows) stop below their cap, at the restatement's count +- 1, with
    the pseudo-inverse's solution; sgpu_amg_create's hierarchy runs to the cap on the same input"""
    Ac = ns.hierarchy(name)["A"][-1]
    n = Ac.shape[0]
    op = gpu_op(capi, Ac)
    rhs = ns.rhs_for(n) + 0.5
    u_w, it_w = sr.coarsest_cg(Ac, ns.center(rhs)[0])
    G = capi.Amg([op], [], [], coarse_solver=coarse, null_space="constant")
    du = Padded(capi, np.zeros(n))
    it = G.coarsest_solve(du, capi.DeviceVector(n, rhs))
    u = du.head()
    x = ns.solve_plus(Ac, rhs)[0]
    l2, lmax = ns.spectrum(Ac)
    print(f"{name} {coarse}: {n} rows, {it} iterations (restatement {it_w}, cap {sr.CG_MAX_ITER - 1}), rel {sr.rel(u, x):.2e}, mean {np.mean(u):.1e}")
    assert it < sr.CG_MAX_ITER - 1 and abs(it - it_w) <= 1
    assert sr.rel(u, u_w) <= 1e-11                                              # the contract of tests/test_gpu_solver_layer.py
    assert sr.rel(u, x) <= 2 * (lmax / l2) * sr.CG_TOL
    it0 = capi.Amg([op], [], [], coarse_solver=coarse).coarsest_solve(Padded(capi, np.zeros(n)), capi.DeviceVector(n, rhs))
    assert it0 == sr.CG_MAX_ITER - 1                                            # what the centring is for: kind 0 runs to the cap


# ---------------------------------------------------------------------------
# solvers
@pytest.mark.parametrize("smoother", SMOOTHERS)
@pytest.mark.parametrize("name", ns.SOLVE_HIERARCHIES)
def test_pcg(capi, name, smoother):
    """sgpu_solve_pCG on rhs and on rhs + 0.5, under every coarsest solver the hierarchy can take: the four checks; use_graph 0 and 1
    give the same bits"""
    H = ns.hierarchy(name)
    n = H["A"][0].shape[0]
    for coarse in coarse_kinds(H):
        G = amg(capi, H, smoother, coarse)
        G0 = amg(capi, H, smoother, coarse, use_graph=False)
        for shift in (0.0, 0.5):
            rhs = ns.rhs_for(n) + shift
            want = ns.pcg(H, rhs, smoother, coarse)
            du, drhs = Padded(capi, np.full(n, np.nan)), capi.DeviceVector(n, rhs)
            it, hist, conv = G.solve_pCG(du, drhs)
            u = du.head()
            check_solution(H, u, hist, conv, rhs, want, f"{name} {smoother} {coarse} +{shift}")
            assert np.array_equal(bits(drhs.download()), bits(rhs))             # the caller's right-hand side stays
            it0, hist0, conv0 = G0.solve_pCG(du, drhs)
            assert it0 == it and np.array_equal(bits(hist0), bits(hist)) and np.array_equal(bits(du.head()), bits(u))


@pytest.mark.parametrize("smoother", SMOOTHERS)
@pytest.mark.parametrize("name", ns.SOLVE_HIERARCHIES)
def test_the_other_solvers(capi, name, smoother):
    """sgpu_solve under every coarsest solver the hierarchy can take (the host-driven and the device CG past 1 024 rows included),
    sgpu_solve_CG and sgpu_solve_smoother, on rhs and rhs + 0.5: the same four checks, and for sgpu_solve -- whose captured V-cycle
    reads the hierarchy's own centred copy of rhs -- the same bits with use_graph 0 and 1.  The two without a coarse correction get
    the iterations they need"""
    H = ns.hierarchy(name)
    n = H["A"][0].shape[0]
    for coarse in coarse_kinds(H):
        for solver, max_iter in (("solve", ns.MAX_ITER), ("solve_CG", 400), ("solve_smoother", 2000)):
            if solver != "solve" and coarse != "direct":
                continue                                                        # (no coarsest solve in them)
            if solver == "solve_smoother" and name not in ns.SMOOTHER_HIERARCHIES:
                continue
            G = amg(capi, H, smoother, coarse, max_iter=max_iter)
            for shift in (0.0, 0.5):
                rhs = ns.rhs_for(n) + shift
                if solver == "solve":
                    want = ns.stationary(H, rhs, smoother, coarse)
                elif solver == "solve_CG":
                    want = ns.pcg(H, rhs, smoother, coarse, max_iter=max_iter, precond=False)
                else:
                    want = ns.stationary(H, rhs, smoother, coarse, max_iter=max_iter, with_coarse=False)
                du, drhs = Padded(capi, np.full(n, np.nan)), capi.DeviceVector(n, rhs)
                it, hist, conv = getattr(G, solver)(du, drhs)
                u = du.head()
                check_solution(H, u, hist, conv, rhs, want, f"{name} {smoother} {coarse} {solver} +{shift}")
                assert np.array_equal(bits(drhs.download()), bits(rhs))
                if solver == "solve":
                    it0, hist0, _ = amg(capi, H, smoother, coarse, max_iter=max_iter, use_graph=False).solve(du, drhs)
                    assert it0 == it and np.array_equal(bits(hist0), bits(hist)) and np.array_equal(bits(du.head()), bits(u))


@pytest.mark.parametrize("name,coarse,smoother", [("neumann8", "direct", "jacobi"), ("neumann8", "cg", "jacobi"), ("wgrid40", "direct", "jacobi"),
                                                  ("neumann16cut", "device_cg", "jacobi"), ("neumann8", "direct", "chebyshev"),
                                                  ("wgrid40", "cg", "chebyshev")])
def test_pcg_block_has_the_bits_of_scalar_solves(capi, name, coarse, smoother):
    """sgpu_solve_pCG_block at K = 4: column j has the bits (u, history, count) of sgpu_solve_pCG on that column.  On operators of
    their own with one lane per row in the scalar and in the block kernel: include/saena_gpu.h promises a block column the scalar
    entry point's bits where both add a row's products in sequence"""
    H = ns.hierarchy(name)
    n, K = H["A"][0].shape[0], 4
    GA, GP, GR = [gpu_op(capi, A) for A in H["A"]], [gpu_op(capi, P, False) for P in H["P"]], [gpu_op(capi, R, False) for R in H["R"]]
    for o in GA + GP + GR:
        o.set_lanes_per_row(1)
        o.set_block_lanes(1)
    G = capi.Amg(GA, GP, GR, eig_max=H["eig"], smoother=smoother, coarse_solver=coarse, max_iter=ns.MAX_ITER, tol=ns.TOL, null_space="constant")
    RHS = np.stack([c + 0.5 * (j % 2) for j, c in enumerate(sr.block_columns(n, K))], axis=1)
    dU, dR = capi.BlockVector(n, K, np.full((n, K), np.nan)), capi.BlockVector(n, K, RHS)
    its, hists, conv = G.solve_pCG_block(dU, dR)
    Ub = dU.download()
    assert conv
    for j in range(K):
        du = capi.DeviceVector(n)
        it, hist, cj = G.solve_pCG(du, capi.DeviceVector(n, RHS[:, j]))
        assert cj and it == its[j], (j, it, its[j])
        assert np.array_equal(bits(hist), bits(hists[j])), j
        assert np.array_equal(bits(du.download()), bits(Ub[:, j])), j


# ---------------------------------------------------------------------------
# refusals
def test_creation_refusals(capi):
    """a pinned row, null_space = 2: SGPU_ERR_ARG with the reason, and no hierarchy (no device memory) stays behind"""
    H = ns.hierarchy("neumann8")
    GA, GP, GR = ops_of(capi, H)
    pin0 = gpu_op(capi, ns.pinned(H["A"][0]))
    pinc = gpu_op(capi, ns.pinned(H["A"][-1]))
    pinp = gpu_op(capi, ns.pinned(ns.path(65)))
    before = capi.live_bytes()
    for coarse in ("direct", "cg"):
        with pytest.raises(capi.SgpuError, match=r"level 0 does not annihilate constants: max\|A 1\| / max\|a_ii\| = 1\.\d+e-01"):
            capi.Amg([pin0] + GA[1:], GP, GR, coarse_solver=coarse, null_space="constant")
        with pytest.raises(capi.SgpuError, match="level 2 does not annihilate constants"):
            capi.Amg(GA[:-1] + [pinc], GP, GR, coarse_solver=coarse, null_space="constant")
        with pytest.raises(capi.SgpuError, match="level 0 does not annihilate constants"):
            capi.Amg([pinp], [], [], coarse_solver=coarse, null_space="constant")
    for kind in (2, -1):
        with pytest.raises(capi.SgpuError, match="null_space is 0 .none. or 1 .constants."):
            capi.Amg(GA, GP, GR, null_space=kind)
    assert capi.live_bytes() == before
    # the pinned operators are what sgpu_amg_create is for
    G = capi.Amg([pinp], [], [], coarse_solver="direct")
    assert G.null_space == 0


TWO_RANK_WORKER = r"""
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import null_space_ref as ns
L = capi.lib()
XF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int)
AF = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)
xf, af = XF(lambda *a: 1), AF(lambda *a: 1)                 # never called: nothing is exchanged or reduced before the refusal
capi.check(L.sgpu_debug_init_host_transport(0, 0, 2, C.cast(xf, C.c_void_p), C.cast(af, C.c_void_p), None))
capi._initialised = True
A = ns.path(9)
op = capi.Operator(M=9, N_local=9, col_offset=0, nnzPerRow_local=np.diff(A.indptr), col_local=A.indices, val_local=A.data, inv_diag=1.0 / A.diagonal())
before = capi.live_bytes()
try:
    capi.Amg([op], [], [], null_space="constant")
    print("RESULT created")
except capi.SgpuError as e:
    print("RESULT", capi.live_bytes() - before, e)
x = capi.DeviceVector(9, np.ones(9))
print("CENTER", L.sgpu_vec_center(x.ptr, x.ptr, 9, None), L.sgpu_last_error().decode())
"""


def test_refused_in_a_context_of_two_ranks(capi):
    """a host-transport context of two ranks (its callbacks are never reached): creation with the null space is refused with "one
    rank" and leaves nothing behind; sgpu_vec_center too"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", TWO_RANK_WORKER % dict(root=root)], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    assert line.split()[1] == "0" and "status -1" in line and "one rank (this context has 2)" in line, line
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("CENTER ")][-1]
    assert line.split()[1] == "-1" and "one rank only" in line, line


def test_solver_refusals(capi):
    """FGMRES (symmetric solvers only) and the three unconstrained LOBPCG entry points (they name sgpu_eigs_LOBPCG_locked)"""
    H = ns.hierarchy("neumann8")
    n, K = H["A"][0].shape[0], 4
    G = amg(capi, H)
    du, drhs = capi.DeviceVector(n), capi.DeviceVector(n, ns.rhs_for(n))
    with pytest.raises(capi.SgpuError, match="symmetric solvers only"):
        G.solve_fgmres(du, drhs)
    dX = capi.BlockVector(n, K, lr.start_block(n, K)[0])
    with pytest.raises(capi.SgpuError, match="eigs_LOBPCG: .*sgpu_eigs_LOBPCG_locked"):
        G.lobpcg(dX, 2)
    with pytest.raises(capi.SgpuError, match="eigs_LOBPCG_gen: .*sgpu_eigs_LOBPCG_locked"):
        G.lobpcg(dX, 2, B=ops_of(capi, H)[0][0])
    with pytest.raises(capi.SgpuError, match="eigs_LOBPCG_many: .*sgpu_eigs_LOBPCG_locked"):
        G.lobpcg_many(n, 6, K)


# ---------------------------------------------------------------------------
# eigenpairs
def test_the_smallest_nonzero_eigenpairs(capi):
    """neumann3d(12, 8, 5): sgpu_eigs_LOBPCG_locked with the normalised constant vector locked, K = 4, nev = 3, within eig_lock_ref's
    iteration rule of the CPU restatement and at 2 - 2 cos(pi / 12), 2 - 2 cos(pi / 8) and their sum"""
    H = eig_hierarchy()
    A = H["A"][0]
    n, K, nev = A.shape[0], 4, 3
    G = amg(capi, H)
    q = np.full((n, 1), 1.0 / np.sqrt(n))
    X0 = lr.start_block(n, K)[0]
    want = eig_reference()
    dX, dQ = capi.BlockVector(n, K, X0), capi.DeviceVector(n, q[:, 0])
    lam, res, it, hist, conv, lead = G.lobpcg_locked(dX, nev, dQ, n, 1, tol=lr.TOL)
    exact = np.array([2 - 2 * np.cos(np.pi / 12), 2 - 2 * np.cos(np.pi / 8), 4 - 2 * np.cos(np.pi / 12) - 2 * np.cos(np.pi / 8)])
    print(f"{it} iterations (restatement {want['iters']}), lambda {lam[:nev]}, exact {exact}")
    assert conv and lead >= nev and want["converged"]
    assert it <= int(np.ceil(1.25 * want["iters"])) + 2
    assert np.max(np.abs(lam[:nev] - exact) / exact) <= 1e-9                    # tests/test_eig_lock_ref.py's tolerance for locked solves
    X = dX.download()
    assert np.max(np.abs(q.T @ X[:, :nev])) <= 1e-12


_eig = {}


def eig_hierarchy():
    if "H" not in _eig:
        _eig["H"] = ns.hierarchy("neumann12x8x5")
    return _eig["H"]


def eig_reference():
    if "ref" not in _eig:
        _eig["ref"] = ns.lobpcg_constant_locked(eig_hierarchy(), 4, 3)
    return _eig["ref"]


# ---------------------------------------------------------------------------
# sgpu_amg_set_operator
def test_set_operator(capi):
    """a rescaled Neumann operator is accepted on level 0 and on the coarsest level and solves; a pinned one is refused on either, and
    the hierarchy then solves with the bits it had before"""
    H = ns.hierarchy("neumann8")
    n = H["A"][0].shape[0]
    rhs = ns.rhs_for(n) + 0.5
    drhs = capi.DeviceVector(n, rhs)
    for coarse in ("direct", "cg"):
        G = amg(capi, H, "jacobi", coarse)
        du = capi.DeviceVector(n)
        it, hist, conv = G.solve_pCG(du, drhs)
        u = du.download()
        for level in (0, len(H["A"]) - 1):
            bad = gpu_op(capi, ns.pinned(H["A"][level]))
            with pytest.raises(capi.SgpuError, match=f"sgpu_amg_set_operator: the operator of level {level} does not annihilate constants"):
                G.set_operator(level, bad)
            it2, hist2, conv2 = G.solve_pCG(du, drhs)
            assert conv2 and it2 == it and np.array_equal(bits(hist2), bits(hist)) and np.array_equal(bits(du.download()), bits(u))
        # twice the operator on every level: the same problem scaled, half the solution
        fresh = [gpu_op(capi, 2.0 * A) for A in H["A"]]
        for level in (len(H["A"]) - 1, 1, 0):
            G.set_operator(level, fresh[level], H["eig"][level])
        it3, hist3, conv3 = G.solve_pCG(du, drhs)
        assert conv3 and it3 == it
        assert sr.rel(2.0 * du.download(), u) <= 1e-12
        G.destroy()


# ---------------------------------------------------------------------------
# the unchanged path
def test_kind_zero_is_sgpu_amg_create(capi):
    """the Dirichlet Poisson hierarchy of tests/hierarchy.py: sgpu_amg_create_null_space(..., 0, ...) and sgpu_amg_create give the same
    bits of u and res_hist and the same launch counts, for sgpu_solve_pCG and sgpu_solve_pCG_block; kind 0 launches no centring"""
    As, Ps, Rs = hierarchy.poisson_hierarchy(10, 2)
    n, K = As[0].shape[0], 4
    GA, GP, GR = [gpu_op(capi, A) for A in As], [gpu_op(capi, P, False) for P in Ps], [gpu_op(capi, R, False) for R in Rs]
    rhs = ns.rhs_for(n)
    RHS = np.stack(sr.block_columns(n, K), axis=1)
    out = []
    for null_space in (None, "none", 0):
        G = capi.Amg(GA, GP, GR, smoother="jacobi", max_iter=60, tol=1e-8, null_space=null_space)
        assert G.null_space == 0
        du, drhs = capi.DeviceVector(n), capi.DeviceVector(n, rhs)
        dU, dR = capi.BlockVector(n, K), capi.BlockVector(n, K, RHS)
        G.solve_pCG(du, drhs); G.solve_pCG_block(dU, dR)                        # (the captures and the block work space: outside the count)
        l0 = capi.launch_count()
        it, hist, conv = G.solve_pCG(du, drhs)
        l1 = capi.launch_count()
        its, hists, convb = G.solve_pCG_block(dU, dR)
        l2 = capi.launch_count()
        assert conv and convb
        out.append((it, hist, du.download(), l1 - l0, its, np.concatenate(hists), dU.download(), l2 - l1))
        G.destroy()
    for o in out[1:]:
        for a, b in zip(out[0], o):
            assert np.array_equal(bits(np.asarray(a, np.float64)), bits(np.asarray(b, np.float64)))
