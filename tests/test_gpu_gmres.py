"""sgpu_solve_FGMRES and its two Gram-Schmidt kernels on the GPU, held to a written contract.

Inputs, references and bounds come from tests/gmres_ref.py and tests/solver_ref.py; tests/test_gmres_ref.py shows on the CPU that a
correct implementation stays inside every bound asserted here.  The kernels are reached through sgpu_debug_gs_dots / _gs_update,
which run the solver's own launch helpers (their chunks of 8 columns, their grid) on the caller's arrays.

Which paths run where:
  * rows are walked in pairs (16-byte accesses), thread 0 of block 0 takes the last row of an odd n: n = 1, 2, 3 and every odd n;
    with an odd n the leading dimension is n + 1 and the row of padding holds a NaN, which an access past n would pick up;
  * at most 1024 blocks of 256 pairs: rows >= 524288 send the kernels on a second grid-stride trip (GS_WRAP + 5, 1048576, ...);
  * 8 columns per pass: 1, 7, 8 columns are one pass, 9 two, 17 three, 65 nine (the most a solve with restart 64 asks for).
Columns 8 .. 64 of V are columns 0 .. 7 scaled by signed powers of two: scaling by a power of two commutes with every rounding, so
their coefficients are known bit for bit from the first eight, and the host holds eight columns whatever n is.
"""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as orc
from tests import gmres_ref as gr, hierarchy, solver_ref as sr, util
from tests.test_gpu_solver_layer import SENTINEL, Padded, bits, one_level
from tests.test_gpu_vcycle import build

pytestmark = pytest.mark.gpu

NCOLS = (1, gr.GS_C - 1, gr.GS_C, gr.GS_C + 1, 2 * gr.GS_C + 1, 65)
SIZES = sr.vec_sizes() + (gr.GS_WRAP + 5,)
SCALE = np.array([(-1.0) ** (c // 8) * 2.0 ** ((c // 8) % 5 - 2) if c >= 8 else 1.0 for c in range(65)])
TOL = 1e-8


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


class At:
    """a device pointer `offset` doubles into a DeviceVector"""

    def __init__(self, vec, offset):
        self.ptr = C.c_void_p(vec.ptr.value + 8 * offset)


def upload_at(capi, vec, offset, host):
    host = np.ascontiguousarray(host, np.float64)
    capi.check(capi.lib().sgpu_vec_upload(At(vec, offset).ptr, host.ctypes.data, host.size))


class Basis:
    """65 columns of n rows on the device, leading dimension n rounded up to even; column c = base[:, c % 8] * SCALE[c]; the row of
    padding of an odd n holds the sentinel NaN"""

    def __init__(self, capi, n):
        self.capi, self.n, self.ld = capi, n, max(2, (n + 1) & ~1)
        self.d = capi.DeviceVector(self.ld * 65)
        self.ptr = self.d.ptr

    def upload(self, base):
        self.base = base
        col = np.full(self.ld, SENTINEL)
        for c in range(65):
            col[:self.n] = self.column(c)
            upload_at(self.capi, self.d, c * self.ld, col)
        return self

    def column(self, c):
        return self.base[:, c % 8] * SCALE[c]


def dot_case(n, kind):
    """-> (base (n, 8), w): dot_inputs' x of seed c as column c, its y of seed 0 as w (with `cancelling`, every column's second
    half-block undoes the first against w)"""
    base = np.stack([sr.dot_inputs(n, kind, seed=c)[0] for c in range(8)], axis=1) if n else np.zeros((0, 8))
    return base, (sr.dot_inputs(n, kind, seed=0)[1] if n else np.zeros(0))


# ---------------------------------------------------------------------------
# the kernels
@pytest.mark.parametrize("n", SIZES)
def test_gs_dots(capi, n):
    """every coefficient within gs_dot_bound of the longdouble dot; a second run gives the same bits; a column's coefficient does
    not depend on how many columns ride with it, nor on the chunk it falls in"""
    V, dw = Basis(capi, n), Padded(capi, np.zeros(n))
    for kind in ("normal", "positive", "cancelling"):
        base, w = dot_case(n, kind)
        V.upload(base); dw.upload(w)
        full = capi.gs_dots(V, V.ld, 65, dw, n)
        assert np.array_equal(bits(full), bits(capi.gs_dots(V, V.ld, 65, dw, n))), "not reproducible"
        worst = 0.0
        for c in range(8):
            ref, bound = sr.dot_hp(base[:, c], w), gr.gs_dot_bound(base[:, c], w)
            err = abs(float(np.longdouble(full[c]) - ref))
            worst = max(worst, err / bound if bound else 0.0)
            assert err <= bound, (kind, c, err, bound)
        print(f"n={n} {kind}: worst error / bound {worst:.3f}; column 0 equals the numpy restatement of the order: {full[0] == gr.gs_dot_blocked(base[:, 0], w)}")
        scaled = full[np.arange(65) % 8] * SCALE + 0.0                        # (+ 0.0: a sum that is exactly zero is +0 under any scaling)
        assert np.array_equal(bits(full), bits(scaled)), "a column's coefficient depends on its chunk"
        for k in NCOLS[:-1]:
            assert np.array_equal(bits(capi.gs_dots(V, V.ld, k, dw, n)), bits(full[:k])), (kind, k)
        single = capi.gs_dots(At(V.d, 9 * V.ld), V.ld, 1, dw, n)             # column 9 alone, first of its pass
        assert bits(single)[0] == bits(full[9:10])[0]
        dw.head()                                                             # (the sentinel behind w is intact)


@pytest.mark.parametrize("n", SIZES)
def test_gs_update(capi, n):
    """w bit for bit the numpy restatement (ascending columns, product rounded, then subtracted) for every column count; the fused
    norm within the dot bound of the new w; nothing written behind w"""
    base, w = dot_case(n, "normal")
    V, dw = Basis(capi, n).upload(base), Padded(capi, w)
    h = np.random.default_rng(77).standard_normal(65)
    want, done = w.copy(), 0
    for k in NCOLS:                                                           # ascending: the running value continues
        for c in range(done, k):
            want = want - h[c] * V.column(c)
        done = k
        dw.upload(w)
        nrm = capi.gs_update(V, V.ld, k, h[:k], dw, n, norm=True)
        got = dw.head()
        assert np.array_equal(bits(got), bits(want)), (k, int(np.sum(bits(got) != bits(want))))
        err = abs(float(np.longdouble(nrm) - sr.dot_hp(want, want)))
        assert err <= gr.gs_dot_bound(want, want), (k, err)
        dw.upload(w)
        assert capi.gs_update(V, V.ld, k, h[:k], dw, n, norm=False) is None
        assert np.array_equal(bits(dw.head()), bits(want)), k
    # the negated coefficients of u += Z y: the same bits as adding
    dw.upload(w)
    capi.gs_update(V, V.ld, 9, -h[:9], dw, n)
    want = w.copy()
    for c in range(9):
        want = want + h[c] * V.column(c)
    assert np.array_equal(bits(dw.head()), bits(want))


def test_gs_entry_points_refuse_what_the_kernels_cannot_take(capi):
    V, w = capi.DeviceVector(64), capi.DeviceVector(8)
    out = np.zeros(66)
    for args, msg in (((V.ptr, 7, 2, w.ptr, 7), "even"), ((V.ptr, 6, 2, w.ptr, 7), "at least n"), ((V.ptr, 8, 66, w.ptr, 7), "65"),
                      ((At(V, 1).ptr, 8, 2, w.ptr, 7), "aligned"), ((V.ptr, 8, 2, At(w, 1).ptr, 7), "aligned")):
        with pytest.raises(capi.SgpuError, match=msg):
            capi.check(capi.lib().sgpu_debug_gs_dots(*args, out.ctypes.data_as(C.POINTER(C.c_double))))


# ---------------------------------------------------------------------------
# the solver
def gpu_hierarchy(capi, c, smoother="jacobi", max_iter=100, tol=TOL, coarse_solver="direct"):
    OA, OP, OR = hierarchy.oracle_hierarchy(c["As"], c["Ps"], c["Rs"])
    eig = hierarchy.eig_estimates(c["As"])
    ops = [[util.gpu_operator(o) for o in L] for L in (OA, OP, OR)]
    G = capi.Amg(*ops, eig_max=eig, pre=3, post=3, smoother=smoother, max_iter=max_iter, tol=tol, coarse_solver=coarse_solver)
    return G, ops


def check_against(ref, it, hist, u, what):
    """the contract: the reference's iteration count (or one off it where the reference's deciding estimate sits on the threshold
    within the history bound), every estimate within 1e-10 ||r_0|| of the reference's and within 1e-6 of its own size, the solution
    to 1e-9"""
    rh = ref["hist"]
    m = min(len(hist), len(rh))
    d = np.abs(hist[:m] - rh[:m])
    print(f"{what}: iterations {it} (reference {ref['iters']}, {ref['restarts']} restarts), max |hist - ref| / r0 = {d.max() / rh[0]:.3e}, "
          f"/ own size = {(d / rh[:m]).max():.3e}, rel-l2 of u {sr.rel(u, ref['u']):.3e}")
    if it != ref["iters"]:
        k = min(it, ref["iters"])
        assert abs(it - ref["iters"]) == 1 and abs(rh[k] - TOL * rh[0]) <= gr.TOL_HIST * rh[0] + 1e-6 * rh[k], (what, it, ref["iters"])
    assert len(hist) == it + 1
    assert gr.hist_within(hist, rh), (what, hist, rh)
    assert sr.rel(u, ref["u"]) <= 1e-9, what


@pytest.mark.parametrize("restart", [5, 30])
def test_fgmres_without_a_preconditioner(capi, restart):
    c = gr.case(8, 4.0)
    n = c["A"].shape[0]
    G, _ = gpu_hierarchy(capi, c, max_iter=400)
    du, dr = Padded(capi, np.ones(n)), capi.DeviceVector(n, c["rhs"])
    it, hist, conv, true_res = G.solve_fgmres(du, dr, restart=restart, precond=False)
    ref = gr.fgmres(c["A"], c["rhs"], restart, tol=TOL, max_iter=400, dot=gr.gs_dot_blocked)
    assert conv and ref["converged"]
    check_against(ref, it, hist, du.head(), f"GMRES({restart})")
    assert ref["restarts"] == (7 if restart == 5 else 0)


@pytest.mark.parametrize("restart", [5, 30])
@pytest.mark.parametrize("n,pe", [(14, 4.0), (8, 1.0)])
def test_fgmres_preconditioned(capi, n, pe, restart):
    """the reference's preconditioner is the GPU's own V-cycle on a zero iterate: only the new code differs between the two sides.
    Independently of any reference: the residual recomputed on the host is below the tolerance and is what the solve reports, and
    the estimates do not increase within a cycle"""
    c = gr.case(n, pe)
    N = c["A"].shape[0]
    G, _ = gpu_hierarchy(capi, c)
    dz, dv = capi.DeviceVector(N), capi.DeviceVector(N)

    def M(v):
        dv.upload(v); dz.fill(0.0)
        G.vcycle(dz, dv)
        return dz.download()

    du, dr = Padded(capi, np.ones(N)), capi.DeviceVector(N, c["rhs"])
    it, hist, conv, true_res = G.solve_fgmres(du, dr, restart=restart)
    u = du.head()
    ref = gr.fgmres(c["A"], c["rhs"], restart, tol=TOL, precond=M, dot=gr.gs_dot_blocked)
    assert conv and ref["converged"]
    check_against(ref, it, hist, u, f"convdiff({n}, {pe}) FGMRES({restart})")
    assert ref["restarts"] == (1 if restart == 5 else 0)                     # restart 5: a restart happens
    res = sr.residual_hp(c["A"], u, c["rhs"])
    print(f"recomputed residual {res:.6e}, reported {true_res:.6e}, last estimate {hist[-1]:.6e}, tolerance {TOL * hist[0]:.6e}")
    assert res <= TOL * hist[0] * (1 + 1e-6)
    assert abs(res - true_res) <= 1e-6 * res
    assert gr.monotone_within_cycles(hist, restart, 1e-12)
    it2, hist2, _, _ = G.solve_fgmres(du, dr, restart=restart)               # the graph replayed, the work space reused: the same bits
    assert it2 == it and np.array_equal(bits(hist2), bits(hist)) and np.array_equal(bits(du.head()), bits(u))


@pytest.fixture(scope="module")
def poisson():
    return hierarchy.poisson_hierarchy(18, 4)      # the hierarchy of tests/test_gpu_vcycle.py: 4096 -> 512 -> 64 -> 8 rows


def test_fgmres_is_flexible(capi, poisson):
    """the CG coarsest solver and the Chebyshev smoother make the V-cycle no fixed linear map: FGMRES converges all the same, to the
    solution solve_pCG finds (both held to rtol 1e-8 on a well-conditioned problem)"""
    _, G, (OA, _, _), _ = build(capi, poisson, "chebyshev", coarse_solver="CG")
    n = OA[0].Mbig
    rhs = orc.laplacian3d_rhs(18)
    du, dp, dr = capi.DeviceVector(n), capi.DeviceVector(n), capi.DeviceVector(n, rhs)
    it, hist, conv, true_res = G.solve_fgmres(du, dr, restart=30)
    it_p, hist_p, conv_p = G.solve_pCG(dp, dr)
    print(f"FGMRES {it} iterations to {true_res / hist[0]:.2e}, pCG {it_p}; rel-l2 {sr.rel(du.download(), dp.download()):.2e}")
    assert conv and conv_p and true_res <= TOL * hist[0]
    assert sr.rel(du.download(), dp.download()) <= 1e-7


def test_fgmres_leaves_the_scalar_graph_cache_alone(capi, poisson):
    """eight captured scalar V-cycles survive an FGMRES solve (it preconditions through one fixed pair and a graph of its own),
    solve_pCG returns the bits it returned before, and from the second inner iteration on every iteration costs the same number of
    launches: nothing is captured again"""
    _, G, (OA, _, _), _ = build(capi, poisson, "jacobi")
    n = OA[0].Mbig
    rhs = orc.laplacian3d_rhs(18)
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, rhs)
    it0, hist0, _ = G.solve_pCG(du, dr)
    u0 = du.download()
    pairs = [(capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, rhs * (1 + j))) for j in range(8)]
    for u, r in pairs:
        G.vcycle(u, r)                                                       # captured

    def replays_as_one_launch():
        for u, r in pairs:
            l0 = capi.launch_count()
            G.vcycle(u, r)
            assert capi.launch_count() - l0 == 1
    replays_as_one_launch()
    dg = capi.DeviceVector(n)
    launches = []
    for k in range(1, 7):                                                    # k inner iterations and the end of the cycle, no convergence
        G.set_solve_params(k, 1e-14, "jacobi", 3, 3)
        l0 = capi.launch_count()
        it, _, conv, _ = G.solve_fgmres(dg, dr, restart=30)
        launches.append(capi.launch_count() - l0)
        assert it == k and not conv
    per_iteration = np.diff(launches)
    print(f"launches of a solve of 1..6 iterations: {launches}")
    assert np.all(per_iteration[1:] == per_iteration[1]) and 0 < per_iteration[1] <= 16, launches
    assert per_iteration[0] <= per_iteration[1]                              # (the first solve also captured the V-cycle)
    G.set_solve_params(60, 1e-8, "jacobi", 3, 3)
    it, hist, conv, _ = G.solve_fgmres(dg, dr, restart=30)
    assert conv
    replays_as_one_launch()
    it1, hist1, _ = G.solve_pCG(du, dr)
    assert it1 == it0 and np.array_equal(bits(hist1), bits(hist0)) and np.array_equal(bits(du.download()), bits(u0))


def test_fgmres_zero_right_hand_side(capi):
    c = gr.case(8, 1.0)
    n = c["A"].shape[0]
    G, _ = gpu_hierarchy(capi, c)
    du, dr = Padded(capi, np.ones(n)), capi.DeviceVector(n, np.zeros(n))
    for precond in (True, False):
        it, hist, conv, true_res = G.solve_fgmres(du, dr, restart=5, precond=precond)
        assert conv and it == 0 and true_res == 0.0 and list(hist) == [0.0]
        assert not du.head().any()


def test_fgmres_refusals(capi):
    c = gr.case(8, 1.0)
    n = c["A"].shape[0]
    G, _ = gpu_hierarchy(capi, c)
    du, dr = capi.DeviceVector(n, np.ones(n)), capi.DeviceVector(n, c["rhs"])
    for restart in (0, 65):
        with pytest.raises(capi.SgpuError, match="restart length must be in 1..64"):
            G.solve_fgmres(du, dr, restart=restart)
    assert np.all(du.download() == 1.0)                                      # refused before anything was written
    big = sr.case("tri", 1025)
    _, Gb, _ = one_level(capi, big["A"], "CG")                               # one more row than the LDS-resident coarsest solvers hold
    db, dbr = capi.DeviceVector(1025), capi.DeviceVector(1025, big["rhs"])
    with pytest.raises(capi.SgpuError, match="host-driven CG"):
        Gb.solve_fgmres(db, dbr, restart=5)
    it, _, conv = Gb.solve_pCG(db, dbr)                                      # the scalar solve on the same handle still works
    assert conv


def test_pcg_is_not_enough_for_this_operator(capi):
    """why the feature exists (existing code only): with the same V-cycle, pCG does not reach 1e-8 on convdiff(14, 4.0)"""
    c = gr.case(14, 4.0)
    n = c["A"].shape[0]
    G, _ = gpu_hierarchy(capi, c, max_iter=60)
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, c["rhs"])
    st = capi.lib().sgpu_solve_pCG(G.h, du.ptr, dr.ptr, None, None, 0)
    assert st == -6                                                          # SGPU_ERR_NOCONV
