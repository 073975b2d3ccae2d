"""The solver layer on the GPU, held to a contract: the streaming vector kernels and the dot, the two LDS-resident
coarsest solvers (k_dense_solve behind the host's Gauss-Jordan inverse, k_coarse_cg), the host-driven coarsest CG, and
the two Krylov update kernels each past its own grid-stride threshold (256 * 1024 and 256 * 2048 rows).

Inputs, references and bounds come from tests/solver_ref.py; tests/test_solver_ref.py shows on the CPU that a correct
implementation stays inside every bound asserted here.  Sizes are the strides' edges: 256 threads over rows, 8 lanes over
a row's entries, 64 lanes over a dense row, 1024 rows in LDS; 256 * 1024 elements per trip of the dot and
2 * 256 * 2048 per trip of fill / axpby.
"""
import ctypes as C

import numpy as np
import pytest

from tests import hierarchy, inputs, solver_ref as sr, util

pytestmark = pytest.mark.gpu

TOL_HIST = 1e-10
PAD = 8
SENTINEL_BITS = np.uint64(0x7FF8C0DEFACE0001)                 # a NaN with a payload: any read of it poisons, any write of it shows
SENTINEL = np.array([SENTINEL_BITS], np.uint64).view(np.float64)[0]
VEC_WRAP = 2 * sr.BLOCK * 2048                                # first element of the second grid-stride trip of k_fill / k_axpby
IDS = lambda c: f"{c[0]}{c[1]}"      # noqa: E731


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Padded:
    """the first n elements of an allocation of n + 8 whose tail holds the sentinel"""

    def __init__(self, capi, values):
        values = np.ascontiguousarray(values, np.float64)
        self.capi, self.n = capi, len(values)
        self.v = capi.DeviceVector(self.n + PAD, np.concatenate([values, np.full(PAD, SENTINEL)]))
        self.ptr = self.v.ptr

    def upload(self, values):
        self.v.upload(np.concatenate([np.ascontiguousarray(values, np.float64), np.full(PAD, SENTINEL)]))
        return self

    def poke(self, j, value):
        one = np.array([value], np.float64)
        self.capi.check(self.capi.lib().sgpu_vec_upload(C.c_void_p(self.ptr.value + 8 * j), one.ctypes.data, 1))

    def head(self):
        """the n elements, after checking that the tail came back with the sentinel's bits"""
        a = self.v.download()
        assert np.all(bits(a[self.n:]) == SENTINEL_BITS), "wrote past n"
        return a[:self.n]


def gpu_dot(capi, x, y):
    out = C.c_double(-1.0)
    capi.check(capi.lib().sgpu_dot(x.ptr, y.ptr, x.n, C.byref(out)))
    return out.value


def vec_inputs(n):
    x, y = inputs.v2(n), inputs.rhs2(n)
    if n > 2:                                                  # signed zeros in the body and in an odd n's tail element
        x[n // 2], y[n // 2] = -0.0, 0.0
        x[n - 1] = -0.0
    return x, y


def poison_positions(n, wrap):
    return sorted({j for j in (0, n - 1, wrap - 1, wrap, wrap + 1) if 0 <= j < n})


# ---------------------------------------------------------------------------
# vector kernels
@pytest.mark.parametrize("n", sr.vec_sizes())
def test_fill(capi, n):
    d = Padded(capi, np.full(n, SENTINEL))
    for a in (3.25, -0.0, np.inf):
        capi.check(capi.lib().sgpu_vec_fill(d.ptr, a, n))
        assert np.all(bits(d.head()) == bits([a])[0]), a


@pytest.mark.parametrize("n", sr.vec_sizes())
def test_copy(capi, n):
    x, _ = vec_inputs(n)
    for k, j in enumerate(poison_positions(n, VEC_WRAP)):
        x[j] = (np.nan, -np.inf, -0.0)[k % 3]
    src, dst = Padded(capi, x), Padded(capi, np.full(n, SENTINEL))
    capi.check(capi.lib().sgpu_vec_copy(dst.ptr, src.ptr, n))
    assert np.array_equal(bits(dst.head()), bits(x))
    assert np.array_equal(bits(src.head()), bits(x))


@pytest.mark.parametrize("a,b", [(2.5, -0.5), (1.0, 1.0), (-1.0, 0.0), (0.0, 0.0), (0.0, 1.0)])
@pytest.mark.parametrize("n", sr.vec_sizes())
def test_axpby(capi, n, a, b):
    """y = a x + b y with a rounding per operation (the library is built without contraction): numpy's bits, the sign of
    zero included.  b == 0 never reads y; with b != 0 a NaN or Inf in element j of x or y reaches element j alone."""
    lib = capi.lib()
    x, y = vec_inputs(n)
    dx, dy = Padded(capi, x), Padded(capi, y)
    if b == 0.0:
        dy.upload(np.full(n, np.nan))
        capi.check(lib.sgpu_vec_axpby(a, dx.ptr, b, dy.ptr, n))
        got = dy.head()
        assert not np.any(np.isnan(got))
        assert np.array_equal(bits(got), bits(a * x))
        assert np.array_equal(bits(dx.head()), bits(x))
        return
    capi.check(lib.sgpu_vec_axpby(a, dx.ptr, b, dy.ptr, n))
    clean = dy.head()
    assert np.array_equal(bits(clean), bits(a * x + b * y))
    assert np.array_equal(bits(dx.head()), bits(x))
    J = poison_positions(n, VEC_WRAP)
    if not J:
        return
    others = np.ones(n, bool)
    others[J] = False
    for in_x, special in ((True, np.nan), (True, np.inf), (False, np.nan), (False, -np.inf)):
        xp, yp = x.copy(), y.copy()
        (xp if in_x else yp)[J] = special
        dx.upload(xp); dy.upload(yp)
        capi.check(lib.sgpu_vec_axpby(a, dx.ptr, b, dy.ptr, n))
        got = dy.head()
        with np.errstate(invalid="ignore"):
            want = a * xp + b * yp
        assert np.array_equal(bits(got[others]), bits(clean[others])), (in_x, special)
        assert np.array_equal(np.isnan(got[J]), np.isnan(want[J])), (in_x, special)
        fin = ~np.isnan(want[J])
        assert np.array_equal(got[J][fin], want[J][fin]), (in_x, special)      # +-inf, or untouched where a == 0 multiplies a finite x


@pytest.mark.parametrize("n", sr.vec_sizes())
def test_dot(capi, n):
    """|got - longdouble sum| <= k u sum|x y| / (1 - k u), k = the roundings on the longest path of the kernel's summation
    (solver_ref.dot_roundings: 23 to 35 here; the old 1e-12 sum|x y| allowed about 9000)"""
    nb = sr.dot_blocks(n)
    if n == 0:
        e = Padded(capi, np.zeros(0))
        assert gpu_dot(capi, e, e) == 0.0 and not np.signbit(gpu_dot(capi, e, e))
        return
    dx, dy = Padded(capi, np.zeros(n)), Padded(capi, np.zeros(n))
    for kind in ("normal", "positive", "cancelling"):
        x, y = sr.dot_inputs(n, kind)
        dx.upload(x); dy.upload(y)
        got = gpu_dot(capi, dx, dy)
        err = abs(float(np.longdouble(got) - sr.dot_hp(x, y)))
        print(f"n={n} {kind}: {err / (sr.U * float(np.sum(np.abs(x * y)))):.2f} roundings of {sr.dot_roundings(n)}")
        assert err <= sr.dot_bound(x, y), (kind, got, err, sr.dot_bound(x, y))
        assert gpu_dot(capi, dx, dy) == got                     # a fixed summation order
    # (x, y) is the cancelling pair now; a NaN anywhere gives NaN
    J = sorted({j for j in (0, 255, 256, sr.BLOCK * nb - 1, sr.BLOCK * nb, n - 1) if 0 <= j < n})
    for j in (J[0], J[-1]):
        dx.poke(j, np.nan)
        assert np.isnan(gpu_dot(capi, dx, dy)), j
        dx.poke(j, x[j])
    # +inf * positive, the rest finite -> +inf
    x, y = sr.dot_inputs(n, "positive")
    dx.upload(x); dy.upload(y)
    for j in (J[0], J[-1]):
        dx.poke(j, np.inf)
        assert gpu_dot(capi, dx, dy) == np.inf, j
        dx.poke(j, x[j])
    # every element is counted once: ones . ones = n, e_j . y = y[j]
    dx.upload(np.ones(n)); dy.upload(np.ones(n))
    assert gpu_dot(capi, dx, dy) == float(n)
    x, y = sr.dot_inputs(n, "normal")
    dx.upload(np.zeros(n)); dy.upload(y)
    for j in J:
        dx.poke(j, 1.0)
        assert gpu_dot(capi, dx, dy) == y[j], j
        dx.poke(j, 0.0)
    assert np.array_equal(bits(dy.head()), bits(y)) and np.all(dx.head() == 0.0)


def test_dot_does_not_depend_on_what_the_partials_held(capi):
    """the partials buffer is shared by all dots: a 3-element dot after one that filled all 1024 partials, and the reverse"""
    big, small = 2097155, 3
    xb, yb = sr.dot_inputs(big, "normal")
    xs, ys = sr.dot_inputs(small, "normal")
    dxb, dyb, dxs, dys = (Padded(capi, v) for v in (xb, yb, xs, ys))
    want_s, want_b = gpu_dot(capi, dxs, dys), gpu_dot(capi, dxb, dyb)
    assert gpu_dot(capi, dxs, dys) == want_s                    # after the big one
    assert gpu_dot(capi, dxb, dyb) == want_b                    # after the small one
    assert gpu_dot(capi, dxb, dyb) == want_b
    assert gpu_dot(capi, dxs, dys) == want_s
    assert abs(float(np.longdouble(want_s) - sr.dot_hp(xs, ys))) <= sr.dot_bound(xs, ys)


# ---------------------------------------------------------------------------
# coarsest solvers: one-level hierarchies ([A], [], [])
def one_level(capi, A, coarse_solver, cg_max_iter=sr.CG_MAX_ITER, max_iter=100, tol=1e-8):
    """-> (oracle hierarchy, GPU hierarchy, GPU operator) over the same arrays"""
    O, OA = hierarchy.single_level_oracle(A, cg_max_iter=cg_max_iter, cg_tol=sr.CG_TOL, max_iter=max_iter, tol=tol)
    op = util.gpu_operator(OA)
    G = capi.Amg([op], [], [], coarse_solver=coarse_solver, cg_max_iter=cg_max_iter, cg_tol=sr.CG_TOL, max_iter=max_iter, tol=tol)
    return O, G, op


def check_cg_contracts(c, u, it, u_o, it_o):
    """the project's figures against the oracle, and the two contracts against the high-precision solution that
    tests/test_solver_ref.py shows the oracle itself meets"""
    nrm = np.linalg.norm(c["rhs"])
    print(f"it {it} (oracle {it_o}), rel oracle {sr.rel(u, u_o):.2e}, rel hp {sr.rel(u, c['x']):.2e} of {2 * c['cond'] * sr.CG_TOL:.2e}, "
          f"residual {sr.residual_hp(c['A'], u, c['rhs']) / nrm:.2e}")
    assert abs(it - it_o) <= 1, (it, it_o)
    assert sr.rel(u, u_o) <= 1e-11
    assert sr.rel(u, c["x"]) <= 2 * c["cond"] * sr.CG_TOL
    assert sr.residual_hp(c["A"], u, c["rhs"]) <= 2 * sr.CG_TOL * nrm


@pytest.mark.parametrize("case", sr.DIRECT_CASES, ids=IDS)
def test_coarsest_direct(capi, case):
    """u = inverse(A) rhs, the inverse by Gauss-Jordan with partial pivoting on the host: within 4 (n + 4) u cond_2(A) of the
    high-precision solution whatever u held; `shifted` is where the pivot search and the row swaps run"""
    f, n = case
    c = sr.case(f, n)
    O, G, _ = one_level(capi, c["A"], "direct")
    dr = capi.DeviceVector(n, c["rhs"])
    du = capi.DeviceVector(n, np.ones(n))
    assert G.coarsest_solve(du, dr) == 0
    u = du.download()
    err = sr.rel(u, c["x"])
    print(f"{f}({n}): err / (n u cond) = {err / (n * sr.U * c['cond']):.3g}")
    assert err <= sr.direct_bound(n, c["cond"])
    du.upload(np.full(n, np.nan))
    assert G.coarsest_solve(du, dr) == 0
    assert np.array_equal(bits(du.download()), bits(u))
    if f != "shifted":                                         # (not symmetric: no CG)
        u_o, _ = O.coarsest_cg(c["rhs"])
        assert sr.rel(u, u_o) <= sr.direct_bound(n, c["cond"]) + 2 * c["cond"] * sr.CG_TOL      # the two contracts, added
    dr.upload(np.zeros(n))
    du.upload(np.ones(n))
    assert G.coarsest_solve(du, dr) == 0
    assert np.all(du.download() == 0.0)


def test_coarsest_direct_refuses_a_singular_operator(capi):
    O, OA = hierarchy.single_level_oracle(sr.singular(65))
    op = util.gpu_operator(OA)
    with pytest.raises(capi.SgpuError, match="singular"):
        capi.Amg([op], [], [], coarse_solver="direct")
    # the context is still usable, and so is the operator under the solver that needs no inverse of it
    c = sr.case("tri", 65)
    _, G, _ = one_level(capi, c["A"], "direct")
    du, dr = capi.DeviceVector(65, np.ones(65)), capi.DeviceVector(65, c["rhs"])
    assert G.coarsest_solve(du, dr) == 0
    assert sr.rel(du.download(), c["x"]) <= sr.direct_bound(65, c["cond"])
    capi.Amg([op], [], [], coarse_solver="CG")


@pytest.mark.parametrize("case", sr.CG_CASES, ids=IDS)
def test_coarsest_cg(capi, case):
    c = sr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], "CG")
    u_o, it_o = O.coarsest_cg(c["rhs"])
    du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, c["rhs"])
    it = G.coarsest_solve(du, dr)
    check_cg_contracts(c, du.download(), it, u_o, it_o)


@pytest.mark.parametrize("case", sr.CAPPED_CASES, ids=IDS)
def test_coarsest_cg_iteration_cap(capi, case):
    """CG_coarsest_max_iter = 6: five updates on both sides, the same unconverged iterate"""
    c = sr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], "CG", cg_max_iter=6)
    u_o, it_o = O.coarsest_cg(c["rhs"])
    du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, c["rhs"])
    it = G.coarsest_solve(du, dr)
    assert it == 5 and it_o == 5
    assert sr.rel(du.download(), u_o) <= 1e-11
    assert sr.rel(u_o, c["x"]) > 1e-6                           # (the cap ended it, not the tolerance)


@pytest.mark.parametrize("case", sr.EARLY_OUT_CASES, ids=IDS)
def test_coarsest_cg_early_outs(capi, case):
    """rhs = 0, and ||rhs|| = 1e-13 so that rhs.rhs < tol^2: no iteration, u keeps its bits, the oracle's count; in the
    LDS kernel (257 rows) and in the host-driven loop (1025)"""
    c = sr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], "CG")
    u0 = inputs.v2(n)
    u0[0] = -0.0
    tiny = c["rhs"] * (1e-13 / np.linalg.norm(c["rhs"]))
    for rhs in (np.zeros(n), tiny):
        _, it_o = O.coarsest_cg(rhs)
        du, dr = capi.DeviceVector(n, u0), capi.DeviceVector(n, rhs)
        assert G.coarsest_solve(du, dr) == it_o
        assert np.array_equal(bits(du.download()), bits(u0))


@pytest.mark.parametrize("coarse_solver", ["CG", "direct"])
@pytest.mark.parametrize("case", sr.FALLBACK_CASES, ids=IDS)
def test_coarsest_host_driven_fallback(capi, case, coarse_solver):
    """1025 rows are one more than the LDS-resident solvers hold: both settings run the host-driven CG over the device
    kernels, to the CG contracts (a nonzero iteration count under "direct" shows which path ran)"""
    c = sr.case(*case)
    n = case[1]
    O, G, _ = one_level(capi, c["A"], coarse_solver)
    u_o, it_o = O.coarsest_cg(c["rhs"])
    du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, c["rhs"])
    it = G.coarsest_solve(du, dr)
    assert it > 0
    check_cg_contracts(c, du.download(), it, u_o, it_o)


# ---------------------------------------------------------------------------
# Krylov scalars on the device, past the grid-stride thresholds of their two grids
@pytest.mark.parametrize("n", sr.KRYLOV_SIZES)
def test_cg_update_kernels_past_the_grid_stride_threshold(capi, n):
    """solve_CG on tri(n).  At 262401 rows k_pcg_update_dev (the update fused with the new r.r, on the dot's grid of at
    most 1024 blocks) takes a second grid-stride trip; k_pcg_direction_dev runs on up to 2048 blocks of 256 and makes
    one trip there, so 524545 rows are what sends it round again.  The oracle's iteration count and history; and,
    because the history alone cannot see a wrong u update, the residual of the downloaded u recomputed on the host in
    longdouble."""
    assert n > sr.BLOCK * sr.N_PARTIALS
    A = sr.tri(n)
    rhs = inputs.rhs2(n)
    O, G, _ = one_level(capi, A, "CG", max_iter=100, tol=1e-8)
    u_o, it_o, hist_o = O.solve_CG(rhs)
    du, dr = capi.DeviceVector(n), capi.DeviceVector(n, rhs)
    it, hist, conv = G.solve_CG(du, dr)
    u = du.download()
    print(f"{it} iterations (oracle {it_o}), last {hist[-1]:.3e} of {hist[0]:.3e}")
    assert conv and it == it_o and 10 < it < 100
    assert len(hist) == len(hist_o)
    assert np.all(np.abs(hist - hist_o) <= TOL_HIST * hist_o[0]), (hist, hist_o)
    assert np.all(np.abs(hist - hist_o) <= 1e-6 * hist_o), (hist, hist_o)
    assert sr.rel(u, u_o) <= 1e-9
    assert abs(sr.residual_hp(A, u, rhs) - hist[-1]) <= TOL_HIST * hist[0]
    it2, hist2, conv2 = G.solve_CG(du, dr)
    assert conv2 and it2 == it and np.array_equal(bits(hist2), bits(hist))
    assert np.array_equal(bits(du.download()), bits(u))
