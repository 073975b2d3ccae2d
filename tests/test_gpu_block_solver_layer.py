"""The block solver layer on the GPU (K = 2, 4, 8 right-hand sides), held to the contract tests/test_gpu_solver_layer.py holds
the scalar one to: the block dot (k_dot_block_partial, k_reduce_partials_block), the two block pCG updates, pack / unpack, the
two coarsest solvers behind a block (k_dense_solve_block<C> in one and in two passes; k_coarse_cg column by column), the block
V-cycle over a large coarsest level, block pCG past both grid-stride thresholds, the two graph caches, and an operator whose
rows hold no entry.

Inputs, references and bounds come from tests/solver_ref.py; tests/test_solver_ref.py shows on the CPU that a correct
implementation stays inside every bound asserted here.  The vector kernels are reached through sgpu_debug_block_dot /
_pcg_update / _pcg_direction, which run the launch code of sgpu_solve_pCG_block (its K switch and its grids) on the caller's
vectors.  Block vectors are staged here, not by k_block_pack: host.ravel() of an (n, K) C-ordered array is X[i * K + j], in an
allocation of n K + 8 doubles whose tail holds a sentinel.

Which paths run where:
  * the dot and the fused update run on at most 1024 blocks of 256: rows >= 262145 send them on a second grid-stride trip;
  * direction, pack and unpack run on at most 2048 blocks: rows >= 524289;
  * k_dense_solve_block<C>, C = min(K, pow2floor(4096 / n)) columns of the right-hand side in LDS per pass: 512 rows at K = 8 fill
    it with C = 8; 513, 729, 1023 and 1024 rows at K = 8 take two passes of C = 4 (the j0 loop, its barrier between passes and the
    j0 + c indexing); 1024 rows at K = 4 fill it with C = 4; 1024 rows at K = 2 is C = 2, 200 rows is C = min(K, 16) = K.
"""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import hierarchy, inputs, solver_ref as sr, util
from tests.test_gpu_block_vcycle import check_column
from tests.test_gpu_solver_layer import SENTINEL, SENTINEL_BITS, TOL_HIST, Padded, bits, gpu_dot, one_level
from tests.test_gpu_vcycle import TOL_VCYCLE, build

pytestmark = pytest.mark.gpu

KS = (2, 4, 8)
MASKS = {2: (0b11, 0b01, 0b10), 4: (0b1111, 0b0101, 0b1000), 8: (0xFF, 0b10010110, 0b01000001)}     # all, then two partial masks
DOT_WRAP = sr.BLOCK * sr.N_PARTIALS                           # first row of the second trip of the dot and the fused update
DIR_WRAP = sr.BLOCK * 2048                                    # ... of direction, pack and unpack
IDS = lambda c: f"{c[0]}{c[1]}"      # noqa: E731


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def H(capi):
    """a hierarchy for the debug wrappers: they take it for its per-K state (the dots' partial sums) and index nothing of it"""
    return one_level(capi, sr.tri(9), "direct")[1]


class Blk:
    """an (n, K) host array as the block vector X[i * K + j], in an allocation of n K + 8 with the sentinel in its tail"""

    def __init__(self, capi, host):
        host = np.ascontiguousarray(host, np.float64)
        self.n, self.K = host.shape
        self.d = Padded(capi, host.ravel())
        self.ptr = self.d.ptr

    def upload(self, host):
        host = np.ascontiguousarray(host, np.float64)
        assert host.shape == (self.n, self.K)
        self.d.upload(host.ravel())
        return self

    def get(self):
        """the (n, K) array, after checking the tail"""
        return self.d.head().reshape(self.n, self.K)


def cols_of(mask, K):
    return [j for j in range(K) if (mask >> j) & 1]


def same_bits(a, b, what=""):
    np.testing.assert_array_equal(bits(a), bits(b), err_msg=str(what))


# ---------------------------------------------------------------------------
# the dot
_DOT = {}


def dot_columns(n, kind):
    """-> (X, Y) of shape (n, 8), column j from another seed; the last (n, kind) is kept"""
    if _DOT.get("key") != (n, kind):
        xy = [sr.dot_inputs(n, kind, seed=j) for j in range(8)]
        _DOT.update(key=(n, kind), X=np.stack([x for x, _ in xy], axis=1), Y=np.stack([y for _, y in xy], axis=1))
    return _DOT["X"], _DOT["Y"]


def block_dot(H, dX, dY, n, K, mask, out):
    H.debug_block_dot(dX, dY, n, K, mask, out)
    return out.head()


@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_block_dot(capi, H, n):
    """per column: within dot_bound of the longdouble sum; the bits of sgpu_dot on that column alone (the same element-to-thread map,
    tree and grid, no contraction); the same bits at K = 2, 4 and 8.  Under a partial mask the other out[j] keep a sentinel's bits,
    the NaN and Inf those columns hold reach no active column, and no tail is written"""
    if n == 0:
        for K in KS:
            e, out = Blk(capi, np.zeros((0, K))), Padded(capi, np.full(K, SENTINEL))
            got = block_dot(H, e, e, 0, K, MASKS[K][1], out)
            for j in range(K):
                assert bits(got[j]) == (bits(0.0) if (MASKS[K][1] >> j) & 1 else SENTINEL_BITS)
        return
    col = Padded(capi, np.zeros(n)), Padded(capi, np.zeros(n))
    for kind in ("normal", "positive", "cancelling"):
        X, Y = dot_columns(n, kind)
        scalar = np.empty(8)
        for j in range(8):
            col[0].upload(X[:, j]); col[1].upload(Y[:, j])
            scalar[j] = gpu_dot(capi, col[0], col[1])
            err = abs(float(np.longdouble(scalar[j]) - sr.dot_hp(X[:, j], Y[:, j])))
            assert err <= sr.dot_bound(X[:, j], Y[:, j]), (kind, j, err)
        blocked = [sr.dot_blocked(X[:, j], Y[:, j]) for j in range(2)]
        print(f"n={n} {kind}: columns 0, 1 equal the numpy restatement of the summation order: {[blocked[j] == scalar[j] for j in range(2)]}")
        for K in KS:
            dX, dY, out = Blk(capi, X[:, :K]), Blk(capi, Y[:, :K]), Padded(capi, np.full(K, SENTINEL))
            got = block_dot(H, dX, dY, n, K, MASKS[K][0], out).copy()
            same_bits(got, scalar[:K], (kind, K))               # hence within dot_bound, and the same at every K
            same_bits(block_dot(H, dX, dY, n, K, MASKS[K][0], out), got)
            if kind != "normal":
                continue
            for mask in MASKS[K][1:]:
                on = cols_of(mask, K)
                off = [j for j in range(K) if j not in on]
                Xp, Yp = X[:, :K].copy(), Y[:, :K].copy()
                Xp[:, off] = np.nan
                Yp[n // 2, off] = np.inf
                dX.upload(Xp); dY.upload(Yp); out.upload(np.full(K, SENTINEL))
                got = block_dot(H, dX, dY, n, K, mask, out)
                same_bits(got[on], scalar[on], (K, mask))
                assert np.all(bits(got[off]) == SENTINEL_BITS), (K, mask)
                same_bits(dX.get(), Xp); same_bits(dY.get(), Yp)


@pytest.mark.parametrize("K", [2, 8])
def test_block_dot_does_not_depend_on_what_the_partials_held(capi, H, K):
    """the 1024 x K partial sums are shared by every dot of a hierarchy: a 3-row dot after one that filled them all, and the reverse"""
    big, small = DOT_WRAP + 257, 3
    Xb, Yb = (a[:, :K] for a in dot_columns(big, "normal"))
    xs = [sr.dot_inputs(small, "normal", seed=j) for j in range(K)]
    Xs, Ys = np.stack([x for x, _ in xs], axis=1), np.stack([y for _, y in xs], axis=1)
    dXb, dYb, dXs, dYs = (Blk(capi, a) for a in (Xb, Yb, Xs, Ys))
    out = Padded(capi, np.full(K, SENTINEL))
    full = MASKS[K][0]
    want_s = block_dot(H, dXs, dYs, small, K, full, out).copy()
    want_b = block_dot(H, dXb, dYb, big, K, full, out).copy()
    same_bits(block_dot(H, dXs, dYs, small, K, full, out), want_s)     # after the big one
    same_bits(block_dot(H, dXb, dYb, big, K, full, out), want_b)       # after the small one
    same_bits(block_dot(H, dXb, dYb, big, K, full, out), want_b)
    same_bits(block_dot(H, dXs, dYs, small, K, full, out), want_s)
    for j in range(K):
        assert abs(float(np.longdouble(want_s[j]) - sr.dot_hp(Xs[:, j], Ys[:, j]))) <= sr.dot_bound(Xs[:, j], Ys[:, j])
        assert abs(float(np.longdouble(want_b[j]) - sr.dot_hp(Xb[:, j], Yb[:, j]))) <= sr.dot_bound(Xb[:, j], Yb[:, j])


# ---------------------------------------------------------------------------
# the two pCG updates
_UPD = {}


def update_inputs(n):
    """-> dict of five (n, 8) arrays and four rows of 8 scalars; signed zeros in the body; the last n is kept"""
    if _UPD.get("n") != n:
        rng = np.random.default_rng(77 + n)
        v = {k: rng.standard_normal((n, 8)) for k in ("p", "h", "u", "r", "z")}
        if n > 2:
            v["p"][n // 2], v["h"][n // 2], v["u"][n - 1], v["z"][n - 1] = -0.0, 0.0, -0.0, -0.0
        v["num"], v["num2"] = rng.standard_normal(8), rng.standard_normal(8)
        v["den"], v["den2"] = 1.0 + rng.random(8), -1.0 - rng.random(8)
        _UPD.clear()
        _UPD.update(v, n=n)
    return _UPD


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", sr.BLOCK_VEC_SIZES)
def test_block_pcg_update_and_direction(capi, H, n, K):
    """all columns active and two partial masks.  Active columns of U, R and P: numpy's bits with a rounding per operation;
    rr[j]: the bits of the block dot of the new R with itself.  A column outside the mask holds NaNs with a payload in U, R and P and
    num = den = 0 (0 / 0 if it were formed): every bit of it stays, and so does its rr[j]; no tail is written.  262145 rows and more
    are the update's second grid-stride trip, 524289 and more the direction's"""
    v = update_inputs(n)
    P0, Hh, U0, R0, Z = (v[k][:, :K] for k in ("p", "h", "u", "r", "z"))
    dP, dH, dU, dR, dZ = (Blk(capi, a) for a in (P0, Hh, U0, R0, Z))
    num, den, rr, rr2 = (Padded(capi, np.zeros(K)) for _ in range(4))
    for mask in MASKS[K]:
        on = cols_of(mask, K)
        off = [j for j in range(K) if j not in on]
        Pm, Um, Rm = P0.copy(), U0.copy(), R0.copy()
        for a in (Pm, Um, Rm):
            a[:, off] = SENTINEL
        sc = {k: v[k][:K].copy() for k in ("num", "den", "num2", "den2")}
        for a in sc.values():
            a[off] = 0.0
        want_U, want_R, want_P = Um.copy(), Rm.copy(), Pm.copy()
        for j in on:
            want_U[:, j], want_R[:, j] = sr.pcg_update(sc["num"][j], sc["den"][j], P0[:, j], Hh[:, j], U0[:, j], R0[:, j])
            want_P[:, j] = sr.pcg_direction(sc["num2"][j], sc["den2"][j], Z[:, j], P0[:, j])
        dP.upload(Pm); dU.upload(Um); dR.upload(Rm)
        num.upload(sc["num"]); den.upload(sc["den"]); rr.upload(np.full(K, SENTINEL)); rr2.upload(np.full(K, SENTINEL))
        H.debug_block_pcg_update(num, den, dP, dH, dU, dR, n, K, mask, rr)
        same_bits(dU.get(), want_U, (K, mask, "U"))
        same_bits(dR.get(), want_R, (K, mask, "R"))
        same_bits(dP.get(), Pm, (K, mask, "P is read only"))
        same_bits(dH.get(), Hh)
        H.debug_block_dot(dR, dR, n, K, mask, rr2)
        got_rr = rr.head()
        same_bits(got_rr, rr2.head(), (K, mask, "rr"))
        assert np.all(bits(got_rr[off]) == SENTINEL_BITS) and not np.any(np.isnan(got_rr[on]))
        for j in on[:2]:
            assert abs(float(np.longdouble(got_rr[j]) - sr.dot_hp(want_R[:, j], want_R[:, j]))) <= sr.dot_bound(want_R[:, j], want_R[:, j])
        same_bits(num.head(), sc["num"]); same_bits(den.head(), sc["den"])
        num.upload(sc["num2"]); den.upload(sc["den2"])
        H.debug_block_pcg_direction(num, den, dZ, dP, n, K, mask)
        same_bits(dP.get(), want_P, (K, mask, "P"))
        same_bits(dZ.get(), Z)


# ---------------------------------------------------------------------------
# pack and unpack past their grid
@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("n", [DIR_WRAP, DIR_WRAP + 1, 1048577])
def test_pack_unpack_past_the_grid_stride_threshold(capi, n, K):
    """column-major n x K -> block -> column-major against numpy, exactly; -0.0 and Inf at the first row, the rows about the wrap
    and the last one"""
    Hm = np.random.default_rng(n + K).standard_normal((n, K))
    for k, i in enumerate(i for i in (0, DIR_WRAP - 1, DIR_WRAP, n - 1) if i < n):
        Hm[i, k % K], Hm[i, (k + 1) % K] = -0.0, (np.inf, -np.inf)[k % 2]
    colmajor = np.asfortranarray(Hm).ravel(order="F")
    src, blk, back = Padded(capi, colmajor), Padded(capi, np.full(n * K, SENTINEL)), Padded(capi, np.full(n * K, SENTINEL))
    capi.check(capi.lib().sgpu_block_pack(src.ptr, blk.ptr, n, K))
    same_bits(blk.head(), Hm.ravel())
    capi.check(capi.lib().sgpu_block_unpack(blk.ptr, back.ptr, n, K))
    same_bits(back.head(), colmajor)
    same_bits(src.head(), colmajor); same_bits(blk.head(), Hm.ravel())


# ---------------------------------------------------------------------------
# coarsest solvers behind a block: one-level hierarchies, whose block V-cycle is the coarsest solve alone
def scalar_coarsest(capi, G, n, u0, rhs):
    du, dr = capi.DeviceVector(n, u0), capi.DeviceVector(n, rhs)
    G.coarsest_solve(du, dr)
    return du.download()


@pytest.mark.parametrize("case", sr.BLOCK_DIRECT_CASES, ids=IDS)
def test_block_coarsest_direct(capi, case):
    """K = 2, 4, 8 (see the module's docstring for which case is which pass structure): every column within direct_bound of its
    high-precision solution and equal to the scalar direct solve of that column bit for bit (k_dense_solve_block keeps the
    scalar's wave per row and lane-to-column sum); what U held is ignored; the all-zero column gives exact zeros"""
    f, n = case
    c = sr.case(f, n)
    _, G, _ = one_level(capi, c["A"], "direct")
    B8, X8 = sr.coarse_columns(f, n, 8)
    scalar = np.stack([scalar_coarsest(capi, G, n, np.full(n, np.nan), B8[:, j]) for j in range(8)], axis=1)
    for K in KS:
        dU, dB = Blk(capi, np.ones((n, K))), Blk(capi, B8[:, :K])
        G.vcycle_block(dU, dB)
        got = dU.get().copy()
        for j in range(K):
            err = sr.rel(got[:, j], X8[:, j])
            print(f"{f}({n}) K={K} column {j}: err / (n u cond) = {err / (n * sr.U * c['cond']):.3g}")
            assert err <= sr.direct_bound(n, c["cond"]), (K, j, err)
        same_bits(got, scalar[:, :K], K)
        assert not got[:, 1].any() and not np.signbit(got[:, 1]).any()
        dU.upload(np.full((n, K), np.nan))
        G.vcycle_block(dU, dB)
        same_bits(dU.get(), got, K)
        same_bits(dB.get(), B8[:, :K])


def guess(n, K):
    """a nonzero initial guess per column, with a -0.0"""
    U0 = np.stack([inputs.v2(n, ofs=9 * j) + 0.5 for j in range(K)], axis=1)
    U0[0, :] = -0.0
    return U0


@pytest.mark.parametrize("K", [2, 8])
@pytest.mark.parametrize("case", sr.BLOCK_CG_CASES, ids=IDS)
def test_block_coarsest_cg(capi, case, K):
    """k_coarse_cg column by column through the unpacked copies.  From a zero block, and from a nonzero one (the branch that
    unpacks U: the oracle's CG adds its updates to what u held, its residual starting from rhs): every column within 1e-11 of the
    oracle on that column, equal to the scalar coarsest solve of that column bit for bit, and inside the two high-precision
    contracts -- which, from a guess u0, hold for u - u0"""
    f, n = case
    c = sr.case(f, n)
    O, G, _ = one_level(capi, c["A"], "CG")
    B, X = sr.coarse_columns(f, n, K)
    for U0 in (np.zeros((n, K)), guess(n, K)):
        dU, dB = Blk(capi, U0), Blk(capi, B)
        G.vcycle_block(dU, dB)
        got = dU.get()
        for j in range(K):
            u_o = O.vcycle(U0[:, j], B[:, j])
            same_bits(got[:, j], scalar_coarsest(capi, G, n, U0[:, j], B[:, j]), (j, "scalar"))
            if j == 1:                                          # the zero right-hand side: U's bits stay
                same_bits(got[:, j], U0[:, j])
                continue
            d = got[:, j] - U0[:, j]
            nrm = np.linalg.norm(B[:, j])
            print(f"{f}({n}) K={K} column {j}: rel oracle {sr.rel(got[:, j], u_o):.2e}, rel hp {sr.rel(d, X[:, j]):.2e} of "
                  f"{2 * c['cond'] * sr.CG_TOL:.2e}, residual {sr.residual_hp(c['A'], d, B[:, j]) / nrm:.2e}")
            assert sr.rel(got[:, j], u_o) <= 1e-11, j
            assert sr.rel(d, X[:, j]) <= 2 * c["cond"] * sr.CG_TOL, j
            assert sr.residual_hp(c["A"], d, B[:, j]) <= 2 * sr.CG_TOL * nrm, j
        same_bits(dB.get(), B)


def test_block_coarsest_cg_early_outs_per_column(capi):
    """one block of a normal column, a zero right-hand side, a ||rhs|| = 1e-13 column and another normal one: the second and
    third keep U's bits, -0.0 included, the others are the scalar solves"""
    n, K = 257, 4
    c = sr.case("tri", n)
    O, G, _ = one_level(capi, c["A"], "CG")
    B = np.array(sr.coarse_columns("tri", n, K)[0])
    B[:, 2] = c["rhs"] * (1e-13 / np.linalg.norm(c["rhs"]))
    assert not B[:, 1].any() and float(B[:, 2] @ B[:, 2]) < sr.CG_TOL ** 2
    U0 = guess(n, K)
    dU, dB = Blk(capi, U0), Blk(capi, B)
    G.vcycle_block(dU, dB)
    got = dU.get()
    same_bits(got[:, 1:3], U0[:, 1:3])
    for j in (0, 3):
        same_bits(got[:, j], scalar_coarsest(capi, G, n, U0[:, j], B[:, j]))
        assert sr.rel(got[:, j], O.vcycle(U0[:, j], B[:, j])) <= 1e-11
        assert sr.rel(got[:, j] - U0[:, j], sr.solve_hp(c["dense"], B[:, j])[0]) <= 2 * c["cond"] * sr.CG_TOL


@pytest.mark.parametrize("K", [2, 8])
def test_block_coarsest_cg_iteration_cap(capi, K):
    """CG_coarsest_max_iter = 6 on tri(300): five updates per column, the oracle's unconverged iterate"""
    n = 300
    c = sr.case("tri", n)
    O, G, _ = one_level(capi, c["A"], "CG", cg_max_iter=6)
    B, X = sr.coarse_columns("tri", n, K)
    dU, dB = Blk(capi, np.zeros((n, K))), Blk(capi, B)
    G.vcycle_block(dU, dB)
    got = dU.get()
    for j in range(K):
        u_o, it_o = O.coarsest_cg(B[:, j])
        if j == 1:
            assert not got[:, j].any()
            continue
        assert it_o == 5
        assert sr.rel(got[:, j], u_o) <= 1e-11, j
        assert sr.rel(u_o, X[:, j]) > 1e-6                       # (the cap ended it, not the tolerance)
        same_bits(got[:, j], scalar_coarsest(capi, G, n, np.zeros(n), B[:, j]))


def test_block_solves_refuse_a_host_driven_coarsest_level(capi):
    """1025 rows are one more than the LDS-resident solvers hold: the block entry points refuse, and the scalar solve on the same
    handle still works"""
    n, K = 1025, 2
    c = sr.case("tri", n)
    O, G, _ = one_level(capi, c["A"], "CG")
    dU, dB = Blk(capi, np.zeros((n, K))), Blk(capi, np.stack([c["rhs"], c["rhs"]], axis=1))
    with pytest.raises(capi.SgpuError, match="host-driven CG"):
        G.vcycle_block(dU, dB)
    with pytest.raises(capi.SgpuError, match="host-driven CG"):
        capi.check(capi.lib().sgpu_solve_pCG_block(G.h, dU.ptr, dB.ptr, K, None, None, 0))
    assert not dU.get().any()
    du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, c["rhs"])
    it = G.coarsest_solve(du, dr)
    u_o, it_o = O.coarsest_cg(c["rhs"])
    assert it > 0 and abs(it - it_o) <= 1
    assert sr.rel(du.download(), u_o) <= 1e-11 and sr.rel(du.download(), c["x"]) <= 2 * c["cond"] * sr.CG_TOL


# ---------------------------------------------------------------------------
# the block V-cycle over a large coarsest level
_HIER = {}


def poisson2(m):
    if m not in _HIER:
        _HIER[m] = hierarchy.poisson_hierarchy(m, 2)
    return _HIER[m]


def vc_columns(n, K):
    return (np.stack([inputs.rhs2(n, ofs=50 * j) + 0.1 * j for j in range(K)], axis=1),
            np.stack([0.01 * inputs.v2(n, ofs=9 * j) for j in range(K)], axis=1))


@pytest.mark.parametrize("coarse", ["direct", "CG"])
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("m,nc", [(18, 512), (20, 729), (22, 1000)])
def test_block_vcycle_over_a_large_coarsest_level(capi, m, nc, smoother, coarse):
    """two levels, the coarsest of 512, 729 and 1000 rows (the direct solve's C = 8 full, then two passes of C = 4 at K = 8):
    K = 8 and 4, every column within 1e-11 of the oracle's V-cycle on it; the captured graph, replayed, equals the eager launches
    bit for bit"""
    hier = poisson2(m)
    assert hier[0][1].shape[0] == nc
    O, Gg, (OA, _, _), _ = build(capi, hier, smoother, pre=2, post=1, coarse_solver=coarse, use_graph=True)
    _, Ge, _, _ = build(capi, hier, smoother, pre=2, post=1, coarse_solver=coarse, use_graph=False)
    n = OA[0].Mbig
    RHS, U0 = vc_columns(n, 8)
    want = [O.vcycle(U0[:, j], RHS[:, j]) for j in range(8)]
    for K in (8, 4):
        dUg, dUe, dR = Blk(capi, U0[:, :K]), Blk(capi, U0[:, :K]), Blk(capi, RHS[:, :K])
        for call in range(3):
            l0 = capi.launch_count()
            Gg.vcycle_block(dUg, dR)
            launches = capi.launch_count() - l0
            Ge.vcycle_block(dUe, dR)
            got = dUg.get()
            same_bits(got, dUe.get(), (K, call))
            assert call == 0 or launches == 1
            if call == 0:
                for j in range(K):
                    e = sr.rel(got[:, j], want[j])
                    print(f"m={m} {smoother} {coarse} K={K} column {j}: rel-l2 {e:.3e}")
                    assert e <= TOL_VCYCLE, (K, j, e)


# ---------------------------------------------------------------------------
# block pCG past the grid-stride thresholds
_PCG = {}


def two_level(n, agg):
    if ("h", n) not in _PCG:
        _PCG[("h", n)] = sr.tri_two_level(n, agg)
    return _PCG[("h", n)]


def pcg_reference(O, n, smoother):
    """-> [(u, iters, history)] of the eight block_columns, once per (n, smoother)"""
    if (n, smoother) not in _PCG:
        _PCG[(n, smoother)] = [O.solve_pCG(c) for c in sr.block_columns(n, 8)]
    return _PCG[(n, smoother)]


def solve_block(G, capi, cols):
    dU, dB = Blk(capi, np.zeros((len(cols[0]), len(cols)))), Blk(capi, np.stack(cols, axis=1))
    it, hist, conv = G.solve_pCG_block(dU, dB)
    return dU.get().copy(), it, hist, conv


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
@pytest.mark.parametrize("n,agg", sr.TWO_LEVEL)
def test_block_pcg_past_the_grid_stride_thresholds(capi, n, agg, smoother):
    """tri_two_level: 262401 rows send the block dot and the fused update round their grid again, 524545 the direction update
    too; the columns stop at different iterations, so columns are frozen while the others run on past the wrap.  Per column the
    oracle's count, history and solution, and -- the history cannot see a wrong u update -- the residual of the downloaded column
    recomputed in longdouble.  K = 2 on the first two columns equals them in the K = 8 solve; a second run reproduces every bit;
    a column that is exactly zero takes no iteration and moves no bit of the others"""
    assert n > DOT_WRAP and (n > 2 * DOT_WRAP) == (agg == 513)
    hier = two_level(n, agg)
    O, G, _, _ = build(capi, hier, smoother, pre=2, post=1, max_iter=60, tol=1e-8)
    A = hier[0][0]
    cols = sr.block_columns(n, 8)
    ref = pcg_reference(O, n, smoother)
    assert len({r[1] for r in ref}) >= 2 and ref[0][1] != ref[1][1] and all(3 < r[1] < 60 for r in ref)

    u8, it8, hist8, conv = solve_block(G, capi, cols)
    assert conv
    for j in range(8):
        check_column(u8[:, j], it8[j], hist8[j], ref[j], what=f"n={n} {smoother} K=8 column {j}")
        assert abs(sr.residual_hp(A, u8[:, j], cols[j]) - hist8[j][-1]) <= TOL_HIST * hist8[j][0], j

    u2, it2, hist2, conv = solve_block(G, capi, cols[:2])
    assert conv and it2 == it8[:2]
    same_bits(u2, u8[:, :2])
    for a, b in zip(hist2, hist8[:2]):
        same_bits(a, b)
    for j in range(2):
        check_column(u2[:, j], it2[j], hist2[j], ref[j], what=f"n={n} {smoother} K=2 column {j}")
        assert abs(sr.residual_hp(A, u2[:, j], cols[j]) - hist2[j][-1]) <= TOL_HIST * hist2[j][0], j

    ub, itb, histb, conv = solve_block(G, capi, cols)
    assert conv and itb == it8
    same_bits(ub, u8)
    for a, b in zip(histb, hist8):
        same_bits(a, b)

    z = 3
    uz, itz, histz, conv = solve_block(G, capi, cols[:z] + [np.zeros(n)] + cols[z + 1:])
    others = [j for j in range(8) if j != z]
    assert conv and itz[z] == 0 and not uz[:, z].any() and histz[z].tolist() == [0.0]
    assert [itz[j] for j in others] == [it8[j] for j in others]
    same_bits(uz[:, others], u8[:, others])
    for j in others:
        same_bits(histz[j], hist8[j])


# ---------------------------------------------------------------------------
# the graph caches: eight (u, rhs) pairs each
@pytest.fixture(scope="module")
def hier4():
    return hierarchy.poisson_hierarchy(18, 4)


@pytest.mark.parametrize("K", [0, 4], ids=["scalar", "block4"])
def test_graph_cache_evicts_the_oldest_of_nine_pairs(capi, hier4, K):
    """nine distinct (u, rhs) pairs in turn, the first again (evicted: captured again), the ninth (still cached: one launch);
    every result equals the eager hierarchy's bit for bit"""
    _, Gg, (OA, _, _), _ = build(capi, hier4, "jacobi", use_graph=True)
    _, Ge, _, _ = build(capi, hier4, "jacobi", use_graph=False)
    n = OA[0].Mbig
    if K:
        mk = lambda a: Blk(capi, a)                                                   # noqa: E731
        get = lambda d: d.get()                                                       # noqa: E731
        run = lambda G, u, r: G.vcycle_block(u, r)                                    # noqa: E731
        u0 = [np.stack([0.01 * inputs.v2(n, ofs=9 * j + 100 * i) for j in range(K)], axis=1) for i in range(9)]
        rhs = [np.stack([inputs.rhs2(n, ofs=50 * j + 7 * i) + 0.1 * j for j in range(K)], axis=1) for i in range(9)]
    else:
        mk = lambda a: Padded(capi, a)                                                # noqa: E731
        get = lambda d: d.head()                                                      # noqa: E731
        run = lambda G, u, r: G.vcycle(u, r)                                          # noqa: E731
        u0 = [0.01 * inputs.v2(n, ofs=100 * i) for i in range(9)]
        rhs = [inputs.rhs2(n, ofs=7 * i) for i in range(9)]
    dU, dR = [mk(a) for a in u0], [mk(a) for a in rhs]
    eU, eR = mk(u0[0]), mk(rhs[0])
    want = []
    for i in range(9):
        eU.upload(u0[i]); eR.upload(rhs[i])
        run(Ge, eU, eR)
        want.append(get(eU).copy())
    assert len({w.tobytes() for w in want}) == 9

    def graph(i):
        dU[i].upload(u0[i])
        l0 = capi.launch_count()
        run(Gg, dU[i], dR[i])
        launches = capi.launch_count() - l0
        same_bits(get(dU[i]), want[i], i)
        return launches
    first = [graph(i) for i in range(9)]
    assert min(first) > 1                                      # nine captures
    assert graph(8) == 1 and graph(1) == 1                     # cached: a replay is one launch
    assert graph(0) > 1                                        # the first pair was evicted by the ninth: captured again
    assert graph(8) == 1 and graph(0) == 1
    assert graph(1) > 1                                        # ... which evicted the second


def test_block_graphs_are_dropped_by_set_block_lanes_and_set_solve_params(capi, hier4):
    """a cached block V-cycle after sgpu_op_set_block_lanes on A[0]: the bits of an eager hierarchy with the same lane setting --
    and, from 16 lanes per row to 1, not the stale graph's.  After sgpu_amg_set_solve_params switched smoother and sweep counts:
    the bits of a hierarchy built with those parameters"""
    K = 4
    _, Gg, (OA, _, _), (GAg, _, _) = build(capi, hier4, "jacobi", use_graph=True)
    _, Ge, _, (GAe, _, _) = build(capi, hier4, "jacobi", use_graph=False)
    n = OA[0].Mbig
    RHS, U0 = vc_columns(n, K)
    dUg, dUe, dR = Blk(capi, U0), Blk(capi, U0), Blk(capi, RHS)

    def both():
        dUg.upload(U0); dUe.upload(U0)
        l0 = capi.launch_count()
        Gg.vcycle_block(dUg, dR)
        launches = capi.launch_count() - l0
        Ge.vcycle_block(dUe, dR)
        got = dUg.get().copy()
        same_bits(got, dUe.get())
        return got, launches
    GAg[0].set_block_lanes(16); GAe[0].set_block_lanes(16)
    r16, _ = both()
    r16b, launches = both()
    assert launches == 1
    same_bits(r16b, r16)
    GAg[0].set_block_lanes(1); GAe[0].set_block_lanes(1)
    r1, launches = both()
    assert launches > 1                                        # captured again
    assert np.any(bits(r1) != bits(r16))                       # another summation order: the stale graph would have given r16
    assert sr.rel(r1, r16) <= 1e-12
    assert both()[1] == 1
    GAg[0].set_block_lanes(0); GAe[0].set_block_lanes(0)
    both()
    Gg.set_solve_params(60, 1e-8, "chebyshev", 1, 2)
    _, Gf, _, _ = build(capi, hier4, "chebyshev", pre=1, post=2, use_graph=False)
    dUg.upload(U0); dUe.upload(U0)
    l0 = capi.launch_count()
    Gg.vcycle_block(dUg, dR)
    assert capi.launch_count() - l0 > 1
    Gf.vcycle_block(dUe, dR)
    got = dUg.get().copy()
    same_bits(got, dUe.get())
    assert np.any(bits(got) != bits(r1))
    dUg.upload(U0)
    l0 = capi.launch_count()
    Gg.vcycle_block(dUg, dR)
    assert capi.launch_count() - l0 == 1
    same_bits(dUg.get(), got)


# ---------------------------------------------------------------------------
def test_an_operator_with_rows_and_no_entries(capi):
    """5 x 3, every row empty: Y = A X is written (zeros) by the scalar and the block product, U -= A E leaves U alone"""
    M, N = 5, 3
    O = orc.OracleOp(np.zeros(0, orc.COO_DTYPE), M, N, orc.split_even(M, 1), orc.split_even(N, 1), square=False)
    assert not O.matvec(np.ones(N)).any()
    G = util.gpu_operator(O)
    assert G.info()["nnz_local"] == 0 and G.info()["M"] == M
    x, y = Padded(capi, inputs.v2(N)), Padded(capi, np.full(M, SENTINEL))
    G.spmv(x, y)
    same_bits(y.head(), O.matvec(inputs.v2(N)))
    u0 = inputs.ec(M)
    u = Padded(capi, u0)
    G.prolong_correct(x, u)
    same_bits(u.head(), u0 - O.matvec(inputs.v2(N)))
    for K in KS:
        for lanes in (0, 1, 16):
            G.set_block_lanes(lanes)
            Xh = np.stack([inputs.v2(N, ofs=j) for j in range(K)], axis=1)
            Uh = np.stack([inputs.ec(M, ofs=j) for j in range(K)], axis=1)
            X, Y, U = Blk(capi, Xh), Blk(capi, np.full((M, K), SENTINEL)), Blk(capi, Uh)
            G.spmv_block(X, Y)
            same_bits(Y.get(), np.zeros((M, K)), (K, lanes))
            G.prolong_correct_block(X, U)
            same_bits(U.get(), Uh, (K, lanes))
            same_bits(X.get(), Xh)
