"""Block V-cycle and block pCG (sgpu_vcycle_block, sgpu_solve_pCG_block) against the oracle's vcycle / solve_pCG applied to every
column alone, on the hierarchy of tests/test_gpu_vcycle.py (4096 -> 512 -> 64 -> 8 rows) and with its bounds: a V-cycle within
rel-l2 1e-11 per column; pCG with the oracle's iteration count per column, every history entry within 1e-10 ||r_0|| and 1e-6 of its
own size, the solution within rel-l2 1e-9."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import hierarchy, inputs, util
from tests.test_gpu_vcycle import TOL_HIST, TOL_VCYCLE, build, rel

pytestmark = pytest.mark.gpu
M_GRID = 18
TOL_SOLVE = 1e-8


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def hier():
    return hierarchy.poisson_hierarchy(M_GRID, 4)


def vc_column(n, j):
    return inputs.rhs2(n, ofs=50 * j) + 0.1 * j, 0.01 * inputs.v2(n, ofs=9 * j)


_VC_REF = {}


def vc_oracle(O, key, n, j):
    if (key, j) not in _VC_REF:
        rhs, u0 = vc_column(n, j)
        _VC_REF[(key, j)] = O.vcycle(u0, rhs)
    return _VC_REF[(key, j)]


@pytest.mark.parametrize("coarse", ["direct", "CG"])
@pytest.mark.parametrize("pre,post", [(3, 3), (0, 2), (1, 0)])
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_vcycle_block(capi, hier, smoother, pre, post, coarse):
    """K = 2, 4, 8: every column within 1e-11 of the oracle's V-cycle on that column; a second run gives the same bits"""
    O, G, (OA, _, _), _ = build(capi, hier, smoother, pre, post, coarse_solver=coarse)
    n = OA[0].Mbig
    for K in (2, 4, 8):
        RHS = np.stack([vc_column(n, j)[0] for j in range(K)], axis=1)
        U0 = np.stack([vc_column(n, j)[1] for j in range(K)], axis=1)
        dU, dR = capi.BlockVector(n, K, U0), capi.BlockVector(n, K, RHS)
        G.vcycle_block(dU, dR)
        got = dU.download()
        for j in range(K):
            e = rel(got[:, j], vc_oracle(O, (smoother, pre, post), n, j))
            print(f"{smoother} ({pre},{post}) {coarse} K={K} column {j}: rel-l2 {e:.3e}")
            assert e <= TOL_VCYCLE, (K, j, e)
        dU2 = capi.BlockVector(n, K, U0)
        G.vcycle_block(dU2, dR)
        np.testing.assert_array_equal(bits(dU2.download()), bits(got))


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_block_graph_replay_equals_eager(capi, hier, smoother):
    """the captured block V-cycle, also when replayed, equals the eager launches bit for bit"""
    _, Gg, (OA, _, _), _ = build(capi, hier, smoother, use_graph=True)
    _, Ge, _, _ = build(capi, hier, smoother, use_graph=False)
    n, K = OA[0].Mbig, 4
    RHS = np.stack([vc_column(n, j)[0] for j in range(K)], axis=1)
    U0 = np.stack([vc_column(n, j)[1] for j in range(K)], axis=1)
    dUg, dUe, dR = capi.BlockVector(n, K, U0), capi.BlockVector(n, K, U0), capi.BlockVector(n, K, RHS)
    for call in range(3):
        l0 = capi.launch_count()
        Gg.vcycle_block(dUg, dR)
        launches = capi.launch_count() - l0
        Ge.vcycle_block(dUe, dR)
        np.testing.assert_array_equal(bits(dUg.download()), bits(dUe.download()))
        assert call == 0 or launches == 1                     # a replay is one launch


def klass(a):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_vcycle_block_columns_are_independent(capi, hier, smoother):
    """permuted columns give permuted results; a zero column, or one holding a NaN and an Inf, leaves the others' bits alone, and
    the poisoned column's NaN / Inf classes are those of the oracle's V-cycle on that column"""
    O, G, (OA, _, _), _ = build(capi, hier, smoother)
    n, K = OA[0].Mbig, 4
    RHS = np.stack([vc_column(n, j)[0] for j in range(K)], axis=1)
    U0 = np.stack([vc_column(n, j)[1] for j in range(K)], axis=1)

    def run(U, B):
        dU, dB = capi.BlockVector(n, K, U), capi.BlockVector(n, K, B)
        G.vcycle_block(dU, dB)
        return dU.download()
    clean = run(U0, RHS)
    perm = [3, 1, 0, 2]
    np.testing.assert_array_equal(bits(run(U0[:, perm], RHS[:, perm])), bits(clean[:, perm]))
    j, others = 2, [0, 1, 3]
    Bz, Uz = RHS.copy(), U0.copy()
    Bz[:, j] = 0.0; Uz[:, j] = 0.0
    got = run(Uz, Bz)
    np.testing.assert_array_equal(bits(got[:, others]), bits(clean[:, others]))
    assert not got[:, j].any()
    Bp = RHS.copy()
    Bp[n // 3, j], Bp[n // 2, j] = np.nan, np.inf
    got = run(U0, Bp)
    np.testing.assert_array_equal(bits(got[:, others]), bits(clean[:, others]))
    want = O.vcycle(U0[:, j], Bp[:, j])
    assert (klass(want) != 0).any()
    np.testing.assert_array_equal(klass(got[:, j]), klass(want))


# ---- pCG -------------------------------------------------------------------------------------------------------------------------
EXPECTED_ITERS = {"jacobi": [7, 8, 6, 7], "chebyshev": [6, 7, 6, 7]}      # the oracle's solve_pCG, (3,3) sweeps, tol 1e-8


def pcg_columns(n):
    e_mid = np.zeros(n)
    e_mid[n // 2] = 1.0
    return [orc.laplacian3d_rhs(M_GRID), inputs.rhs2(n), inputs.ec(n), e_mid]


_PCG_REF = {}


def pcg_oracle(O, smoother, n):
    """-> [(u, iters, history)] of the four columns, once per smoother"""
    if smoother not in _PCG_REF:
        _PCG_REF[smoother] = [O.solve_pCG(c) for c in pcg_columns(n)]
    return _PCG_REF[smoother]


def check_column(got_u, it_g, hist_g, ref, scale=1.0, what=""):
    u_o, it_o, hist_o = ref
    hist_o = scale * hist_o
    print(f"{what}: iters {it_g} (oracle {it_o}), max |hist - oracle| / r0 = {np.max(np.abs(hist_g - hist_o[:len(hist_g)])) / hist_o[0]:.3e}, "
          f"rel-l2 of u {rel(got_u, scale * u_o):.3e}")
    assert it_g == it_o, (what, it_g, it_o)
    assert len(hist_g) == len(hist_o), (what, len(hist_g), len(hist_o))
    assert np.all(np.abs(hist_g - hist_o) <= TOL_HIST * hist_o[0]), (what, hist_g, hist_o)
    assert np.all(np.abs(hist_g - hist_o) <= 1e-6 * hist_o), (what, hist_g, hist_o)
    assert rel(got_u, scale * u_o) <= 1e-9, what


def solve_block(capi, G, n, cols):
    K = len(cols)
    dU, dB = capi.BlockVector(n, K), capi.BlockVector(n, K, np.stack(cols, axis=1))
    it, hist, conv = G.solve_pCG_block(dU, dB)
    return dU.download(), it, hist, conv


@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_pcg_block(capi, hier, smoother):
    """K = 4, 2 and 8: columns that converge at different iterations, each with the oracle's count, history and solution; a zero
    column; columns scaled by 4; a K = 4 solve equals two K = 2 solves bit for bit"""
    O, G, (OA, _, _), _ = build(capi, hier, smoother, tol=TOL_SOLVE)
    n = OA[0].Mbig
    cols = pcg_columns(n)
    ref = pcg_oracle(O, smoother, n)
    # preconditions, on the oracle: the columns stop at different iterations, and no ||r_k|| lies within 10 % of its column's
    # threshold tol ||r_0|| -- so a summation-order difference cannot flip a count
    assert [r[1] for r in ref] == EXPECTED_ITERS[smoother]
    assert len({r[1] for r in ref}) >= 2
    for _, _, h in ref:
        ratio = h / (TOL_SOLVE * h[0])
        assert not np.any((ratio > 0.9) & (ratio < 1.1)), ratio

    u4, it4, hist4, conv = solve_block(capi, G, n, cols)
    assert conv
    for j in range(4):
        check_column(u4[:, j], it4[j], hist4[j], ref[j], what=f"{smoother} K=4 column {j}")

    u2, it2, hist2, conv = solve_block(capi, G, n, [cols[1], cols[2]])
    assert conv
    for j, src in enumerate((1, 2)):
        check_column(u2[:, j], it2[j], hist2[j], ref[src], what=f"{smoother} K=2 column {j}")

    # K = 8: the four columns, a zero column, three of them scaled by 4 (a power of two: the same counts, histories scaled exactly)
    cols8 = cols + [np.zeros(n)] + [4.0 * c for c in cols[:3]]
    u8, it8, hist8, conv = solve_block(capi, G, n, cols8)
    assert conv
    for j in range(4):
        check_column(u8[:, j], it8[j], hist8[j], ref[j], what=f"{smoother} K=8 column {j}")
    assert it8[4] == 0 and not u8[:, 4].any() and hist8[4].tolist() == [0.0]
    for j, src in ((5, 0), (6, 1), (7, 2)):
        check_column(u8[:, j], it8[j], hist8[j], ref[src], scale=4.0, what=f"{smoother} K=8 column {j} (4 x column {src})")
        np.testing.assert_array_equal(bits(hist8[j]), bits(4.0 * hist8[src]))
        np.testing.assert_array_equal(bits(u8[:, j]), bits(4.0 * u8[:, src]))
    # the zero column changes nothing for the others: they are what they are in a block without it
    np.testing.assert_array_equal(bits(u8[:, :4]), bits(u4))
    assert it8[:4] == it4 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(hist8[:4], hist4))

    # the K instantiations share their per-column arithmetic: a K = 4 solve is two K = 2 solves
    ua, ita, hista, _ = solve_block(capi, G, n, cols[:2])
    ub, itb, histb, _ = solve_block(capi, G, n, cols[2:])
    np.testing.assert_array_equal(bits(np.concatenate([ua, ub], axis=1)), bits(u4))
    assert ita + itb == it4
    for a, b in zip(hista + histb, hist4):
        np.testing.assert_array_equal(bits(a), bits(b))


def test_pcg_block_hits_max_iter(capi, hier):
    """max_iter = 3: SGPU_ERR_NOCONV, three iterations' history entries per column (after ||r_0||), iterates valid"""
    O, G, (OA, _, _), _ = build(capi, hier, "jacobi", max_iter=3, tol=TOL_SOLVE)
    n = OA[0].Mbig
    cols = pcg_columns(n)
    u, it, hist, conv = solve_block(capi, G, n, cols)
    assert not conv and it == [3, 3, 3, 3]
    for j in range(4):
        u_o, it_o, hist_o = O.solve_pCG(cols[j])
        assert len(hist[j]) == 4 and len(hist_o) >= 4
        assert np.all(np.abs(hist[j] - hist_o[:4]) <= TOL_HIST * hist_o[0])
        assert np.all(np.isfinite(u[:, j])) and rel(u[:, j], u_o) <= 1e-9


def test_block_hierarchy_refusals(capi, hier):
    _, G, (OA, _, _), _ = build(capi, hier, "jacobi")
    n = OA[0].Mbig
    for K in (1, 3, 16):
        d = capi.DeviceVector(n * K)
        assert capi.lib().sgpu_vcycle_block(G.h, d.ptr, d.ptr, K) == -1
        assert capi.lib().sgpu_solve_pCG_block(G.h, d.ptr, d.ptr, K, None, None, 0) == -1
