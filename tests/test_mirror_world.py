"""The mirror world's construction (tests/mirror_world.py), proved on the CPU with the oracle: for every catalogued case rank 0 of the
2-rank oracle sends exactly what it receives, both ranks compute the same bits, and those are S x to the forms' contract on both
wires; the catalogue's geometric claims hold; a hierarchy mirrored level by level is the one-rank hierarchy."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import hierarchy, inputs
from tests import mirror_world as mw
from tests.test_gpu_forms import TOL, bits
from tests.test_gpu_vcycle import TOL_HIST, TOL_VCYCLE

CASES = mw.catalogue()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_rank_0_of_the_mirrored_operator_is_the_operator(case):
    p = mw.problem(case.problem)
    O = mw.mirror_oracle(p, case.mask)
    R0, R1 = O.rank(0), O.rank(1)
    for r, R in ((0, R0), (1, R1)):
        assert R.recvSize == R.vIndexSize > 0 and R.numRecvProc == 1 and R.numSendProc == 1
        assert O.rank_array(r, "recvProcRank", 1, np.int32).tolist() == [1 - r] and O.rank_array(r, "sendProcRank", 1, np.int32).tolist() == [1 - r]
    vi = mw.v_index(O, 0)
    np.testing.assert_array_equal(vi, mw.v_index(O, 1))
    assert np.all(np.diff(vi) > 0)
    if p.square:                                               # the diagonal stayed in B: inv_diag is S's
        np.testing.assert_array_equal(bits(O.rank_array(0, "inv_diag", p.M, np.float64)), bits(mw.F.inv_diag(p)))
    # what the catalogue says the case is there for
    cl = case.claims
    if "halo" in cl:
        assert R0.vIndexSize == cl["halo"]
    if "halo_over" in cl:
        assert R0.vIndexSize > cl["halo_over"]
    if "boundary" in cl:
        want = np.arange(p.M) if isinstance(cl["boundary"], str) else cl["boundary"]
        np.testing.assert_array_equal(mw.boundary_rows(O), want)
    if case.name == "long-halo":
        assert mw.boundary_rows(O).size == p.M - p.M // 10
    if case.name == "mask-edges":
        b = mw.boundary_rows(O)
        assert sorted({int(r) >> 5 for r in b}) == [0, 1, 2, 63] and {int(r) & 31 for r in b} == {0, 31} and (p.M - 1) & 31 == 0
    x = mw.case_vectors(p)["x"]
    b = mw.abs_bound(p, x)
    for fp32 in (False, True):
        O.set_use_double(not fp32)
        y = O.matvec(mw.twice(x))
        np.testing.assert_array_equal(bits(mw.rank0(O, y)), bits(mw.rank1(O, y)))
        ref = mw.apply_plain(p, x, case.mask, fp32)
        bad = np.flatnonzero(~(np.abs(mw.rank0(O, y) - ref) <= TOL * b + 2 * mw.EPS * np.abs(ref)))
        assert bad.size == 0, f"{case.name}, fp32={fp32}: rows {bad[:10].tolist()}"
        if fp32 and case.name != "all-boundary":               # the float wire is visible (and only through C: apply_plain rounds nothing else)
            assert not np.array_equal(ref, mw.apply_plain(p, x, case.mask, False))


def test_the_catalogue_holds_the_documented_cases():
    names = [c.name for c in CASES]
    fifth = [f"{n}%5" for n in ("poisson13", "band", "L1", "P0", "R0", "empty", "hub", "dense", "uneven")]
    assert names == fifth + ["poisson13/last-planes", "circulant%2", "long-halo", "all-boundary", "mask-edges"]
    assert [c.name for c in CASES if c.forms] == fifth + ["poisson13/last-planes", "circulant%2"]      # (two operators beyond the halo tests' set: see catalogue())
    O = mw.mirror_oracle(mw.problem("circulant"), CASES[names.index("circulant%2")].mask)
    assert set(O.rank_array(0, "nnzPerRow_local", 16384, np.int32).tolist()) == {8}
    assert [c.name for c in CASES if c.block] == ["poisson13%5", "hub%5", "long-halo", "mask-edges"]
    assert [mw.problem(c.problem).M for c in CASES if c.problem in ("empty", "hub", "dense", "uneven")] == [3001, 45369, 300, 4999]


def rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.mark.parametrize("coarsest", [False, True], ids=["coarsest-plain", "coarsest-mirrored"])
@pytest.mark.parametrize("smoother", ["jacobi", "chebyshev"])
def test_a_mirrored_hierarchy_is_the_one_rank_hierarchy(smoother, coarsest):
    As, Ps, Rs = mw.hier()
    eig = hierarchy.eig_estimates(As)
    one = hierarchy.oracle_hierarchy(As, Ps, Rs)
    two = mw.mirror_hierarchy(As, Ps, Rs, coarsest)
    for ops in (one, two):
        for a, e in zip(ops[0], eig):
            a.set_eig(e)
    assert two[0][-1].rank(0).recvSize == (4 if coarsest else 0)
    n = As[0].shape[0]
    rhs_s = orc.laplacian3d_rhs(18)
    for pre, post in ((3, 3), (1, 0)):
        O1 = orc.OracleAmg(*one, pre=pre, post=post, smoother=smoother, max_iter=60, tol=1e-8)
        O2 = orc.OracleAmg(*two, pre=pre, post=post, smoother=smoother, max_iter=60, tol=1e-8)
        rhs, u0 = inputs.rhs2(n), inputs.v2(n) * 0.01
        got = O2.vcycle(mw.twice(u0), mw.twice(rhs))
        np.testing.assert_array_equal(bits(got[:n]), bits(got[n:]))
        assert rel(got[:n], O1.vcycle(u0, rhs)) <= TOL_VCYCLE
        for name in ("solve", "solve_pCG"):
            _, it1, h1 = getattr(O1, name)(rhs_s)
            u2, it2, h2 = getattr(O2, name)(mw.twice(rhs_s))
            h2 = h2 / np.sqrt(2.0)                              # the norm of the doubled vector
            assert it1 == it2 and len(h1) == len(h2), (name, it1, it2)
            assert np.all(np.abs(h2 - h1) <= TOL_HIST * h1[0]) and np.all(np.abs(h2 - h1) <= 1e-6 * h1), (name, pre, post, h1, h2)
            # only pCG under the one-sided (1, 0) cycle runs out of its 60 iterations: its whole history is held all the same
            assert (h1[-1] <= 1e-8 * h1[0]) == ((name, pre, post) != ("solve_pCG", 1, 0)), (name, pre, post, it1)
