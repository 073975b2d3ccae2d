"""Block vectors (include/saena_gpu.h, sgpu_*_block): K right-hand sides through one pass over the operator.

Contract: every column of a block result is held to the scalar contract of tests/test_gpu_forms.py against the CPU oracle applied
to that column alone --
  * one lane per row: every epilogue equals the oracle BIT FOR BIT (the kernel adds a row's products in stored order whatever the
    row's length, the hub operator's 3 000-entry row included);
  * 4 / 16 / 64 lanes per row: |got - ref| <= 1e-13 (|A||x|)_r times the epilogue's factor plus one rounding of the epilogue's own
    operation; several sweeps within rel-l2 1e-12 (TOL and TOL_SWEEPS of test_gpu_forms.py, through its own checker);
  * column j never reads column j': permuting, zeroing or poisoning columns moves no bit of the others;
  * the scalar path on the same handles is not disturbed.
The operators are test_gpu_forms.py's builders: the smallest shapes at which the kernel can go wrong (a partial wave and a partial
last row block, empty rows, a row longer than what a workgroup stages, rectangular transfers, a smoothed-aggregation level)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import hierarchy, inputs, util
from tests import test_gpu_forms as forms

pytestmark = pytest.mark.gpu

OPERATORS = ["small", "poisson11", "empty", "hub", "P0", "R0", "L1"]
KS = [2, 4, 8]
LANES = [1, 4, 16, 64, 0]                    # 0: from the operator's mean row length
EIG, bits, klass = forms.EIG, forms.bits, forms.klass


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def column(p, j):
    """the inputs of column j (the same whatever block it sits in): distinct columns from the generators of tests/inputs.py"""
    return dict(x=inputs.v2(p.N, ofs=1000 * j) * (1.0 + 0.5 * j), rhs=inputs.rhs2(p.M, ofs=77 * j) + 0.125 * j,
                u=inputs.ec(p.M, ofs=13 * j), w=inputs.v_sin(p.M) + 2.0, c=0.37)


EPIS = ("spmv", "prolong_correct", "residual", "jacobi1", "jacobi3", "chebyshev1", "chebyshev3")
_REF = {}


def oracle_column(name, j):
    """the oracle's outputs for column j alone; computed once per (operator, column) and shared"""
    if (name, j) not in _REF:
        p = forms.problem(name)
        _REF[(name, j)] = forms.run_oracle(forms.oracle_op(p), p, column(p, j), EPIS)
    return _REF[(name, j)]


def stack(p, K, key):
    return np.stack([column(p, j)[key] for j in range(K)], axis=1)


def run_block(capi, G, p, K, X=None, epis=EPIS, RHS=None, U=None):
    """-> {entry point: (M, K) result}; X / RHS / U: the blocks, by default columns 0..K-1 in their order"""
    X = stack(p, K, "x") if X is None else X
    RHS = stack(p, K, "rhs") if RHS is None else RHS
    U = stack(p, K, "u") if U is None else U
    dX, dY = capi.BlockVector(p.N, K, X), capi.BlockVector(p.M, K)
    out = {}
    if "spmv" in epis:
        G.spmv_block(dX, dY)
        out["spmv"] = dY.download()
    if "prolong_correct" in epis:
        dU = capi.BlockVector(p.M, K, U)
        G.prolong_correct_block(dX, dU)
        out["prolong_correct"] = dU.download()
    if not p.square:
        return out
    dR = capi.BlockVector(p.M, K, RHS)
    if "residual" in epis:
        G.residual_block(dX, dR, dY)
        out["residual"] = dY.download()
    for it in (1, 3):                                           # (odd sweep counts end in the ping-pong partner: copied back)
        if f"jacobi{it}" in epis:
            dU = capi.BlockVector(p.M, K, X)
            G.jacobi_block(it, dU, dR)
            out[f"jacobi{it}"] = dU.download()
        if f"chebyshev{it}" in epis:
            dU = capi.BlockVector(p.M, K, X)
            G.chebyshev_block(it, EIG, dU, dR)
            out[f"chebyshev{it}"] = dU.download()
    return out


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", OPERATORS)
def test_every_block_entry_point_against_the_oracle_per_column(capi, name, K):
    """spmv, residual, Jacobi (1 and 3 sweeps), Chebyshev (1 and 3 steps), U -= A E at 1, 4, 16, 64 lanes per row and the
    operator's own choice"""
    p = forms.problem(name)
    G = util.gpu_operator(forms.oracle_op(p))
    for lanes in LANES:
        G.set_block_lanes(lanes)
        eff = G.block_lanes()
        assert eff in (1, 4, 16, 64) and (lanes == 0 or eff == lanes)
        got = run_block(capi, G, p, K)
        assert set(got) == (set(EPIS) if p.square else {"spmv", "prolong_correct"})
        seq = np.full(p.M, eff == 1)
        for j in range(K):
            forms.check_against_oracle(p, {k: a[:, j] for k, a in got.items()}, oracle_column(name, j), column(p, j), seq,
                                       f"{name} K={K} lanes={lanes or 'auto'} ({eff}) column {j}:")


def poisoned(p, x):
    """a column holding a NaN and an Inf"""
    x = x.copy()
    x[p.N // 3] = np.nan
    x[(2 * p.N) // 3] = -np.inf
    return x


@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("name", ["poisson11", "hub", "L1"])
def test_columns_are_independent_bit_for_bit(capi, name, lanes):
    """permuting the columns permutes the results; a zero column, or one holding a NaN and an Inf, leaves the other columns' bits
    alone -- spmv and three Jacobi sweeps; the poisoned column's NaN / Inf classes are the oracle's on that column"""
    p = forms.problem(name)
    O = forms.oracle_op(p)
    G = util.gpu_operator(O)
    G.set_block_lanes(lanes)
    K, epis = 4, ("spmv", "jacobi3")
    X = stack(p, K, "x")
    clean = run_block(capi, G, p, K, X, epis)
    perm = [2, 0, 3, 1]
    got = run_block(capi, G, p, K, X[:, perm], epis, RHS=stack(p, K, "rhs")[:, perm])      # every block of the call permuted alike
    for k in epis:
        np.testing.assert_array_equal(bits(got[k]), bits(clean[k][:, perm]), err_msg=f"{name} permuted {k}")
    j = 1
    for what, col in (("zero", np.zeros(p.N)), ("poison", poisoned(p, X[:, j]))):
        Xp = X.copy()
        Xp[:, j] = col
        got = run_block(capi, G, p, K, Xp, epis)
        others = [c for c in range(K) if c != j]
        for k in epis:
            np.testing.assert_array_equal(bits(got[k][:, others]), bits(clean[k][:, others]), err_msg=f"{name} {what} {k}")
        if what == "poison":
            v = dict(column(p, j), x=col)
            ref = forms.run_oracle(O, p, v, epis)
            for k in epis:
                np.testing.assert_array_equal(klass(got[k][:, j]), klass(ref[k]), err_msg=f"{name} poison {k}: classes")
            assert (klass(ref["spmv"]) != 0).any() and (klass(ref["spmv"]) == 0).any()


def test_a_column_s_bits_do_not_depend_on_K(capi):
    """the K instantiations perform the same operations per column: column j of a K = 8 block equals it in a K = 2 and a K = 4 block"""
    for name in ("empty", "L1"):
        p = forms.problem(name)
        G = util.gpu_operator(forms.oracle_op(p))
        G.set_block_lanes(16)
        got = {K: run_block(capi, G, p, K, None, ("spmv", "chebyshev3")) for K in KS}
        for k in ("spmv", "chebyshev3"):
            np.testing.assert_array_equal(bits(got[8][k][:, :2]), bits(got[2][k]))
            np.testing.assert_array_equal(bits(got[8][k][:, :4]), bits(got[4][k]))


def test_refusals(capi):
    p = forms.problem("small")
    G = util.gpu_operator(forms.oracle_op(p))
    for K in (1, 3, 16):
        with pytest.raises(capi.SgpuError, match="2, 4 or 8"):
            x = capi.DeviceVector(p.N * K)
            y = capi.DeviceVector(p.M * K)
            capi.check(capi.lib().sgpu_spmv_block(G.h, x.ptr, y.ptr, K))
        for fn, args in (("sgpu_residual_block", lambda d: (G.h, d.ptr, d.ptr, d.ptr, K)),
                         ("sgpu_jacobi_block", lambda d: (G.h, 1, 0.0, d.ptr, d.ptr, K)),
                         ("sgpu_chebyshev_block", lambda d: (G.h, 1, EIG, d.ptr, d.ptr, K)),
                         ("sgpu_prolong_correct_block", lambda d: (G.h, d.ptr, d.ptr, K)),
                         ("sgpu_block_pack", lambda d: (d.ptr, d.ptr, p.M, K)),
                         ("sgpu_block_unpack", lambda d: (d.ptr, d.ptr, p.M, K))):
            d = capi.DeviceVector(p.M * max(K, 1))
            assert getattr(capi.lib(), fn)(*args(d)) == -1, fn                     # SGPU_ERR_ARG
    for lanes in (2, 8, 32, 3, 128, -1):
        with pytest.raises(capi.SgpuError, match="block lanes"):
            G.set_block_lanes(lanes)
    # an operator with a remote part (two emulated ranks on the one-rank context)
    p = forms.problem("poisson11")
    W = util.EmulatedWorld(forms.oracle_op(p, 2))
    H = W.g[0]
    X, Y = capi.BlockVector(H.N_local, 2), capi.BlockVector(H.M, 2)
    with pytest.raises(capi.SgpuError, match="remote part"):
        H.spmv_block(X, Y)
    with pytest.raises(capi.SgpuError, match="remote part"):
        H.jacobi_block(1, Y, Y)


def test_the_scalar_path_is_undisturbed(capi):
    """the same handles before and after block calls: sgpu_spmv and a scalar V-cycle give the same bits, get_variant is unchanged
    and a replayed scalar V-cycle is still one launch"""
    As, Ps, Rs = hierarchy.poisson_hierarchy(18, 4)
    OA, OP, OR = hierarchy.oracle_hierarchy(As, Ps, Rs)
    GA, GP, GR = ([util.gpu_operator(o) for o in ops] for ops in (OA, OP, OR))
    A = capi.Amg(GA, GP, GR, eig_max=hierarchy.eig_estimates(As), smoother="jacobi")
    n = OA[0].Mbig
    x, rhs = inputs.v2(n), inputs.rhs2(n)
    dx, dy, dr = capi.DeviceVector(n, x), capi.DeviceVector(n), capi.DeviceVector(n, rhs)

    def scalar():
        GA[0].spmv(dx, dy)
        y = dy.download()
        du_fixed.upload(0.01 * x)
        A.vcycle(du_fixed, dr)
        l0 = capi.launch_count()
        A.vcycle(du_fixed, dr)
        return y, du_fixed.download(), capi.launch_count() - l0, [g_.variant() for g_ in GA + GP + GR], [g_.info() for g_ in GA + GP + GR]
    du_fixed = capi.DeviceVector(n)
    before = scalar()
    assert before[2] == 1
    K = 4
    X = np.stack([inputs.v2(n, ofs=j) for j in range(K)], axis=1)
    B = np.stack([inputs.rhs2(n, ofs=j) for j in range(K)], axis=1)
    dX, dY, dB = capi.BlockVector(n, K, X), capi.BlockVector(n, K), capi.BlockVector(n, K, B)
    for lanes in (0, 4, 1):
        GA[0].set_block_lanes(lanes)
        GA[0].spmv_block(dX, dY)
        GA[0].jacobi_block(3, dX, dB)
        GA[0].chebyshev_block(2, EIG, dX, dB)
        A.vcycle_block(dX, dB)
        A.vcycle_block(dX, dB)
    dU = capi.BlockVector(n, 2)
    A.solve_pCG_block(dU, capi.BlockVector(n, 2, B[:, :2]))
    after = scalar()
    np.testing.assert_array_equal(bits(after[0]), bits(before[0]))
    np.testing.assert_array_equal(bits(after[1]), bits(before[1]))
    assert after[2] == before[2] == 1 and after[3] == before[3] and after[4] == before[4]


@pytest.mark.parametrize("n", [1, 63, 64, 1000, 4097])
@pytest.mark.parametrize("K", KS)
def test_pack_unpack_round_trip(capi, n, K):
    """column-major n x K -> block -> column-major: exact, n not a multiple of 64 included; the block layout is X[i*K + j]"""
    H = np.stack([inputs.v2(n, ofs=31 * j) for j in range(K)], axis=1)
    H[0, 0], H[n - 1, K - 1] = -0.0, np.inf
    B = capi.BlockVector(n, K, H)
    np.testing.assert_array_equal(bits(B.download()), bits(H))
    raw = capi.DeviceVector(n * K)
    capi.check(capi.lib().sgpu_vec_copy(raw.ptr, B.ptr, n * K))
    np.testing.assert_array_equal(bits(raw.download().reshape(n, K)), bits(H))
