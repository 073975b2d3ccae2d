"""Block vectors on operators with a remote part: K columns through one halo exchange (one process, emulated ranks).

tests/block_world.py routes a block halo between P simulated ranks of the 1-rank context: k_pack_block packs it, the host moves the
segments (K times the scalar sizes), sgpu_debug_inject_halo_block hands it to the receiver, and the block applies that follow run
k_csr_block with the boundary mask and k_csr_boundary_block.  Contract, per column, against the CPU oracle of the same world applied
to that column alone, with the bounds tests/test_gpu_forms.py::test_emulated_halos uses (its TOL, TOL_SWEEPS and abs_bound):
  * spmv, residual, two Jacobi sweeps and one Chebyshev step (a fresh exchange per sweep), u -= A e for the transfers; K = 2, 4, 8,
    block lanes 1, 16 and the operator's own choice, fp64 and fp32 wire;
  * one lane per row: column j equals, BIT FOR BIT, the scalar emulated world on k_csr_cc16 at one lane with one lane per boundary
    row (SAENA_BOUNDARY_LANES=1: the reference's order, the local loop first and the remote contributions after it);
  * column j never reads column j': permuting the columns permutes the results, a NaN or an Inf that crosses the halo in one column
    moves no bit of the others; a column's bits depend neither on K nor on the run.
The worlds: Poisson 11^3 at 2 and 3 ranks, the hub operator (a 3 000-entry row) at 2, a full band of 64 rows at 2 (every row is a
boundary row: the interior launch writes nothing), the rectangular P0 / R0 at 2 and 3, and a split that leaves a rank without rows."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests import test_gpu_block as blk
from tests import test_gpu_forms as forms
from tests.block_world import BlockWorld

pytestmark = pytest.mark.gpu

KS = [2, 4, 8]
LANES = [1, 16, 0]
WORLDS = ["poisson11@2", "poisson11@3", "hub@2", "band64_63@2", "P0@2", "P0@3", "R0@2", "R0@3", "poisson11/norows@3"]
TOL, TOL_SWEEPS, EPS, OMEGA, EIG = forms.TOL, forms.TOL_SWEEPS, forms.EPS, forms.OMEGA, forms.EIG
bits, klass = forms.bits, forms.klass
REF_EPIS = ("spmv", "prolong_correct", "residual", "jacobi1", "chebyshev1")


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


_BAND = None


def problem(world):
    global _BAND
    name = world.split("@")[0].split("/")[0]
    if name == "band64_63":
        if _BAND is None:
            _BAND = forms.Problem(orc.band_matrix(64, 63), 64, 64, True)
        return _BAND
    return forms.problem(name)


_ORACLE = {}


def oracle_world(world, fp32):
    """the OracleOp of a world on one wire type (shared by every test; its use_double flag is set once and left)"""
    if (world, fp32) not in _ORACLE:
        p = problem(world)
        nprocs = int(world.split("@")[1])
        split = None
        if "/norows" in world:                                  # the last rank owns no row (and no column)
            split = np.array([0, p.M // 2, p.M, p.M], np.int32)
        O = forms.oracle_op(p, nprocs, split)
        O.set_use_double(not fp32)
        _ORACLE[(world, fp32)] = O
    return _ORACLE[(world, fp32)]


_REF = {}


def oracle_column(world, fp32, j):
    """the oracle's outputs of the world for column j alone; computed once and shared"""
    if (world, fp32, j) not in _REF:
        p, O = problem(world), oracle_world(world, fp32)
        v = blk.column(p, j)
        ref = forms.run_oracle(O, p, v, REF_EPIS)
        if p.square:
            ref["jacobi2"] = O.jacobi(2, v["x"], v["rhs"])
        _REF[(world, fp32, j)] = ref
    return _REF[(world, fp32, j)]


def make_world(world, fp32, monkeypatch):
    monkeypatch.setenv("SAENA_BOUNDARY_LANES", "1")           # the scalar anchor's boundary rows in the reference's order
    try:
        return BlockWorld(oracle_world(world, fp32), halo_fp32=fp32)
    finally:
        monkeypatch.delenv("SAENA_BOUNDARY_LANES", raising=False)


def block_world_outputs(capi, p, O, W, X, RHS, U):
    """forms.world_outputs on blocks: spmv, residual, two Jacobi sweeps (a block halo exchanged before each), a Chebyshev step;
    U -= A E for the transfers.  -> {entry point: (M, K)}"""
    split_r, split_c = O.split_row, O.split_col
    K = X.shape[1]
    out = {}
    Xs, Ys = W.slices_block(X, split_c), [capi.BlockVector(int(split_r[r + 1] - split_r[r]), K) for r in range(W.P)]
    W.exchange_block(Xs)
    for r in range(W.P):
        W.g[r].spmv_block(Xs[r], Ys[r])
    out["spmv"] = W.gather_block(Ys)
    if not p.square:
        Us = W.slices_block(U, split_r)
        for r in range(W.P):
            W.g[r].prolong_correct_block(Xs[r], Us[r])
        out["prolong_correct"] = W.gather_block(Us)
        return out
    Rs = W.slices_block(RHS, split_r)
    for r in range(W.P):
        W.g[r].residual_block(Xs[r], Rs[r], Ys[r])
    out["residual"] = W.gather_block(Ys)
    Us = W.slices_block(X, split_r)
    for sweep in range(2):
        W.exchange_block(Us)
        for r in range(W.P):
            W.g[r].jacobi_block(1, Us[r], Rs[r])
        out[f"jacobi{sweep + 1}"] = W.gather_block(Us)
    Us = W.slices_block(X, split_r)
    W.exchange_block(Us)
    for r in range(W.P):
        W.g[r].chebyshev_block(1, EIG, Us[r], Rs[r])
    out["chebyshev1"] = W.gather_block(Us)
    return out


def run(capi, world, W, fp32, K, cols=None, X=None):
    p = problem(world)
    cols = list(range(K)) if cols is None else cols
    st = {k: np.stack([blk.column(p, j)[k] for j in cols], axis=1) for k in ("x", "rhs", "u")}
    return block_world_outputs(capi, p, oracle_world(world, fp32), W, st["x"] if X is None else X, st["rhs"], st["u"])


def check_bounds(p, got, ref, x, where):
    """test_emulated_halos' comparison with the oracle"""
    b = forms.abs_bound(p.entries, p.M, x)
    for k, g in got.items():
        r = ref[k]
        if k in ("jacobi2", "chebyshev1"):
            err, lim = np.linalg.norm(g - r), TOL_SWEEPS * np.linalg.norm(r)
            assert err <= lim, f"{where} {k}: rel-l2 {err / np.linalg.norm(r):.3e}"
            continue
        lim = TOL * (b * np.abs(OMEGA * forms.inv_diag(p)) if k == "jacobi1" else b) + 2 * EPS * np.abs(r) + 1e-300
        bad = np.flatnonzero(~(np.abs(g - r) <= lim))
        assert bad.size == 0, f"{where} {k}: rows {bad[:10].tolist()} outside the bound"


_ANCHOR = {}


def scalar_anchor(capi, world, W, fp32, j):
    """the scalar emulated world on k_csr_cc16 at one lane (forms.ANCHOR) for column j, on the same operators"""
    if (world, fp32, j) not in _ANCHOR:
        p = problem(world)
        anchors = []
        for G in W.g:                                           # a slice k_csr_cc16 refuses (a rank without rows): k_csr_stream at one lane, the same order
            try:
                G.set_variant(forms.ANCHOR[0])
                anchors.append(forms.ANCHOR)
            except capi.SgpuError as e:
                assert forms.REFUSAL[forms.ANCHOR[0]] in str(e), str(e)
                anchors.append((0, 1, 0))
        _ANCHOR[(world, fp32, j)] = forms.world_outputs(capi, p, oracle_world(world, fp32), W, anchors, blk.column(p, j), fp32)
    return _ANCHOR[(world, fp32, j)]


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("world", WORLDS)
def test_block_halo_against_the_oracle_per_column(capi, world, K, monkeypatch):
    p = problem(world)
    if world.startswith("band64_63"):
        O = oracle_world(world, False)
        assert all(int(O.rank(r).nnz_l_remote) > 0 for r in range(2))
        rows, cols = np.asarray(p.entries["row"]), np.asarray(p.entries["col"])
        other = (rows < O.split_row[1]) != (cols < O.split_row[1])
        assert np.unique(rows[other]).size == p.M, "every row of the full band is a boundary row"
    if "/norows" in world:
        assert int(oracle_world(world, False).rank(2).M) == 0
    for fp32 in (False, True):
        W = make_world(world, fp32, monkeypatch)
        for lanes in LANES:
            W.set_block_lanes(lanes)
            eff = [G.block_lanes() for G in W.g]
            got = run(capi, world, W, fp32, K)
            assert set(got) == ({"spmv", "residual", "jacobi1", "jacobi2", "chebyshev1"} if p.square else {"spmv", "prolong_correct"})
            for j in range(K):
                where = f"{world} K={K} lanes={lanes or 'auto'} {eff} fp32={fp32} column {j}:"
                gj = {k: a[:, j] for k, a in got.items()}
                check_bounds(p, gj, oracle_column(world, fp32, j), blk.column(p, j)["x"], where)
                if lanes == 1:
                    anchor = scalar_anchor(capi, world, W, fp32, j)
                    for k in anchor:
                        np.testing.assert_array_equal(bits(gj[k]), bits(anchor[k]), err_msg=f"{where} {k} against the scalar world")
            if lanes == 1:                                        # a second run gives the same bits
                again = run(capi, world, W, fp32, K)
                for k in got:
                    np.testing.assert_array_equal(bits(again[k]), bits(got[k]), err_msg=f"{world} K={K} fp32={fp32} {k}: second run")


def crossing_columns(O):
    """global column indices whose x value is packed into some rank's send buffer"""
    out = []
    for r in range(O.nprocs):
        R = O.rank(r)
        vi = O.rank_array(r, "vIndex", R.vIndexSize, np.int32)
        if vi.size:
            out += [int(O.split_col[r]) + int(vi[0]), int(O.split_col[r]) + int(vi[-1])]
    return out


@pytest.mark.parametrize("lanes", [1, 16])
@pytest.mark.parametrize("world", ["poisson11@3", "hub@2", "P0@2"])
def test_columns_stay_independent_across_the_halo(capi, world, lanes, monkeypatch):
    """permuting the columns permutes the results bit for bit; a NaN and an Inf that cross the halo in one column leave the other
    columns' bits alone, and the poisoned column's NaN / Inf classes are the oracle's on that column"""
    p = problem(world)
    for fp32 in (False, True):
        O = oracle_world(world, fp32)
        W = make_world(world, fp32, monkeypatch)
        W.set_block_lanes(lanes)
        K = 4
        clean = run(capi, world, W, fp32, K)
        perm = [2, 0, 3, 1]
        got = run(capi, world, W, fp32, K, cols=perm)
        for k in clean:
            np.testing.assert_array_equal(bits(got[k]), bits(clean[k][:, perm]), err_msg=f"{world} fp32={fp32} permuted {k}")
        cross = crossing_columns(O)
        assert len(cross) >= 2
        j = 1
        X = np.stack([blk.column(p, c)["x"] for c in range(K)], axis=1)
        X[cross[0], j], X[cross[-1], j] = np.nan, -np.inf
        got = run(capi, world, W, fp32, K, X=X)
        others = [c for c in range(K) if c != j]
        for k in clean:
            np.testing.assert_array_equal(bits(got[k][:, others]), bits(clean[k][:, others]), err_msg=f"{world} fp32={fp32} poison {k}")
        ref = forms.run_oracle(O, p, dict(blk.column(p, j), x=X[:, j]), ("spmv",))["spmv"]
        np.testing.assert_array_equal(klass(got["spmv"][:, j]), klass(ref), err_msg=f"{world} fp32={fp32} poison: classes")
        assert (klass(ref) != 0).any() and (klass(ref) == 0).any()
        assert (klass(got["spmv"][:, j]) != klass(clean["spmv"][:, j])).any(), "the poison crossed the halo"


@pytest.mark.parametrize("world", ["poisson11@3", "hub@2"])
def test_a_column_s_bits_do_not_depend_on_K_across_the_halo(capi, world, monkeypatch):
    for fp32 in (False, True):
        W = make_world(world, fp32, monkeypatch)
        W.set_block_lanes(16)
        got = {K: run(capi, world, W, fp32, K) for K in KS}
        for k in got[8]:
            np.testing.assert_array_equal(bits(got[8][k][:, :2]), bits(got[2][k]), err_msg=f"{world} fp32={fp32} {k}: K = 8 against 2")
            np.testing.assert_array_equal(bits(got[8][k][:, :4]), bits(got[4][k]), err_msg=f"{world} fp32={fp32} {k}: K = 8 against 4")


def test_the_dense_variant_with_a_halo_runs_the_block_path_from_its_csr(capi, monkeypatch):
    """an operator on the dense scalar form (variant 5) still holds the CSR of both parts and the boundary mask: the block applies
    give the bits they give on the default form, and the oracle's numbers"""
    world = "dense@2"
    p = forms.problem("dense")
    K = 4
    W = make_world(world, False, monkeypatch)
    W.set_block_lanes(1)
    before = run(capi, world, W, False, K)
    for G in W.g:
        G.set_variant(5)
        assert G.variant()[0] == 5
    after = run(capi, world, W, False, K)
    for k in before:
        np.testing.assert_array_equal(bits(after[k]), bits(before[k]), err_msg=k)
    for j in range(K):
        check_bounds(p, {k: a[:, j] for k, a in after.items()}, oracle_column(world, False, j), blk.column(p, j)["x"], f"dense@2 variant 5 column {j}:")


def test_refusals_that_remain(capi, monkeypatch):
    p = problem("poisson11@2")
    W = make_world("poisson11@2", False, monkeypatch)
    H = W.g[0]
    X, Y = capi.BlockVector(H.N_local, 2), capi.BlockVector(H.M, 2)
    with pytest.raises(capi.SgpuError, match="remote part"):        # no block halo injected in a one-rank context
        H.spmv_block(X, Y)
    H.debug_inject_halo(np.zeros(int(W.plans[0][4].sum())))          # a scalar halo is not a block halo
    with pytest.raises(capi.SgpuError, match="remote part"):
        H.spmv_block(X, Y)
    H.debug_inject_halo_block(np.zeros((int(W.plans[0][4].sum()), 2)))
    H.spmv_block(X, Y)                                                # injected for K = 2 ...
    X4, Y4 = capi.BlockVector(H.N_local, 4), capi.BlockVector(H.M, 4)
    with pytest.raises(capi.SgpuError, match="remote part"):        # ... and not for K = 4
        H.residual_block(X4, Y4, Y4)
    # a hierarchy over an operator with a remote part: the block V-cycle and pCG want its halo, LOBPCG and FGMRES stay one rank
    W2 = make_world("poisson11@2", False, monkeypatch)
    A = capi.Amg([W2.g[0]], [], [], coarse_solver="cg")
    n = W2.g[0].M
    U, B = capi.BlockVector(n, 2), capi.BlockVector(n, 2)
    with pytest.raises(capi.SgpuError, match="remote part"):
        A.vcycle_block(U, B)
    with pytest.raises(capi.SgpuError, match="remote part"):
        A.solve_pCG_block(U, B)
    W2.g[0].debug_inject_halo_block(np.zeros((int(W2.plans[0][4].sum()), 2)))
    with pytest.raises(capi.SgpuError, match="remote part"):        # an injected block halo does not lift LOBPCG's refusal
        A.lobpcg(U, 1)
    u, b = capi.DeviceVector(n), capi.DeviceVector(n)
    with pytest.raises(capi.SgpuError, match="remote part"):
        A.solve_fgmres(u, b)
