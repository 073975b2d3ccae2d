"""Every SpMV form at its eligibility limit and one step past it (tests/form_limits.py; tests/test_form_limits.py proves on the CPU that
the pairs sit where they claim), and what sgpu_op_create requires of its input.

At the limit the form must take the operator -- a refusal is a failure -- under the expected kernel name, and meet the contract of
tests/test_gpu_forms.py: sequential forms the oracle's bits, tree forms |got - ref| <= 1e-13 (|A||x|)_r + 2 eps |ref| per row, for the
product and a fused epilogue (u -= A e; on the square operators the residual and a Jacobi sweep).  Where the kernel name does not show
the sub-form (the x-in-LDS plan: windows, their width, sums in LDS or in global memory) the plan's debug export is held to it.  One step past, the form refuses with its documented message, which carries the limit the generator was
built for (or the named next sub-form serves the operator to the same contract); the plan-time autotune then leaves a plan that
meets the per-row bound."""
import re

import numpy as np
import pytest

from oracle import oracle as orc
from tests import form_limits as L, util
from tests.test_gpu_forms import (REFUSAL, SEQ, TREE, Form, Problem, check_against_oracle, name_matches, run_gpu, run_oracle,
                                  sequential_rows, vectors)

pytestmark = pytest.mark.gpu
# the product and fused epilogues: u -= A e on the rectangular operators, the residual and a Jacobi sweep on the square ones
EPIS = {False: ("spmv", "prolong_correct"), True: ("spmv", "residual", "jacobi1")}
assert (L.SEQ, L.TREE) == (SEQ, TREE)


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


_REF = {}


def reference(key, which):
    """(operator, Problem, OracleOp, vectors, oracle outputs), computed once per operator"""
    if (key, which) not in _REF:
        op = getattr(L.case(key), which)
        p = Problem(L.coo(op), op.M, op.N, op.square)
        O = L.oracle_op(op, p.entries)
        v = vectors(p)
        _REF[(key, which)] = (op, p, O, v, run_oracle(O, p, v, EPIS[op.square]))
    return _REF[(key, which)]


def forced(capi, O, run, monkeypatch):
    """-> (operator, kernel name) or (operator, None, the refusal): created and forced under the run's environment"""
    for k, v in run.env.items():
        monkeypatch.setenv(k, v)
    try:
        G = util.gpu_operator(O)
        try:
            G.set_variant(run.variant)
        except capi.SgpuError as e:
            return G, None, str(e)
        G.set_lanes_per_row(run.lanes)
        return G, G.variant()[1], ""
    finally:
        for k in run.env:
            monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("key", list(L.GENERATORS))
def test_at_the_limit_and_one_past(capi, key, monkeypatch):
    c = L.case(key)
    for run in c.runs:
        form = Form(key, run.variant, "", run.lanes, run.cls, run.env, run.tile)
        for which, verdict in zip(("at", "past"), c.verdicts):
            if which == "past" and c.past is c.at:
                continue
            op, p, O, v, ref = reference(key, which)
            want = run.names[verdict]
            where = f"{key} ({which}: {verdict}), variant {run.variant} {run.env or ''}:"
            G, name, what = forced(capi, O, run, monkeypatch)
            if want is None:
                assert name is None, f"{where} served by {name}, expected a refusal"
                assert REFUSAL[run.variant] in what, f"{where} {what}"
                printed = tuple(int(t) for t in re.findall(r"\d+", what))
                n = len(run.printed)
                assert any(printed[i:i + n] == tuple(run.printed) for i in range(len(printed) - n + 1)), \
                    f"{where} the message carries {printed}, the generator was built for {run.printed}"
                G.autotune()                                    # the plan-time choice leaves the form out
                check_against_oracle(p, run_gpu(capi, G, p, v, ("spmv",)), ref, v, np.zeros(p.M, bool), where + " after autotune")
                continue
            assert name is not None, f"{where} refused: {what}"
            assert name_matches(form._replace(name=want), name), f"{where} served by {name}, expected {want}"
            if c.plan and run.variant in (10, 12, 16):          # the sub-form the name does not show: windows, their width, where the sums live
                plan = G.xlds_plan()
                assert (plan["windows"], plan["window_columns"], plan["sums_in_lds"]) == c.plan[verdict], f"{where} {plan}"
            check_against_oracle(p, run_gpu(capi, G, p, v, EPIS[op.square]), ref, v, sequential_rows(form, p), where)


# ---- what sgpu_op_create requires of col_local -----------------------------------------------------------------------------------
def _two_window_rows():
    """64 rows of 4 entries, two either side of column 30 000: the x-in-LDS form gives every row a chunk of its own that reaches
    over two windows of x -- the operator whose 16-bit window-relative columns wrap where a row does not ascend"""
    r = np.arange(64)[:, None]
    return L.make_op(np.full(64, 4), (r + np.array([0, 1, 30000, 30001])[None, :]).ravel(), 30100)


def _arrays(O):
    R = O.rank(0)
    return dict(M=R.M, N_local=int(O.split_col[1] - O.split_col[0]), col_offset=0,
                nnzPerRow_local=O.rank_array(0, "nnzPerRow_local", R.M, np.int32),
                col_local=O.rank_array(0, "col_local", R.nnz_l_local, np.int32),
                val_local=O.rank_array(0, "val_local", R.nnz_l_local, np.float64))


def test_create_requires_ascending_distinct_columns_per_row(capi):
    op = _two_window_rows()
    p = Problem(L.coo(op), op.M, op.N, False)
    O = L.oracle_op(op, p.entries)
    a = _arrays(O)
    np.testing.assert_array_equal(a["col_local"], op.col)          # the oracle's members are row-major with ascending columns
    G = capi.Operator(**a)                                        # the untouched arrays: accepted, and served over two windows
    G.set_variant(10); G.set_lanes_per_row(8)
    plan = G.xlds_plan()
    assert (plan["chunks"], plan["windows"], plan["max_rows_per_chunk"]) == (64, 2, 1), plan
    v = vectors(p)
    check_against_oracle(p, run_gpu(capi, G, p, v, EPIS[False]), run_oracle(O, p, v, EPIS[False]), v, np.zeros(p.M, bool), "two windows")
    k = 4 * 5 + 1                                                 # row 5: its second and third entry
    swapped = dict(a, col_local=a["col_local"].copy(), val_local=a["val_local"].copy())
    for n in ("col_local", "val_local"):
        swapped[n][[k, k + 1]] = swapped[n][[k + 1, k]]
    with pytest.raises(capi.SgpuError, match=r"row 5 of col_local steps back to column 6 at position 2 of the row"):
        capi.Operator(**swapped)
    repeated = dict(a, col_local=a["col_local"].copy())
    repeated["col_local"][k + 1] = repeated["col_local"][k]
    with pytest.raises(capi.SgpuError, match=r"row 5 of col_local repeats column 6 at position 2 of the row"):
        capi.Operator(**repeated)
    both = dict(swapped, col_local=swapped["col_local"].copy())   # several rows at fault: the lowest is named
    both["col_local"][[4 * 40, 4 * 40 + 1]] = both["col_local"][[4 * 40 + 1, 4 * 40]]
    with pytest.raises(capi.SgpuError, match=r"row 5 of col_local"):
        capi.Operator(**both)


def test_create_refuses_a_row_twice_in_one_receive_column(capi):
    """rank 0 of a band matrix on two ranks: its receive columns hold several rows each"""
    O = orc.OracleOp(orc.band_matrix(200, 9), 200, 200, orc.split_even(200, 2))
    G = util.gpu_operator(O)                                      # as the oracle lays it out: accepted
    R = O.rank(0)
    npc = O.rank_array(0, "nnzPerCol_remote", R.col_remote_size, np.int32)
    rr = O.rank_array(0, "row_remote", R.nnz_l_remote, np.int32)
    j = int(np.flatnonzero(npc >= 2)[0])
    k = int(npc[:j].sum())
    rr[k + 1] = rr[k]
    kw = dict(M=R.M, N_local=int(O.split_col[1]), col_offset=0,
              nnzPerRow_local=O.rank_array(0, "nnzPerRow_local", R.M, np.int32), col_local=O.rank_array(0, "col_local", R.nnz_l_local, np.int32),
              val_local=O.rank_array(0, "val_local", R.nnz_l_local, np.float64), nnzPerCol_remote=npc, row_remote=rr,
              val_remote=O.rank_array(0, "val_remote", R.nnz_l_remote, np.float64),
              recvProcRank=O.rank_array(0, "recvProcRank", R.numRecvProc, np.int32), recvProcCount=O.rank_array(0, "recvProcCount", R.numRecvProc, np.int32),
              sendProcRank=O.rank_array(0, "sendProcRank", R.numSendProc, np.int32), sendProcCount=O.rank_array(0, "sendProcCount", R.numSendProc, np.int32),
              vIndex=O.rank_array(0, "vIndex", R.vIndexSize, np.int32), inv_diag=O.rank_array(0, "inv_diag", R.M, np.float64))
    with pytest.raises(capi.SgpuError, match=rf"row {int(rr[k])} appears twice in receive column {j}"):
        capi.Operator(**kw)
