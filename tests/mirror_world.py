"""The mirror world: a reference for the exchanged apply that works for any operator.

Take S (M x N) and split its entries into S = B + C.  The 2-rank global operator G = [[B, C], [C, B]], rows split [0, M, 2M],
columns split [0, N, 2N], applied to the duplicated vector [x; x], gives S x on both ranks.  Rank 0 of OracleOp(G) has one
neighbour each way, sends exactly what it receives (vIndexSize == recvSize, its vIndex is rank 1's), so its descriptor with the peer
rewired to itself runs over a 1-rank communicator and exchanges for real: what arrives is what rank 1 would have sent.

C is chosen by a mask: a boolean array over the columns (the masked columns go to C; on a square S the diagonal always stays in B, so
inv_diag is S's), or ("rows", [r, ...]): the off-diagonal entries of those rows.

No GPU import here: tests/test_mirror_world.py proves the construction on the CPU, tests/rccl_mirror.py runs it on a card."""
from collections import namedtuple

import numpy as np

from oracle import oracle as orc
from tests import hierarchy, inputs
from tests import test_gpu_forms as F

EPS = np.finfo(np.float64).eps
PACK_GRID_STRIDE = 32768                     # PACK_MAX_BLOCKS x BLOCK of the pack kernel: more halo entries than this and its blocks loop


# ---- the construction ------------------------------------------------------------------------------------------------------------
def in_c(p, mask):
    """-> per entry of p.entries: True where it goes to C"""
    e = p.entries
    if isinstance(mask, tuple):
        assert mask[0] == "rows"
        pick = np.zeros(p.M, bool)
        pick[np.asarray(mask[1])] = True
        return pick[e["row"]] & (e["row"] != e["col"])
    mask = np.asarray(mask, bool)
    assert mask.shape == (p.N,)
    c = mask[e["col"]]
    return c & (e["row"] != e["col"]) if p.square else c


def mirror(p, mask):
    """-> (COO entries of G = [[B, C], [C, B]], 2M, 2N)"""
    e, c = p.entries, in_c(p, mask)
    row, col, val = e["row"].astype(np.int64), e["col"].astype(np.int64), e["val"]
    rows = np.concatenate([row, row + p.M])
    cols = np.concatenate([np.where(c, col + p.N, col), np.where(c, col, col + p.N)])
    return orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), np.concatenate([val, val])), 2 * p.M, 2 * p.N


def mirror_oracle(p, mask):
    """the 2-rank OracleOp of the mirrored operator"""
    G, M2, N2 = mirror(p, mask)
    sr, sc = np.array([0, p.M, 2 * p.M], np.int32), np.array([0, p.N, 2 * p.N], np.int32)
    return orc.OracleOp(G, M2, N2, sr) if p.square else orc.OracleOp(G, M2, N2, sr, sc, square=False)


def rank0_descriptor(O, halo_fp32=False):
    """rank 0's arrays of the 2-rank oracle as capi.Operator's keywords, its peer rewired to itself; every other array the oracle's"""
    R = O.rank(0)
    arr = lambda name, cnt, dt: O.rank_array(0, name, cnt, dt)     # noqa: E731
    d = dict(M=R.M, N_local=int(O.split_col[1] - O.split_col[0]), col_offset=0,
             nnzPerRow_local=arr("nnzPerRow_local", R.M, np.int32), col_local=arr("col_local", R.nnz_l_local, np.int32),
             val_local=arr("val_local", R.nnz_l_local, np.float64), halo_fp32=halo_fp32,
             inv_diag=arr("inv_diag", R.M, np.float64) if bool(R.inv_diag) and R.M > 0 else None)
    if R.numRecvProc or R.numSendProc:
        assert R.numRecvProc == 1 and R.numSendProc == 1 and R.vIndexSize == R.recvSize
        d.update(nnzPerCol_remote=arr("nnzPerCol_remote", R.col_remote_size, np.int32), row_remote=arr("row_remote", R.nnz_l_remote, np.int32),
                 val_remote=arr("val_remote", R.nnz_l_remote, np.float64), recvProcRank=[0], recvProcCount=arr("recvProcCount", 1, np.int32),
                 sendProcRank=[0], sendProcCount=arr("sendProcCount", 1, np.int32), vIndex=arr("vIndex", R.vIndexSize, np.int32))
    return d


def v_index(O, r=0):
    return O.rank_array(r, "vIndex", O.rank(r).vIndexSize, np.int32)


def boundary_rows(O):
    """rows of rank 0 that own a remote entry, ascending"""
    R = O.rank(0)
    return np.unique(O.rank_array(0, "row_remote", R.nnz_l_remote, np.int32))


_ROW_ORDER = {}


def _row_order(p):
    """the entries of p in row-major order, columns ascending (computed once per operator)"""
    k = id(p.entries)
    if k not in _ROW_ORDER:
        _ROW_ORDER[k] = (p.entries, np.lexsort((p.entries["col"], p.entries["row"])))
    return _ROW_ORDER[k][1]


def apply_plain(p, x, mask, fp32=False):
    """S x by a plain fp64 row loop, entries of a row in ascending column order; on the fp32 wire the x of the entries in C goes
    through float, and nothing else does"""
    e, c, order = p.entries, in_c(p, mask), _row_order(p)
    x = np.asarray(x, np.float64)
    xw = x.astype(np.float32).astype(np.float64) if fp32 else x
    row, col, val, c = e["row"][order], e["col"][order], e["val"][order], c[order]
    # bincount's loop is y[row[k]] += product k for k in order: each row's products rounded, then added one by one, columns ascending
    return np.bincount(row, weights=val * np.where(c, xw[col], x[col]), minlength=p.M)


def abs_bound(p, x):
    """(|S| |x|)_r"""
    e = p.entries
    return np.bincount(e["row"], weights=np.abs(e["val"] * np.asarray(x, np.float64)[e["col"]]), minlength=p.M)


def rank0(O, v2):
    """rank 0's slice of a 2-rank row vector"""
    return v2[:O.split_row[1]]


def rank1(O, v2):
    return v2[O.split_row[1]:]


# ---- the catalogue ---------------------------------------------------------------------------------------------------------------
# claims: what the case is in the catalogue for, asserted on the CPU -- halo_over: more halo entries than this; boundary: the
# boundary rows, as an array or "all"; halo: the halo length
# forms: the case runs under every form of tests/test_gpu_forms.py that takes rank 0's local part; block: under the block applies too
Case = namedtuple("Case", "name problem mask claims block forms", defaults=(False, False))
OPERATORS = [n for n in F.HALO_OPERATORS if n != "poisson20" and "/" not in n]
BLOCK_K = (2, 8)
EDGE_ROWS = [0, 31, 32, 63, 64, 2016]        # first and last bit of mask words 0 and 1, first bit of word 2, the only bit of the last word


def _bidiagonal(M=40000):
    """diagonal and first superdiagonal"""
    i = np.arange(M)
    rows, cols = np.concatenate([i, i[:-1]]), np.concatenate([i, i[:-1] + 1])
    vals = np.concatenate([4.0 + np.sin(0.01 * i), -1.0 - 0.5 * np.cos(0.03 * i[:-1])])
    return F.Problem(orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals), M, M, True)


def _tridiagonal(M=2017):
    i = np.arange(M)
    rows, cols = np.concatenate([i, i[:-1], i[1:]]), np.concatenate([i, i[:-1] + 1, i[1:] - 1])
    vals = np.concatenate([4.0 + np.sin(0.01 * i), -1.0 - 0.5 * np.cos(0.03 * i[:-1]), -1.0 + 0.25 * np.sin(0.07 * i[1:])])
    return F.Problem(orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals), M, M, True)


def _circulant(M=16384, half=6):
    """the diagonal and the columns i - half .. i + half + 2, wrapping round (as many odd offsets as even ones): with every second
    column masked each row keeps its diagonal and half + 1 entries, an even count, and the 256 nnz-balanced row chunks of the x-in-LDS
    plan hold 64 rows each -- whole slices of k_sellx"""
    i = np.arange(M)
    offs = np.array([s for s in range(-half, half + 3) if s])
    rows = np.concatenate([i, np.repeat(i, offs.size)])
    cols = np.concatenate([i, ((i[:, None] + offs[None, :]) % M).ravel()])
    vals = np.concatenate([30.0 + np.sin(0.01 * i), -1.0 - 0.5 * np.cos(0.03 * rows[M:] + 0.11 * cols[M:])])
    return F.Problem(orc.coo_from_arrays(rows.astype(np.int32), cols.astype(np.int32), vals), M, M, True)


_OWN = {}
_MAKE = {"bidiagonal": _bidiagonal, "tridiagonal": _tridiagonal, "circulant": _circulant}


def problem(name):
    if name in _MAKE:
        if name not in _OWN:
            _OWN[name] = _MAKE[name]()
        return _OWN[name]
    return F.problem(name)


def every(k, n):
    return np.arange(n) % k == 0


def catalogue():
    cases = [Case(f"{n}%5", n, every(5, problem(n).N), {}, n in ("poisson13", "hub"), True) for n in OPERATORS]
    # every fifth column out leaves no operator of the set with the ONE table of row patterns that k_sellp, k_sellp2 and k_vidx need, nor
    # with k_sellx's padding (<= 25 % over slices of 64 rows in each of 256 row chunks): the last three planes of the Poisson cube
    # masked keep the local part's rows to a handful of patterns, the circulant's chunks are whole slices of even rows
    cases.append(Case("poisson13/last-planes", "poisson13", np.arange(1331) >= 8 * 121, dict(halo=3 * 121), False, True))
    cases.append(Case("circulant%2", "circulant", every(2, 16384), dict(halo=8192, boundary="all"), False, True))
    nine_of_ten = ~every(10, 40000)
    cases.append(Case("long-halo", "bidiagonal", nine_of_ten, dict(halo=36000, halo_over=PACK_GRID_STRIDE, boundary=np.flatnonzero(nine_of_ten[1:])), True))
    cases.append(Case("all-boundary", "band", np.ones(1000, bool), dict(boundary="all")))
    cases.append(Case("mask-edges", "tridiagonal", ("rows", EDGE_ROWS), dict(boundary=np.array(EDGE_ROWS)), True))
    return cases


def case_vectors(p, k=0):
    """the k-th input set of a case: four different inputs for the back-to-back applies"""
    return dict(x=inputs.v2(p.N, ofs=37 * k) * (1.0 + 0.5 * k), rhs=inputs.rhs2(p.M, ofs=11 * k), w=inputs.v_sin(p.M, ofs=5 * k) + 2.0, c=0.37,
                u=inputs.rhs2(p.M, ofs=3 + 7 * k))


# ---- hierarchies -----------------------------------------------------------------------------------------------------------------
HIER_MASKS = (3, 4, 5, 2)                    # level l: every HIER_MASKS[l]-th column of A_l, P_l (columns of level l + 1) and R_l


def hier():
    return hierarchy.poisson_hierarchy(18, 4)


def _as_problem(S, square):
    return F.Problem(hierarchy.scipy_to_coo(S), S.shape[0], S.shape[1], square)


def mirror_hierarchy(As, Ps, Rs, coarsest=False):
    """-> (OA, OP, OR): 2-rank OracleOps of the mirrored levels; the coarsest A is mirrored only when asked (otherwise [[A, 0], [0, A]]:
    rank 0's share is the one-rank operator, no halo)"""
    L = len(As)
    OA = [mirror_oracle(_as_problem(A, True), every(HIER_MASKS[l], A.shape[1]) if (l < L - 1 or coarsest) else np.zeros(A.shape[1], bool))
          for l, A in enumerate(As)]
    OP = [mirror_oracle(_as_problem(P, False), every(HIER_MASKS[l], P.shape[1])) for l, P in enumerate(Ps)]
    OR = [mirror_oracle(_as_problem(R, False), every(HIER_MASKS[l], R.shape[1])) for l, R in enumerate(Rs)]
    return OA, OP, OR


def rank0_hierarchy(OA, OP, OR, halo_fp32=False):
    """rank 0's descriptors of every level, peers rewired"""
    return [rank0_descriptor(o, halo_fp32) for o in OA], [rank0_descriptor(o, halo_fp32) for o in OP], [rank0_descriptor(o, halo_fp32) for o in OR]


def twice(v):
    return np.concatenate([v, v])
