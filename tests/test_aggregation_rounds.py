"""The setup's aggregation (host/amg_setup.cpp: aggregate(), and its row-distributed form) against the reference's rounds
restated the plain way -- every undecided row scans ALL its strong neighbours in EVERY round (aggregation_1_dist,
src/saena_object_setup1.cpp:724-995; strength: src/strength_matrix.cpp:233-453, setup1:520-719).  The product evaluates a row
again only when the one row it waits for changes state and looks at nothing but the first eligible column below the diagonal
(DESIGN.md 5); on random irregular graphs -- uneven degrees, weights over four decades, so that the strength relation is far
from symmetric in which of its two tests fires -- the aggregates must be the same row for row, at one rank and row-distributed."""
import numpy as np
import pytest

from saena_amd import host
from tests import setup_ref, spgemm_ref


def random_spd_graph(n, deg, seed):
    """symmetric M-matrix of a random graph: off-diagonals -w_ij (w over four decades), diagonal = sum of the row's weights + 1"""
    rng = np.random.default_rng(seed)
    r = np.repeat(np.arange(n), deg)
    c = rng.integers(0, n, size=n * deg)
    # a few long-range edges, mostly near neighbours (so that aggregates form)
    near = rng.random(n * deg) < 0.85
    c[near] = np.clip(r[near] + rng.integers(-6, 7, size=int(near.sum())), 0, n - 1)
    keep = r != c
    r, c = r[keep], c[keep]
    lo, hi = np.minimum(r, c), np.maximum(r, c)
    e = np.unique(np.stack([lo, hi], 1), axis=0)
    w = 10.0 ** rng.uniform(-2, 2, size=len(e))
    rows = np.concatenate([e[:, 0], e[:, 1]]); cols = np.concatenate([e[:, 1], e[:, 0]]); vals = np.concatenate([-w, -w])
    diag = np.zeros(n); np.add.at(diag, rows, -vals)
    rows = np.concatenate([rows, np.arange(n)]); cols = np.concatenate([cols, np.arange(n)]); vals = np.concatenate([vals, diag + 1.0])
    return rows.astype(np.int32), cols.astype(np.int32), vals


@pytest.mark.parametrize("n,deg,seed", [(600, 4, 1), (1500, 7, 2), (2500, 3, 3)])
def test_aggregates_equal_the_plain_rounds(n, deg, seed):
    rows, cols, vals = random_spd_graph(n, deg, seed)
    L = host.load("host")
    A = host.Matrix(host.Comm("host", "self"))
    A.set_many(rows, cols, vals)
    A.assemble()
    opts = dict(host.OPTIONS001)
    S = host.AmgSolver(A, host.options(L, **opts))
    got, ngot = S.level_aggregates(0)
    Ar = setup_ref.from_coo(n, rows, cols, vals)
    want, nwant = setup_ref.plain_rounds(Ar, setup_ref.strength(Ar, opts.get("connStrength", 0.2)))
    assert ngot == nwant
    np.testing.assert_array_equal(got, want)


def gather_entries(layouts, row_split, col_split):
    """the entries (global ids, sorted by row then column) of an operator from every rank's layout of its rows: the local
    part as it stands, the halo part with slot s of rank r's receive buffer named by the sender's send list (vIndex)"""
    world = len(layouts)
    rows, cols, vals = [], [], []
    for r, d in enumerate(layouts):
        assert d["M"] == row_split[r + 1] - row_split[r] and d["col_offset"] == col_split[r]
        rows.append(np.repeat(np.arange(d["M"]), d["nnzPerRow_local"]) + row_split[r]); cols.append(d["col_local"]); vals.append(d["val_local"])
        slots = []
        for q in d["recvProcRank"]:
            src = layouts[q]
            ofs = np.concatenate([[0], np.cumsum(src["sendProcCount"])])
            k = int(np.flatnonzero(src["sendProcRank"] == r)[0])
            slots.append(src["vIndex"][ofs[k]:ofs[k + 1]] + col_split[q])
        slots = np.concatenate(slots + [np.zeros(0, np.int64)]).astype(np.int64)
        assert len(slots) == len(d["nnzPerCol_remote"]) and int(d["recvProcCount"].sum()) == len(slots)
        rows.append(d["row_remote"] + row_split[r]); cols.append(np.repeat(slots, d["nnzPerCol_remote"])); vals.append(d["val_remote"])
    rows, cols, vals = np.concatenate(rows).astype(np.int64), np.concatenate(cols).astype(np.int64), np.concatenate(vals)
    order = np.lexsort((cols, rows))
    assert world == len(row_split) - 1
    return rows[order], cols[order], vals[order]


def _worker(rank, world, name, n, deg, seed, ret):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    try:
        rows, cols, vals = random_spd_graph(n, deg, seed)
        L = host.load("host")
        A = host.Matrix(host.Comm("host", "shm", (name, rank, world)))
        mine = rows % world == rank                     # every rank contributes a share of the entries; assemble() routes them
        A.set_many(rows[mine], cols[mine], vals[mine])
        A.assemble()
        S = host.AmgSolver(A, host.options(L, **host.OPTIONS001))
        counts = [(S.level_info(l)["rows"], S.level_info(l)["nnzA"], S.level_info(l)["nnzP"]) for l in range(S.num_levels)]
        layouts = [(S.level_split(l), S.level_layout(l, 0), S.level_layout(l, 1) if l < S.num_levels - 1 else None) for l in range(S.num_levels)]
        ret[rank] = (counts, layouts)
    except Exception as e:                              # noqa: BLE001 -- reported to the parent
        ret[rank] = f"{type(e).__name__}: {e}"


@pytest.mark.parametrize("world", [2, 3])
def test_row_distributed_aggregation_builds_the_one_rank_hierarchy(world):
    """the same random graph row-distributed over 2 / 3 ranks (native shared-memory communicator): every level has the rows and
    the entries of the one-rank hierarchy -- one row joining another aggregate would change them"""
    import multiprocessing as mp
    import os
    n, deg, seed = 4000, 6, 7
    rows, cols, vals = random_spd_graph(n, deg, seed)
    L = host.load("host")
    A1 = host.Matrix(host.Comm("host", "self"))
    A1.set_many(rows, cols, vals)
    A1.assemble()
    S1 = host.AmgSolver(A1, host.options(L, **host.OPTIONS001))
    want = [(S1.level_info(l)["rows"], S1.level_info(l)["nnzA"], S1.level_info(l)["nnzP"]) for l in range(S1.num_levels)]
    assert len(want) >= 3
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_worker, args=(r, world, f"aggr_{os.getpid()}_{world}", n, deg, seed, ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(240)
        for p in procs:
            if p.is_alive():
                p.terminate()
        got = dict(ret)
    for r in range(world):
        assert not isinstance(got.get(r), str) and got.get(r) is not None, (r, got.get(r))
        assert got[r][0] == want, (r, got[r][0], want)
    # ... and the entries: every level's A and P, the ranks' rows gathered by the level's partition, are the one-rank hierarchy's
    for l in range(S1.num_levels):
        splits = [got[r][1][l][0] for r in range(world)]
        for s in splits[1:]:
            np.testing.assert_array_equal(s, splits[0])
        for which in (0, 1) if l < S1.num_levels - 1 else (0,):
            col_split = splits[0] if which == 0 else got[0][1][l + 1][0]
            rows_, cols_, vals_ = gather_entries([got[r][1][l][1 + which] for r in range(world)], splits[0], col_split)
            one = S1.level_layout(l, which)
            assert splits[0][-1] == one["M"] and col_split[-1] == one["N_local"]
            np.testing.assert_array_equal(rows_, np.repeat(np.arange(one["M"]), one["nnzPerRow_local"]), err_msg=f"level {l} op {which}: rows")
            np.testing.assert_array_equal(cols_, one["col_local"], err_msg=f"level {l} op {which}: columns")
            spgemm_ref.assert_same_values(vals_, one["val_local"], f"level {l} op {which}, {world} ranks")
