"""update2 restated the plain way: new operator values through the transfer operators a hierarchy already has.  Built from
tests/setup_ref.py (galerkin, filter, filter_thresholds, lanczos_eig), which tests/test_setup_ref.py anchors; it shares no
code with saena_amd/csrc/host/amg_setup.cpp.

  update2   level 0 is A_new.  For every coarsening step l, in order, with the step's P and R as they are: A_(l+1) = (R A_l) P
            by setup_ref.galerkin (the products' drop rule included), then the filter at the threshold the SETUP's schedule has
            at step l -- the schedule is walked again from its start, from the options -- where that step is filtered.  The
            number of levels is the hierarchy's.  Nothing of the old A_(l+1) enters: not its values, not its pattern.
  update1   level 0 is A_new, every other level is the old one.

Also here: the inputs of tests/test_update_contract.py and tests/test_gpu_update.py -- operators of one size with other values or
another pattern, made from the entries of an assembled operator -- and what a hierarchy is hashed by."""
import hashlib

import numpy as np

from saena_amd import host
from tests import setup_ref


def levels_of(S):
    """the product's hierarchy as setup_ref.Level records (A, P, R as Csr; the aggregates where the setup kept them)"""
    out = []
    n = S.num_levels
    for l in range(n):
        A = setup_ref.from_layout(S.level_layout(l, 0))
        if l == n - 1:
            out.append(setup_ref.Level(A, None, None, None, None, 0))
            continue
        agg, nagg = S.level_aggregates(l)
        out.append(setup_ref.Level(A, agg, nagg, setup_ref.from_layout(S.level_layout(l, 1)), setup_ref.from_layout(S.level_layout(l, 2)), 0))
    return out


def update2(levels, A_new, options):
    """-> [A of every level] of the updated hierarchy; levels: [setup_ref.Level] (P and R are read, nothing else)"""
    steps = len(levels) - 1
    thre = setup_ref.filter_thresholds(options, steps)
    out, A = [A_new], A_new
    for step in range(steps):
        A = setup_ref.galerkin(levels[step].R, A, levels[step].P)
        if thre[step] is not None:
            A = setup_ref.filter(A, thre[step])
        out.append(A)
    return out


def update1(levels, A_new):
    return [A_new] + [lv.A for lv in levels[1:]]


# ---- inputs -----------------------------------------------------------------------------------------------------------
def entries_of(A):
    """(rows, cols, vals) of an assembled one-rank host.Matrix, row-major"""
    c = setup_ref.from_layout(A.layout())
    return setup_ref.rows_of(c).astype(np.int32), c.col.astype(np.int32), c.val.copy()


def matrix_from(rows, cols, vals, which="host", kind="self"):
    """an assembled operator of exactly these entries (no boundary row is removed: the size is the point)"""
    B = host.Matrix(host.Comm(which, kind))
    B.set_remove_boundary(False)
    B.set_many(np.asarray(rows, np.int32), np.asarray(cols, np.int32), np.asarray(vals, np.float64))
    return B.assemble()


def _pair_noise(rows, cols):
    """one number in [-1, 1) per entry, the same for (i, j) and (j, i)"""
    lo, hi = np.minimum(rows, cols).astype(np.uint64), np.maximum(rows, cols).astype(np.uint64)
    x = (lo * np.uint64(2654435761) + hi * np.uint64(40503) + np.uint64(12345)) % np.uint64(1 << 20)
    return x.astype(np.float64) / float(1 << 19) - 1.0


def variant(A, kind):
    """entries of an operator of A's size: 'copy' the same entries; 'shift' a positive field added to the diagonal; 'perturb'
    every entry scaled by 1 + 0.2 s_ij with s symmetric in (i, j); 'pattern' symmetric pairs (i, j), (j, i) of entries A does not
    store, small and negative, their weight added to both diagonals; 'scale' every entry times 0.05 (values cross a filter's
    threshold without any single entry standing out)"""
    r, c, v = entries_of(A)
    n = int(A.num_rows)
    on = r == c
    if kind == "copy":
        return r, c, v
    if kind == "shift":
        field = np.abs(v[on]).mean() * (0.25 + 0.5 * (np.arange(n) % 5) / 4.0)
        v = v.copy()
        v[on] = v[on] + field[r[on]]
        return r, c, v
    if kind == "perturb":
        return r, c, v * (1.0 + 0.2 * _pair_noise(r, c))
    if kind == "scale":
        return r, c, v * 0.05
    if kind == "pattern":
        i = np.arange(0, n - 11, 3, dtype=np.int64)
        j = i + 11
        have = set((r.astype(np.int64) * n + c).tolist())
        new = np.array([(a * n + b) not in have and (b * n + a) not in have for a, b in zip(i.tolist(), j.tolist())], bool)
        i, j = i[new], j[new]
        assert len(i) > n // 8, "the case must add entries"
        w = 0.01 * np.abs(v[on]).mean() * (1.0 + (i % 7) / 7.0)
        v = v.copy()
        d = np.zeros(n)
        np.add.at(d, i, w); np.add.at(d, j, w)
        v[on] = v[on] + d[r[on]]
        return (np.concatenate([r, i, j]).astype(np.int32), np.concatenate([c, j, i]).astype(np.int32), np.concatenate([v, -w, -w]))
    raise ValueError(kind)


def csr_of_entries(n, rows, cols, vals):
    return setup_ref.from_coo(n, np.asarray(rows, np.int64), np.asarray(cols, np.int64), vals)


# ---- what "the hierarchy is as it was" is measured by --------------------------------------------------------------------
def state(S, aggregates=True):
    """sha256 of every array of every level's A, P and R (and of the aggregates), the rows and the eigenvalue estimates"""
    out = {"levels": S.num_levels}
    for l in range(S.num_levels):
        info = S.level_info(l)
        out[f"{l}.info"] = (info["rows"], info["nnzA"], info["nnzP"], float(info["eig_max"]).hex())
        for which in (0, 1, 2) if l < S.num_levels - 1 else (0,):
            d = S.level_layout(l, which)
            for k, a in d.items():            # local and remote parts, the halo plan, inv_diag
                if isinstance(a, np.ndarray):
                    out[f"{l}.{'APR'[which]}.{k}"] = hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()
        if aggregates and l < S.num_levels - 1:
            out[f"{l}.agg"] = hashlib.sha256(np.ascontiguousarray(S.level_aggregates(l)[0]).tobytes()).hexdigest()
    return out


def transfers(state_):
    """the part of state() an update must leave alone: P, R and the aggregates"""
    return {k: v for k, v in state_.items() if ".P." in k or ".R." in k or k.endswith(".agg") or k == "levels"}
