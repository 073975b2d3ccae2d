"""The generators of tests/form_limits.py against the limits restated there, and the plain reference against the oracle.  No GPU: this
is what keeps tests/test_gpu_form_limits.py from passing vacuously -- every at-limit operator is one the restated limit admits, every
one-past operator one it refuses (or hands to the named next sub-form), and the two differ by a single step."""
import numpy as np
import pytest

from tests import form_limits as L, inputs

KEYS = list(L.GENERATORS)


@pytest.mark.parametrize("key", KEYS)
def test_the_pair_sits_on_either_side_of_the_restated_limit(key):
    c = L.case(key)
    assert (c.predicate(c.at), c.predicate(c.past)) == c.verdicts
    assert c.verdicts[0].startswith("served")
    for run in c.runs:                                          # every forced form knows what to expect of both operators
        assert set(c.verdicts) <= set(run.names), run
        assert run.names[c.verdicts[0]] is not None
    if key != "tile":
        assert c.verdicts[0] != c.verdicts[1]


@pytest.mark.parametrize("key", [k for k in KEYS if k != "tile"])
def test_the_pair_differs_by_one_step(key):
    """at most one row's worth of entries differs between the two operators (dense: the one row more)"""
    a, p = L.case(key).at, L.case(key).past
    assert abs(p.M - a.M) <= 1 and p.N - a.N in (0, 1)
    la, lp = np.diff(a.rp), np.diff(p.rp)
    m = min(a.M, p.M)
    if key == "pattern_ids":                                    # one pattern more, in either mode
        assert [len(L.patterns(o, rb)[1]) for o in (a, p) for rb in (False, True)] == [65535, 65535, 65536, 65536]
        assert int(a.rp[-1]) // 8 + 65536 >= 3 * 65536           # the patterns' table is admitted: the ids are what refuses
        return
    if key in ("one_table", "group_table", "rowt", "longest_row", "sellpx_windows", "sellpx_lds", "sellpx_s"):
        # the step is in the patterns / templates (one more, one of another length, one an entry longer or a column wider), and every
        # row that follows the changed one changes with it
        def distinct(op):
            return {(op.col[op.rp[r]:op.rp[r + 1]] - r).tobytes() + (op.val[op.rp[r]:op.rp[r + 1]].tobytes() if key == "rowt" else b"")
                    for r in range(op.M)}
        assert 1 <= len(distinct(a) ^ distinct(p)) <= 2
        return
    changed = [r for r in np.flatnonzero(la[:m] != lp[:m])]
    same = np.flatnonzero(la[:m] == lp[:m])
    changed += [r for r in same if not np.array_equal(a.col[a.rp[r]:a.rp[r + 1]], p.col[p.rp[r]:p.rp[r + 1]])]
    assert len(changed) <= 1, changed


def test_the_printed_numbers_are_the_documented_ones():
    """what the generators were built for, spelled out: a changed constant fails here and in the GPU test until both are updated"""
    assert (L.TILE, L.ONE_TABLE, L.GROUP_TABLE, L.GROUP_ROWS, L.PATTERNS) == ((2048, 4096), 4096, 8192, 1024, 65535)
    assert (L.SPX_WINDOWS, L.SPX_LDS, L.XL_MAXT * L.XL_MAX, L.RT_BYTES, L.DENSE_ROWS) == (16, 81920, 161792, 32768, 8192)
    c = L.case("group_table")
    ids, pats = L.patterns(c.at)
    assert len(pats) + 1 + sum(1 + n for n in pats) == 8192
    ids, pats = L.patterns(c.past)
    assert len(pats) + 1 + sum(1 + n for n in pats) == 8193
    assert L.templates(L.case("rowt").at) == 431 and 431 * 7 % 2 == 1
    assert int(L.case("pair").at.rp[-1]) == 16 * 256 and int(L.case("pair").past.rp[-1]) == 16 * 256 - 1


@pytest.mark.parametrize("key", KEYS)
def test_seq_matvec_is_the_oracle_s_product(key):
    c = L.case(key)
    for op in (c.at, c.past):
        x = inputs.v2(op.N)
        np.testing.assert_array_equal(L.seq_matvec(op.rp, op.col, op.val, x).view(np.uint64), L.oracle_op(op).matvec(x).view(np.uint64))
