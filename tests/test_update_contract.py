"""saena_amg_update on the host (amg_hierarchy::update, saena_amd/csrc/host/amg_setup.cpp) against its restatement
(tests/update_ref.py, built from tests/setup_ref.py).  No device: libsaena_host.so.

The contract.  update2 leaves P, R and the aggregates of every level bit for bit and the number of levels as it was; every
level >= 1 -- pattern and values -- is the restatement's bit for bit: (R A) P by the products' contract over the KEPT transfer
operators, the filter on the setup's threshold schedule walked again from its start.  With a second matrix object of the same
entries it reproduces the hierarchy, eigenvalue estimates included, bit for bit.  update1 touches level 0 only.  A refused
update says why and leaves every array of the hierarchy as it was.  All of it at SAENA_SETUP_THREADS 1 and 16.

The eigenvalue estimate of an updated level is held to setup_ref.lanczos_eig within 1e-12 relative, the bound and the reason
of tests/test_setup_contract.py (the order of the sums in the Lanczos dots); against the product itself -- the identity case, the
thread counts -- it is bit for bit.

Cases: the irregular operators of tests/setup_cases.py (wgrid36 in the thread-count children only, SiH4 on one variant: what the
restatement of their products costs is in that file), Poisson 12^3 and 16^3 at three coarsening steps, both smoothers.  The
host hierarchy has no coarsest solver: the two of them are tests/test_gpu_update.py's."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from saena_amd import host
from tests import setup_cases, setup_ref, spgemm_ref, update_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EIG_BOUND = 1e-12


def assert_same_csr(got, want, what):
    assert (got.nrows, got.ncols) == (want.nrows, want.ncols), what
    np.testing.assert_array_equal(got.ptr, want.ptr, err_msg=f"{what}: row pointers")
    np.testing.assert_array_equal(got.col, want.col, err_msg=f"{what}: columns")
    spgemm_ref.assert_same_values(got.val, want.val, what)


@pytest.fixture(scope="module")
def tmpdir_mtx(tmp_path_factory):
    return tmp_path_factory.mktemp("mtx")


POISSON = {"poisson12": 12, "poisson16": 16}


def case_options(name, **kw):
    if name in POISSON:             # three coarsening steps whatever the aggregate counts: four levels
        return dict(host.OPTIONS001, dynamic_levels=0, max_level=3, **kw)
    return setup_cases.options(name, **kw)


def build(name, tmpdir, **kw):
    """-> (A, AmgSolver, options dict), fresh: an update changes the solver"""
    o = case_options(name, **kw)
    if name in POISSON:
        A = host.Matrix(host.Comm("host", "self")).laplacian3D(POISSON[name]).assemble()
    else:
        A = setup_cases.assemble(name, tmpdir)
    return A, host.AmgSolver(A, host.options(host.load("host"), **o)), o


def check_update2(S, before, A_new, entries, o, what):
    """S after update(A_new, 2) against the restatement over the levels `before` (update_ref.levels_of, taken before the update)"""
    n = S.level_info(0)["rows"]
    want = update_ref.update2(before, update_ref.csr_of_entries(n, *entries), o)
    assert S.num_levels == len(before), f"{what}: {S.num_levels} levels after the update, {len(before)} before"
    for l, A in enumerate(want):
        got = setup_ref.from_layout(S.level_layout(l, 0))
        assert_same_csr(got, A, f"{what} A{l}")
        d = S.level_layout(l, 0)["inv_diag"]
        np.testing.assert_array_equal(d, 1.0 / setup_ref.diagonal(A), err_msg=f"{what} inv_diag of level {l}")
        if o["smoother"] == "chebyshev":
            e, ew = S.level_info(l)["eig_max"], setup_ref.lanczos_eig(A)
            assert abs(e - ew) <= EIG_BOUND * ew, (what, l, e, ew)
    return want


# ---- identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wgrid16", "fxm3_6", "plat362", "SiH4", "poisson12", "poisson16"])
@pytest.mark.parametrize("smoother", ["chebyshev", "jacobi"])
def test_update2_with_the_same_entries_reproduces_the_hierarchy(name, smoother, tmpdir_mtx):
    A, S, _ = build(name, tmpdir_mtx, smoother=smoother)
    before = update_ref.state(S)
    if name in POISSON:
        assert S.num_levels == 4
    A2 = update_ref.matrix_from(*update_ref.variant(A, "copy"))
    S.update(A2, 2)
    A.free()                        # the old matrix may go: nothing of the hierarchy refers to it any more
    after = update_ref.state(S)
    assert after == before, {k: (before.get(k), after.get(k)) for k in set(before) | set(after) if before.get(k) != after.get(k)}


# ---- changed values, changed pattern ----------------------------------------------------------------------------------
CHANGED = [(n, k) for n in ("wgrid16", "fxm3_6", "plat362", "poisson12", "poisson16") for k in ("shift", "perturb", "pattern")] + [("SiH4", "shift")]


@pytest.mark.parametrize("name,kind", CHANGED, ids=[f"{n}-{k}" for n, k in CHANGED])
def test_update2_is_the_restatement_s(name, kind, tmpdir_mtx):
    """'shift' and 'perturb' keep the pattern of A, 'pattern' adds symmetric entries at equal size"""
    A, S, o = build(name, tmpdir_mtx, smoother="chebyshev")
    before, s0 = update_ref.levels_of(S), update_ref.state(S)
    entries = update_ref.variant(A, kind)
    if kind == "pattern":
        assert len(entries[0]) > A.nnz
    A2 = update_ref.matrix_from(*entries)
    S.update(A2, 2)
    s1 = update_ref.state(S)
    assert update_ref.transfers(s1) == update_ref.transfers(s0), "P, R or the aggregates changed"
    want = check_update2(S, before, A2, entries, o, f"{name}, {kind}")
    assert any(not np.array_equal(w.val, b.A.val) for w, b in zip(want[1:], before[1:])), "the case changes no coarse level"
    print(name, kind, [(w.nrows, len(w.col), len(b.A.col)) for w, b in zip(want, before)])


def test_a_value_crosses_the_filter_threshold(tmpdir_mtx):
    """wgrid16 under a coarse filter (1e-3, then 1e-1: every coarse level loses entries at setup), then every entry times 0.05:
    values that stayed now fall under the thresholds, so coarse levels change their STORED ENTRY COUNT -- a refresh over the old
    pattern, or a numeric-only product into it, cannot produce these levels"""
    kw = dict(filter_thre=1e-3, filter_max=1e-1)
    A, S, o = build("wgrid16", tmpdir_mtx, smoother="chebyshev", **kw)
    before = update_ref.levels_of(S)
    assert setup_ref.filter_thresholds(o, 3) == [1e-3, 1e-1, 1e-1]
    entries = update_ref.variant(A, "scale")
    A2 = update_ref.matrix_from(*entries)
    S.update(A2, 2)
    want = check_update2(S, before, A2, entries, o, "wgrid16 scaled")
    counts = [(len(b.A.col), len(w.col), S.level_info(l)["nnzA"]) for l, (b, w) in enumerate(zip(before, want))]
    print(counts)
    assert all(got == new for _, new, got in counts)
    assert any(old != new for old, new, _ in counts[1:]), "no coarse level changed its entry count"
    # ... and a second update from there walks the schedule from its start again, not from where the first one left it
    entries3 = update_ref.variant(A, "shift")
    A3 = update_ref.matrix_from(*entries3)
    S.update(A3, 2)
    check_update2(S, before, A3, entries3, o, "wgrid16 shifted, second update")


# ---- mode 1 -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wgrid16", "poisson12"])
@pytest.mark.parametrize("smoother", ["chebyshev", "jacobi"])
def test_update1_replaces_level_0_only(name, smoother, tmpdir_mtx):
    A, S, o = build(name, tmpdir_mtx, smoother=smoother)
    s0 = update_ref.state(S)
    entries = update_ref.variant(A, "shift")
    A2 = update_ref.matrix_from(*entries)
    S.update(A2, 1)
    s1 = update_ref.state(S)
    level0 = {k for k in s0 if k.startswith("0.A.") or k == "0.info"}
    assert {k: v for k, v in s1.items() if k not in level0} == {k: v for k, v in s0.items() if k not in level0}
    want = update_ref.csr_of_entries(A.num_rows, *entries)
    assert_same_csr(setup_ref.from_layout(S.level_layout(0, 0)), want, f"{name} level 0")
    if smoother == "chebyshev":     # not set on A2 before the update: computed by it
        e, ew = S.level_info(0)["eig_max"], setup_ref.lanczos_eig(want)
        assert abs(e - ew) <= EIG_BOUND * ew
        assert float(e).hex() != s0["0.info"][3]


# ---- refusals ---------------------------------------------------------------------------------------------------------
def test_refused_updates_leave_the_hierarchy_alone(tmpdir_mtx):
    A, S, _ = build("plat362", tmpdir_mtx, smoother="chebyshev")
    s0 = update_ref.state(S)
    r, c, v = update_ref.entries_of(A)
    n = A.num_rows
    good = update_ref.matrix_from(r, c, v)
    keep = (r < n - 1) & (c < n - 1)
    smaller = update_ref.matrix_from(r[keep], c[keep], v[keep])
    assert smaller.num_rows == n - 1
    loose = host.Matrix(host.Comm("host", "self"))
    loose.set_many(r, c, v)         # never assembled
    for B, mode, msg in ((smaller, 2, "rows"), (smaller, 1, "rows"), (loose, 2, "not assembled"), (good, 0, "mode 0"), (good, 3, "mode 3")):
        with pytest.raises(host.SgpuError, match=msg):
            S.update(B, mode)
        assert update_ref.state(S) == s0, (mode, msg)
    S.update(good, 2)               # and the solver still takes a good one
    assert update_ref.state(S) == s0


def test_update_before_set_matrix_is_refused():
    L = host.load("host")
    A = update_ref.matrix_from([0, 1], [0, 1], [1.0, 1.0])
    h = L.saena_amg_new()
    try:
        for mode in (1, 2):
            assert L.saena_amg_update(h, A.h, mode) != 0
            assert "set_matrix" in L.saena_last_error().decode()
        assert L.saena_amg_num_levels(h) == 0
    finally:
        L.saena_amg_free(h)


def _two_rank_worker(rank, world, name, ret):
    sys.path.insert(0, ROOT)
    try:
        rows, cols, vals = setup_cases.wgrid(12, 9)
        L = host.load("host")

        def matrix():
            A = host.Matrix(host.Comm("host", "shm", (name, rank, world)))
            mine = rows % world == rank
            A.set_many(rows[mine], cols[mine], vals[mine])
            return A.assemble()
        A = matrix()
        S = host.AmgSolver(A, host.options(L, **dict(host.OPTIONS001, smoother="chebyshev")))
        s0 = update_ref.state(S, aggregates=False)
        B = matrix()
        msgs = []
        for mode in (1, 2):
            try:
                S.update(B, mode)
                msgs.append("accepted")
            except host.SgpuError as e:
                msgs.append(str(e))
        ret[rank] = (S.num_levels, msgs, update_ref.state(S, aggregates=False) == s0)
    except Exception as e:                              # noqa: BLE001 -- reported to the parent
        ret[rank] = f"{type(e).__name__}: {e}"


def test_a_two_rank_hierarchy_is_refused():
    """built over the native shared-memory communicator, no device: both modes are refused with "one rank" on every rank, and
    every array of this rank's share of the hierarchy is as it was"""
    import multiprocessing as mp
    world = 2
    ctx = mp.get_context("spawn")
    with ctx.Manager() as mgr:
        ret = mgr.dict()
        procs = [ctx.Process(target=_two_rank_worker, args=(r, world, f"upd_{os.getpid()}", ret)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(120)
        for p in procs:
            if p.is_alive():
                p.terminate()
        got = dict(ret)
    for r in range(world):
        assert isinstance(got.get(r), tuple), (r, got.get(r))
        levels, msgs, same = got[r]
        assert levels >= 2 and same, (r, got[r])
        assert len(msgs) == 2 and all("one rank" in m for m in msgs), msgs


# ---- thread count -----------------------------------------------------------------------------------------------------
WORKER = r"""
import sys, json
sys.path.insert(0, %(root)r)
from tests import setup_cases, update_ref
out = {}
for name in ("wgrid36", "wgrid16"):
    A, S = setup_cases.solver(name, smoother="chebyshev")
    for kind, mode in (("shift", 2), ("pattern", 2), ("perturb", 1)):
        B = update_ref.matrix_from(*update_ref.variant(A, kind))
        S.update(B, mode)
        out[name + " " + kind] = update_ref.state(S)
print("RESULT " + json.dumps(out))
"""


def test_one_thread_and_sixteen_update_to_the_same_hierarchy():
    """SAENA_SETUP_THREADS is read once per process: two fresh children.  wgrid36's level 0 is above the row count from which
    the products and the filter deal rows to threads.  Every array and every eigenvalue estimate after every update is
    byte-identical between them; the second child also prints the phases of its updates"""
    procs = []
    for threads, timing in ((1, False), (16, True)):
        env = dict(os.environ, SAENA_SETUP_THREADS=str(threads))
        env.pop("SAENA_SETUP_TIMING", None)
        if timing:
            env["SAENA_SETUP_TIMING"] = "1"
        procs.append(subprocess.Popen([sys.executable, "-c", WORKER % dict(root=ROOT)], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd=ROOT))
    res = []
    for p in procs:
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, out[-2000:] + err[-3000:]
        res.append((json.loads([ln for ln in out.splitlines() if ln.startswith("RESULT ")][-1][7:]), err))
    (one, err1), (sixteen, err16) = res
    assert one == sixteen, [k for k in one if one[k] != sixteen.get(k)]
    assert one["wgrid36 shift"]["0.info"][0] > 32768
    assert "[update L" not in err1
    for phase in ("R*A", "(RA)*P", "filter", "find_eig"):       # SAENA_SETUP_TIMING=1: PhaseTimer's lines, tagged "update"
        assert any(ln.startswith("[update L0] " + phase) for ln in err16.splitlines()), (phase, err16[-1500:])
    assert any(ln.startswith("[update L1] ") for ln in err16.splitlines())
