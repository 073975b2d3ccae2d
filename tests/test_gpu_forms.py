"""Conformance of every SpMV form (include/saena_gpu.h, variants 0..17 and their sub-forms) to one contract.

The plan-time autotune picks a form per operator by timing alone, so any form may serve any level and any fused epilogue.
Each form is checked here against the CPU oracle on the same operators, through every entry point, on one rank and with
emulated halos, and for where a non-finite input goes:
  * "sequential" forms add a row's products in the reference's order: every epilogue equals the oracle BIT FOR BIT;
  * "tree" forms add them across lanes: the per-row bound |got - ref| <= 1e-13 (|A||x|)_r (times the epilogue's factor), plus
    one rounding of the epilogue's own operation; several sweeps within rel-l2 1e-12;
  * a NaN or Inf in x (or in a stored value) reaches exactly the rows that own it, with the oracle's class and sign; every other
    row keeps the bits of the same form on the clean input.
NaN payloads are never compared: the device and the oracle may propagate different ones."""
import json
import os
import re
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

from oracle import oracle as orc
from tests import hierarchy, inputs, irregular, util

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEQ, TREE = "sequential", "tree"
TOL = 1e-13
TOL_SWEEPS = 1e-12
EPS = np.finfo(np.float64).eps
OMEGA = float(np.float32(2.0 / 3))          # the oracle's jacobi_omega (a float, as in saena_matrix.h)
EIG = 1.9371
KEEP = {"SAENA_KEEP_HOST_VALUES": "1"}
XL_MAX, NCU = 20224, 256                     # doubles of x in one LDS window; CUs of an MI355X (one x-in-LDS chunk each)

# key, variant, kernel name (a trailing "*" matches a prefix), lanes per row, summation class, environment, tile:
# the tile forms (0, 1, 3, 4, 7, 8) keep the sequential order at one lane per row for rows of at most `tile` entries; xw: rows per
# workgroup of the x-window launch mode of variant 17 (set_x_windows after set_variant; 0: the variant as it stands)
Form = namedtuple("Form", "key variant name lanes cls env tile xw", defaults=(0,))
FORMS = [
    Form("stream16", 0, "k_csr_stream<16KiB>", 1, SEQ, {}, 2048),
    Form("stream16.l8", 0, "k_csr_stream<16KiB>", 8, TREE, {}, 0),
    Form("stream32", 1, "k_csr_stream<32KiB>", 1, SEQ, {}, 4096),
    Form("stream32.l16", 1, "k_csr_stream<32KiB>", 16, TREE, {}, 0),
    Form("vector", 2, "k_csr_vector", 8, TREE, {}, 0),
    Form("cc16_16", 3, "k_csr_cc16<16KiB*", 1, SEQ, {}, 2048),
    Form("cc16_16.l4", 3, "k_csr_cc16<16KiB*", 4, TREE, {}, 0),
    Form("cc16_32", 4, "k_csr_cc16<32KiB*", 1, SEQ, {}, 4096),
    Form("cc16_32.l16", 4, "k_csr_cc16<32KiB*", 16, TREE, {}, 0),
    Form("dense", 5, "k_dense_rows", 1, TREE, {}, 0),
    Form("wave", 6, "k_csr_wave", 16, TREE, {}, 0),
    Form("cm16", 7, "k_csr_cm<16KiB*", 1, SEQ, KEEP, 2048),
    Form("cm16.l4", 7, "k_csr_cm<16KiB*", 4, TREE, KEEP, 0),
    Form("cm32", 8, "k_csr_cm<32KiB*", 1, SEQ, KEEP, 4096),
    Form("cm32.l8", 8, "k_csr_cm<32KiB*", 8, TREE, KEEP, 0),
    Form("sell", 9, "k_sell", 1, SEQ, {}, 0),
    Form("sell.sorted", 9, "k_sell<sorted>", 1, SEQ, {"SAENA_SELL_SORTED": "1"}, 0),
    Form("xlds.l8", 10, "k_csr_xlds", 8, TREE, {}, 0),
    Form("xlds.l64", 10, "k_csr_xlds", 64, TREE, {}, 0),
    Form("xlds.global", 10, "k_csr_xlds", 16, TREE, {"SAENA_XLDS_GLOBAL_ACC": "1"}, 0),
    Form("xlds.natural", 10, "k_csr_xlds", 8, TREE, {"SAENA_XLDS_NATURAL_ORDER": "1"}, 0),
    Form("sellp", 11, "k_sellp", 1, SEQ, {}, 0),
    Form("sellp.wide", 11, "k_sellp<wide>", 1, SEQ, {}, 0),
    Form("sellp.rowbase", 11, "k_sellp<rowbase>", 1, SEQ, {}, 0),
    Form("sellx", 12, "k_sellx", 1, TREE, KEEP, 0),
    Form("rowt", 13, "k_rowt", 1, SEQ, KEEP, 0),
    Form("sellp2", 14, "k_sellp2", 1, SEQ, {}, 0),
    Form("sellp2.wide", 14, "k_sellp2<wide>", 1, SEQ, {}, 0),
    Form("sellpx", 15, "k_sellpx", 1, SEQ, {}, 0),
    Form("xldsr.l4", 16, "k_csr_xldsr", 4, TREE, {}, 0),
    Form("xldsr.l16", 16, "k_csr_xldsr", 16, TREE, {}, 0),
    Form("xldsr.global", 16, "k_csr_xldsr", 8, TREE, {"SAENA_XLDS_GLOBAL_ACC": "1"}, 0),
    Form("xldsr.natural", 16, "k_csr_xldsr", 8, TREE, {"SAENA_XLDS_NATURAL_ORDER": "1"}, 0),
    Form("vidx", 17, "k_vidx", 1, SEQ, {}, 0),
    Form("vidx.rowbase", 17, "k_vidx<rowbase>", 1, SEQ, {}, 0),
    Form("vidx.w256", 17, "k_vidx", 1, SEQ, {}, 0, 256),
    Form("vidx.w512", 17, "k_vidx", 1, SEQ, {}, 0, 512),
    Form("vidx.w1024", 17, "k_vidx", 1, SEQ, {}, 0, 1024),
]
BY_KEY = {f.key: f for f in FORMS}
# what set_variant says when a form does not apply (variants 0, 1, 2 and 6 apply to every operator)
REFUSAL = {3: "column segments", 4: "column segments", 5: "too large for the dense form", 7: "column-major", 8: "column-major",
           9: "sliced-ELLPACK form", 10: "x-in-LDS form", 11: "row-pattern form needs", 12: "sliced-ELLPACK-in-LDS",
           13: "row-template", 14: "row-paired", 15: "x in LDS", 16: "x-in-LDS form", 17: "value-indexed"}
X_WINDOWS_REFUSAL = "x windows"              # what set_x_windows says where the operator is on variant 17 and the mode does not apply


def refused_as_documented(form, what):
    """the form's own message; for the window keys either the variant's or the mode's (make_gpu and form_world hold a refusal of
    set_x_windows itself to the mode's)"""
    return (form.variant in REFUSAL and REFUSAL[form.variant] in what) or (form.xw != 0 and X_WINDOWS_REFUSAL in what)


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def klass(a):
    """0 finite, 1 NaN, 2 +Inf, 3 -Inf"""
    a = np.asarray(a)
    return np.where(np.isnan(a), 1, np.where(a == np.inf, 2, np.where(a == -np.inf, 3, 0)))


def name_matches(form, name):
    return name.startswith(form.name[:-1]) if form.name.endswith("*") else name == form.name


# ---- the operators ------------------------------------------------------------------------------------------------------------
Problem = namedtuple("Problem", "entries M N square")


def _coo(rows, cols, vals, M, N):
    key = rows.astype(np.int64) * N + cols
    _, first = np.unique(key, return_index=True)
    return orc.coo_from_arrays(rows[first].astype(np.int32), cols[first].astype(np.int32), np.asarray(vals, np.float64)[first])


def _empty_rows(M=3001, seed=17):
    """irregular rows of 1..120 entries, and one row in seven with no entry at all (no diagonal: the oracle's inverse diagonal is 1)"""
    rng = np.random.default_rng(seed)
    lens = rng.choice([1, 2, 3, 5, 9, 17, 40, 120], size=M)
    lens[rng.random(M) < 1.0 / 7] = 0
    rows = np.repeat(np.arange(M), lens)
    cols = np.concatenate([rng.choice(M, size=k, replace=False) for k in lens])
    vals = rng.standard_normal(rows.size)
    d = np.flatnonzero(lens)
    rows, cols, vals = np.concatenate([d, rows]), np.concatenate([d, cols]), np.concatenate([40 + rng.random(d.size), vals])
    return _coo(rows, cols, vals, M, M)


def _uneven_rows(M=4999, seed=5):
    """three row lengths in random order around the diagonal: plain slices of 64 pad > 12 %, sorted ones < 5 % (k_sell<sorted>)"""
    rng = np.random.default_rng(seed)
    lens = rng.choice([12, 18, 27], size=M, p=[0.3, 0.4, 0.3])
    rows = np.repeat(np.arange(M), lens - 1)
    cols = np.concatenate([np.sort(rng.choice(np.setdiff1d(np.arange(max(0, r - 60), min(M, r + 60)), [r]), size=k - 1, replace=False))
                           for r, k in enumerate(lens)])
    vals = np.sin(0.3 * rows + 0.7 * cols) + 1.5
    d = np.arange(M)
    return _coo(np.concatenate([rows, d]), np.concatenate([cols, d]), np.concatenate([vals, np.full(M, 90.0)]), M, M)


_HIER = None


def _hier():
    global _HIER
    if _HIER is None:
        _HIER = hierarchy.poisson_hierarchy(34, 3)
    return _HIER


def _build(name):
    if name.startswith("poisson"):
        e, M = orc.laplacian3d(int(name[7:]))
        return Problem(e, M, M, True)
    if name == "band":
        return Problem(orc.band_matrix(1000, 9), 1000, 1000, True)
    if name == "small":                                        # 27 rows: one partial slice, one row pair without a partner
        e, M = orc.laplacian3d(5)
        return Problem(e, M, M, True)
    if name == "dense":                                        # 300 rows, band 150: about 75 % of the entries stored
        return Problem(orc.band_matrix(300, 150), 300, 300, True)
    if name == "empty":
        return Problem(_empty_rows(), 3001, 3001, True)
    if name == "uneven":
        return Problem(_uneven_rows(), 4999, 4999, True)
    if name == "hub":
        # configs[4]'s generator at 9 blocks (45 369 rows and columns, a hub row of 3 000 entries), and 400 symmetric couplings between
        # the first block and the last four: the x-in-LDS chunks of those blocks reach over two and three windows of x
        r, c, v, M = irregular.sih4_replicated(9)
        rng = np.random.default_rng(29)
        n = M // 9
        i, j = rng.integers(0, n, 400), rng.integers(5 * n, M, 400)
        w = 0.01 * (0.5 + rng.random(400))
        rows, cols = np.concatenate([r, i, j]), np.concatenate([c, j, i])
        return Problem(_coo(rows, cols, np.concatenate([v, w, w]), M, M), M, M, True)
    As, Ps, Rs = _hier()
    S = {"L1": As[1], "P0": Ps[0], "R0": Rs[0]}[name]
    return Problem(hierarchy.scipy_to_coo(S), S.shape[0], S.shape[1], name == "L1")


OPERATORS = ["poisson11", "poisson13", "band", "L1", "P0", "R0", "empty", "hub", "small", "dense", "uneven"]
_PROBLEMS = {}


def problem(name):
    name = name.split("/")[0]                                   # ("poisson13/planes": the same operator on another partition)
    if name not in _PROBLEMS:
        _PROBLEMS[name] = _build(name)
    return _PROBLEMS[name]


def oracle_op(p, nprocs=1, split=None):
    if p.square:
        split = orc.split_nnz(p.entries, p.M, nprocs) if split is None else split
        return orc.OracleOp(p.entries, p.M, p.M, split)
    return orc.OracleOp(p.entries, p.M, p.N, orc.split_even(p.M, nprocs), orc.split_even(p.N, nprocs), square=False)


def row_lengths(p):
    return np.bincount(np.asarray(p.entries["row"]), minlength=p.M)


def abs_bound(entries, M, x):
    b = np.zeros(M)
    np.add.at(b, entries["row"], np.abs(entries["val"] * x[entries["col"]]))
    return b


def sequential_rows(form, p):
    """rows whose sums this form adds in the reference's order at its lane count (None: every row)"""
    if form.cls == TREE:
        return np.zeros(p.M, bool)
    if form.tile:
        return row_lengths(p) <= form.tile
    return np.ones(p.M, bool)


def make_gpu(capi, O, form, monkeypatch, r=0, halo_fp32=False):
    """-> the rank's operator forced to the form, or the refusal's message"""
    for k, v in form.env.items():
        monkeypatch.setenv(k, v)
    try:
        G = util.gpu_operator(O, r, halo_fp32)
        try:
            G.set_variant(form.variant)
        except capi.SgpuError as e:
            return None, str(e)
        G.set_lanes_per_row(form.lanes)
        if form.xw:
            try:
                G.set_x_windows(form.xw)
            except capi.SgpuError as e:
                assert X_WINDOWS_REFUSAL in str(e), str(e)
                return None, str(e)
            assert G.x_windows() == form.xw
        return G, G.variant()[1]
    finally:
        for k in form.env:
            monkeypatch.delenv(k, raising=False)


# ---- every entry point on one rank ---------------------------------------------------------------------------------------------
def vectors(p):
    return dict(x=inputs.v2(p.N), rhs=inputs.rhs2(p.M), w=inputs.v_sin(p.M) + 2.0, c=0.37, u=inputs.rhs2(p.M))


def run_gpu(capi, G, p, v, epis=None):
    x, rhs, w, u = v["x"], v["rhs"], v["w"], v["u"]
    dx, dy = capi.DeviceVector(p.N, x), capi.DeviceVector(p.M)
    out = {}
    want = set(epis) if epis else None

    def on(k):
        return want is None or k in want
    if on("spmv"):
        G.spmv(dx, dy)
        out["spmv"] = dy.download()
    if on("spmv_host"):
        out["spmv_host"] = G.spmv_host(x)
    if on("prolong_correct"):
        du = capi.DeviceVector(p.M, u)
        G.prolong_correct(dx, du)
        out["prolong_correct"] = du.download()
    if not p.square:
        return out
    dr, dres, dw = capi.DeviceVector(p.M, rhs), capi.DeviceVector(p.M), capi.DeviceVector(p.M, w)
    if on("residual"):
        G.residual(dx, dr, dres)
        out["residual"] = dres.download()
    if on("residual_negative"):
        G.residual_negative(dx, dr, dres)
        out["residual_negative"] = dres.download()
    if on("residual_multiply"):
        G.residual_multiply(dx, dr, dres, dw, v["c"])
        out["residual_multiply"] = dres.download()
    for it in (1, 3):
        if on(f"jacobi{it}"):
            du = capi.DeviceVector(p.M, x)
            G.jacobi(it, du, dr)
            out[f"jacobi{it}"] = du.download()
        if on(f"chebyshev{it}"):
            du = capi.DeviceVector(p.M, x)
            G.chebyshev(it, EIG, du, dr)
            out[f"chebyshev{it}"] = du.download()
    return out


def run_oracle(O, p, v, epis=None):
    x, rhs, w, u = v["x"], v["rhs"], v["w"], v["u"]
    s = O.matvec(x)
    out = {"spmv": s, "spmv_host": s, "prolong_correct": u - s}
    if p.square:
        O.set_eig(EIG)
        out["residual"] = O.residual(x, rhs)
        out["residual_negative"] = O.residual_negative(x, rhs)
        out["residual_multiply"] = O.residual_multiply(x, rhs, w, v["c"])
        for it in (1, 3):
            out[f"jacobi{it}"] = O.jacobi(it, x, rhs)
            out[f"chebyshev{it}"] = O.chebyshev(it, x, rhs)
    return {k: a for k, a in out.items() if epis is None or k in epis}


def inv_diag(p):
    d = np.ones(p.M)
    e = p.entries[p.entries["row"] == p.entries["col"]]
    d[e["row"]] = 1.0 / e["val"]
    return d


def check_against_oracle(p, got, ref, v, seq, where):
    """seq: rows held to the oracle's bits; the others to the per-row bound (single launches) or rel-l2 (several sweeps)"""
    b = abs_bound(p.entries, p.M, v["x"])
    factor = {"residual_multiply": np.abs(v["c"] * v["w"]), "jacobi1": np.abs(OMEGA * inv_diag(p)) if p.square else None}
    for k, g in got.items():
        r = ref[k]
        msg = f"{where} {k}"
        if seq.all():
            np.testing.assert_array_equal(bits(g), bits(r), err_msg=msg)
            continue
        if seq.any() and k in ("spmv", "spmv_host"):
            np.testing.assert_array_equal(bits(g[seq]), bits(r[seq]), err_msg=msg)
        if k in ("jacobi3", "chebyshev1", "chebyshev3"):
            assert np.linalg.norm(g - r) <= TOL_SWEEPS * np.linalg.norm(r), msg
            continue
        f = factor.get(k)
        lim = TOL * b * (1.0 if f is None else f) + 2 * EPS * np.abs(r) + 1e-300
        bad = np.flatnonzero(~(np.abs(g - r) <= lim))
        assert bad.size == 0, f"{msg}: rows {bad[:10].tolist()} outside the bound"


def test_catalogue_covers_every_variant(capi):
    """the library's own bound ("variant must be 0..N"): every variant in 0..N has a catalogue entry, so a new form fails the
    suite until it is described here"""
    G = util.gpu_operator(oracle_op(problem("small")))
    with pytest.raises(capi.SgpuError, match=r"variant must be 0\.\.\d+") as e:
        G.set_variant(10 ** 6)
    n = int(re.search(r"variant must be 0\.\.(\d+)", str(e.value)).group(1))
    with pytest.raises(capi.SgpuError, match="variant must be"):
        G.set_variant(n + 1)
    assert sorted({f.variant for f in FORMS}) == list(range(n + 1))
    assert all(f.variant in REFUSAL or f.variant in (0, 1, 2, 6) for f in FORMS)


_ORACLE_OUT = {}


def oracle_outputs(name):
    if name not in _ORACLE_OUT:
        p = problem(name)
        _ORACLE_OUT[name] = run_oracle(oracle_op(p), p, vectors(p))
    return _ORACLE_OUT[name]


@pytest.mark.parametrize("key", [f.key for f in FORMS])
def test_every_entry_point_against_the_oracle(capi, key, monkeypatch):
    """every operator the form takes: spmv, spmv_host, residual, residual_negative, residual_multiply, Jacobi (1 and 3 sweeps),
    Chebyshev (1 and 3 steps), u -= A e; an operator the form refuses gets the form's own message"""
    form = BY_KEY[key]
    served = []
    for name in OPERATORS:
        p = problem(name)
        O = oracle_op(p)
        G, what = make_gpu(capi, O, form, monkeypatch)
        if G is None:
            assert refused_as_documented(form, what), (name, what)
            continue
        if not name_matches(form, what):
            continue                                            # another sub-form of the variant serves this operator
        served.append(name)
        v = vectors(p)
        check_against_oracle(p, run_gpu(capi, G, p, v), oracle_outputs(name), v, sequential_rows(form, p), f"{key} on {name}:")
    assert served, f"no operator of the set is served by {key}"


# ---- emulated halos ------------------------------------------------------------------------------------------------------------
# split by nnz, as the reference partitions; "/planes": the Poisson cube split between planes of the grid, where every rank's slice
# keeps the few row patterns / templates of the whole operator (the pattern forms refuse slices cut through a plane on small cubes)
HALO_OPERATORS = ["poisson13", "poisson20", "poisson13/planes", "band", "L1", "P0", "R0", "empty", "hub", "dense", "uneven"]


def world_outputs(capi, p, O, W, forms, v, fp32):
    """spmv, residual, two Jacobi sweeps (halo exchanged before each), a Chebyshev step; u -= A e for the transfers.  forms[r]:
    the form of rank r as (variant, lanes, rows per workgroup of the x-window mode)"""
    split_r, split_c = O.split_row, O.split_col
    for r, (G, f) in enumerate(zip(W.g, forms)):
        G.set_variant(f[0]); G.set_lanes_per_row(f[1])
        if f[2]:
            G.set_x_windows(f[2])
        assert G.variant()[0] == f[0] and G.x_windows() == f[2]
    out = {}
    xs, ys = W.slices(v["x"], split_c), [capi.DeviceVector(int(split_r[r + 1] - split_r[r])) for r in range(W.P)]
    W.exchange(xs)
    for r in range(W.P):
        W.g[r].spmv(xs[r], ys[r])
    out["spmv"] = W.gather(ys)
    if not p.square:
        us = W.slices(v["u"], split_r)
        for r in range(W.P):
            W.g[r].prolong_correct(xs[r], us[r])
        out["prolong_correct"] = W.gather(us)
        return out
    rs = W.slices(v["rhs"], split_r)
    for r in range(W.P):
        W.g[r].residual(xs[r], rs[r], ys[r])
    out["residual"] = W.gather(ys)
    us = W.slices(v["x"], split_r)
    for sweep in range(2):
        W.exchange(us)
        for r in range(W.P):
            W.g[r].jacobi(1, us[r], rs[r])
        out[f"jacobi{sweep + 1}"] = W.gather(us)
    if not fp32:
        us = W.slices(v["x"], split_r)
        W.exchange(us)
        for r in range(W.P):
            W.g[r].chebyshev(1, EIG, us[r], rs[r])
        out["chebyshev1"] = W.gather(us)
    return out


ANCHOR = (4, 1, 0)                           # k_csr_cc16 at one lane: what a rank runs where its slice refuses the form, and the halo tests' anchor


def form_world(capi, O, fp32, form, monkeypatch):
    """-> (world, [(variant, lanes, x-window rows)] per rank): the form where the rank's slice takes it, variant 4 at 1 lane where it
    refuses"""
    out = []
    for k, v in form.env.items():
        monkeypatch.setenv(k, v)
    try:
        W = util.EmulatedWorld(O, halo_fp32=fp32)
        for G in W.g:
            try:
                G.set_variant(form.variant)
                ok = name_matches(form, G.variant()[1])
            except capi.SgpuError as e:
                assert form.variant in REFUSAL and REFUSAL[form.variant] in str(e), str(e)
                ok = False
            if ok and form.xw:
                try:
                    G.set_x_windows(form.xw)
                except capi.SgpuError as e:
                    assert X_WINDOWS_REFUSAL in str(e), str(e)
                    ok = False
            out.append((form.variant, form.lanes, form.xw) if ok else ANCHOR)
    finally:
        for k in form.env:
            monkeypatch.delenv(k, raising=False)
    return W, out


_WORLD_ORACLE = {}


def world_oracle(name, nprocs, fp32):
    """(OracleOp, reference outputs) of an emulated world, shared by every form"""
    k = (name, nprocs, fp32)
    if k not in _WORLD_ORACLE:
        p = problem(name)
        split = None
        if name.endswith("/planes"):
            n = round(p.M ** (1 / 3))
            split = (np.round(np.linspace(0, n, nprocs + 1)).astype(np.int64) * n * n).astype(np.int32)
        O = oracle_op(p, nprocs, split)
        O.set_use_double(not fp32)
        v = vectors(p)
        ref = run_oracle(O, p, v, ("spmv", "prolong_correct", "residual", "jacobi1", "chebyshev1"))
        if p.square:
            ref["jacobi2"] = O.jacobi(2, v["x"], v["rhs"])
        _WORLD_ORACLE[k] = (O, ref)
    return _WORLD_ORACLE[k]


@pytest.mark.parametrize("nprocs", [2, 3])
@pytest.mark.parametrize("key", [f.key for f in FORMS])
def test_emulated_halos(capi, key, nprocs, monkeypatch):
    """the HALO instantiations (boundary rows masked out of the local launch, computed by k_csr_boundary) at 2 and 3 ranks, fp64
    and fp32 wire: sequential forms give the bits of the same world on k_csr_cc16 at one lane; tree forms the oracle's bound.  A
    rank whose slice the form refuses stays on k_csr_cc16 at one lane; at least one rank runs the form."""
    form = BY_KEY[key]
    ran = []
    for name in HALO_OPERATORS:
        p = problem(name)
        for fp32 in (False, True):
            O, ref = world_oracle(name, nprocs, fp32)
            W, forms = form_world(capi, O, fp32, form, monkeypatch)
            if all(f[0] != form.variant for f in forms):
                continue
            ran.append((name, fp32, [f[0] for f in forms]))
            v = vectors(p)
            got = world_outputs(capi, p, O, W, forms, v, fp32)
            where = f"{key} on {name} at {nprocs} ranks (variants {[f[0] for f in forms]}), fp32={fp32}:"
            if form.variant == 5 and fp32:
                # the dense rows on the float wire are the reference's matvec_dense_float: x rounded to float as a whole
                b = abs_bound(p.entries, p.M, v["x"])
                assert np.all(np.abs(got["spmv"] - O.matvec_dense(v["x"], as_float=True)) <= TOL * b + 1e-300), where
                continue
            if form.cls == SEQ and sequential_rows(form, p).all():
                anchor = world_outputs(capi, p, O, W, [ANCHOR] * nprocs, v, fp32)
                for k in got:
                    np.testing.assert_array_equal(bits(got[k]), bits(anchor[k]), err_msg=f"{where} {k}")
            b = abs_bound(p.entries, p.M, v["x"])
            for k, g in got.items():
                r = ref[k]
                if k in ("jacobi2", "chebyshev1"):
                    assert np.linalg.norm(g - r) <= TOL_SWEEPS * np.linalg.norm(r), f"{where} {k}"
                    continue
                lim = TOL * (b * np.abs(OMEGA * inv_diag(p)) if k == "jacobi1" else b) + 2 * EPS * np.abs(r) + 1e-300
                bad = np.flatnonzero(~(np.abs(g - r) <= lim))
                assert bad.size == 0, f"{where} {k}: rows {bad[:10].tolist()} outside the bound"
    # (k_sellx pads more than 25 % on every slice of three ranks in this set: it refuses them all, and runs at two ranks)
    assert ran or (key, nprocs) == ("sellx", 3), f"no rank of any operator ran {key} at {nprocs} ranks"


# ---- the restriction's fused first sweep of the next level (RSWEEP) -----------------------------------------------------------
def test_restriction_with_the_next_level_s_first_sweep(capi, monkeypatch):
    """one V-cycle (Jacobi and Chebyshev) with R0 forced to each form that takes it: the restriction runs the coarse level's first
    sweep in its epilogue.  Sequential forms give the bits of the V-cycle with R0 on k_csr_cc16 at one lane, tree forms agree to
    rel-l2 1e-12."""
    As, Ps, Rs = _hier()
    OA, OP, OR = hierarchy.oracle_hierarchy(As, Ps, Rs)
    eig = hierarchy.eig_estimates(As)
    n = OA[0].Mbig

    def vcycle(form, smoother):
        GA = [util.gpu_operator(a) for a in OA]
        GP = [util.gpu_operator(q) for q in OP]
        GR = [util.gpu_operator(r) for r in OR]
        if form is None:
            GR[0].set_variant(4); GR[0].set_lanes_per_row(1)
        else:
            GR[0], _ = make_gpu(capi, OR[0], form, monkeypatch)
        A = capi.Amg(GA, GP, GR, eig_max=eig, pre=2, post=2, smoother=smoother, coarse_solver="direct")
        du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, inputs.rhs2(n))
        A.vcycle(du, dr)
        assert GR[0].variant()[0] == (4 if form is None else form.variant)
        A.destroy()
        return du.download()
    anchor = {sm: vcycle(None, sm) for sm in ("jacobi", "chebyshev")}
    served = []
    for form in FORMS:
        G, what = make_gpu(capi, OR[0], form, monkeypatch)
        if G is None:
            assert refused_as_documented(form, what), (form.key, what)
            continue
        if not name_matches(form, what):
            continue
        served.append(form.key)
        for sm in ("jacobi", "chebyshev"):
            g = vcycle(form, sm)
            if form.cls == SEQ:
                np.testing.assert_array_equal(bits(g), bits(anchor[sm]), err_msg=f"{form.key}, {sm}")
            else:
                assert np.linalg.norm(g - anchor[sm]) <= TOL_SWEEPS * np.linalg.norm(anchor[sm]), (form.key, sm)
    assert {"stream16", "cc16_32", "sellp.rowbase", "vidx.rowbase", "xlds.l8", "xldsr.l4"} <= set(served) or \
        {"stream16", "cc16_32", "sellp", "vidx", "xlds.l8", "xldsr.l4"} <= set(served), served


# ---- non-finite containment ----------------------------------------------------------------------------------------------------
SPECIALS = [np.nan, np.inf, -np.inf]
CONTAIN_EPIS = ("spmv", "residual", "jacobi1")


def xlds_second_windows(p):
    """the library's x-in-LDS plan (build_xlds): one nnz-balanced row chunk per CU, windows from the chunk's first column, shortened
    by the chunk's partial sums kept in LDS; -> (first column of a chunk's second window, a row of that chunk whose entries reach
    both sides of it, the CSR position of that row's first entry in the second window), or None"""
    M = p.M
    col = np.asarray(p.entries["col"])[csr_order(p)]
    rp = np.concatenate([[0], np.cumsum(row_lengths(p))])
    nb = min(NCU, M)
    blk = np.maximum.accumulate([0] + [min(M, int(np.searchsorted(rp, len(col) * b // nb))) for b in range(1, nb)] + [M])
    for b in range(nb):
        r0, r1 = blk[b], blk[b + 1]
        if r1 <= r0 or rp[r1] == rp[r0]:
            continue
        lo, hi = int(col[rp[r0]:rp[r1]].min()), int(col[rp[r0]:rp[r1]].max())
        if hi - lo < XL_MAX:
            continue
        first = lo + XL_MAX - (r1 - r0 + 63) // 64 * 64
        for r in range(r0, r1):
            c = col[rp[r]:rp[r + 1]]
            if c.size >= 8 and c.min() < first - 200 and c.max() >= first + 200:
                return first, r, int(rp[r] + np.searchsorted(c, first))
    return None


def x_columns(name, p):
    """an interior column, the first and the last, columns at slice and row-pair edges; on the hub operator the first column of a
    chunk's second window of x and the one before it"""
    cols = {p.N // 2, 0, p.N - 1}
    for k in (64, 128, 256):
        cols |= {c for c in (k - 1, k, k + 1) if c < p.N}
    if name == "hub":
        w = xlds_second_windows(p)
        assert w is not None
        cols |= {int(w[0]), int(w[0]) - 1}
    return sorted(cols)


def csr_order(p):
    return np.lexsort((np.asarray(p.entries["col"]), np.asarray(p.entries["row"])))


def value_positions(name, p):
    """CSR positions (row-major, columns ascending) to hold a special value: the first and last entry of rows at slice and row-pair
    edges, the two entries either side of a row boundary that falls inside a quad; on the hub operator the entries within three
    positions of a window boundary inside a row that spans two windows (k_csr_xlds's pieces)"""
    rp = np.concatenate([[0], np.cumsum(row_lengths(p))])
    pos = set()
    for r in (0, 63, 64, 127, 128, 255, 256, p.M // 2, p.M - 1):
        if r < p.M and rp[r + 1] > rp[r]:
            pos |= {int(rp[r]), int(rp[r + 1] - 1)}
    for r in range(1, p.M):                                     # row r's first quad carries row r-1's last entries
        if rp[r] % 4 and rp[r + 1] > rp[r] and rp[r] > rp[r - 1]:
            pos |= {int(rp[r]), int(rp[r] - 1)}
            break
    if name == "hub":
        k = xlds_second_windows(p)[2]
        pos |= {k - 3, k - 1, k, k + 2}
    return sorted(pos)


def with_value(p, pos, special):
    e = p.entries.copy()
    k = csr_order(p)[pos]
    e["val"][k] = special
    return Problem(orc.coo_from_arrays(e["row"], e["col"], e["val"]), p.M, p.N, p.square), int(e["row"][k])


def check_contained(got, clean, ref, msg, may_change=None):
    """non-finite rows exactly the oracle's, with its class and sign; every other row (but those in may_change, whose finite inputs
    changed) the clean run's bits"""
    for k, g in got.items():
        bad = klass(g) != 0
        np.testing.assert_array_equal(np.flatnonzero(bad), np.flatnonzero(klass(ref[k]) != 0), err_msg=f"{msg} {k}: non-finite rows")
        np.testing.assert_array_equal(klass(g)[bad], klass(ref[k])[bad], err_msg=f"{msg} {k}: class")
        keep = ~bad if may_change is None else ~(bad | may_change)
        np.testing.assert_array_equal(bits(g[keep]), bits(clean[k][keep]), err_msg=f"{msg} {k}: other rows")


CONTAIN_OPERATORS = OPERATORS
_X_REF = {}


@pytest.mark.parametrize("key", [f.key for f in FORMS])
def test_a_non_finite_x_stays_in_the_rows_that_own_its_column(capi, key, monkeypatch):
    """x[c] = NaN, +Inf, -Inf: the non-finite rows are the rows that own column c, with the oracle's class, for the product, the
    residual and a Jacobi sweep; every other row keeps the bits of the same form on the clean x"""
    form = BY_KEY[key]
    ran = 0
    for name in CONTAIN_OPERATORS:
        p = problem(name)
        O = oracle_op(p)
        G, what = make_gpu(capi, O, form, monkeypatch)
        if G is None or not name_matches(form, what):
            continue
        ran += 1
        v = vectors(p)
        epis = CONTAIN_EPIS if p.square else ("spmv",)
        clean = run_gpu(capi, G, p, v, epis)
        rows, cols = np.asarray(p.entries["row"]), np.asarray(p.entries["col"])
        for c in x_columns(name, p):
            owners = np.zeros(p.M, bool)
            owners[rows[cols == c]] = True
            for s in SPECIALS:
                vs = dict(v, x=v["x"].copy())
                vs["x"][c] = s
                got = run_gpu(capi, G, p, vs, epis)
                msg = f"{key} on {name}, x[{c}] = {s}:"
                if form.variant == 5:
                    # k_dense_rows multiplies the zeros it stores, as the reference's dense matvec does (0 * Inf is NaN in every row):
                    # its product is held to OracleOp.matvec_dense, not to the sparse rows' containment
                    np.testing.assert_array_equal(klass(got["spmv"]), klass(O.matvec_dense(vs["x"])), err_msg=msg)
                    continue
                if (name, c, str(s)) not in _X_REF:
                    _X_REF[(name, c, str(s))] = run_oracle(O, p, vs, epis)
                ref = _X_REF[(name, c, str(s))]
                np.testing.assert_array_equal(klass(ref["spmv"]) != 0, owners, err_msg="oracle")
                check_contained(got, clean, ref, msg)
    assert ran, f"no containment operator is served by {key}"


@pytest.mark.parametrize("name", ["poisson13", "empty", "hub", "dense", "L1"])
def test_a_non_finite_value_stays_in_its_row(capi, name, monkeypatch):
    """one stored value NaN / +Inf / -Inf at a time, under every form that takes the operator: only its row turns non-finite (product,
    residual, a Jacobi sweep), with the oracle's class; every other row keeps the clean operator's bits under the same form"""
    p = problem(name)
    v = vectors(p)
    clean, ran = {}, []
    for form in FORMS:
        G, what = make_gpu(capi, oracle_op(p), form, monkeypatch)
        if G is not None and name_matches(form, what):
            clean[form.key] = run_gpu(capi, G, p, v, CONTAIN_EPIS)
    assert clean
    for pos in value_positions(name, p):
        for s in SPECIALS:
            q, row = with_value(p, pos, s)
            O = oracle_op(q)
            ref = run_oracle(O, q, v, CONTAIN_EPIS)
            assert np.flatnonzero(klass(ref["spmv"]) != 0).tolist() == [row]
            for form in FORMS:
                if form.key not in clean:
                    continue
                G, what = make_gpu(capi, O, form, monkeypatch)
                if G is None:                                   # the special may take the operator out of a form (k_vidx's dictionary)
                    assert form.variant == 17 and REFUSAL[17] in what, (form.key, what)      # (the window keys too: the variant itself goes)
                    continue
                ran.append(form.key)
                got = run_gpu(capi, G, q, v, CONTAIN_EPIS)
                check_contained(got, clean[form.key], ref, f"{form.key} on {name}, value {s} at CSR position {pos} (row {row}):")
    if name == "poisson13":
        assert {"vidx", "vidx.w256", "vidx.w512", "vidx.w1024"} <= set(ran)
    if name == "hub":
        assert {"xlds.l8", "xlds.l64", "xlds.global", "xlds.natural", "xldsr.l4", "xldsr.l16", "xldsr.global", "xldsr.natural"} <= set(ran)


@pytest.mark.parametrize("key", [f.key for f in FORMS])
def test_a_non_finite_halo_value_stays_in_the_receiving_rows(capi, key, monkeypatch):
    """a special at a column rank 1 sends to rank 0: only the rows that own the column, on either rank, change; on the fp32 wire a
    finite 1e300 arrives as Inf exactly in the receiving rows that own it (OracleOp.set_use_double(False))"""
    form = BY_KEY[key]
    ran = 0
    for name in ("poisson13", "poisson20", "poisson13/planes", "L1", "P0", "empty", "hub", "uneven"):
        p = problem(name)
        for fp32 in (False, True):
            O, _ = world_oracle(name, 2, fp32)
            W, forms = form_world(capi, O, fp32, form, monkeypatch)
            if all(f[0] != form.variant for f in forms):
                continue
            ran += 1
            v = vectors(p)
            vidx = O.rank_array(1, "vIndex", O.rank(1).vIndexSize, np.int32)
            assert len(vidx)
            c = int(O.split_col[1]) + int(vidx[len(vidx) // 2])
            rows, cols = np.asarray(p.entries["row"]), np.asarray(p.entries["col"])
            owners = np.zeros(p.M, bool)
            owners[rows[cols == c]] = True
            assert owners[:O.split_row[1]].any() and owners[O.split_row[1]:].any()
            clean = world_outputs(capi, p, O, W, forms, v, fp32)
            for s in SPECIALS + ([1e300] if fp32 else []):
                vs = dict(v, x=v["x"].copy())
                vs["x"][c] = s
                got = world_outputs(capi, p, O, W, forms, vs, fp32)
                msg = f"{key} on {name} (variants {[f[0] for f in forms]}), fp32={fp32}, x[{c}] = {s}:"
                if form.variant == 5:                           # (the stored zeros of the dense rows: see the x side above)
                    np.testing.assert_array_equal(klass(got["spmv"]), klass(O.matvec_dense(vs["x"], as_float=fp32)), err_msg=msg)
                    continue
                got = {k: got[k] for k in ("spmv", "residual", "jacobi1") if k in got}
                ref = run_oracle(O, p, vs, tuple(got))
                nonfinite = klass(ref["spmv"]) != 0
                if s == 1e300:                                  # Inf in every receiving row that owns the column, nowhere else off it;
                    recv = owners.copy()                        # the sender's rows that own it read the finite value
                    recv[O.split_row[1]:] = False
                    assert recv.any() and nonfinite[recv].all() and not nonfinite[~owners].any(), "oracle"
                    changed = owners.copy()
                    changed[c] = p.square                       # (a Jacobi sweep updates x[c] itself)
                    check_contained(got, clean, ref, msg, changed)
                else:
                    np.testing.assert_array_equal(nonfinite, owners, err_msg="oracle")
                    check_contained(got, clean, ref, msg)
    assert ran, f"no rank ran {key}"


# ---- the switches read once per process ---------------------------------------------------------------------------------------
NT_FORMS = ["sell", "sell.sorted", "sellp", "sellp.wide", "sellp2", "sellp2.wide", "sellpx", "vidx", "vidx.w256", "vidx.w512", "vidx.w1024"]
NT_WORKER = r"""
import sys, json, hashlib
sys.path.insert(0, %(root)r)
from saena_amd import capi
from tests import test_gpu_forms as T
capi.init(0)
print("RESULT " + json.dumps(T.nt_outputs(capi)))
"""


class _Env:
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def nt_outputs(capi, monkeypatch=None):
    """hashes of every epilogue of forms 9, 11, 14, 15 and 17 on the Poisson and level-1 operators, and on the uneven rows that
    k_sell<sorted> is built for (SAENA_SELL_SORTED is read per build: make_gpu sets it in either process)"""
    import hashlib
    monkeypatch = monkeypatch or _Env()
    out = {}
    for name in ("poisson13", "L1", "uneven"):
        p = problem(name)
        O = oracle_op(p)
        v = vectors(p)
        for key in NT_FORMS:
            G, what = make_gpu(capi, O, BY_KEY[key], monkeypatch)
            if G is None or not name_matches(BY_KEY[key], what):
                continue
            for k, a in run_gpu(capi, G, p, v).items():
                out[f"{name}/{key}/{k}"] = hashlib.sha256(bits(a).tobytes()).hexdigest()
    return out


def test_non_temporal_and_non_pre_instantiations_give_the_same_bits(capi, monkeypatch):
    """SAENA_SELL_NT, SAENA_SELLP_NT and SAENA_SELLP2_PRE are read once per process: a child process with SAENA_SELL_NT=1
    SAENA_SELLP_NT=1 SAENA_SELLP2_PRE=0 runs the NT instantiations of 9 (k_sell, plain and sorted), 11, 14, 15 and 17 (k_vidx and,
    with the x windows on, k_vidxw) and 14 without PRE on operators far below the size where they switch on"""
    here = nt_outputs(capi, monkeypatch)
    assert {k.split("/")[1] for k in here} == set(NT_FORMS)
    env = dict(os.environ, SAENA_SELL_NT="1", SAENA_SELLP_NT="1", SAENA_SELLP2_PRE="0")
    out = subprocess.run([sys.executable, "-c", NT_WORKER % dict(root=ROOT)], env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    child = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert child == here, sorted(k for k in here if child.get(k) != here[k])
