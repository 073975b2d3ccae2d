"""Who owns an operator's device memory, and what a settled plan keeps of it.

The local part of an operator stores its kernel forms in groups of device arrays (sgpu_debug_op_storage names them, one bit each);
when the plan settles on a variant (sgpu_op_autotune), every group outside that variant's keep-set is freed.  The sets below restate,
by variant, the table the library keeps in ONE place (plan_keeps in forms.h; the sets live in tests/form_table.py, which
tests/test_forms_header.py holds the header to on the host).  The operators are those of test_gpu_forms.py
with fewer than 200 000 entries: their autotune goes straight to the clean-up for the variant in use.

The library counts the bytes of every device and pinned array it owns (vectors from sgpu_vec_alloc are the caller's and are not
counted): whatever was created and destroyed again leaves that count exactly where it was.
"""
import numpy as np
import pytest

from tests import inputs, util
from tests.form_table import KEEPS, XWIN
from tests.test_gpu_forms import BY_KEY, FORMS, OPERATORS, _hier, bits, make_gpu, name_matches, oracle_op, problem
from tests.test_gpu_vcycle import build

pytestmark = pytest.mark.gpu

AUTOTUNE_SWEEPS_FROM = 200000                # entries from which sgpu_op_autotune times candidates instead of keeping the variant in use
SGPU_ERR_STATE = -4


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


def groups(capi, G):
    m = G.storage_mask()
    assert m >> len(capi.STORAGE_GROUPS) == 0, hex(m)
    return {g for i, g in enumerate(capi.STORAGE_GROUPS) if m >> i & 1}


def expected(form):
    return {"csr"} | KEEPS[form.variant] | ({XWIN[form.xw]} if form.xw else set())


def small_operators():
    return [n for n in OPERATORS if len(problem(n).entries["row"]) < AUTOTUNE_SWEEPS_FROM]


def first_served(capi, form, monkeypatch):
    """-> (name, problem, oracle operator, GPU operator) of the first operator below the autotune's threshold that the form serves"""
    for name in small_operators():
        p = problem(name)
        O = oracle_op(p)
        G, what = make_gpu(capi, O, form, monkeypatch)
        if G is None:
            continue
        if name_matches(form, what):
            return name, p, O, G
        G.destroy()
    raise AssertionError(f"no operator below the autotune's threshold is served by {form.key}")


def product(capi, G, p):
    dx, dy = capi.DeviceVector(p.N, inputs.v2(p.N)), capi.DeviceVector(p.M)
    G.spmv(dx, dy)
    y = dy.download()
    dx.free(); dy.free()
    return y


_CHECKED = {}


def check_keep_set(capi, key, monkeypatch):
    form = BY_KEY[key]
    monkeypatch.delenv("SAENA_KEEP_HOST_VALUES", raising=False)
    name, p, O, G = first_served(capi, form, monkeypatch)
    state = (G.variant(), G.x_windows())
    before = product(capi, G, p)
    held = groups(capi, G)
    G.autotune()
    got = groups(capi, G)
    print(f"{key} on {name}: held {sorted(held)} -> kept {sorted(got)}")
    assert got == expected(form), (key, name, sorted(got), sorted(expected(form)))
    assert got <= held
    assert (G.variant(), G.x_windows()) == state and state[0][0] == form.variant and state[1] == form.xw
    assert np.array_equal(bits(product(capi, G, p)), bits(before)), (key, name)
    G.destroy()
    _CHECKED[key] = form.variant


@pytest.mark.parametrize("key", [f.key for f in FORMS])
def test_a_settled_plan_keeps_its_variant_s_groups(capi, key, monkeypatch):
    """set_variant (+ set_x_windows), a product, autotune(): the groups that hold memory are exactly the variant's keep-set; variant,
    kernel name and x-window setting are unchanged; the product afterwards has the same bits"""
    check_keep_set(capi, key, monkeypatch)


def test_every_variant_was_checked(capi, monkeypatch):
    """no variant is skipped: every key of the catalogue went through the check above (run here if this test runs on its own)"""
    for f in FORMS:
        if f.key not in _CHECKED:
            check_keep_set(capi, f.key, monkeypatch)
    assert sorted(set(_CHECKED.values())) == list(range(18))
    assert sorted(KEEPS) == list(range(18))


def settled(capi, name, key, monkeypatch):
    form = BY_KEY[key]
    p = problem(name)
    O = oracle_op(p)
    G, what = make_gpu(capi, O, form, monkeypatch)
    assert G is not None and name_matches(form, what), what
    G.autotune()
    assert groups(capi, G) == expected(form)
    return p, O, G


def test_freed_forms_can_be_built_again(capi, monkeypatch):
    """what a settled plan freed is not barred: the forms are rebuilt from the CSR arrays on the device"""
    monkeypatch.delenv("SAENA_KEEP_HOST_VALUES", raising=False)
    p, O, G = settled(capi, "poisson13", "sellp", monkeypatch)
    want = O.matvec(inputs.v2(p.N))
    for v in (17, 14):
        G.set_variant(v)
        assert G.variant()[0] == v
        assert np.array_equal(bits(product(capi, G, p)), bits(want)), v
    G.destroy()
    p, O, G = settled(capi, "poisson13", "vidx.w512", monkeypatch)
    assert "xwin256" not in groups(capi, G)
    G.set_x_windows(256)
    assert G.x_windows() == 256 and {"xwin256", "xwin512"} <= groups(capi, G)
    assert np.array_equal(bits(product(capi, G, p)), bits(want))
    G.destroy()


def test_x_in_lds_is_refused_after_the_plan_settled_on_sellx(capi, monkeypatch):
    """k_sellx keeps the chunk plan and drops k_csr_xlds's columns: variant 10 is then refused (SGPU_ERR_STATE) without a launch --
    by the launch's own guard on the missing columns, at the first product"""
    monkeypatch.delenv("SAENA_KEEP_HOST_VALUES", raising=False)
    form = BY_KEY["sellx"]
    name, p, O, G = first_served(capi, form, monkeypatch)
    G.autotune()
    assert groups(capi, G) == expected(form)
    dx, dy = capi.DeviceVector(p.N, inputs.v2(p.N)), capi.DeviceVector(p.M)
    n0 = capi.launch_count()
    with pytest.raises(capi.SgpuError, match=rf"status {SGPU_ERR_STATE}: the x-in-LDS form was not built"):
        G.set_variant(10)
        G.spmv(dx, dy)
    assert capi.launch_count() == n0
    assert "xlds_columns" not in groups(capi, G)
    G.destroy()


@pytest.mark.parametrize("name,keys,winner", [("poisson13", ["sell", "sellp", "sellp2", "sellpx", "vidx.w256", "xlds.l8", "cc16_16"], "cc16_16"),
                                              ("dense", ["dense", "stream16"], "stream16"),
                                              ("dense", ["stream16", "dense"], "dense")])
def test_keep_host_values_keeps_every_form_but_a_losing_dense_one(capi, name, keys, winner, monkeypatch):
    """SAENA_KEEP_HOST_VALUES=1 (development sweeps switch variants after the autotune): the mask after autotune() is the mask before
    it, minus the dense rows when variant 5 did not win"""
    monkeypatch.setenv("SAENA_KEEP_HOST_VALUES", "1")
    p = problem(name)
    G = util.gpu_operator(oracle_op(p))
    for key in keys:
        G.set_variant(BY_KEY[key].variant)
        if BY_KEY[key].xw:
            G.set_x_windows(BY_KEY[key].xw)
    assert G.variant()[0] == BY_KEY[winner].variant
    held = groups(capi, G)
    assert held >= set().union(*(expected(BY_KEY[k]) for k in keys))
    G.autotune()
    assert groups(capi, G) == (held if winner == "dense" else held - {"dense"})
    G.destroy()


def test_nothing_outlives_its_owner(capi, monkeypatch):
    """every variant created, settled and destroyed; a three-level hierarchy through a V-cycle, a block V-cycle, FGMRES and LOBPCG and
    destroyed: the library's live-byte count is exactly what it was (it counts the library's own allocations: no allowance)"""
    monkeypatch.delenv("SAENA_KEEP_HOST_VALUES", raising=False)
    first = capi.live_bytes()
    seen = set()
    for form in FORMS:
        if form.variant in seen:
            continue
        seen.add(form.variant)
        name, p, O, G = first_served(capi, form, monkeypatch)
        assert capi.live_bytes() > first
        G.autotune()
        G.destroy()
        assert capi.live_bytes() == first, form.key
    assert seen == set(range(18))
    _, G, (OA, _, _), ops = build(capi, _hier(), "chebyshev")       # hierarchy.poisson_hierarchy(34, 3)
    n, K = OA[0].Mbig, 2
    rhs = inputs.rhs2(n)
    du, dr = capi.DeviceVector(n, np.zeros(n)), capi.DeviceVector(n, rhs)
    G.vcycle(du, dr)
    dU, dR = capi.BlockVector(n, K, np.zeros((n, K))), capi.BlockVector(n, K, np.stack([rhs, 2.0 * rhs], axis=1))
    G.vcycle_block(dU, dR)
    du.fill(0.0)
    G.solve_fgmres(du, dr, restart=10)
    dX = capi.BlockVector(n, K, np.stack([inputs.v2(n), inputs.v_sin(n)], axis=1))
    G.lobpcg(dX, 1, max_iter=5)
    during = capi.live_bytes()
    assert during > first
    G.destroy()
    assert first < capi.live_bytes() < during                     # (the operators outlive the hierarchy built over them)
    for o in (o for level in ops for o in level):
        o.destroy()
    assert capi.live_bytes() == first


def test_a_refused_operator_leaves_nothing_behind(capi):
    """sgpu_op_create that fails half-way -- a send index outside the rank's columns, found after the CSR arrays were uploaded --
    frees what it had made"""
    p = problem("small")
    rows, cols, vals = (np.asarray(p.entries[k]) for k in ("row", "col", "val"))
    order = np.lexsort((cols, rows))
    first = capi.live_bytes()
    with pytest.raises(capi.SgpuError, match="vIndex out of range"):
        capi.Operator(M=p.M, N_local=p.N, col_offset=0, nnzPerRow_local=np.bincount(rows, minlength=p.M), col_local=cols[order],
                      val_local=vals[order], sendProcRank=[0], sendProcCount=[1], vIndex=[p.N], inv_diag=np.ones(p.M))
    assert capi.live_bytes() == first
