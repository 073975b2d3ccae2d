"""tests/device_cg_ref.py on the CPU: the numpy restatement of the device-resident coarsest CG, its dots in the blocked order of the
kernels, stays inside every bound tests/test_gpu_device_cg.py asserts, on every case that module uses -- so a failure there is the
kernels', not the bounds'.  The oracle here is solver_ref.coarsest_cg (the recurrence with numpy's own dots)."""
import numpy as np
import pytest

from tests import device_cg_ref as dr, solver_ref as sr

IDS = lambda c: f"{c[0]}{c[1]}"      # noqa: E731


@pytest.mark.parametrize("case", dr.CONTRACT_CASES + dr.EXTRA_CASES + dr.SET_OPERATOR, ids=IDS)
def test_the_restatement_meets_the_four_contracts(case):
    c = dr.case(*case)
    assert case[1] > sr.CG_MAXN
    u_o, it_o = sr.coarsest_cg(c["A"], c["rhs"])
    u, it, worked = dr.device_cg(c["A"], c["rhs"])
    dr.check_contracts(c, u, it, u_o, it_o)
    assert 1 < it < sr.CG_MAX_ITER - 1                                   # (converged: the cap is another test)
    assert worked == 2 + 3 * it and worked < dr.launches(sr.CG_MAX_ITER)  # the launches after the stop do nothing


def test_the_big_tridiagonal_case():
    """262 401 rows: against coarsest_cg and the high-precision residual only"""
    n = dr.BIG_TRI
    assert n > sr.BLOCK * sr.N_PARTIALS
    A, rhs = sr.tri(n), sr.rhs_for(n)
    u_o, it_o = sr.coarsest_cg(A, rhs)
    u, it, _ = dr.device_cg(A, rhs)
    print(f"it {it} (oracle {it_o}), rel {sr.rel(u, u_o):.2e}")
    assert abs(it - it_o) <= dr.IT_SLACK and it < 100
    assert sr.rel(u, u_o) <= dr.REL_ORACLE
    assert sr.residual_hp(A, u, rhs) <= dr.RESID_FACTOR * sr.CG_TOL * np.linalg.norm(rhs)


@pytest.mark.parametrize("case", dr.EARLY_OUT_CASES, ids=IDS)
def test_early_outs(case):
    c = sr.case(*case)
    n = case[1]
    u0 = np.linspace(-1.0, 1.0, n)
    u0[0] = -0.0
    tiny = c["rhs"] * (1e-13 / np.linalg.norm(c["rhs"]))
    for rhs in (np.zeros(n), tiny):
        _, it_o = sr.coarsest_cg(c["A"], rhs, u0)
        u, it, worked = dr.device_cg(c["A"], rhs, u0)
        assert it == it_o == 1 and worked == 2
        assert np.array_equal(u.view(np.uint64), u0.view(np.uint64))


@pytest.mark.parametrize("case", dr.CAPPED_CASES, ids=IDS)
def test_the_cap(case):
    c = sr.case(*case)
    u_o, it_o = sr.coarsest_cg(c["A"], c["rhs"], max_iter=dr.CAP)
    u, it, worked = dr.device_cg(c["A"], c["rhs"], max_iter=dr.CAP)
    assert it == 5 and it_o == 5 and worked == dr.launches(dr.CAP) == 17
    assert sr.rel(u, u_o) <= dr.REL_ORACLE
    assert sr.rel(u_o, c["x"]) > 1e-6                                    # (the cap ended it, not the tolerance)


@pytest.mark.parametrize("cap", dr.CAPS)
@pytest.mark.parametrize("case", dr.CAPS_CASES, ids=IDS)
def test_the_smallest_and_the_odd_caps(case, cap):
    """caps 1, 2, 3 and 7 past 1 024 rows: coarsest_cg's count (cap - 1: the cap ended it), its iterate, every launch of the sequence
    at work; at cap 1 nothing touches u, a -0.0 included"""
    c = dr.case(*case)
    n = case[1]
    u0 = np.linspace(-1.0, 1.0, n)
    u0[0] = -0.0
    u_o, it_o = sr.coarsest_cg(c["A"], c["rhs"], u0, max_iter=cap)
    u, it, worked = dr.device_cg(c["A"], c["rhs"], u0, max_iter=cap)
    print(f"cap {cap}: it {it} (coarsest_cg {it_o}), {worked} launches, rel {sr.rel(u, u_o):.2e}")
    assert it == it_o == dr.CAPS_COUNT[cap]
    assert worked == dr.launches(cap) == 2 + 3 * (cap - 1)
    assert sr.rel(u, u_o) <= dr.REL_ORACLE
    if cap == 1:
        assert np.array_equal(u.view(np.uint64), u0.view(np.uint64)) and np.array_equal(u_o.view(np.uint64), u0.view(np.uint64))
    else:
        assert not np.array_equal(u, u0)
        assert sr.rel(sr.coarsest_cg(c["A"], c["rhs"], max_iter=cap)[0], c["x"]) > 1e-6      # (the cap ended it, not the tolerance)


@pytest.mark.parametrize("max_iter", [0, 1, 2, 3])
def test_the_count_at_the_smallest_caps(max_iter):
    """solve_coarsest_CG's convention where the loop runs not at all, or once"""
    c = sr.case("tri", 1025)
    u_o, it_o = sr.coarsest_cg(c["A"], c["rhs"], max_iter=max_iter)
    u, it, _ = dr.device_cg(c["A"], c["rhs"], max_iter=max_iter)
    assert it == it_o
    assert sr.rel(u, u_o) <= dr.REL_ORACLE if np.any(u_o) else not np.any(u)


def test_lanes_per_row_of_the_cases():
    """the cases reach the product kernel's four instantiations"""
    got = {f: dr.lanes_per_row(dr.case(f, n)["A"]) for f, n in dr.CONTRACT_CASES + dr.EXTRA_CASES}
    assert got == {"tri": 1, "band17": 4, "arrow": 1, "band49": 16, "dense_spd": 64}
