"""The opt-in device estimate of eig_max in the one-rank setup and in update1 / update2 (saena_amg_set_device_eig, SAENA_DEVICE_EIG,
host.AmgSolver(device_eig=...)), and a caller's own estimate (host.Matrix.estimate_eig + set_eig).

Poisson 16^3 (2744 rows), the reference's options001 with the Chebyshev smoother.  What is held:
  * built with the switch on, every level's eig_max is within 1e-12 relative of the host loop's and not all of them are the same bits
    (the device path ran); solve_pCG on both builds takes the same iterations and gives solutions within rel-l2 1e-9 -- the bound
    tests/test_gpu_block_multirank.py uses between rank counts -- after checking that no residual of the host build's history lies
    within a factor 1 +- 1e-3 of the threshold;
  * update2 / update1 with the switch on: the refreshed levels' eig_max within 1e-12 of tests/setup_ref.lanczos_eig on
    tests/update_ref.py's operators; a value the caller set on the new matrix is kept exactly;
  * with the switch off and the hook installed, setup and update2 give the bits of libsaena_host.so, which has no hook at all;
  * estimate_eig composed with set_eig, then update1 with the switch off, is the switch-on update1 within 1e-12.

Operators are made without the plan-time autotune (SAENA_NO_AUTOTUNE): both builds then hold every level in the same form."""
import os

import numpy as np
import pytest

from tests import setup_ref, update_ref

pytestmark = pytest.mark.gpu
BOUND = 1e-12
M = 16


@pytest.fixture(scope="module")
def capi():
    from saena_amd import capi as c
    c.init(0)
    return c


@pytest.fixture(scope="module")
def host(capi):
    from saena_amd import host as h
    saved = {k: os.environ.get(k) for k in ("SAENA_NO_AUTOTUNE", "SAENA_DEVICE_EIG")}
    os.environ["SAENA_NO_AUTOTUNE"] = "1"
    os.environ.pop("SAENA_DEVICE_EIG", None)
    yield h
    for k, v in saved.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v


def options(host):
    return dict(host.OPTIONS001, smoother="chebyshev")


def build(host, device_eig, which="gpu"):
    A = host.Matrix(host.Comm(which, "rccl" if which == "gpu" else "self")).laplacian3D(M).assemble()
    return A, host.AmgSolver(A, host.options(host.load(which), **options(host)), device_eig=device_eig)


def eigs(S):
    return [S.level_info(l)["eig_max"] for l in range(S.num_levels)]


def close(got, want, what):
    rel = [abs(g - w) / abs(w) for g, w in zip(got, want)]
    print(f"{what}: {got} against {want}: relative differences {['%.2e' % r for r in rel]}")
    assert len(got) == len(want) and max(rel) <= BOUND, (what, got, want)


@pytest.fixture(scope="module")
def pair(host):
    """(A, S) built with the switch off and with it on"""
    return build(host, False), build(host, True)


def test_setup_takes_its_estimates_from_the_device(pair):
    (_, off), (_, on) = pair
    assert off.num_levels == on.num_levels >= 3
    close(eigs(on), eigs(off), "setup, switch on against off")
    assert [float(e).hex() for e in eigs(on)] != [float(e).hex() for e in eigs(off)], "every level has the host loop's bits: the device path did not run"
    for l in range(off.num_levels):                       # nothing else of the hierarchy depends on the switch
        a, b = off.level_layout(l, 0), on.level_layout(l, 0)
        assert all(np.array_equal(a[k], b[k]) for k in ("nnzPerRow_local", "col_local", "val_local", "inv_diag"))


def test_solve_pcg_on_both_builds(host, pair):
    (A, off), (_, on) = pair
    n = A.num_local_rows
    rhs = np.sin(0.37 * np.arange(n) + 0.1) + 0.05
    tol = options(host)["relative_tol"]
    off.to_device(); on.to_device()
    u0, it0, h0, ok0 = off.solve_pCG(rhs)
    u1, it1, h1, ok1 = on.solve_pCG(rhs)
    thr = tol * h0[0]
    print("host build:", it0, h0, "threshold", thr, "; device build:", it1, h1)
    assert ok0 and not np.any((h0 > thr * (1 - 1e-3)) & (h0 < thr * (1 + 1e-3))), f"a history entry sits at its threshold: {h0}, {thr}"
    assert ok1 and it1 == it0
    err = np.linalg.norm(u1 - u0) / np.linalg.norm(u0)
    print(f"rel-l2 difference of the solutions {err:.2e}")
    assert err <= 1e-9


def shifted(host, A, which="gpu", eig=None):
    entries = update_ref.variant(A, "shift")
    B = host.Matrix(host.Comm(which, "rccl" if which == "gpu" else "self"))
    B.set_remove_boundary(False)
    B.set_many(*entries)
    if eig is not None:
        B.set_eig(eig)
    return B.assemble(), entries


def test_update2_with_the_switch_on(host):
    A, S = build(host, True)
    before = update_ref.levels_of(S)
    B, entries = shifted(host, A)
    S.update(B, 2)
    want = update_ref.update2(before, update_ref.csr_of_entries(A.num_rows, *entries), options(host))
    close(eigs(S), [setup_ref.lanczos_eig(W) for W in want], "update2, switch on, against the restatement")
    _, H = build(host, False, "host")                     # the host loop on the same update
    BH, _ = shifted(host, A, "host")
    H.update(BH, 2)
    close(eigs(S), eigs(H), "update2, switch on, against the host library")
    assert [float(e).hex() for e in eigs(S)] != [float(e).hex() for e in eigs(H)], "the device path did not run"
    # a value the caller set on the new matrix is kept exactly; the coarse levels are still estimated
    C_, _ = shifted(host, A, eig=1.2345)
    S.update(C_, 2)
    assert eigs(S)[0] == 1.2345
    close(eigs(S)[1:], eigs(H)[1:], "update2 with a set value: the coarse levels")


def test_update1_with_the_switch_on(host):
    A, S = build(host, True)
    e0 = eigs(S)
    B, entries = shifted(host, A)
    S.update(B, 1)
    e1 = eigs(S)
    close(e1[:1], [setup_ref.lanczos_eig(update_ref.csr_of_entries(A.num_rows, *entries))], "update1, switch on, level 0")
    assert e1[0] != e0[0] and [float(e).hex() for e in e1[1:]] == [float(e).hex() for e in e0[1:]]
    C_, _ = shifted(host, A, eig=1.2345)
    S.update(C_, 1)
    assert eigs(S) == [1.2345] + e0[1:]


def test_switch_off_keeps_the_host_bits_with_the_hook_installed(host, pair):
    (A, off), _ = pair
    _, H = build(host, False, "host")                     # libsaena_host.so: no hook exists
    assert [float(e).hex() for e in eigs(off)] == [float(e).hex() for e in eigs(H)]
    _, S = build(host, None)                              # the library's default, the environment variable unset
    assert [float(e).hex() for e in eigs(S)] == [float(e).hex() for e in eigs(H)]
    B, _ = shifted(host, A)
    BH, _ = shifted(host, A, "host")
    S.update(B, 2); H.update(BH, 2)
    assert [float(e).hex() for e in eigs(S)] == [float(e).hex() for e in eigs(H)]
    os.environ["SAENA_DEVICE_EIG"] = "1"                  # the environment variable is read at every call
    try:
        B2, _ = shifted(host, A)
        S.update(B2, 2)
    finally:
        os.environ.pop("SAENA_DEVICE_EIG", None)
    close(eigs(S), eigs(H), "update2 under SAENA_DEVICE_EIG=1")
    assert [float(e).hex() for e in eigs(S)] != [float(e).hex() for e in eigs(H)], "SAENA_DEVICE_EIG=1 did not reach the device path"


def test_a_callers_own_estimate(host):
    A, on = build(host, True)
    _, off = build(host, False)
    B, _ = shifted(host, A)
    on.update(B, 1)
    C_, _ = shifted(host, A)
    e = C_.estimate_eig()
    assert C_.estimate_eig(0) == e and C_.estimate_eig(5) < e
    C_.set_eig(e)
    off.update(C_, 1)
    assert eigs(off)[0] == e
    close(eigs(off)[:1], eigs(on)[:1], "estimate_eig + set_eig + update1 (switch off) against update1 with the switch on")
