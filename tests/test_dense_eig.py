"""saena_debug_sym_geig (saena_amd/csrc/host/dense_eig.cpp: Cholesky with a relative pivot test, cyclic Jacobi on L^-1 A L^-T) --
the Rayleigh-Ritz step of sgpu_eigs_LOBPCG -- through libsaena_host.so, against numpy.linalg.eigh / scipy.linalg.eigh.

Bounds.  One Jacobi sweep perturbs the reduced matrix C = L^-1 A L^-T by about n u ||C|| (its n (n - 1) / 2 rotations act on
disjoint pairs in groups of n / 2); forming C and transforming the vectors back cost two more such terms; so with s sweeps
    ||A v - w B v|| <= c n u ||A|| ||v||   and   max |V^T B V - I| <= c n u,     c = 2 (s + 2),
the bound the issue sets, which holds for a well-conditioned B and for an ill-conditioned B whose condition comes from a grading
D B0 D that A shares (the reduction is invariant under it).  For an UNSTRUCTURED B of condition 1e8 no method that goes through
B = L L^T can meet it: the residual is L (C q - w q), so the bound carries cond_2(B) -- scipy.linalg.eigh (LAPACK) misses the plain
bound by the same five to six orders of magnitude (measured: 1.2e5 to 3.9e6 times n u ||A|| ||v|| for LAPACK, 1.6e5 to 3.2e6 for
this code, orders 2 to 24).  That extra case is held to c n u (cond_2(B) / 10) ||A|| ||v||: the derivation's cond_2(B) is a worst case,
the tenth of it still lies above every figure measured.
"""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg

from saena_amd import host
from tests import solver_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = sr.U
ORDERS = (1, 2, 3, 6, 12, 24)


def sym(n, seed):
    A = np.random.default_rng(seed).standard_normal((n, n))
    return 0.5 * (A + A.T)


def spd(n, cond, seed):
    """Q diag(1 .. 1 / cond, log-spaced) Q^T"""
    Q, _ = np.linalg.qr(np.random.default_rng(seed).standard_normal((n, n)))
    d = np.logspace(0, -np.log10(cond), n) if n > 1 else np.ones(1)
    B = (Q * d) @ Q.T
    return 0.5 * (B + B.T)


def check(A, B, extra=1.0, what=""):
    n = A.shape[0]
    st, w, V, sweeps = host.sym_geig(A, B)
    assert st == 0, (what, st)
    c = 2 * (sweeps + 2)
    nA = np.linalg.norm(A, 2)
    worst = 0.0
    for k in range(n):
        v = V[:, k]
        r = np.linalg.norm(A @ v - w[k] * (B @ v))
        worst = max(worst, r / (n * U * nA * np.linalg.norm(v)))
        assert r <= c * n * U * nA * np.linalg.norm(v) * extra, (what, k, r)
    defect = np.max(np.abs(V.T @ B @ V - np.eye(n)))
    print(f"{what} order {n}: {sweeps} sweeps, residual / (n u |A| |v|) = {worst:.2f}, |V^T B V - I| / (n u) = {defect / (n * U):.2f}, c = {c}")
    assert defect <= c * n * U * extra, (what, defect)
    assert np.all(np.diff(w) >= 0.0)
    w_ref = scipy.linalg.eigh(A, B, eigvals_only=True)
    assert np.max(np.abs(w - w_ref)) <= c * n * U * nA * np.linalg.norm(np.linalg.inv(B), 2) * max(extra, 1.0), what
    return w, V


@pytest.mark.parametrize("n", ORDERS)
def test_well_conditioned_b(n):
    check(sym(n, n), spd(n, 10.0, 100 + n), what="cond 10")
    A = sym(n, 7 + n)
    w, V = check(A, np.eye(n), what="B = I")
    assert np.max(np.abs(w - np.linalg.eigh(A)[0])) <= 16 * n * U * np.linalg.norm(A, 2)


@pytest.mark.parametrize("n", ORDERS[1:])
def test_b_of_condition_1e8(n):
    """graded: B = D B0 D, A = D A0 D, D = diag(1 .. 1e-4): the issue's bound; unstructured: the bound with cond_2(B) / 10 (see the
    module's docstring)"""
    D = np.logspace(0, -4, n)
    A, B = sym(n, n) * D[:, None] * D[None, :], spd(n, 10.0, 100 + n) * D[:, None] * D[None, :]
    assert 3e7 <= np.linalg.cond(B) <= 3e8
    check(A, B, what="graded, cond 1e8")
    B = spd(n, 1e8, 100 + n)
    check(sym(n, n), B, extra=0.1 * np.linalg.cond(B), what="unstructured, cond 1e8")


@pytest.mark.parametrize("n", ORDERS[2:])
def test_repeated_eigenvalues(n):
    """A = B^1/2-congruent to diag(1, 1, 1, 2, 2, 5, ...): clusters of three and two equal eigenvalues, each vector still an
    eigenvector to the bound and the set B-orthonormal"""
    B = spd(n, 10.0, 300 + n)
    L = np.linalg.cholesky(B)
    d = np.array(([1.0, 1.0, 1.0, 2.0, 2.0] + [5.0 + k for k in range(n)])[:n])
    Q, _ = np.linalg.qr(np.random.default_rng(n).standard_normal((n, n)))
    A = L @ (Q * d) @ Q.T @ L.T
    w, _ = check(0.5 * (A + A.T), B, what="repeated")
    assert np.max(np.abs(w - np.sort(d))) <= 64 * n * U * np.linalg.norm(A, 2) * np.linalg.norm(np.linalg.inv(B), 2)


@pytest.mark.parametrize("n", ORDERS)
def test_a_b_that_is_not_positive_definite_is_reported(n):
    """indefinite, singular (a dependent Rayleigh-Ritz basis: a repeated row and column), zero and NaN: status -1, and nothing is
    written to w or V"""
    A = sym(n, n)
    good = spd(n, 10.0, 100 + n)
    bad = [good - 2.0 * np.eye(n), np.zeros((n, n)), np.full((n, n), np.nan)]
    if n > 1:
        S = np.random.default_rng(n).standard_normal((40, n))
        S[:, n - 1] = S[:, 0]
        bad.append(S.T @ S)
    for B in bad:
        st, w, V, _ = host.sym_geig(A, B)
        assert st == -1
        assert np.all(np.isnan(w)) and np.all(np.isnan(V))


def test_orders_outside_the_range_are_refused():
    for n in (25, 30):
        st, _, _, _ = host.sym_geig(np.eye(n), np.eye(n))
        assert st == -3


def test_dense_eig_under_the_sanitizers(tmp_path):
    """tools/sanitize_dense_eig.cpp with host/dense_eig.cpp, -fsanitize=address,undefined, as a stand-alone program with the
    sanitizer runtimes linked in statically: it runs in whatever environment the suite runs in"""
    exe = str(tmp_path / "sanitize_dense_eig")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tools", "sanitize_dense_eig.cpp"), os.path.join(ROOT, "saena_amd", "csrc", "host", "dense_eig.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)       # (the environment as it is)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
