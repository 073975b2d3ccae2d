"""The reference of LOBPCG with hard locking (tests/eig_lock_ref.py) on the CPU: with no locked vectors it IS eig_ref.lobpcg /
geig_ref.lobpcg_gen, bit for bit; a correct implementation of the constrained solve and of the driver stays inside every bound
tests/test_gpu_eig_lock.py asserts; the numbers that file takes from eig_lock_ref (total iterations, sweeps, B-orthonormality) are what
the reference gives; the sweep bookkeeping of saena_amd/csrc/eig_lock_plan.h, compiled with g++, agrees with its restatement and runs
its edge cases clean under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

from tests import eig_lock_ref as lr, eig_ref as er, geig_ref as gg, solver_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_RUN = {}


def run(shape):
    """the reference driver on one shape, once"""
    if shape not in _RUN:
        (m, K, nev, sweep_nev), mass = shape
        c = er.case(m)
        _, B = lr.operators(shape)
        _RUN[shape] = lr.many(c["A"], B, nev, K, sweep_nev, precond=er.vcycle_block(c))
    return _RUN[shape]


# ---- no locked vectors ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mass", (None,) + gg.MASSES)
def test_without_locked_vectors_it_is_the_unconstrained_reference(mass):
    """X, lambda, res, the history and the count of eig_ref.lobpcg (no B) and geig_ref.lobpcg_gen, bit for bit; an empty Q is no Q"""
    shape = er.SHAPES[0]
    m, K, nev = shape
    c = er.case(m)
    X0 = er.start_vectors(m ** 3, K)
    if mass:
        B = gg.mass(mass, m)
        want = gg.lobpcg_gen(c["A"], B, X0, nev, precond=er.vcycle_block(c))
    else:
        B = None
        want = er.lobpcg(c["A"], X0, nev, precond=er.vcycle_block(c))
    for Q in (None, np.zeros((m ** 3, 0))):
        got = lr.lobpcg_locked(c["A"], B, X0, nev, Q, Q, precond=er.vcycle_block(c))
        assert got["iters"] == want["iters"] and got["converged"] and got["leading"] >= nev
        for k in ("X", "lam", "res", "hist"):
            assert np.array_equal(got[k].view(np.uint64), want[k].view(np.uint64)), (mass, k)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", lr.SHAPES, ids=str)
def test_reference_converges_inside_the_bounds(shape):
    """every assertion of the GPU test on the reference itself, and the recorded numbers"""
    (m, K, nev, sweep_nev), mass = shape
    r = run(shape)
    assert r["converged"] and r["nlocked"] == nev and r["Q"].shape == (m ** 3, nev)
    rhos = lr.check_pairs(shape, r["Q"], r["lam"])
    defect = lr.ortho_defect(shape, r["Q"])
    print(f"{shape}: {r['iters']} iterations in {r['sweeps']} sweeps {r['per_sweep']}, max |Q^T B Q - I| = {defect:.3e}")
    assert r["iters"] == lr.ITERS[shape] and r["sweeps"] == lr.SWEEPS[shape] and sum(r["per_sweep"]) == r["iters"]
    assert r["iters"] <= lr.iteration_bound(shape) <= lr.MAX_ITER
    assert defect <= 2 * lr.ORTHO[shape]                        # recorded here; twice: another BLAS adds in another order
    assert np.all(np.diff(r["lam"]) >= 0.0)
    assert r["sweeps"] >= -(-nev // K) and nev > K                # more pairs than one block holds
    _, B = lr.operators(shape)
    for j in range(nev):                                        # the reported residual is the recomputed one of the locking sweep
        x = r["Q"][:, j]
        scale = np.linalg.norm(B @ x) if mass else np.linalg.norm(x)
        assert r["res"][j] < lr.TOL * r["lam"][j] * scale
        assert abs(r["res"][j] - rhos[j] * scale) <= 1e-3 * r["res"][j] + 1e-12 * r["lam"][j]


def test_the_shapes_cut_clusters():
    """nev = 20 at sweeps of 4 cuts clusters of equal eigenvalues (1 + 3 + 3 + 3 + 1 + 6 + 3 ... on 8^3), and the driver still returns
    each eigenvalue with its multiplicity: no value missed, none repeated beyond it"""
    shape = lr.SHAPES[0]
    want = lr.exact(shape)
    gaps = np.diff(want) / want[1:]
    starts = [0] + [int(i) + 1 for i in np.flatnonzero(gaps > 1e-9)]
    sizes = np.diff(starts + [len(want)])
    assert list(sizes[:5]) == [1, 3, 3, 3, 1] and any(s % 4 for s in np.cumsum(sizes)[:-1])
    r = run(shape)
    assert np.max(np.abs(r["lam"] - want) / want) <= 1e-9


def test_a_locked_solve_returns_the_next_pairs():
    """with the exact eigenvectors of the 4 smallest eigenvalues locked, the constrained solve for 4 pairs returns pairs 5 to 8 and X
    stays orthogonal to the locked set; the same for the generalised problem with mass27 (B-normalised, B-orthogonal)"""
    m, K, nev = 8, 8, 4
    c = er.case(m)
    s = [np.sin(np.pi * k * np.arange(1, m + 1) / (m + 1.0)) for k in (1, 2)]
    Q0 = np.stack([np.kron(np.kron(s[a], s[b]), s[d]) for a, b, d in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1))], axis=1)
    for mass in (None, "mass27"):
        B = gg.mass(mass, m) if mass else None
        BQ = B @ Q0 if mass else Q0
        Q = Q0 / np.sqrt(np.sum(Q0 * BQ, axis=0))[None, :]
        BQ = B @ Q if mass else Q
        r = lr.lobpcg_locked(c["A"], B, er.start_vectors(m ** 3, K), nev, Q, BQ, precond=er.vcycle_block(c))
        want = lr.exact(((m, K, 8, 4), mass))
        assert r["converged"] and r["leading"] >= nev
        assert np.max(np.abs(r["lam"][:nev] - want[4:8]) / want[4:8]) <= 1e-9
        assert np.max(np.abs(BQ.T @ r["X"])) <= 1e-13


def test_a_small_max_iter_returns_the_pairs_locked_so_far():
    shape = lr.SHAPES[0]
    (m, K, nev, sweep_nev), _ = shape
    c = er.case(m)
    budget = lr.ITERS[shape] // 2
    r = lr.many(c["A"], None, nev, K, sweep_nev, max_iter=budget, precond=er.vcycle_block(c))
    assert not r["converged"] and 0 < r["nlocked"] < nev and r["iters"] <= budget
    assert np.all(np.diff(r["lam"]) >= 0.0)
    lr.check_pairs(shape, r["Q"], r["lam"], nev=r["nlocked"], what="locked so far")


# ---- the kernels' restatements ----------------------------------------------------------------------------------------------------------
def test_restatements_of_the_kernels():
    rng = np.random.default_rng(11)
    n, L, K = 300, 9, 4
    Q, W, Cm = rng.standard_normal((n, L)), rng.standard_normal((n, K)), rng.standard_normal((L, K))
    got = lr.lock_project(Q, Cm, W)
    want = np.zeros((n, K))
    for i in (0, 17, n - 1):
        for b in range(K):
            acc = 0.0
            for l in range(L):
                acc = acc + Q[i, l] * (-Cm[l, b])
            want[i, b] = acc + W[i, b]
        assert np.array_equal(got[i], want[i])
    assert np.max(np.abs(got - (W - Q @ Cm))) <= 1e-13
    Q4 = Q[:, :K]
    assert np.array_equal(lr.lock_project(Q4, Cm[:K], W), er.block_mix([Q4], [-Cm[:K]], add=W))      # k_block_mix's order with its Add operand
    G = lr.lock_gram(Q, W)
    assert G.shape == (L, K) and np.max(np.abs(G - Q.T @ W)) <= 1e-12
    assert G[3, 2] == sr.dot_blocked(Q[:, 3], W[:, 2])
    assert np.array_equal(lr.lock_gram(Q[:, 3:4], W[:, 2:3]), G[3:4, 2:3])   # an entry depends on its two columns alone


def test_the_refill_generator():
    """exact in [-1, 1) on the grid of 2^-52, the values of the integer recipe in plain Python, no column repeats another"""
    mask = 2 ** 64 - 1

    def one(row, counter):
        z = (row * 0x9E3779B97F4A7C15 + (counter + 1) * 0xD1B54A32D192ED03) & mask
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & mask
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & mask
        z ^= z >> 31
        return (z >> 11) / 2.0 ** 52 - 1.0
    for counter in (0, 1, 7, 2 ** 32 - 1):
        v = lr.refill(1000, counter)
        assert np.all(v >= -1.0) and np.all(v < 1.0)
        assert np.array_equal(v * 2.0 ** 52, np.round(v * 2.0 ** 52))
        for row in (0, 1, 2, 999):
            assert v[row] == one(row, counter)
    big = lr.refill(100003, 3)
    assert abs(big.mean()) < 0.02 and abs(big.std() - 1 / np.sqrt(3)) < 0.02 and len(np.unique(big)) == len(big)
    X, counter = lr.start_block(512, 8)
    assert counter == 8 and np.linalg.matrix_rank(X) == 8 and np.array_equal(X[:, 5], lr.refill(512, 5))


# ---- the bookkeeping header -------------------------------------------------------------------------------------------------------------
PROGRAM = r"""
#include "eig_lock_plan.h"
#include <cstdio>
#include <iostream>
#include <string>
// lines: "sweep K nev nlocked sweep_nev leading counter" -> "want take counter' col:ctr ..." | "order L v0 v1 ..." -> the permutation
int main() {
    std::string what;
    while (std::cin >> what) {
        if (what == "sweep") {
            int K, nev, nlocked, sweep_nev, leading; unsigned long counter;
            std::cin >> K >> nev >> nlocked >> sweep_nev >> leading >> counter;
            uint32_t c = (uint32_t)counter;
            const int want = eig_lock::sweep_want(nev, nlocked, sweep_nev ? sweep_nev : eig_lock::default_sweep_nev(K));
            const int take = eig_lock::sweep_take(K, nev, nlocked, leading);
            const std::vector<eig_lock::Refill> plan = eig_lock::refill_plan(take, &c);
            std::printf("%d %d %lu", want, take, (unsigned long)c);
            for (const eig_lock::Refill &r : plan) std::printf(" %d:%lu", r.col, (unsigned long)r.counter);
            std::printf("\n");
        } else {
            int L; std::cin >> L;
            std::vector<double> v((size_t)L);
            for (double &x : v) std::cin >> x;
            for (int p : eig_lock::final_order(L, v.data())) std::printf("%d ", p);
            std::printf("\n");
        }
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("eig_lock_plan_check")
    src, out = str(d / "eig_lock_plan_check.cpp"), str(d / "eig_lock_plan_check")
    with open(src, "w") as f:
        f.write(PROGRAM)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "saena_amd", "csrc"), src, "-o", out]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    return out


def test_the_bookkeeping_header_agrees_with_its_restatement(exe):
    """how many pairs a sweep asks for, how many columns it locks, which columns are refilled with which counter values, and the final
    permutation: eig_lock_plan.h against eig_lock_ref on every (K, nev, nlocked, sweep_nev, leading) of a grid that holds nev no
    multiple of sweep_nev, a sweep that locks all K columns, nev = 1, the default sweep_nev, and ties in the final order"""
    cases, want = [], []
    for K in (2, 4, 8):
        for nev in (1, 3, 7, 20, 64):
            for nlocked in sorted({0, 1, nev // 2, nev - 1}):
                if nlocked >= nev:
                    continue
                for sweep_nev in (0, 1, K // 2, K):
                    for leading in (0, 1, K // 2, K):
                        counter = 8 + 3 * nlocked
                        cases.append(f"sweep {K} {nev} {nlocked} {sweep_nev} {leading} {counter}")
                        take = lr.sweep_take(K, nev, nlocked, leading)
                        plan, after = lr.refill_plan(take, counter)
                        want.append([str(lr.sweep_want(nev, nlocked, sweep_nev or lr.default_sweep_nev(K))), str(take), str(after)]
                                    + [f"{col}:{ctr}" for col, ctr in plan])
    rng = np.random.default_rng(3)
    for L in (1, 2, 5, 20, 64):
        v = np.round(rng.standard_normal(L), 1)                  # one decimal: ties
        cases.append(f"order {L} " + " ".join(repr(float(x)) for x in v))
        want.append([str(p) for p in lr.final_order(v)])
    r = subprocess.run([exe], input="\n".join(cases) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = [ln.split() for ln in r.stdout.splitlines()]
    assert len(got) == len(want)
    for c, g, w in zip(cases, got, want):
        assert g == w, (c, g, w)


def test_the_bookkeeping_under_the_sanitizers(tmp_path):
    """a stand-alone program with the sanitizer runtimes linked in statically: it runs in whatever environment the suite runs in"""
    exe = str(tmp_path / "sanitize_eig_lock")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
           os.path.join(ROOT, "tools", "sanitize_eig_lock.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stdout + b.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("ok"), r.stdout + r.stderr
