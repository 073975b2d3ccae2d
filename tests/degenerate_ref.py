"""The contract of include/saena_gpu.h, "Degenerate right-hand sides", in numpy (test infrastructure: no GPU, no oracle).

  rule 1   ||r_0||^2 == 0: u = 0, 0 iterations, res_hist[0] = 0.0, converged, nothing iterated
  rule 2   null_space 1: ||rhs - m||^2 <= n (k u |m|)^2, m the mean the centring computed, k = solver_ref.dot_roundings(n), is rule 1
  rule 3   the first ||r_k||^2 that is not finite ends the solve: not converged, iters = k, res_hist[k] holds the value

Where the criterion of rule 2 comes from.  The centring is y = x - S / n with S summed on sgpu_dot's grid.  For x = c 1
every partial sum is an exact multiple of c times (1 + theta), and at most k_s = dot_roundings(n) - 2 additions lie between an
element and S (dot_roundings counts the product and the rounding of the reference too: neither exists here).  So S = n c (1 + t_1),
|t_1| <= gamma(k_s); the division adds one rounding, m = c (1 + t_2), |t_2| <= gamma(k_s + 1); the subtraction is
y_i = (c - m)(1 + d) = -c t_2 (1 + d).  With |c| <= |m| / (1 - gamma(k_s + 1)):
    |y_i| <= (k_s + 1) u |m| (1 + O(k u)) <= k u |m|,   k = k_s + 2,
the factor (k_s + 2) / (k_s + 1) >= 1.03 covering the second-order terms (k u < 1e-14) and the roundings of the dot itself.  Hence
||y||^2 <= n (k u |m|)^2 for every constant right-hand side, whatever n and c: the bound is derived, not measured.
"""
import numpy as np
import scipy.sparse as sp

from tests import solver_ref as sr

U = sr.U
A_PERTURB = 1e-3          # the perturbed constant of the tests: rhs = c + a |c| v, v of zero mean and unit RMS


def criterion(n, mean):
    """rule 2's bound on ||rhs - mean||^2"""
    e = sr.dot_roundings(n) * U * abs(float(mean))
    return n * e * e


def at_start(init_dot, n=None, mean=None, null_space=False):
    """-> "nonfinite", "zero" or None (iterate), from the initial ||r_0||^2; rule 3 is tested first (a NaN compares false anyway)"""
    if not np.isfinite(init_dot):
        return "nonfinite"
    if init_dot == 0.0 or (null_space and init_dot <= criterion(n, mean)):
        return "zero"
    return None


def start_result(kind, n, init_dot):
    """what a solve returns when at_start says it ends at iteration 0"""
    h0 = 0.0 if kind == "zero" else float(np.sqrt(init_dot)) if init_dot == init_dot and init_dot >= 0 else float("nan")
    return dict(u=np.zeros(n), iters=0, hist=np.array([h0]), converged=kind == "zero", stopped=kind)


def constant(n, c):
    return np.full(n, float(c))


def unit_rms_direction(n):
    """the centred rhs_for(n) scaled to unit RMS"""
    from tests import null_space_ref as ns
    v = ns.center(ns.rhs_for(n))[0]
    return v / np.sqrt(np.mean(v * v))


def perturbed(n, c, a=A_PERTURB):
    """c + a |c| v: a constant with a centred part far above the criterion"""
    return float(c) + a * abs(float(c)) * unit_rms_direction(n)


def indefinite_diag():
    """diag(+1 x 32, -1 x 32): with rhs = 1 the first p . A p of CG is exactly 0"""
    return sp.diags([np.concatenate([np.ones(32), -np.ones(32)])], [0], format="csr")


def cg(A, rhs, M=None, tol=1e-8, max_iter=50):
    """sgpu_solve_CG (M None) / sgpu_solve_pCG (M: the preconditioner) of a kind-0 hierarchy with the three rules; the residual is
    A u - rhs and corrections are subtracted, as in the library -> dict(u, iters, hist, converged, stopped)"""
    n = A.shape[0]
    u = np.zeros(n)
    with np.errstate(all="ignore"):
        r = A @ u - np.asarray(rhs, np.float64)
        init = float(r @ r)
        kind = at_start(init)
        if kind:
            return start_result(kind, n, init)
        hist, thr = [np.sqrt(init)], init * tol * tol
        rho = r if M is None else M(r)
        p = rho.copy()
        rr = float(r @ rho)
        for _ in range(max_iter):
            hh = A @ p
            alpha = np.float64(rr) / np.float64(p @ hh)
            u = u - alpha * p
            r = r - alpha * hh
            cur = float(r @ r)
            hist.append(np.sqrt(cur))
            if cur < thr:
                return dict(u=u, iters=len(hist) - 1, hist=np.array(hist), converged=True, stopped=None)
            if not np.isfinite(cur):
                return dict(u=u, iters=len(hist) - 1, hist=np.array(hist), converged=False, stopped="nonfinite")
            rho = r if M is None else M(r)
            rr_new = float(r @ rho)
            p = rho + (rr_new / rr) * p
            rr = rr_new
    return dict(u=u, iters=len(hist) - 1, hist=np.array(hist), converged=False, stopped=None)


def four_checks(H, u, hist, conv, rhs, want, what=""):
    """the four checks of tests/test_gpu_null_space.check_solution for a solve of A u = rhs - mean(rhs), with the reference
    null_space_ref.solve_plus of THIS right-hand side: convergence at the restatement's count +- 1 from res_hist[0] = ||rhs - mean||,
    the residual, the error and the mean of u.  -> the figures"""
    from tests import null_space_ref as ns
    A = H["A"][0]
    n = A.shape[0]
    bt = ns.center(rhs)[0]
    nb = np.linalg.norm(bt)
    res = sr.residual_hp(A, u, bt)
    x = ns.solve_plus(A, bt)[0]
    err, mean = sr.rel(u, x), abs(float(np.sum(np.asarray(u, np.longdouble)) / n))
    print(f"{what}: {len(hist) - 1} iterations (restatement {want['iters']}), residual {res / nb:.2e} of {1.01 * ns.TOL:.2e}, error {err:.2e} of "
          f"{ns.error_bound(A):.2e}, |mean u| {mean:.1e} of {sr.dot_bound(u, np.ones(n)) / n:.1e}")
    assert conv and want["converged"]
    assert abs((len(hist) - 1) - want["iters"]) <= 1
    assert abs(hist[0] - nb) <= 1e-13 * nb
    assert res <= 1.01 * ns.TOL * nb
    assert err <= ns.error_bound(A)
    assert mean <= sr.dot_bound(u, np.ones(n)) / n
    return dict(res=res / nb, err=err, mean=mean)
