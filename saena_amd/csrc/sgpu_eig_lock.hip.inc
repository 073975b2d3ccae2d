// sgpu_eig_lock.hip.inc -- hard locking for LOBPCG (include/saena_gpu.h): sgpu_eigs_LOBPCG_locked, the block solve of
// sgpu_eig.hip.inc constrained to the B-orthogonal complement of up to 64 locked vectors, and
// sgpu_eigs_LOBPCG_many, the driver that sweeps it to more than K eigenpairs.  Part of sgpu_runtime.hip, after sgpu_eig.hip.inc;
// kernels: kernels_eig_lock.hip.h; the sweep bookkeeping: eig_lock_plan.h (pure host); DESIGN.md section 18.
//
// The loop is the unconstrained one (lobpcg_run, either problem) with a locked set handed in: X <- X - Q (Z^T X) twice
// before the start orthonormalisation, W <- W - Q (Z^T W) once right after W = M R; Z = Q, or B Q for the generalised problem.  The
// coefficients Z^T W go from the reduce kernel to the projection through device memory: a locked iteration has the three host
// synchronisations of an unlocked one.  The lock kernels are eager launches; the V-cycle keeps its fixed (R, W) pair and its graph.
// With no locked column neither kernel is launched and nothing of AmgLock is allocated.
namespace {

// the hierarchy's lock work space: made at the first use
int amg_lock(sgpu_amg *h, AmgLock **out) {
    if (!h->lock) {
        std::unique_ptr<AmgLock> Lk(new AmgLock());
        HIPCHK(alloc_vec(Lk->part, (size_t)(sk::LOCK_MAX / sk::LOCK_C) * g.n_partials * sk::LOCK_C * 8));
        HIPCHK(alloc_vec(Lk->coef, (size_t)sk::LOCK_MAX * 8));
        h->lock = std::move(Lk);
    }
    *out = h->lock.get();
    return SGPU_OK;
}

using LockGramFn = void (*)(const double *, size_t, const double *, size_t, double *);
LockGramFn lock_gram_fn(int K, int nc) {
    return per_K(K, [&](auto k) { return among<1, 2, 3, 4, 5, 6, 7, 8>(nc, [](auto c) -> LockGramFn { return sk::k_lock_gram_partial<decltype(k)::value, c()>; }); });
}
static_assert(sk::LOCK_C == 8, "the list above names 1 .. 8 locked columns a pass");

// out[l * K + b] (device) = Z[:, l] . Y[:, b], l < L: ceil(L / 8) passes into slots of their own, one reduce
int lock_gram(AmgLock &Lk, const double *Z, size_t ld, int L, const double *Y, size_t n, int K, double *out) {
    if (L <= 0) return SGPU_OK;
    const int nb = dot_nblocks(n);
    const size_t slot = (size_t)g.n_partials * sk::LOCK_C * K;
    for (int l = 0, pass = 0; l < L; l += sk::LOCK_C, ++pass) {
        const int nc = std::min(sk::LOCK_C, L - l);
        SGPU_LAUNCH_COLS("k_lock_gram_partial", K, lock_gram_fn(K, nc), dim3(nb), dim3(sk::BLOCK), 0, g.cs, Z + (size_t)l * ld, ld, Y, n, Lk.part + (size_t)pass * slot);
    }
    SGPU_LAUNCH(sk::k_gram_reduce, dim3(L * K), dim3(sk::BLOCK), 0, g.cs, (const double *)Lk.part, nb, sk::LOCK_C * K, slot, out);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// W <- W - Q C, C (L x K, row-major) in device memory
int lock_project(const double *Q, size_t ld, const double *C, int L, double *W, size_t n, int K) {
    if (!n || L <= 0) return SGPU_OK;
    const int gd = (int)std::min<size_t>(2048, (n + sk::BLOCK - 1) / sk::BLOCK);
    SGPU_LAUNCH_COLS("k_lock_project", K, per_K(K, [](auto k) { return sk::k_lock_project<k()>; }), dim3(gd), dim3(sk::BLOCK), 0, g.cs, Q, ld, C, L, W, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

int eig_lock_project(sgpu_amg *h, const EigLock &lk, double *V, size_t n, int K) {
    if (lk.L <= 0) return SGPU_OK;
    AmgLock *Lk = nullptr;
    CHK(amg_lock(h, &Lk));
    CHK(lock_gram(*Lk, lk.Z, lk.ld, lk.L, V, n, K, Lk->coef));
    return lock_project(lk.Q, lk.ld, Lk->coef, lk.L, V, n, K);
}

int grid_rows(size_t n) { return (int)std::min<size_t>(2048, std::max<size_t>(1, (n + sk::BLOCK - 1) / sk::BLOCK)); }

int block_refill(double *X, size_t n, int K, int col, uint32_t counter) {
    if (!n) return SGPU_OK;
    SGPU_LAUNCH(sk::k_block_refill, dim3(grid_rows(n)), dim3(sk::BLOCK), 0, g.cs, X, n, K, col, counter);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

int block_col_get(const double *X, size_t n, int K, int col, double *dst) {
    if (!n) return SGPU_OK;
    SGPU_LAUNCH(sk::k_block_col_get, dim3(grid_rows(n)), dim3(sk::BLOCK), 0, g.cs, X, n, K, col, dst);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// what both entry points ask of a locked set
int lock_args_check(const char *what, size_t n, int K, const void *Q, const void *BQ, bool gen, size_t ld, int nlocked) {
    if (nlocked < 0 || nlocked > sk::LOCK_MAX) return fail(SGPU_ERR_ARG, "%s: nlocked must be in 0..%d (got %d)", what, sk::LOCK_MAX, nlocked);
    if (ld < n || (ld & 1)) return fail(SGPU_ERR_ARG, "%s: ld must be even and at least the %zu rows (got %zu)", what, n, ld);
    if (nlocked > 0 && !Q) return fail(SGPU_ERR_ARG, "%s: Q is null with %d locked columns", what, nlocked);
    if (nlocked > 0 && gen && !BQ) return fail(SGPU_ERR_ARG, "%s: BQ is null with B given and %d locked columns", what, nlocked);
    if (n < (size_t)nlocked + 3 * (size_t)K)
        return fail(SGPU_ERR_ARG, "%s: the operator has %zu rows; %d locked vectors and the Rayleigh-Ritz basis of 3 K = %d need at least %d", what, n, nlocked, 3 * K, nlocked + 3 * K);
    return SGPU_OK;
}

} // namespace

extern "C" {

// ---- tests (include/saena_gpu_debug.h): the solver's own launch helpers on the caller's arrays ----
int sgpu_debug_lock_gram(sgpu_amg *h, const value_t *Z, size_t ld, int L, const value_t *Y, size_t n, int K, value_t *out_dev) {
    CHK(need_ctx());
    if (!h || !Z || !Y || !out_dev) return fail(SGPU_ERR_ARG, "debug_lock_gram: null argument");
    CHK(block_check(nullptr, K, "debug_lock_gram"));
    if (L < 1 || L > sk::LOCK_MAX || ld < n || (ld & 1)) return fail(SGPU_ERR_ARG, "debug_lock_gram: L is 1..%d, ld even and >= n", sk::LOCK_MAX);
    if (!gs_aligned(Y)) return fail(SGPU_ERR_ARG, "debug_lock_gram: Y must be 16-byte aligned");
    AmgLock *Lk = nullptr;
    CHK(amg_lock(h, &Lk));
    return lock_gram(*Lk, Z, ld, L, Y, n, K, out_dev);
}

int sgpu_debug_lock_project(const value_t *Q, size_t ld, const value_t *C_dev, int L, value_t *W, size_t n, int K) {
    CHK(need_ctx());
    if (!Q || !C_dev || !W) return fail(SGPU_ERR_ARG, "debug_lock_project: null argument");
    CHK(block_check(nullptr, K, "debug_lock_project"));
    if (L < 1 || L > sk::LOCK_MAX || ld < n || (ld & 1)) return fail(SGPU_ERR_ARG, "debug_lock_project: L is 1..%d, ld even and >= n", sk::LOCK_MAX);
    if (!gs_aligned(W)) return fail(SGPU_ERR_ARG, "debug_lock_project: W must be 16-byte aligned");
    return lock_project(Q, ld, C_dev, L, W, n, K);
}

int sgpu_debug_block_refill(value_t *X, size_t n, int K, int col, unsigned counter) {
    CHK(need_ctx());
    if (!X) return fail(SGPU_ERR_ARG, "debug_block_refill: null argument");
    CHK(block_check(nullptr, K, "debug_block_refill"));
    if (col < 0 || col >= K) return fail(SGPU_ERR_ARG, "debug_block_refill: col must be in 0..K-1 (got %d)", col);
    return block_refill(X, n, K, col, counter);
}

// measurement (tests/perf_eig_many.py): ms per run of `reps` back-to-back runs; kind 0: the lock Gram (passes and reduce), 1: the
// projection (coefficients zeroed first: W stays what it is)
int sgpu_debug_time_lock(sgpu_amg *h, int kind, const value_t *Q, size_t ld, int L, value_t *Y, size_t n, int K, int reps, float *ms) {
    CHK(need_ctx());
    if (!h || !Q || !Y || !ms || reps < 1 || (kind != 0 && kind != 1)) return fail(SGPU_ERR_ARG, "debug_time_lock: bad argument");
    CHK(block_check(nullptr, K, "debug_time_lock"));
    if (L < 1 || L > sk::LOCK_MAX || ld < n || (ld & 1) || !gs_aligned(Y)) return fail(SGPU_ERR_ARG, "debug_time_lock: bad argument");
    AmgLock *Lk = nullptr;
    CHK(amg_lock(h, &Lk));
    CHK(sgpu_vec_fill(Lk->coef, 0.0, (size_t)sk::LOCK_MAX * 8));
    auto once = [&]() -> int { return kind == 0 ? lock_gram(*Lk, Q, ld, L, Y, n, K, Lk->coef) : lock_project(Q, ld, Lk->coef, L, Y, n, K); };
    CHK(once());
    if (kind == 0) CHK(sgpu_vec_fill(Lk->coef, 0.0, (size_t)sk::LOCK_MAX * 8));
    return time_reps(reps, ms, once);
}

int sgpu_eigs_LOBPCG_locked(sgpu_amg *h, sgpu_op *B, const value_t *Q, const value_t *BQ, size_t ld, int nlocked, value_t *X, int K, int nev,
                            int max_iter, value_t tol, int precond, value_t *lambda, value_t *res, int *iters, value_t *res_hist, int hist_cap,
                            int *leading) {
    if (leading) *leading = 0;
    CHK(need_ctx());
    if (!h || !X || !lambda) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_locked: null argument");
    CHK(lobpcg_check(h, K, "eigs_LOBPCG_locked"));
    CHK(lock_args_check("eigs_LOBPCG_locked", (size_t)h->A[0]->M, K, Q, BQ, B != nullptr, ld, nlocked));
    const EigLock lk{Q, B ? BQ : Q, ld, nlocked};
    return lobpcg_run(h, B, X, K, nev, max_iter, tol, precond, lambda, res, iters, res_hist, hist_cap, &lk, leading);
}

int sgpu_eigs_LOBPCG_many(sgpu_amg *h, sgpu_op *B, value_t *Q, size_t ld, int nev, int K, int sweep_nev, const value_t *X0, int max_iter,
                          value_t tol, int precond, value_t *lambda, value_t *res, int *iters, int *nlocked_out, int *sweeps_out) {
    if (iters) *iters = 0;
    if (nlocked_out) *nlocked_out = 0;
    if (sweeps_out) *sweeps_out = 0;
    CHK(need_ctx());
    if (!h || !Q || !lambda) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_many: null argument");
    if (h->null_space == 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_many: the hierarchy knows the constant null space, so lambda = 0 is in the spectrum and the unconstrained solve breaks down; lock the normalised constant vector and call sgpu_eigs_LOBPCG_locked");
    CHK(lobpcg_check(h, K, "eigs_LOBPCG_many"));
    if (nev < 1 || nev > eig_lock::MAX_LOCKED) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_many: nev must be in 1..%d (got %d)", eig_lock::MAX_LOCKED, nev);
    if (sweep_nev < 0 || sweep_nev > K) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_many: sweep_nev must be in 1..K, or 0 for the default K / 2 (sweep_nev = %d, K = %d)", sweep_nev, K);
    if (precond != 0 && precond != 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_many: precond is 0 (none) or 1 (one V-cycle), got %d", precond);
    if (max_iter < 0 || !(tol >= 0.0)) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_many: max_iter and tol must not be negative");
    const size_t n = (size_t)h->A[0]->M;
    CHK(lock_args_check("eigs_LOBPCG_many", n, K, Q, Q, false, ld, nev));      // (the last sweep runs with up to nev - 1 locked; nev is the simpler promise)
    if (X0 && !gs_aligned(X0)) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_many: X0 must be 16-byte aligned");
    if (!sweep_nev) sweep_nev = eig_lock::default_sweep_nev(K);
    AmgLock *Lk = nullptr;
    CHK(amg_lock(h, &Lk));
    // the driver's own arrays, freed at return: the block, B Q, and the copy the final permutation reads
    DevArr<double> X, BQ, tmp;
    HIPCHK(alloc_vec(X, n * K));
    if (B) HIPCHK(alloc_vec(BQ, (size_t)nev * ld));
    uint32_t counter = 0;
    if (X0) CHK(sgpu_vec_copy(X, X0, n * K));
    else for (const eig_lock::Refill &r : eig_lock::refill_plan(K, &counter)) CHK(block_refill(X, n, K, r.col, r.counter));
    std::vector<double> lam((size_t)nev), rs((size_t)nev);
    int L = 0, total = 0, sweeps = 0, status = SGPU_OK;
    while (L < nev) {
        const int want = eig_lock::sweep_want(nev, L, sweep_nev);
        double bl[8], br[8];
        int it = 0, lead = 0;
        const EigLock lk{Q, B ? BQ.get() : Q, ld, L};
        const int st = lobpcg_run(h, B, X, K, want, max_iter - total, tol, precond, bl, br, &it, nullptr, 0, &lk, &lead);
        total += it;
        ++sweeps;
        if (st != SGPU_OK && st != SGPU_ERR_NOCONV) { status = st; break; }
        const int take = eig_lock::sweep_take(K, nev, L, lead);      // every leading column the recomputed norms confirm
        for (int j = 0; j < take; ++j) {
            CHK(block_col_get(X, n, K, j, Q + (size_t)(L + j) * ld));
            if (B) CHK(block_col_get(h->eigs[block_slot(K)]->BX, n, K, j, BQ + (size_t)(L + j) * ld));   // B X as the solve recomputed it
            lam[(size_t)(L + j)] = bl[j];
            rs[(size_t)(L + j)] = br[j];
        }
        L += take;
        if (st != SGPU_OK) { status = st; break; }
        if (!take) { status = fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_many: sweep %d locked no column", sweeps); break; }   // (a converged sweep leads with `want` columns)
        if (L < nev)
            for (const eig_lock::Refill &r : eig_lock::refill_plan(take, &counter)) CHK(block_refill(X, n, K, r.col, r.counter));
    }
    // ascending lambda: a stable sort on the host, the columns of Q permuted on the device
    const std::vector<int> perm = eig_lock::final_order(L, lam.data());
    bool moved = false;
    for (int k = 0; k < L; ++k) moved = moved || perm[(size_t)k] != k;
    if (moved) {
        HIPCHK(alloc_vec(tmp, (size_t)L * ld));
        for (int k = 0; k < L; ++k) CHK(sgpu_vec_copy(tmp + (size_t)k * ld, Q + (size_t)k * ld, n));     // (the padding rows are the caller's)
        for (int k = 0; k < L; ++k)
            if (perm[(size_t)k] != k) CHK(sgpu_vec_copy(Q + (size_t)k * ld, tmp + (size_t)perm[(size_t)k] * ld, n));
    }
    HIPCHK(hipStreamSynchronize(g.cs));
    for (int k = 0; k < L; ++k) {
        lambda[k] = lam[(size_t)perm[(size_t)k]];
        if (res) res[k] = rs[(size_t)perm[(size_t)k]];
    }
    if (iters) *iters = total;
    if (nlocked_out) *nlocked_out = L;
    if (sweeps_out) *sweeps_out = sweeps;
    return status;
}

} // extern "C"
