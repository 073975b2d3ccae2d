// sgpu_geig.hip.inc -- sgpu_eigs_LOBPCG_gen (include/saena_gpu.h): the nev smallest eigenpairs of A x = lambda B x, A the SPD level-0
// operator of a hierarchy, B a second SPD operator of the same size (a mass matrix, consistent or lumped).  Part of sgpu_runtime.hip,
// after sgpu_eig.hip.inc, whose helpers, state and captured V-cycle it shares; the kernel it adds: k_geig_residual (kernels_eig.hip.h).
//
// The steps are sgpu_eigs_LOBPCG's with every Euclidean inner product replaced by the B-inner product, and three more carried block
// vectors BX, BW, BP (DESIGN.md section 17).  The standard solve is not touched: the extra state (the three vectors, the partial sums
// and the K sums of ||(Bx)_j||^2) is made at the first generalised call with a given K, and a process that never makes one allocates
// what it allocated before.
//
// Two rules about B: it is applied by eager launches only (apply_block; it never enters a captured graph -- the V-cycle's graph is
// the standard solve's, neither dropped nor recaptured here), and nothing keeps a pointer to it after the call returns.
//
// Host synchronisations: THREE per iteration, as in the standard solve --
//   1. ||r_j||^2 and ||(Bx)_j||^2 of the carried residual together with (BX)^T W (2 K + K^2 doubles),
//   2. W^T BW and P^T BP after the projection (2 K^2),
//   3. S^T BS and S^T AS, S = [X, W, P]: the upper block triangle of both (12 K^2),
// plus two at the start (X^T BX, X^T AX) and one per recomputed residual at the end of the solve.
namespace {

// R = AX - BX diag(lambda), out_r[j] = ||r_j||^2, out_b[j] = ||(Bx)_j||^2 (device); rpart / bpart: n_partials * K doubles each
int geig_residual(int K, const double *AX, const double *BX, const double *lambda, double *R, size_t n, double *rpart, double *bpart,
                  double *out_r, double *out_b) {
    const int nb = dot_nblocks(n);
    if (K == 2) SGPU_LAUNCH(sk::k_geig_residual<2>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, BX, lambda, R, n, rpart, bpart);
    else if (K == 4) SGPU_LAUNCH(sk::k_geig_residual<4>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, BX, lambda, R, n, rpart, bpart);
    else SGPU_LAUNCH(sk::k_geig_residual<8>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, BX, lambda, R, n, rpart, bpart);
    SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)rpart, nb, K, out_r, (1u << K) - 1u);
    SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)bpart, nb, K, out_b, (1u << K) - 1u);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// the part of the work space only the generalised solve uses: made at its first call with this K
int amg_geig(sgpu_amg *h, int K, AmgEig **out) {
    CHK(amg_eig(h, K, out));
    AmgEig &E = **out;
    if (!E.gen) {                              // (an array a failed earlier attempt left is kept: alloc refuses an owner that holds one)
        const size_t nK = (size_t)h->A[0]->M * K;
        for (DevArr<double> *p : {&E.BX, &E.BW, &E.BP})
            if (!*p) HIPCHK(alloc_vec(*p, nK));
        if (!E.bpart) HIPCHK(alloc_vec(E.bpart, (size_t)g.n_partials * K));
        if (!E.bnrm) HIPCHK(alloc_vec(E.bnrm, (size_t)K));
        if (!E.hbn) HIPCHK(E.hbn.alloc(K));
        E.gen = true;
    }
    return SGPU_OK;
}

} // namespace

extern "C" {

// tests (include/saena_gpu_debug.h): the launch helper of the generalised residual on the caller's arrays
int sgpu_debug_geig_residual(sgpu_amg *h, const value_t *AX, const value_t *BX, const value_t *lambda_dev, value_t *R, size_t n, int K,
                             value_t *rr_dev, value_t *bb_dev) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_geig_residual", &E));
    if (!AX || !BX || !lambda_dev || !R || !rr_dev || !bb_dev) return fail(SGPU_ERR_ARG, "debug_geig_residual: null argument");
    if (!gs_aligned(AX) || !gs_aligned(BX) || !gs_aligned(R)) return fail(SGPU_ERR_ARG, "debug_geig_residual: block vectors must be 16-byte aligned");
    CHK(amg_geig(h, K, &E));
    return geig_residual(K, AX, BX, lambda_dev, R, n, E->rpart, E->bpart, rr_dev, bb_dev);
}

// measurement (tests/perf_geig.py): ms per run of `reps` back-to-back runs of the generalised residual with both reductions
int sgpu_debug_time_geig(sgpu_amg *h, const value_t *AX, const value_t *BX, value_t *R, size_t n, int K, int reps, float *ms) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_time_geig", &E));
    if (!AX || !BX || !R || !ms || reps < 1) return fail(SGPU_ERR_ARG, "debug_time_geig: bad argument");
    if (!gs_aligned(AX) || !gs_aligned(BX) || !gs_aligned(R)) return fail(SGPU_ERR_ARG, "debug_time_geig: block vectors must be 16-byte aligned");
    CHK(amg_geig(h, K, &E));
    CHK(sgpu_vec_fill(E->coef, 0.0, 15 * (size_t)K * K + 2 * K));
    CHK(block_timer_events());
    const double *lam = E->coef + 3 * K * K;
    double *nrm = E->coef + 3 * K * K + K;
    CHK(geig_residual(K, AX, BX, lam, R, n, E->rpart, E->bpart, nrm, E->bnrm));
    HIPCHK(hipEventRecord(g_bt0, g.cs));
    for (int i = 0; i < reps; ++i) CHK(geig_residual(K, AX, BX, lam, R, n, E->rpart, E->bpart, nrm, E->bnrm));
    HIPCHK(hipEventRecord(g_bt1, g.cs));
    HIPCHK(hipEventSynchronize(g_bt1));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, g_bt0, g_bt1));
    *ms = t / reps;
    return SGPU_OK;
}

// sgpu_eigs_LOBPCG_gen's loop, and with a locked set (Z = B Q) sgpu_eigs_LOBPCG_locked's: see eig_lobpcg_run
static int geig_lobpcg_run(sgpu_amg *h, sgpu_op *B, value_t *X, int K, int nev, int max_iter, value_t tol, int precond, value_t *lambda,
                           value_t *res, int *iters, value_t *res_hist, int hist_cap, const EigLock *lk, int *leading) {
    if (leading) *leading = 0;
    CHK(need_ctx());
    if (!h || !X || !lambda) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: null argument");
    if (!B) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: B is null (sgpu_eigs_LOBPCG solves the standard problem)");
    CHK(lobpcg_check(h, K, "eigs_LOBPCG_gen"));
    if (nev < 1 || nev > K) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: nev must be in 1..K (nev = %d, K = %d)", nev, K);
    if (precond != 0 && precond != 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: precond is 0 (none) or 1 (one V-cycle), got %d", precond);
    if (max_iter < 0 || !(tol >= 0.0)) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: max_iter and tol must not be negative");
    sgpu_op *A = h->A[0];
    const size_t n = (size_t)A->M, nK = n * K;
    if (B->M != A->M || B->N_local != A->N_local)
        return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: B is %d x %d, the level-0 operator %d x %d: both must have the same size", (int)B->M, (int)B->N_local, (int)A->M, (int)A->N_local);
    if (B->has_remote || B->recvSize || B->vIndexSize)
        return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: B has a remote part or a halo plan (%d halo entries, %d sent); it takes single-rank operators only", B->recvSize, B->vIndexSize);
    if (n < 3 * (size_t)K) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: the operator has %zu rows; the Rayleigh-Ritz basis of 3 K = %d vectors needs at least as many", n, 3 * K);
    if (!gs_aligned(X)) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: X must be 16-byte aligned");
    AmgBlock *Bp = nullptr;
    AmgEig *Ep = nullptr;
    CHK(amg_block(h, K, &Bp));
    CHK(amg_geig(h, K, &Ep));
    AmgEig &E = *Ep;
    const int KK = K * K;
    double *cmix = E.coef, *clam = E.coef + 3 * KK, *cnrm = clam + K, *cgram = cnrm + K;
    double *hnrm = E.hdown, *hgram = E.hdown + K, *hbn = E.hbn;      // the mirrors of cnrm | cgram, and of bnrm
    auto fetch = [&](int ndoubles, bool with_bn = false) -> int {   // the first ndoubles of (norms | Gram blocks), and the K ||(Bx)_j||^2
        HIPCHK(hipMemcpyAsync(E.hdown, cnrm, (size_t)ndoubles * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        if (with_bn) HIPCHK(hipMemcpyAsync(E.hbn, E.bnrm, (size_t)K * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        return SGPU_OK;
    };
    auto send_mix = [&](int nmat) -> int {
        HIPCHK(hipMemcpyAsync(cmix, E.hmix, (size_t)nmat * KK * sizeof(double), hipMemcpyHostToDevice, g.cs));
        return SGPU_OK;
    };
    auto send_lambda = [&](const double *lam) -> int {
        std::copy(lam, lam + K, E.hlam.get());
        HIPCHK(hipMemcpyAsync(clam, E.hlam, (size_t)K * sizeof(double), hipMemcpyHostToDevice, g.cs));
        return SGPU_OK;
    };
    auto mix1 = [&](double *V, const double *c) -> int { return eig_mix(K, 1, V, c, V, c, V, c, nullptr, V, n); };   // V <- V C
    auto apply_B = [&](const double *V, double *BV) -> int { return apply_block(B, sk::EPI_SPMV, V, BV, EpiArgs(), K); };   // eager, always
    if (iters) *iters = 0;
    std::vector<int> all((size_t)K);
    for (int j = 0; j < K; ++j) all[(size_t)j] = j;

    const bool locked = lk && lk->L > 0;
    if (locked) for (int pass = 0; pass < 2; ++pass) CHK(eig_lock_project(h, *lk, X, n, K));     // X <- X - Q ((B Q)^T X), twice
    // ---- start: B-orthonormalise X, Rayleigh-Ritz on X alone (X^T B X = I: the standard dense problem) ----
    CHK(apply_B(X, E.BX));
    CHK(eig_gram_partial(E, X, E.BX, n, 0));
    CHK(eig_gram_reduce(E, n, 1, cgram));
    CHK(fetch(K + KK));
    if (!eig_ortho_factor(hgram, K, all, E.hmix))
        return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: X^T B X is not numerically positive definite: the start vectors are linearly dependent, or B is not positive definite");
    CHK(send_mix(1));
    CHK(mix1(X, cmix));
    CHK(mix1(E.BX, cmix));
    CHK(apply_block(A, sk::EPI_SPMV, X, E.AX, EpiArgs(), K));
    CHK(eig_gram_partial(E, X, E.AX, n, 0));
    CHK(eig_gram_reduce(E, n, 1, cgram));
    CHK(fetch(K + KK));
    double lam[8], theta[24];
    {
        std::vector<double> S((size_t)KK), Q((size_t)KK);
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) S[(size_t)i * K + j] = 0.5 * (hgram[i * K + j] + hgram[j * K + i]);
        if (saena_host::dense_sym_eig(K, S.data(), lam, Q.data()) < 0)
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: the Rayleigh-Ritz problem of the start vectors did not converge (X^T A X is not finite?)");
        if (!(lam[0] > 0.0)) return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: a Ritz value of the start vectors is %g: A is not symmetric positive definite", lam[0]);
        std::copy(Q.begin(), Q.end(), E.hmix.get());
        CHK(send_mix(1));
        CHK(mix1(X, cmix));
        CHK(mix1(E.AX, cmix));
        CHK(mix1(E.BX, cmix));
    }
    for (int j = 0; j < K; ++j) lambda[j] = lam[j];

    bool hasP = false, fresh_AX = false;      // fresh_AX: AX and BX were just recomputed from X, the norms about to be formed are the true ones
    int it = 0;
    for (;;) {
        // ---- the residual of the carried AX and BX, the preconditioned residual and (BX)^T W: host synchronisation 1 ----
        CHK(send_lambda(lam));
        CHK(geig_residual(K, E.AX, E.BX, clam, E.R, n, E.rpart, E.bpart, cnrm, E.bnrm));
        auto precondition_and_project = [&]() -> int {                 // W = M R and (BX)^T W
            if (precond) CHK(eig_precondition(h, *Bp, E)); else CHK(sgpu_vec_copy(E.W, E.R, nK));
            if (locked) CHK(eig_lock_project(h, *lk, E.W, n, K));
            CHK(eig_gram_partial(E, E.BX, E.W, n, 0));
            return eig_gram_reduce(E, n, 1, cgram);
        };
        if (!fresh_AX) CHK(precondition_and_project());
        CHK(fetch(fresh_AX ? K : K + KK, true));
        std::vector<int> act;
        bool conv = true, finite = true;
        for (int j = 0; j < K; ++j) {
            const double rr = hnrm[j], bb = hbn[j];
            if (!std::isfinite(rr) || !std::isfinite(bb)) finite = false;
            if (res_hist && it < hist_cap) res_hist[(size_t)j * hist_cap + it] = std::sqrt(rr);
            if (res) res[j] = std::sqrt(rr);
            const bool cj = rr < tol * tol * lam[j] * lam[j] * bb;     // ||A x - lambda B x|| < tol lambda ||B x||
            if (!cj) { act.push_back(j); if (j < nev) conv = false; }
        }
        if (iters) *iters = it;
        if (!finite) return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: a residual norm or ||B x_j|| is not finite at iteration %d", it);
        if (conv || it >= max_iter) {
            if (fresh_AX) {                    // these norms come from a recomputed AX and BX: they decide
                if (leading) *leading = act.empty() ? K : act[0];
                if (conv) return SGPU_OK;
                return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: %d of the %d wanted pairs are above the tolerance after %d iterations", (int)std::count_if(act.begin(), act.end(), [&](int j) { return j < nev; }), nev, it);
            }
            CHK(apply_block(A, sk::EPI_SPMV, X, E.AX, EpiArgs(), K));      // end of the solve: only recomputed norms declare convergence
            CHK(apply_B(X, E.BX));
            fresh_AX = true;
            continue;                          // (the same iteration again, on the recomputed AX and BX)
        }
        if (fresh_AX) {                        // the recomputed norms contradict the carried ones and iterations remain: go on from them
            CHK(precondition_and_project());
            CHK(fetch(K + KK));
            fresh_AX = false;
        }
        const int na = (int)act.size();
        // ---- W -= X ((BX)^T W); BW = B W; W^T BW and P^T BP: host synchronisation 2 ----
        std::fill(E.hmix.get(), E.hmix + KK, 0.0);
        for (int a = 0; a < K; ++a)
            for (int j : act) E.hmix[a * K + j] = -hgram[a * K + j];
        CHK(send_mix(1));
        CHK(eig_mix(K, 1, X, cmix, X, cmix, X, cmix, E.W, E.W, n));
        CHK(apply_B(E.W, E.BW));
        CHK(eig_gram_partial(E, E.W, E.BW, n, 0));
        if (hasP) CHK(eig_gram_partial(E, E.P, E.BP, n, 1));
        CHK(eig_gram_reduce(E, n, hasP ? 2 : 1, cgram));
        CHK(fetch(K + (hasP ? 2 : 1) * KK));
        if (!eig_ortho_factor(hgram, K, act, E.hmix))
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: breakdown at iteration %d: W^T B W of the %d active columns is not numerically positive definite (the preconditioned residuals are linearly dependent, or B is not positive definite)", it + 1, na);
        bool useP = hasP;
        if (useP && !eig_ortho_factor(hgram + KK, K, act, E.hmix + KK)) useP = false;      // a restart: this iteration runs without P
        CHK(send_mix(useP ? 2 : 1));
        CHK(mix1(E.W, cmix));                                                               // inactive columns of W and BW become zero
        CHK(mix1(E.BW, cmix));
        CHK(apply_block(A, sk::EPI_SPMV, E.W, E.AW, EpiArgs(), K));
        if (useP) {
            CHK(mix1(E.P, cmix + KK));
            CHK(mix1(E.AP, cmix + KK));
            CHK(mix1(E.BP, cmix + KK));
        }
        if (E.debug_stop == it) {              // tests (sgpu_debug_eig_stop): W, AW, BW, P, AP, BP stay as the orthonormalisation left them
            E.debug_stop = -1;
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: stopped for inspection after the orthonormalisation of iteration %d (%s P)", it + 1, useP ? "with" : "without");
        }
        // ---- the Gram matrices of S = [X, W, P] with BS and AS: host synchronisation 3 ----
        const double *Sv[3] = {X, E.W, E.P}, *ASv[3] = {E.AX, E.AW, E.AP}, *BSv[3] = {E.BX, E.BW, E.BP};
        const int nb3 = useP ? 3 : 2;
        int slotS[3][3], slotA[3][3], ns3 = 0;
        for (int a = 0; a < nb3; ++a)
            for (int b = a; b < nb3; ++b) { slotS[a][b] = ns3; CHK(eig_gram_partial(E, Sv[a], BSv[b], n, ns3++)); }
        for (int a = 0; a < nb3; ++a)
            for (int b = a; b < nb3; ++b) { slotA[a][b] = ns3; CHK(eig_gram_partial(E, Sv[a], ASv[b], n, ns3++)); }
        CHK(eig_gram_reduce(E, n, ns3, cgram));
        CHK(fetch(K + ns3 * KK));
        int m = 0;
        const int st = eig_rayleigh_ritz(E, hgram, slotS, slotA, nb3, act, theta, &m);
        if (st < 0)
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: breakdown at iteration %d: the Rayleigh-Ritz basis of %d vectors is %s", it + 1, m,
                        st == -1 ? "linearly dependent, or B is not positive definite (S^T B S is not numerically positive definite)" : "not finite");
        if (!(theta[0] > 0.0)) return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG_gen: a Ritz value is %g at iteration %d: A is not symmetric positive definite", theta[0], it + 1);
        // E.hmix holds C_X | C_W | C_P: the K smallest Ritz vectors; rows of inactive columns are zero
        CHK(send_mix(3));
        const double *Wv[3] = {E.W, E.AW, E.BW}, *Xv[3] = {X, E.AX, E.BX};
        double *Pv[3] = {E.P, E.AP, E.BP}, *Xo[3] = {X, E.AX, E.BX};
        for (int v = 0; v < 3; ++v) {          // P, AP, BP
            if (useP) CHK(eig_mix(K, 2, Wv[v], cmix + KK, Pv[v], cmix + 2 * KK, Pv[v], cmix, nullptr, Pv[v], n));
            else CHK(eig_mix(K, 1, Wv[v], cmix + KK, Wv[v], cmix, Wv[v], cmix, nullptr, Pv[v], n));
        }
        for (int v = 0; v < 3; ++v) CHK(eig_mix(K, 1, Xv[v], cmix, Xv[v], cmix, Xv[v], cmix, Pv[v], Xo[v], n));   // X, AX, BX
        for (int j = 0; j < K; ++j) { lam[j] = theta[j]; lambda[j] = theta[j]; }
        hasP = true;
        ++it;
    }
}

int sgpu_eigs_LOBPCG_gen(sgpu_amg *h, sgpu_op *B, value_t *X, int K, int nev, int max_iter, value_t tol, int precond, value_t *lambda,
                         value_t *res, int *iters, value_t *res_hist, int hist_cap) {
    if (h && h->null_space == 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: the hierarchy knows the constant null space, so lambda = 0 is in the spectrum and the unconstrained solve breaks down; lock the normalised constant vector and call sgpu_eigs_LOBPCG_locked");
    return geig_lobpcg_run(h, B, X, K, nev, max_iter, tol, precond, lambda, res, iters, res_hist, hist_cap, nullptr, nullptr);
}

} // extern "C"
