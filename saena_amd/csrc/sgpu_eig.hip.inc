// sgpu_eig.hip.inc -- sgpu_eigs_LOBPCG (include/saena_gpu.h): the nev smallest eigenpairs of the SPD level-0 operator by LOBPCG on a
// block of K vectors, one block V-cycle from a zero iterate as preconditioner.  Part of sgpu_runtime.hip (it shares that file's
// context, handles and helpers); kernels: kernels_eig.hip.h; the small dense problems: host/dense_eig.cpp.
//
// Nothing here touches the scalar path, sgpu_solve_pCG_block's vectors or the block cache of eight captured V-cycles.  The state is
// an AmgEig per (hierarchy, K) (sgpu_runtime.hip): six block vectors (AX, R, W, AW, P, AP; X is the caller's), ONE fixed (R, W) pair
// the V-cycle preconditions through (captured once into a graph of its own and replayed by every iteration of every solve), the
// partial sums, the device coefficients and their pinned mirrors.  The V-cycle's work vectors are the AmgBlock's.
//
// Host synchronisations: THREE per iteration --
//   1. ||r_j||^2 of the carried residual together with X^T W (K + K^2 doubles),
//   2. W^T W and P^T P after the projection (2 K^2),
//   3. S^T S and S^T A S, S = [X, W, P]: the upper block triangle of both, diagonal blocks in full (12 K^2 doubles; the host mirrors
//      the rest, takes the rows and columns of the active set and symmetrises),
// plus two at the start (X^T X, X^T A X) and one per recomputed residual at the end of the solve (its K norms alone: no V-cycle
// runs for a residual that only confirms convergence).
namespace {

// the locked set of a constrained solve (sgpu_eig_lock.hip.inc): L columns, column l at Q + l * ld; Z = Q for the standard problem,
// B Q for the generalised one.  A null pointer or L = 0: no constraint, and neither lock kernel is launched
struct EigLock { const double *Q, *Z; size_t ld; int L; };
// V <- V - Q (Z^T V) on a block vector of n rows and K columns: the coefficients stay on the device, no host synchronisation
int eig_lock_project(sgpu_amg *h, const EigLock &lk, double *V, size_t n, int K);

// partial sums of G = X^T Y into Gram slot `slot`
int eig_gram_partial(AmgEig &E, const double *X, const double *Y, size_t n, int slot) {
    const int nb = dot_nblocks(n), K = E.K;
    double *part = E.gpart + (size_t)slot * g.n_partials * K * K;
    if (K == 2) SGPU_LAUNCH(sk::k_gram_block_partial<2>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, X, Y, n, part);
    else if (K == 4) SGPU_LAUNCH(sk::k_gram_block_partial<4>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, X, Y, n, part);
    else SGPU_LAUNCH(sk::k_gram_block_partial<8>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, X, Y, n, part);
    return SGPU_OK;
}
// out[slot * K^2 + a * K + b] for the first nslots slots: one workgroup per entry
int eig_gram_reduce(AmgEig &E, size_t n, int nslots, double *out) {
    const int K = E.K;
    SGPU_LAUNCH(sk::k_gram_reduce, dim3(nslots * K * K), dim3(sk::BLOCK), 0, g.cs, (const double *)E.gpart, dot_nblocks(n), K * K,
                (size_t)g.n_partials * K * K, out);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

using MixFn = void (*)(const double *, const double *, const double *, const double *, const double *, const double *, const double *, double *, size_t);
template <int K>
MixFn eig_mix_fn(int ns) { return ns == 1 ? sk::k_block_mix<K, 1> : ns == 2 ? sk::k_block_mix<K, 2> : sk::k_block_mix<K, 3>; }

// out = sum_{s < ns} S_s C_s (+ add): C_s device, K x K row-major; out may alias any source and add
int eig_mix(int K, int ns, const double *s0, const double *c0, const double *s1, const double *c1, const double *s2, const double *c2,
            const double *add, double *out, size_t n) {
    if (!n) return SGPU_OK;
    const MixFn fn = K == 2 ? eig_mix_fn<2>(ns) : K == 4 ? eig_mix_fn<4>(ns) : eig_mix_fn<8>(ns);
    const int gd = (int)std::min<size_t>(2048, (n + sk::BLOCK - 1) / sk::BLOCK);
    SGPU_LAUNCH(fn, dim3(gd), dim3(sk::BLOCK), 0, g.cs, s0, c0, s1, c1, s2, c2, add, out, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// R = AX - X diag(lambda), out[j] = ||r_j||^2 (device)
int eig_residual(AmgEig &E, const double *AX, const double *X, const double *lambda, double *R, size_t n, double *out) {
    const int nb = dot_nblocks(n), K = E.K;
    if (K == 2) SGPU_LAUNCH(sk::k_eig_residual<2>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, X, lambda, R, n, E.rpart);
    else if (K == 4) SGPU_LAUNCH(sk::k_eig_residual<4>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, X, lambda, R, n, E.rpart);
    else SGPU_LAUNCH(sk::k_eig_residual<8>, dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, X, lambda, R, n, E.rpart);
    SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)E.rpart, nb, K, out, (1u << K) - 1u);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// the hierarchy's LOBPCG work space for K columns: made at the first call
int amg_eig(sgpu_amg *h, int K, AmgEig **out) {
    const int slot = block_slot(K);
    if (!h->eigs[slot]) {
        std::unique_ptr<AmgEig> E(new AmgEig());
        E->K = K;
        const size_t nK = (size_t)h->A[0]->M * K, KK = (size_t)K * K;
        for (DevArr<double> *p : {&E->AX, &E->R, &E->W, &E->AW, &E->P, &E->AP}) HIPCHK(alloc_vec(*p, nK));
        HIPCHK(alloc_vec(E->gpart, 12 * (size_t)g.n_partials * KK));
        HIPCHK(alloc_vec(E->rpart, (size_t)g.n_partials * K));
        HIPCHK(alloc_vec(E->coef, 15 * KK + 2 * K));
        HIPCHK(E->hmix.alloc(3 * KK));
        HIPCHK(E->hlam.alloc(K));
        HIPCHK(E->hdown.alloc(12 * KK + K));
        h->eigs[slot] = std::move(E);
    }
    *out = h->eigs[slot].get();
    return SGPU_OK;
}

// W = one block V-cycle on R from a zero iterate: vcycle_block0's capture and replay on the fixed pair, in a graph the block cache
// never sees
int eig_precondition(sgpu_amg *h, AmgBlock &B, AmgEig &E) {
    if (!h->prm.use_graph) return vcycle_block_eager(h, B, E.W, E.R, true);
    if (E.exec && (E.graph_gen != g_plan_generation || E.block_gen != g_block_generation)) {   // an operator was retuned since the capture
        HIPCHK(hipStreamSynchronize(g.cs));
        E.drop_graph();
    }
    if (!E.exec) {
        HIPCHK(hipStreamBeginCapture(g.cs, hipStreamCaptureModeThreadLocal));
        const int st = vcycle_block_eager(h, B, E.W, E.R, true);
        const hipError_t e = hipStreamEndCapture(g.cs, &E.graph);
        if (st != SGPU_OK) { E.drop_graph(); return st; }
        if (e != hipSuccess) return fail(SGPU_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        HIPCHK(hipGraphInstantiate(&E.exec, E.graph, nullptr, nullptr, 0));
        E.graph_gen = g_plan_generation; E.block_gen = g_block_generation;
    }
    ++g_launches; HIPCHK(hipGraphLaunch(E.exec, g.cs));
    return SGPU_OK;
}

// LOBPCG stays on one rank: its Gram blocks and norms are not summed over the ranks.  No communicator, no host transport, no
// operator with a remote part (an injected block halo does not lift this) -- then what every block solve asks of a hierarchy
int lobpcg_check(sgpu_amg *h, int K, const char *what) {
    CHK(block_one_rank_check(nullptr, K, what));
    for (int l = 0; l < h->nlevels; ++l) {
        CHK(block_one_rank_check(h->A[l], K, what));
        if (l < h->nlevels - 1) { CHK(block_one_rank_check(h->P[l], K, what)); CHK(block_one_rank_check(h->R[l], K, what)); }
    }
    return amg_block_check(h, K, what);
}

// what the debug wrappers check: the hierarchy (for its AmgEig) and K
int eig_debug_args(sgpu_amg *h, int K, const char *what, AmgEig **E) {
    CHK(need_ctx());
    if (!h) return fail(SGPU_ERR_ARG, "%s: null hierarchy", what);
    CHK(block_check(nullptr, K, what));
    return amg_eig(h, K, E);
}

// T (K x K, row-major, zero outside the columns of `act`) = L^-T of the Cholesky factor of the act x act part of the Gram block G.
// -> false when that part is not numerically positive definite
bool eig_ortho_factor(const double *G, int K, const std::vector<int> &act, double *T) {
    const int na = (int)act.size();
    std::fill(T, T + (size_t)K * K, 0.0);
    if (!na) return true;
    std::vector<double> S((size_t)na * na), L((size_t)na * na), Ti((size_t)na * na);
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < na; ++j) S[(size_t)i * na + j] = 0.5 * (G[(size_t)act[i] * K + act[j]] + G[(size_t)act[j] * K + act[i]]);
    if (!saena_host::dense_cholesky(na, S.data(), L.data())) return false;
    saena_host::dense_inv_lower_transposed(na, L.data(), Ti.data());
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < na; ++j) T[(size_t)act[i] * K + act[j]] = Ti[(size_t)i * na + j];
    return true;
}

// The Rayleigh-Ritz step on the host, shared by the standard and the generalised solve: from the downloaded Gram blocks (hgram;
// slotS[a][b] / slotA[a][b], a <= b < nb3: the slots of S_a^T (B) S_b and S_a^T A S_b) the two matrices of order m = K + na (nb3 - 1)
// over X and the active columns of W (and P) -- the lower block triangle mirrored, both symmetrised --, the dense generalised problem,
// and the K smallest Ritz vectors scattered into E.hmix as C_X | C_W | C_P (rows of inactive columns zero).
// -> dense_sym_geig's status (< 0: no coefficients were written); theta[0 .. m) ascending
int eig_rayleigh_ritz(AmgEig &E, const double *hgram, const int (&slotS)[3][3], const int (&slotA)[3][3], int nb3, const std::vector<int> &act,
                      double *theta, int *m_out) {
    const int K = E.K, KK = K * K, na = (int)act.size();
    const int m = K + na * (nb3 - 1);
    *m_out = m;
    std::vector<int> blk((size_t)m), col((size_t)m);
    for (int i = 0; i < K; ++i) { blk[(size_t)i] = 0; col[(size_t)i] = i; }
    for (int b = 1; b < nb3; ++b)
        for (int i = 0; i < na; ++i) { blk[(size_t)(K + (b - 1) * na + i)] = b; col[(size_t)(K + (b - 1) * na + i)] = act[(size_t)i]; }
    std::vector<double> GS((size_t)m * m), GA((size_t)m * m), Vm((size_t)m * m);
    auto entry = [&](const int (&slot)[3][3], int i, int j) {
        const int bi = blk[(size_t)i], bj = blk[(size_t)j];
        return bi <= bj ? hgram[slot[bi][bj] * KK + col[(size_t)i] * K + col[(size_t)j]] : hgram[slot[bj][bi] * KK + col[(size_t)j] * K + col[(size_t)i]];
    };
    for (int i = 0; i < m; ++i)
        for (int j = 0; j < m; ++j) {
            GS[(size_t)i * m + j] = 0.5 * (entry(slotS, i, j) + entry(slotS, j, i));
            GA[(size_t)i * m + j] = 0.5 * (entry(slotA, i, j) + entry(slotA, j, i));
        }
    const int st = saena_host::dense_sym_geig(m, GA.data(), GS.data(), theta, Vm.data());
    if (st < 0) return st;
    std::fill(E.hmix.get(), E.hmix + 3 * KK, 0.0);
    for (int i = 0; i < m; ++i)
        for (int b = 0; b < K; ++b) E.hmix[blk[(size_t)i] * KK + col[(size_t)i] * K + b] = Vm[(size_t)i * m + b];
    return st;
}

} // namespace

extern "C" {

// ---- tests (include/saena_gpu_debug.h): the solver's own launch helpers on the caller's arrays ----
int sgpu_debug_block_gram(sgpu_amg *h, const value_t *X, const value_t *Y, size_t n, int K, value_t *out_dev) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_block_gram", &E));
    if (!X || !Y || !out_dev) return fail(SGPU_ERR_ARG, "debug_block_gram: null argument");
    if (!gs_aligned(X) || !gs_aligned(Y)) return fail(SGPU_ERR_ARG, "debug_block_gram: X and Y must be 16-byte aligned");
    CHK(eig_gram_partial(*E, X, Y, n, 0));
    return eig_gram_reduce(*E, n, 1, out_dev);
}

int sgpu_debug_block_mix(int K, int ns, const value_t *S0, const value_t *C0, const value_t *S1, const value_t *C1, const value_t *S2,
                         const value_t *C2, const value_t *Add, value_t *Out, size_t n) {
    CHK(need_ctx());
    CHK(block_check(nullptr, K, "debug_block_mix"));
    if (ns < 1 || ns > 3) return fail(SGPU_ERR_ARG, "debug_block_mix: 1 to 3 sources (got %d)", ns);
    if (!S0 || !C0 || !Out || (ns > 1 && (!S1 || !C1)) || (ns > 2 && (!S2 || !C2))) return fail(SGPU_ERR_ARG, "debug_block_mix: null argument");
    for (const void *p : {(const void *)S0, (const void *)S1, (const void *)S2, (const void *)Add, (const void *)Out})
        if (!gs_aligned(p)) return fail(SGPU_ERR_ARG, "debug_block_mix: block vectors must be 16-byte aligned");
    return eig_mix(K, ns, S0, C0, ns > 1 ? S1 : S0, ns > 1 ? C1 : C0, ns > 2 ? S2 : S0, ns > 2 ? C2 : C0, Add, Out, n);
}

int sgpu_debug_eig_residual(sgpu_amg *h, const value_t *AX, const value_t *X, const value_t *lambda_dev, value_t *R, size_t n, int K, value_t *rr_dev) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_eig_residual", &E));
    if (!AX || !X || !lambda_dev || !R || !rr_dev) return fail(SGPU_ERR_ARG, "debug_eig_residual: null argument");
    if (!gs_aligned(AX) || !gs_aligned(X) || !gs_aligned(R)) return fail(SGPU_ERR_ARG, "debug_eig_residual: block vectors must be 16-byte aligned");
    return eig_residual(*E, AX, X, lambda_dev, R, n, rr_dev);
}

// a copy of one of the solver's own block vectors after a solve (which: 0 AX, 1 R, 2 W, 3 AW, 4 P, 5 AP; after a generalised solve
// also 6 BX, 7 BW, 8 BP) into dst (device, n K doubles)
int sgpu_debug_eig_vector(sgpu_amg *h, int K, int which, value_t *dst) {
    CHK(need_ctx());
    if (!h || !dst) return fail(SGPU_ERR_ARG, "debug_eig_vector: null argument");
    CHK(block_check(nullptr, K, "debug_eig_vector"));
    AmgEig *E = h->eigs[block_slot(K)].get();
    if (!E) return fail(SGPU_ERR_STATE, "debug_eig_vector: no sgpu_eigs_LOBPCG has run on this hierarchy with K = %d", K);
    if (which < 0 || which > 8) return fail(SGPU_ERR_ARG, "debug_eig_vector: which is 0 .. 8 (got %d)", which);
    if (which > 5 && !E->gen) return fail(SGPU_ERR_STATE, "debug_eig_vector: no sgpu_eigs_LOBPCG_gen has run on this hierarchy with K = %d (which = %d is BX, BW or BP)", K, which);
    const double *src[9] = {E->AX, E->R, E->W, E->AW, E->P, E->AP, E->BX, E->BW, E->BP};
    return sgpu_vec_copy(dst, src[which], (size_t)h->A[0]->M * K);
}

// tests: the next solve with this K returns SGPU_ERR_NOCONV right after the orthonormalisation step of iteration index `iteration`
// (0-based), before the Rayleigh-Ritz update, so that sgpu_debug_eig_vector shows W, AW, P and AP as that step left them; -1: never
int sgpu_debug_eig_stop(sgpu_amg *h, int K, int iteration) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_eig_stop", &E));
    E->debug_stop = iteration;
    return SGPU_OK;
}

// measurement (tests/perf_eig.py): `reps` back-to-back runs of one helper between two events; kind 0: the Gram block of X and Y,
// 1: the mix of ns sources (zero coefficients) into Out, 2: the residual with its norms (X = AX operand, Y = X operand, Out = R)
int sgpu_debug_time_eig(sgpu_amg *h, int kind, int ns, const value_t *X, const value_t *Y, value_t *Out, size_t n, int K, int reps, float *ms) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_time_eig", &E));
    if (!X || !Y || !Out || !ms || reps < 1 || kind < 0 || kind > 2 || ns < 1 || ns > 3) return fail(SGPU_ERR_ARG, "debug_time_eig: bad argument");
    CHK(sgpu_vec_fill(E->coef, 0.0, 15 * (size_t)K * K + 2 * K));
    CHK(block_timer_events());
    const double *c = E->coef, *lam = E->coef + 3 * K * K;
    double *nrm = E->coef + 3 * K * K + K, *gram = nrm + K;
    auto once = [&]() -> int {
        if (kind == 0) { CHK(eig_gram_partial(*E, X, Y, n, 0)); return eig_gram_reduce(*E, n, 1, gram); }
        if (kind == 1) return eig_mix(K, ns, X, c, Y, c + K * K, X, c + 2 * K * K, nullptr, Out, n);
        return eig_residual(*E, X, Y, lam, Out, n, nrm);
    };
    CHK(once());
    HIPCHK(hipEventRecord(g_bt0, g.cs));
    for (int i = 0; i < reps; ++i) CHK(once());
    HIPCHK(hipEventRecord(g_bt1, g.cs));
    HIPCHK(hipEventSynchronize(g_bt1));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, g_bt0, g_bt1));
    *ms = t / reps;
    return SGPU_OK;
}

// sgpu_eigs_LOBPCG's loop, and with a locked set sgpu_eigs_LOBPCG_locked's: X is projected twice before the start orthonormalisation
// and W once right after W = M R.  *leading (may be null): the leading columns converged on recomputed norms
static int eig_lobpcg_run(sgpu_amg *h, value_t *X, int K, int nev, int max_iter, value_t tol, int precond, value_t *lambda, value_t *res, int *iters,
                          value_t *res_hist, int hist_cap, const EigLock *lk, int *leading) {
    if (leading) *leading = 0;
    CHK(need_ctx());
    if (!h || !X || !lambda) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: null argument");
    CHK(lobpcg_check(h, K, "eigs_LOBPCG"));
    if (nev < 1 || nev > K) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: nev must be in 1..K (nev = %d, K = %d)", nev, K);
    if (precond != 0 && precond != 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: precond is 0 (none) or 1 (one V-cycle), got %d", precond);
    if (max_iter < 0 || !(tol >= 0.0)) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: max_iter and tol must not be negative");
    sgpu_op *A = h->A[0];
    const size_t n = (size_t)A->M, nK = n * K;
    if (n < 3 * (size_t)K) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: the operator has %zu rows; the Rayleigh-Ritz basis of 3 K = %d vectors needs at least as many", n, 3 * K);
    if (!gs_aligned(X)) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: X must be 16-byte aligned");
    AmgBlock *Bp = nullptr;
    AmgEig *Ep = nullptr;
    CHK(amg_block(h, K, &Bp));
    CHK(amg_eig(h, K, &Ep));
    AmgEig &E = *Ep;
    const int KK = K * K;
    double *cmix = E.coef, *clam = E.coef + 3 * KK, *cnrm = clam + K, *cgram = cnrm + K;
    double *hnrm = E.hdown, *hgram = E.hdown + K;                  // the mirror of cnrm | cgram
    auto fetch = [&](int ndoubles) -> int {                         // the first ndoubles of (norms | Gram blocks)
        HIPCHK(hipMemcpyAsync(E.hdown, cnrm, (size_t)ndoubles * sizeof(double), hipMemcpyDeviceToHost, g.cs));
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
    if (iters) *iters = 0;
    std::vector<int> all((size_t)K);
    for (int j = 0; j < K; ++j) all[(size_t)j] = j;

    const bool locked = lk && lk->L > 0;
    if (locked) for (int pass = 0; pass < 2; ++pass) CHK(eig_lock_project(h, *lk, X, n, K));     // X <- X - Q (Z^T X), twice
    // ---- start: orthonormalise X, Rayleigh-Ritz on X alone ----
    CHK(eig_gram_partial(E, X, X, n, 0));
    CHK(eig_gram_reduce(E, n, 1, cgram));
    CHK(fetch(K + KK));
    if (!eig_ortho_factor(hgram, K, all, E.hmix))
        return fail(SGPU_ERR_ARG, "eigs_LOBPCG: the start vectors are linearly dependent (X^T X is not numerically positive definite)");
    CHK(send_mix(1));
    CHK(eig_mix(K, 1, X, cmix, X, cmix, X, cmix, nullptr, X, n));
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
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: the Rayleigh-Ritz problem of the start vectors did not converge (X^T A X is not finite?)");
        if (!(lam[0] > 0.0)) return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: a Ritz value of the start vectors is %g: the operator is not symmetric positive definite", lam[0]);
        std::copy(Q.begin(), Q.end(), E.hmix.get());
        CHK(send_mix(1));
        CHK(eig_mix(K, 1, X, cmix, X, cmix, X, cmix, nullptr, X, n));
        CHK(eig_mix(K, 1, E.AX, cmix, E.AX, cmix, E.AX, cmix, nullptr, E.AX, n));
    }
    for (int j = 0; j < K; ++j) lambda[j] = lam[j];

    bool hasP = false, fresh_AX = false;      // fresh_AX: AX was just recomputed from X, the norms about to be formed are the true ones
    int it = 0;
    for (;;) {
        // ---- the residual of the carried AX, the preconditioned residual and X^T W: host synchronisation 1 ----
        CHK(send_lambda(lam));
        CHK(eig_residual(E, E.AX, X, clam, E.R, n, cnrm));
        auto precondition_and_project = [&]() -> int {                 // W = M R and X^T W
            if (precond) CHK(eig_precondition(h, *Bp, E)); else CHK(sgpu_vec_copy(E.W, E.R, nK));
            if (locked) CHK(eig_lock_project(h, *lk, E.W, n, K));
            CHK(eig_gram_partial(E, X, E.W, n, 0));
            return eig_gram_reduce(E, n, 1, cgram);
        };
        if (!fresh_AX) CHK(precondition_and_project());                // (a recomputed residual almost always ends the solve: no W is formed for it)
        CHK(fetch(fresh_AX ? K : K + KK));
        std::vector<int> act;
        bool conv = true, finite = true;
        for (int j = 0; j < K; ++j) {
            const double rr = hnrm[j];
            if (!std::isfinite(rr)) finite = false;
            if (res_hist && it < hist_cap) res_hist[(size_t)j * hist_cap + it] = std::sqrt(rr);
            if (res) res[j] = std::sqrt(rr);
            const bool cj = rr < tol * tol * lam[j] * lam[j];
            if (!cj) { act.push_back(j); if (j < nev) conv = false; }
        }
        if (iters) *iters = it;
        if (!finite) return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: a residual norm is not finite at iteration %d", it);
        if (conv || it >= max_iter) {
            if (fresh_AX) {                    // these norms come from a recomputed AX: they decide
                if (leading) *leading = act.empty() ? K : act[0];
                if (conv) return SGPU_OK;
                return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: %d of the %d wanted pairs are above the tolerance after %d iterations", (int)std::count_if(act.begin(), act.end(), [&](int j) { return j < nev; }), nev, it);
            }
            CHK(apply_block(A, sk::EPI_SPMV, X, E.AX, EpiArgs(), K));      // end of the solve: only recomputed norms declare convergence
            fresh_AX = true;
            continue;                          // (the same iteration again, on the recomputed AX)
        }
        if (fresh_AX) {                        // the recomputed norms contradict the carried ones and iterations remain: go on from them
            CHK(precondition_and_project());
            CHK(fetch(K + KK));
            fresh_AX = false;
        }
        const int na = (int)act.size();
        // ---- W -= X (X^T W); W^T W and P^T P: host synchronisation 2 ----
        std::fill(E.hmix.get(), E.hmix + KK, 0.0);
        for (int a = 0; a < K; ++a)
            for (int j : act) E.hmix[a * K + j] = -hgram[a * K + j];
        CHK(send_mix(1));
        CHK(eig_mix(K, 1, X, cmix, X, cmix, X, cmix, E.W, E.W, n));
        CHK(eig_gram_partial(E, E.W, E.W, n, 0));
        if (hasP) CHK(eig_gram_partial(E, E.P, E.P, n, 1));
        CHK(eig_gram_reduce(E, n, hasP ? 2 : 1, cgram));
        CHK(fetch(K + (hasP ? 2 : 1) * KK));
        if (!eig_ortho_factor(hgram, K, act, E.hmix))
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: breakdown at iteration %d: the preconditioned residuals of the %d active columns are linearly dependent (W^T W is not numerically positive definite)", it + 1, na);
        bool useP = hasP;
        if (useP && !eig_ortho_factor(hgram + KK, K, act, E.hmix + KK)) useP = false;      // a restart: this iteration runs without P
        CHK(send_mix(useP ? 2 : 1));
        CHK(eig_mix(K, 1, E.W, cmix, E.W, cmix, E.W, cmix, nullptr, E.W, n));               // inactive columns of W become zero
        CHK(apply_block(A, sk::EPI_SPMV, E.W, E.AW, EpiArgs(), K));
        if (useP) {
            CHK(eig_mix(K, 1, E.P, cmix + KK, E.P, cmix + KK, E.P, cmix + KK, nullptr, E.P, n));
            CHK(eig_mix(K, 1, E.AP, cmix + KK, E.AP, cmix + KK, E.AP, cmix + KK, nullptr, E.AP, n));
        }
        if (E.debug_stop == it) {              // tests (sgpu_debug_eig_stop): W, AW, P, AP stay as the orthonormalisation left them
            E.debug_stop = -1;
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: stopped for inspection after the orthonormalisation of iteration %d (%s P)", it + 1, useP ? "with" : "without");
        }
        // ---- the Gram matrices of S = [X, W, P]: host synchronisation 3 ----
        const double *Sv[3] = {X, E.W, E.P}, *ASv[3] = {E.AX, E.AW, E.AP};
        const int nb3 = useP ? 3 : 2;
        int slotS[3][3], slotA[3][3], ns3 = 0;
        for (int a = 0; a < nb3; ++a)
            for (int b = a; b < nb3; ++b) { slotS[a][b] = ns3; CHK(eig_gram_partial(E, Sv[a], Sv[b], n, ns3++)); }
        for (int a = 0; a < nb3; ++a)
            for (int b = a; b < nb3; ++b) { slotA[a][b] = ns3; CHK(eig_gram_partial(E, Sv[a], ASv[b], n, ns3++)); }
        CHK(eig_gram_reduce(E, n, ns3, cgram));
        CHK(fetch(K + ns3 * KK));
        int m = 0;
        const int st = eig_rayleigh_ritz(E, hgram, slotS, slotA, nb3, act, theta, &m);
        if (st < 0)
            return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: breakdown at iteration %d: the Rayleigh-Ritz basis of %d vectors is %s", it + 1, m,
                        st == -1 ? "linearly dependent (S^T S is not numerically positive definite)" : "not finite");
        if (!(theta[0] > 0.0)) return fail(SGPU_ERR_NOCONV, "eigs_LOBPCG: a Ritz value is %g at iteration %d: the operator is not symmetric positive definite", theta[0], it + 1);
        // E.hmix holds C_X | C_W | C_P: the K smallest Ritz vectors; rows of inactive columns are zero
        CHK(send_mix(3));
        if (useP) {
            CHK(eig_mix(K, 2, E.W, cmix + KK, E.P, cmix + 2 * KK, E.P, cmix, nullptr, E.P, n));
            CHK(eig_mix(K, 2, E.AW, cmix + KK, E.AP, cmix + 2 * KK, E.AP, cmix, nullptr, E.AP, n));
        } else {
            CHK(eig_mix(K, 1, E.W, cmix + KK, E.W, cmix, E.W, cmix, nullptr, E.P, n));
            CHK(eig_mix(K, 1, E.AW, cmix + KK, E.AW, cmix, E.AW, cmix, nullptr, E.AP, n));
        }
        CHK(eig_mix(K, 1, X, cmix, X, cmix, X, cmix, E.P, X, n));
        CHK(eig_mix(K, 1, E.AX, cmix, E.AX, cmix, E.AX, cmix, E.AP, E.AX, n));
        for (int j = 0; j < K; ++j) { lam[j] = theta[j]; lambda[j] = theta[j]; }
        hasP = true;
        ++it;
    }
}

int sgpu_eigs_LOBPCG(sgpu_amg *h, value_t *X, int K, int nev, int max_iter, value_t tol, int precond, value_t *lambda, value_t *res, int *iters,
                     value_t *res_hist, int hist_cap) {
    if (h && h->null_space == 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: the hierarchy knows the constant null space, so lambda = 0 is in the spectrum and the unconstrained solve breaks down; lock the normalised constant vector and call sgpu_eigs_LOBPCG_locked");
    return eig_lobpcg_run(h, X, K, nev, max_iter, tol, precond, lambda, res, iters, res_hist, hist_cap, nullptr, nullptr);
}

} // extern "C"
