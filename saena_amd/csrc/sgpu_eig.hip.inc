// sgpu_eig.hip.inc -- LOBPCG (include/saena_gpu.h) on a block of K vectors, one block V-cycle from a zero iterate as preconditioner:
// sgpu_eigs_LOBPCG, the nev smallest eigenpairs of the SPD level-0 operator A of a hierarchy, and sgpu_eigs_LOBPCG_gen, those of
// A x = lambda B x with a second SPD operator B of the same size (a mass matrix, consistent or lumped).  Part of sgpu_runtime.hip (it
// shares that file's context, handles and helpers); kernels: kernels_eig.hip.h; the small dense problems: host/dense_eig.cpp.
//
// ONE loop, lobpcg_run, serves both problems and, with a locked set handed in, sgpu_eig_lock.hip.inc's constrained solves.  It is
// written in a metric: every inner product is S^T (M S), and the carried blocks S = X, W, P come with A S and M S.  For the standard
// problem M S IS S (the same pointers: nothing is applied, copied or rotated a second time) and two vectors are carried per block;
// for the generalised one M S = B S are three more block vectors BX, BW, BP, B is applied where a new S appears, the residual kernel
// also sums ||(Bx)_j||^2 and the convergence test carries that factor (DESIGN.md section 17).
//
// Nothing here touches the scalar path, sgpu_solve_pCG_block's vectors or the block cache of eight captured V-cycles.  The state is
// an AmgEig per (hierarchy, K) (sgpu_runtime.hip): six block vectors (AX, R, W, AW, P, AP; X is the caller's), ONE fixed (R, W) pair
// the V-cycle preconditions through (captured once into a graph of its own and replayed by every iteration of every solve of either
// problem), the partial sums, the device coefficients and their pinned mirrors.  The V-cycle's work vectors are the AmgBlock's.  What
// only the generalised problem needs (BX, BW, BP, the partial sums and the K sums of ||(Bx)_j||^2) is made by amg_geig at the first
// generalised call with a given K: a process that never makes one allocates what the standard solve alone allocates.
//
// Two rules about B: it is applied by eager launches only (apply_block; it never enters a captured graph), and nothing keeps a
// pointer to it after the call returns.
//
// Host synchronisations: THREE per iteration --
//   1. ||r_j||^2 of the carried residual together with (M X)^T W (K + K^2 doubles; with B also the K ||(Bx)_j||^2),
//   2. W^T M W and P^T M P after the projection (2 K^2),
//   3. S^T M S and S^T A S, S = [X, W, P]: the upper block triangle of both, diagonal blocks in full (12 K^2 doubles; the host mirrors
//      the rest, takes the rows and columns of the active set and symmetrises),
// plus two at the start (X^T M X, X^T A X) and one per recomputed residual at the end of the solve (its K norms alone: no V-cycle
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
    SGPU_LAUNCH_COLS("k_gram_block_partial", K, per_K(K, [](auto k) { return sk::k_gram_block_partial<k()>; }), dim3(nb), dim3(sk::BLOCK), 0, g.cs, X, Y, n, part);
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
MixFn eig_mix_fn(int K, int ns) {
    return per_K(K, [&](auto k) { return among<1, 2, 3>(ns, [](auto s) -> MixFn { return sk::k_block_mix<decltype(k)::value, s()>; }); });
}

// out = sum_{s < ns} S_s C_s (+ add): C_s device, K x K row-major; out may alias any source and add
int eig_mix(int K, int ns, const double *s0, const double *c0, const double *s1, const double *c1, const double *s2, const double *c2,
            const double *add, double *out, size_t n) {
    if (!n) return SGPU_OK;
    const int gd = (int)std::min<size_t>(2048, (n + sk::BLOCK - 1) / sk::BLOCK);
    SGPU_LAUNCH_COLS("k_block_mix", K, eig_mix_fn(K, ns), dim3(gd), dim3(sk::BLOCK), 0, g.cs, s0, c0, s1, c1, s2, c2, add, out, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// R = AX - MX diag(lambda), out_r[j] = ||r_j||^2 (device).  out_b null: the standard problem (MX is X), k_eig_residual and ONE
// reduce; else the generalised one (MX is BX): k_geig_residual, and a second reduce leaves out_b[j] = ||(Bx)_j||^2 (E.bpart: amg_geig's)
int eig_residual(AmgEig &E, const double *AX, const double *MX, const double *lambda, double *R, size_t n, double *out_r, double *out_b) {
    const int nb = dot_nblocks(n), K = E.K;
    if (!out_b) SGPU_LAUNCH_COLS("k_eig_residual", K, per_K(K, [](auto k) { return sk::k_eig_residual<k()>; }), dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, MX, lambda, R, n, E.rpart);
    else SGPU_LAUNCH_COLS("k_geig_residual", K, per_K(K, [](auto k) { return sk::k_geig_residual<k()>; }), dim3(nb), dim3(sk::BLOCK), 0, g.cs, AX, MX, lambda, R, n, E.rpart, E.bpart);
    SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)E.rpart, nb, K, out_r, (1u << K) - 1u);
    if (out_b) SGPU_LAUNCH(sk::k_reduce_partials_block, dim3(K), dim3(sk::BLOCK), 0, g.cs, (const double *)E.bpart, nb, K, out_b, (1u << K) - 1u);
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
    return eig_residual(*E, AX, X, lambda_dev, R, n, rr_dev, nullptr);
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
    const double *c = E->coef, *lam = E->coef + 3 * K * K;
    double *nrm = E->coef + 3 * K * K + K, *gram = nrm + K;
    auto once = [&]() -> int {
        if (kind == 0) { CHK(eig_gram_partial(*E, X, Y, n, 0)); return eig_gram_reduce(*E, n, 1, gram); }
        if (kind == 1) return eig_mix(K, ns, X, c, Y, c + K * K, X, c + 2 * K * K, nullptr, Out, n);
        return eig_residual(*E, X, Y, lam, Out, n, nrm, nullptr);
    };
    CHK(once());
    return time_reps(reps, ms, once);
}


// tests: the residual of the generalised problem, with both reductions, on the caller's arrays
int sgpu_debug_geig_residual(sgpu_amg *h, const value_t *AX, const value_t *BX, const value_t *lambda_dev, value_t *R, size_t n, int K,
                             value_t *rr_dev, value_t *bb_dev) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_geig_residual", &E));
    if (!AX || !BX || !lambda_dev || !R || !rr_dev || !bb_dev) return fail(SGPU_ERR_ARG, "debug_geig_residual: null argument");
    if (!gs_aligned(AX) || !gs_aligned(BX) || !gs_aligned(R)) return fail(SGPU_ERR_ARG, "debug_geig_residual: block vectors must be 16-byte aligned");
    CHK(amg_geig(h, K, &E));
    return eig_residual(*E, AX, BX, lambda_dev, R, n, rr_dev, bb_dev);
}

// measurement (tests/perf_geig.py): ms per run of `reps` back-to-back runs of the generalised residual with both reductions
int sgpu_debug_time_geig(sgpu_amg *h, const value_t *AX, const value_t *BX, value_t *R, size_t n, int K, int reps, float *ms) {
    AmgEig *E = nullptr;
    CHK(eig_debug_args(h, K, "debug_time_geig", &E));
    if (!AX || !BX || !R || !ms || reps < 1) return fail(SGPU_ERR_ARG, "debug_time_geig: bad argument");
    if (!gs_aligned(AX) || !gs_aligned(BX) || !gs_aligned(R)) return fail(SGPU_ERR_ARG, "debug_time_geig: block vectors must be 16-byte aligned");
    CHK(amg_geig(h, K, &E));
    CHK(sgpu_vec_fill(E->coef, 0.0, 15 * (size_t)K * K + 2 * K));
    const double *lam = E->coef + 3 * K * K;
    double *nrm = E->coef + 3 * K * K + K;
    auto once = [&]() -> int { return eig_residual(*E, AX, BX, lam, R, n, nrm, E->bnrm); };
    CHK(once());
    return time_reps(reps, ms, once);
}

// The loop of every LOBPCG entry point.  B null: the standard problem A x = lambda x; else A x = lambda B x.  lk (may be null) with
// L > 0: the solve of sgpu_eigs_LOBPCG_locked -- X is projected twice before the start orthonormalisation and W once right after
// W = M R (Z = Q, or B Q with B).  *leading (may be null): the leading columns converged on recomputed norms.
//
// The three carried blocks are S[0] = X, S[1] = W, S[2] = P, each with AS[b] = A S[b] and its metric side MS[b]: B S[b] in vectors of
// their own with B, S[b] itself without.  V[b] lists what block b carries, so that "every carried vector of b" is V[b][0 .. nv)
static int lobpcg_run(sgpu_amg *h, sgpu_op *B, value_t *X, int K, int nev, int max_iter, value_t tol, int precond, value_t *lambda, value_t *res,
                      int *iters, value_t *res_hist, int hist_cap, const EigLock *lk, int *leading) {
    const char *who = B ? "eigs_LOBPCG_gen" : "eigs_LOBPCG";
    if (leading) *leading = 0;
    CHK(need_ctx());
    if (!h || !X || !lambda) return fail(SGPU_ERR_ARG, "%s: null argument", who);
    CHK(lobpcg_check(h, K, who));
    if (nev < 1 || nev > K) return fail(SGPU_ERR_ARG, "%s: nev must be in 1..K (nev = %d, K = %d)", who, nev, K);
    if (precond != 0 && precond != 1) return fail(SGPU_ERR_ARG, "%s: precond is 0 (none) or 1 (one V-cycle), got %d", who, precond);
    if (max_iter < 0 || !(tol >= 0.0)) return fail(SGPU_ERR_ARG, "%s: max_iter and tol must not be negative", who);
    sgpu_op *A = h->A[0];
    const size_t n = (size_t)A->M, nK = n * K;
    if (B && (B->M != A->M || B->N_local != A->N_local))
        return fail(SGPU_ERR_ARG, "%s: B is %d x %d, the level-0 operator %d x %d: both must have the same size", who, (int)B->M, (int)B->N_local, (int)A->M, (int)A->N_local);
    if (B && (B->has_remote || B->recvSize || B->vIndexSize))
        return fail(SGPU_ERR_ARG, "%s: B has a remote part or a halo plan (%d halo entries, %d sent); it takes single-rank operators only", who, B->recvSize, B->vIndexSize);
    if (n < 3 * (size_t)K) return fail(SGPU_ERR_ARG, "%s: the operator has %zu rows; the Rayleigh-Ritz basis of 3 K = %d vectors needs at least as many", who, n, 3 * K);
    if (!gs_aligned(X)) return fail(SGPU_ERR_ARG, "%s: X must be 16-byte aligned", who);
    AmgBlock *Bp = nullptr;
    AmgEig *Ep = nullptr;
    CHK(amg_block(h, K, &Bp));
    CHK(B ? amg_geig(h, K, &Ep) : amg_eig(h, K, &Ep));
    AmgEig &E = *Ep;
    const int KK = K * K, nv = B ? 3 : 2;
    double *const S[3] = {X, E.W, E.P}, *const AS[3] = {E.AX, E.AW, E.AP};
    double *const MS[3] = {B ? E.BX.get() : S[0], B ? E.BW.get() : S[1], B ? E.BP.get() : S[2]};
    double *const V[3][3] = {{S[0], AS[0], MS[0]}, {S[1], AS[1], MS[1]}, {S[2], AS[2], MS[2]}};
    double *cmix = E.coef, *clam = E.coef + 3 * KK, *cnrm = clam + K, *cgram = cnrm + K;
    double *hnrm = E.hdown, *hgram = E.hdown + K;                  // the mirror of cnrm | cgram
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
    auto mix1 = [&](double *Y, const double *c) -> int { return eig_mix(K, 1, Y, c, Y, c, Y, c, nullptr, Y, n); };   // Y <- Y C
    auto apply_A = [&](int b) -> int { return apply_block(A, sk::EPI_SPMV, S[b], AS[b], EpiArgs(), K); };
    auto apply_B = [&](int b) -> int { return B ? apply_block(B, sk::EPI_SPMV, S[b], MS[b], EpiArgs(), K) : SGPU_OK; };   // eager, always
    if (iters) *iters = 0;
    std::vector<int> all((size_t)K);
    for (int j = 0; j < K; ++j) all[(size_t)j] = j;

    const bool locked = lk && lk->L > 0;
    if (locked) for (int pass = 0; pass < 2; ++pass) CHK(eig_lock_project(h, *lk, X, n, K));     // X <- X - Q (Z^T X), twice
    // ---- start: orthonormalise X in the metric, Rayleigh-Ritz on X alone (X^T M X = I: the standard dense problem) ----
    CHK(apply_B(0));
    CHK(eig_gram_partial(E, X, MS[0], n, 0));
    CHK(eig_gram_reduce(E, n, 1, cgram));
    CHK(fetch(K + KK));
    if (!eig_ortho_factor(hgram, K, all, E.hmix))
        return B ? fail(SGPU_ERR_ARG, "%s: X^T B X is not numerically positive definite: the start vectors are linearly dependent, or B is not positive definite", who)
                 : fail(SGPU_ERR_ARG, "%s: the start vectors are linearly dependent (X^T X is not numerically positive definite)", who);
    CHK(send_mix(1));
    CHK(mix1(X, cmix));
    if (B) CHK(mix1(MS[0], cmix));
    CHK(apply_A(0));
    CHK(eig_gram_partial(E, X, E.AX, n, 0));
    CHK(eig_gram_reduce(E, n, 1, cgram));
    CHK(fetch(K + KK));
    double lam[8], theta[24];
    {
        std::vector<double> G((size_t)KK), Q((size_t)KK);
        for (int i = 0; i < K; ++i)
            for (int j = 0; j < K; ++j) G[(size_t)i * K + j] = 0.5 * (hgram[i * K + j] + hgram[j * K + i]);
        if (saena_host::dense_sym_eig(K, G.data(), lam, Q.data()) < 0)
            return fail(SGPU_ERR_NOCONV, "%s: the Rayleigh-Ritz problem of the start vectors did not converge (X^T A X is not finite?)", who);
        if (!(lam[0] > 0.0)) return fail(SGPU_ERR_NOCONV, "%s: a Ritz value of the start vectors is %g: A is not symmetric positive definite", who, lam[0]);
        std::copy(Q.begin(), Q.end(), E.hmix.get());
        CHK(send_mix(1));
        for (int v = 0; v < nv; ++v) CHK(mix1(V[0][v], cmix));     // X, AX (, BX)
    }
    for (int j = 0; j < K; ++j) lambda[j] = lam[j];

    bool hasP = false, fresh_AX = false;      // fresh_AX: AX (and BX) were just recomputed from X, the norms about to be formed are the true ones
    int it = 0;
    for (;;) {
        // ---- the residual of the carried AX (and BX), the preconditioned residual and (M X)^T W: host synchronisation 1 ----
        CHK(send_lambda(lam));
        CHK(eig_residual(E, E.AX, MS[0], clam, E.R, n, cnrm, B ? E.bnrm.get() : nullptr));
        auto precondition_and_project = [&]() -> int {                 // W = M R and (M X)^T W
            if (precond) CHK(eig_precondition(h, *Bp, E)); else CHK(sgpu_vec_copy(E.W, E.R, nK));
            if (locked) CHK(eig_lock_project(h, *lk, E.W, n, K));
            CHK(eig_gram_partial(E, MS[0], E.W, n, 0));
            return eig_gram_reduce(E, n, 1, cgram);
        };
        if (!fresh_AX) CHK(precondition_and_project());                // (a recomputed residual almost always ends the solve: no W is formed for it)
        CHK(fetch(fresh_AX ? K : K + KK, B != nullptr));
        std::vector<int> act;
        bool conv = true, finite = true;
        for (int j = 0; j < K; ++j) {
            const double rr = hnrm[j], bb = B ? E.hbn[j] : 1.0;
            if (!std::isfinite(rr) || !std::isfinite(bb)) finite = false;
            if (res_hist && it < hist_cap) res_hist[(size_t)j * hist_cap + it] = std::sqrt(rr);
            if (res) res[j] = std::sqrt(rr);
            const bool cj = rr < tol * tol * lam[j] * lam[j] * bb;     // ||A x - lambda M x|| < tol lambda ||M x||; bb is an exact 1 without B
            if (!cj) { act.push_back(j); if (j < nev) conv = false; }
        }
        if (iters) *iters = it;
        if (!finite) return fail(SGPU_ERR_NOCONV, "%s: a residual norm%s is not finite at iteration %d", who, B ? " or ||B x_j||" : "", it);
        if (conv || it >= max_iter) {
            if (fresh_AX) {                    // these norms come from a recomputed AX (and BX): they decide
                if (leading) *leading = act.empty() ? K : act[0];
                if (conv) return SGPU_OK;
                return fail(SGPU_ERR_NOCONV, "%s: %d of the %d wanted pairs are above the tolerance after %d iterations", who, (int)std::count_if(act.begin(), act.end(), [&](int j) { return j < nev; }), nev, it);
            }
            CHK(apply_A(0));                   // end of the solve: only recomputed norms declare convergence
            CHK(apply_B(0));
            fresh_AX = true;
            continue;                          // (the same iteration again, on the recomputed AX and BX)
        }
        if (fresh_AX) {                        // the recomputed norms contradict the carried ones and iterations remain: go on from them
            CHK(precondition_and_project());
            CHK(fetch(K + KK));
            fresh_AX = false;
        }
        const int na = (int)act.size();
        // ---- W -= X ((M X)^T W); M W; W^T M W and P^T M P: host synchronisation 2 ----
        std::fill(E.hmix.get(), E.hmix + KK, 0.0);
        for (int a = 0; a < K; ++a)
            for (int j : act) E.hmix[a * K + j] = -hgram[a * K + j];
        CHK(send_mix(1));
        CHK(eig_mix(K, 1, X, cmix, X, cmix, X, cmix, E.W, E.W, n));
        CHK(apply_B(1));
        CHK(eig_gram_partial(E, E.W, MS[1], n, 0));
        if (hasP) CHK(eig_gram_partial(E, E.P, MS[2], n, 1));
        CHK(eig_gram_reduce(E, n, hasP ? 2 : 1, cgram));
        CHK(fetch(K + (hasP ? 2 : 1) * KK));
        if (!eig_ortho_factor(hgram, K, act, E.hmix))
            return B ? fail(SGPU_ERR_NOCONV, "%s: breakdown at iteration %d: W^T B W of the %d active columns is not numerically positive definite (the preconditioned residuals are linearly dependent, or B is not positive definite)", who, it + 1, na)
                     : fail(SGPU_ERR_NOCONV, "%s: breakdown at iteration %d: the preconditioned residuals of the %d active columns are linearly dependent (W^T W is not numerically positive definite)", who, it + 1, na);
        bool useP = hasP;
        if (useP && !eig_ortho_factor(hgram + KK, K, act, E.hmix + KK)) useP = false;      // a restart: this iteration runs without P
        CHK(send_mix(useP ? 2 : 1));
        CHK(mix1(E.W, cmix));                                                               // inactive columns of W (and BW) become zero
        if (B) CHK(mix1(MS[1], cmix));
        CHK(apply_A(1));
        if (useP) for (int v = 0; v < nv; ++v) CHK(mix1(V[2][v], cmix + KK));               // P, AP (, BP)
        if (E.debug_stop == it) {              // tests (sgpu_debug_eig_stop): W, AW, P, AP (, BW, BP) stay as the orthonormalisation left them
            E.debug_stop = -1;
            return fail(SGPU_ERR_NOCONV, "%s: stopped for inspection after the orthonormalisation of iteration %d (%s P)", who, it + 1, useP ? "with" : "without");
        }
        // ---- the Gram matrices of S = [X, W, P] with M S and A S: host synchronisation 3 ----
        const int nb3 = useP ? 3 : 2;
        int slotS[3][3], slotA[3][3], ns3 = 0;
        for (int a = 0; a < nb3; ++a)
            for (int b = a; b < nb3; ++b) { slotS[a][b] = ns3; CHK(eig_gram_partial(E, S[a], MS[b], n, ns3++)); }
        for (int a = 0; a < nb3; ++a)
            for (int b = a; b < nb3; ++b) { slotA[a][b] = ns3; CHK(eig_gram_partial(E, S[a], AS[b], n, ns3++)); }
        CHK(eig_gram_reduce(E, n, ns3, cgram));
        CHK(fetch(K + ns3 * KK));
        int m = 0;
        const int st = eig_rayleigh_ritz(E, hgram, slotS, slotA, nb3, act, theta, &m);
        if (st < 0)
            return fail(SGPU_ERR_NOCONV, "%s: breakdown at iteration %d: the Rayleigh-Ritz basis of %d vectors is %s", who, it + 1, m,
                        st != -1 ? "not finite" : B ? "linearly dependent, or B is not positive definite (S^T B S is not numerically positive definite)"
                                                    : "linearly dependent (S^T S is not numerically positive definite)");
        if (!(theta[0] > 0.0)) return fail(SGPU_ERR_NOCONV, "%s: a Ritz value is %g at iteration %d: A is not symmetric positive definite", who, theta[0], it + 1);
        // E.hmix holds C_X | C_W | C_P: the K smallest Ritz vectors; rows of inactive columns are zero
        CHK(send_mix(3));
        for (int v = 0; v < nv; ++v) {         // P, AP (, BP) = W C_W + P C_P of the same kind
            if (useP) CHK(eig_mix(K, 2, V[1][v], cmix + KK, V[2][v], cmix + 2 * KK, V[2][v], cmix, nullptr, V[2][v], n));
            else CHK(eig_mix(K, 1, V[1][v], cmix + KK, V[1][v], cmix, V[1][v], cmix, nullptr, V[2][v], n));
        }
        for (int v = 0; v < nv; ++v) CHK(eig_mix(K, 1, V[0][v], cmix, V[0][v], cmix, V[0][v], cmix, V[2][v], V[0][v], n));   // X, AX (, BX) = . C_X + the new P's
        for (int j = 0; j < K; ++j) { lam[j] = theta[j]; lambda[j] = theta[j]; }
        hasP = true;
        ++it;
    }
}

int sgpu_eigs_LOBPCG(sgpu_amg *h, value_t *X, int K, int nev, int max_iter, value_t tol, int precond, value_t *lambda, value_t *res, int *iters,
                     value_t *res_hist, int hist_cap) {
    if (h && h->null_space == 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG: the hierarchy knows the constant null space, so lambda = 0 is in the spectrum and the unconstrained solve breaks down; lock the normalised constant vector and call sgpu_eigs_LOBPCG_locked");
    return lobpcg_run(h, nullptr, X, K, nev, max_iter, tol, precond, lambda, res, iters, res_hist, hist_cap, nullptr, nullptr);
}

int sgpu_eigs_LOBPCG_gen(sgpu_amg *h, sgpu_op *B, value_t *X, int K, int nev, int max_iter, value_t tol, int precond, value_t *lambda,
                         value_t *res, int *iters, value_t *res_hist, int hist_cap) {
    if (h && h->null_space == 1) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: the hierarchy knows the constant null space, so lambda = 0 is in the spectrum and the unconstrained solve breaks down; lock the normalised constant vector and call sgpu_eigs_LOBPCG_locked");
    if (!B) {                                  // (to the loop a null B is the standard problem: this entry point refuses it where the loop would look at B)
        CHK(need_ctx());
        if (!h || !X || !lambda) return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: null argument");
        return fail(SGPU_ERR_ARG, "eigs_LOBPCG_gen: B is null (sgpu_eigs_LOBPCG solves the standard problem)");
    }
    return lobpcg_run(h, B, X, K, nev, max_iter, tol, precond, lambda, res, iters, res_hist, hist_cap, nullptr, nullptr);
}

} // extern "C"
