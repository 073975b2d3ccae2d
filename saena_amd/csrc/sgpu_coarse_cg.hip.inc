// sgpu_coarse_cg.hip.inc -- the device-resident coarsest CG (sgpu_amg_params.coarse_solver = 2; DESIGN.md section 16) for a coarsest
// level of more than CG_MAXN rows that lives whole on one rank.  Part of sgpu_runtime.hip; kernels: kernels_coarse_cg.hip.h.
//
// The host's share is a fixed launch sequence on the compute stream, 2 + 3 (CG_coarsest_max_iter - 1) launches whatever the data, with
// no read-back: vcycle0 captures it with the rest of the V-cycle, the multi-rank tail graph holds it, and the block solves, FGMRES and
// LOBPCG take the hierarchy (coarse_host_driven stays false).  The work space -- res, dir, mt, the two sets of partial sums, the
// scalars and the flags -- is ONE allocation owned by the hierarchy, made by sgpu_amg_create (never inside a capture) and kept by
// sgpu_amg_set_operator: the incoming coarsest operator has the outgoing one's row count.
namespace {

struct DcgLayout {
    size_t ld;                 // the rows rounded up to an even number: every vector starts on a 16-byte boundary
    size_t total() const { return 3 * ld + 2 * (size_t)g.n_partials + sk::DCG_NSCALAR + sk::DCG_NFLAG / 2; }
};
DcgLayout dcg_layout(size_t n) { return DcgLayout{(n + 1) & ~(size_t)1}; }

// the work space of a hierarchy whose coarsest level takes the device CG on this rank; a no-op where it exists
int ensure_dcg(sgpu_amg *h, int M) {
    if (h->dcg) {
        if (h->dcg_rows != M) return fail(SGPU_ERR_STATE, "device CG: the work space holds %d rows, the coarsest operator has %d", h->dcg_rows, M);
        return SGPU_OK;
    }
    const DcgLayout L = dcg_layout((size_t)M);
    if (h->dcg.alloc(L.total()) != hipSuccess) return fail(SGPU_ERR_NOMEM, "device CG: hipMalloc of %zu doubles failed", L.total());
    HIPCHK(hipMemsetAsync(h->dcg, 0, h->dcg.bytes(), g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    h->dcg_rows = M;
    return SGPU_OK;
}

using DcgMatvecFn = void (*)(const sk::DcgMatvecArgs);
DcgMatvecFn pick_dcg_matvec(int G) {
    return among<1, 4, 16, 64>(G, [&](auto GG) -> DcgMatvecFn { return sk::k_dcg_matvec<GG()>; });
}

int coarse_cg_device(sgpu_amg *h, sgpu_op *A, double *u, const double *rhs, int *iters) {
    const int M = A->M, max_iter = h->prm.CG_coarsest_max_iter;
    if (!h->dcg || h->dcg_rows != M) return fail(SGPU_ERR_STATE, "device CG: the hierarchy has no work space for %d rows", M);
    const size_t n = (size_t)M;
    const DcgLayout L = dcg_layout(n);
    double *res = h->dcg, *dir = res + L.ld, *mt = dir + L.ld, *PA = mt + L.ld, *PR = PA + g.n_partials, *S = PR + g.n_partials;
    int *F = reinterpret_cast<int *>(S + sk::DCG_NSCALAR);
    const int G = block_auto_lanes(A), rpp = sk::BLOCK / G;                       // 1, 4, 16 or 64 lanes per row, as k_csr_block chooses
    const int nb = dot_nblocks(n), nba = (int)std::min<size_t>((size_t)g.n_partials, (n + rpp - 1) / rpp);
    const DcgMatvecFn mv = pick_dcg_matvec(G);
    if (!mv) return fail(SGPU_ERR_ARG, "device CG: no product kernel for %d lanes per row", G);     // a missing kernel is an error
    sk::DcgMatvecArgs a;
    a.row_ptr = A->loc.csr.row_ptr; a.col = A->loc.csr.col; a.val = A->loc.csr.val; a.n = M;
    a.dir = dir; a.mt = mt; a.PA = PA; a.F = F;
    SGPU_LAUNCH(sk::k_dcg_start, dim3(nb), dim3(sk::BLOCK), 0, g.cs, rhs, res, dir, n, PR);
    SGPU_LAUNCH(sk::k_dcg_setup, dim3(1), dim3(sk::BLOCK), 0, g.cs, (const double *)PR, nb, h->prm.CG_coarsest_tol, max_iter, S, F);
    for (int it = 1; it < max_iter; ++it) {
        SGPU_LAUNCH(mv, dim3(nba), dim3(sk::BLOCK), 0, g.cs, a);
        SGPU_LAUNCH(sk::k_dcg_update, dim3(nb), dim3(sk::BLOCK), 0, g.cs, (const double *)PA, nba, (const double *)S, (const int *)F, it,
                    (const double *)dir, (const double *)mt, u, res, n, PR);
        SGPU_LAUNCH(sk::k_dcg_dir, dim3(nb), dim3(sk::BLOCK), 0, g.cs, (const double *)PR, nb, S, F, it, max_iter, (const double *)res, dir, n);
    }
    HIPCHK(hipGetLastError());
    if (iters) {
        HIPCHK(hipMemcpyAsync(g.hint + 1, F + sk::DCG_ITERS, sizeof(int), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        *iters = g.hint[1];
    }
    return SGPU_OK;
}

} // namespace

// tests and tests/perf_coarse_cg.py (include/saena_gpu_debug.h): `reps` launches of the device CG's product kernel on the coarsest
// operator, timed with events as sgpu_time_kernel times the tuned form; x, y: M doubles.  The stop flag is clear for the launches.
extern "C" int sgpu_debug_dcg_matvec_time(sgpu_amg *h, const value_t *x, value_t *y, int reps, float *ms) {
    CHK(need_ctx());
    if (!h || !x || !y || !ms || reps < 1) return fail(SGPU_ERR_ARG, "debug_dcg_matvec_time: bad argument");
    sgpu_op *A = h->A[h->nlevels - 1];
    if (!h->dcg || h->dcg_rows != A->M) return fail(SGPU_ERR_STATE, "debug_dcg_matvec_time: the hierarchy runs no device CG on this rank");
    const size_t n = (size_t)A->M;
    const DcgLayout L = dcg_layout(n);
    double *PA = h->dcg.get() + 3 * L.ld, *S = PA + 2 * (size_t)g.n_partials;
    int *F = reinterpret_cast<int *>(S + sk::DCG_NSCALAR);
    const int G = block_auto_lanes(A), rpp = sk::BLOCK / G;
    const int nba = (int)std::min<size_t>((size_t)g.n_partials, (n + rpp - 1) / rpp);
    const DcgMatvecFn mv = pick_dcg_matvec(G);
    if (!mv) return fail(SGPU_ERR_ARG, "device CG: no product kernel for %d lanes per row", G);
    sk::DcgMatvecArgs a;
    a.row_ptr = A->loc.csr.row_ptr; a.col = A->loc.csr.col; a.val = A->loc.csr.val; a.n = A->M;
    a.dir = x; a.mt = y; a.PA = PA; a.F = F;
    HIPCHK(hipMemsetAsync(F, 0, sk::DCG_NFLAG * sizeof(int), g.cs));
    auto once = [&]() -> int { SGPU_LAUNCH(mv, dim3(nba), dim3(sk::BLOCK), 0, g.cs, a); return SGPU_OK; };
    CHK(once());                                                                  // warm-up launch (code object load)
    CHK(time_reps(reps, ms, once));
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}
