// sgpu_gmres.hip.inc -- sgpu_solve_FGMRES (include/saena_gpu.h): restarted flexible GMRES, right-preconditioned by one V-cycle from a
// zero iterate.  Part of sgpu_runtime.hip (it shares that file's context, handles and helpers); kernels: kernels_gmres.hip.h.
//
// Nothing here touches sgpu_solve_pCG: no plan, no scalar work vector, no entry of the hierarchy's cache of captured V-cycles.  The
// state is an AmgGmres per hierarchy (sgpu_runtime.hip): the basis V, the preconditioned vectors Z, ONE fixed pair of work vectors
// the V-cycle preconditions through (captured once into a graph of its own and replayed by every iteration of every solve), the
// device coefficients with their pinned mirror, and the partial sums of the dots.
namespace {

int gs_nblocks(size_t n) { return (int)std::min<size_t>(sk::GS_MAXBLK, std::max<size_t>(1, ((n >> 1) + sk::BLOCK - 1) / sk::BLOCK)); }

bool gs_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// the instantiation for a pass of nc columns (1 .. GS_C)
using GsDotsFn = void (*)(const double *, size_t, const double *, size_t, double *);
using GsUpdateFn = void (*)(const double *, size_t, const double *, double *, size_t, double *);
GsDotsFn gs_dots_fn(int nc) {
    return among<1, 2, 3, 4, 5, 6, 7, 8>(nc, [](auto c) -> GsDotsFn { return sk::k_gs_dots_partial<c()>; });
}
template <bool NORM>
GsUpdateFn gs_update_fn(int nc) {
    return among<1, 2, 3, 4, 5, 6, 7, 8>(nc, [](auto c) -> GsUpdateFn { return sk::k_gs_update<c(), NORM>; });
}
static_assert(sk::GS_C == 8, "the two lists above name 1 .. 8 columns");

// out[c] = V[:,c] . w for c < ncols (device): one pass over w per GS_C columns, then one workgroup per column over the partials
int gs_dots(const double *V, size_t ld, int ncols, const double *w, size_t n, double *partials, double *out) {
    if (ncols <= 0) return SGPU_OK;
    const int nb = gs_nblocks(n);
    for (int c0 = 0; c0 < ncols; c0 += sk::GS_C) {
        const int nc = std::min(sk::GS_C, ncols - c0);
        SGPU_LAUNCH_COLS("k_gs_dots_partial", nc, gs_dots_fn(nc), dim3(nb), dim3(sk::BLOCK), 0, g.cs, V + (size_t)c0 * ld, ld, w, n, partials + (size_t)c0 * sk::GS_MAXBLK);
    }
    SGPU_LAUNCH(sk::k_gs_reduce, dim3(ncols), dim3(sk::BLOCK), 0, g.cs, (const double *)partials, nb, out);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

// w -= sum_c h[c] V[:,c] (h: device), chunk after chunk on the same running value; norm2 (device, may be null) = the new w . w,
// its partial sums written by the launch of the last chunk
int gs_update(const double *V, size_t ld, int ncols, const double *h, double *w, size_t n, double *partials, double *norm2) {
    const int nb = gs_nblocks(n);
    if (ncols <= 0) return SGPU_OK;
    for (int c0 = 0; c0 < ncols; c0 += sk::GS_C) {
        const int nc = std::min(sk::GS_C, ncols - c0);
        const bool fused = norm2 && c0 + sk::GS_C >= ncols;                // the last chunk also leaves the partial sums of the new w . w
        SGPU_LAUNCH_COLS("k_gs_update", nc, fused ? gs_update_fn<true>(nc) : gs_update_fn<false>(nc), dim3(nb), dim3(sk::BLOCK), 0, g.cs, V + (size_t)c0 * ld, ld, h + c0, w, n,
                         fused ? partials : (double *)nullptr);
    }
    if (norm2) SGPU_LAUNCH(sk::k_gs_reduce, dim3(1), dim3(sk::BLOCK), 0, g.cs, (const double *)partials, nb, norm2);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

int gs_scale(const double *nrm2, const double *w, double *v, size_t n) {
    SGPU_LAUNCH(sk::k_gs_scale, dim3(gs_nblocks(n)), dim3(sk::BLOCK), 0, g.cs, nrm2, w, v, n);
    HIPCHK(hipGetLastError());
    return SGPU_OK;
}

int gmres_check(sgpu_amg *h, const char *what) {
    if (g.nranks > 1 || g.multi()) return fail(SGPU_ERR_ARG, "%s: FGMRES runs on one rank only (this context has %d)", what, g.nranks);
    if (h->coarse_host_driven) return fail(SGPU_ERR_ARG, "%s: the coarsest level has %d rows and needs the host-driven CG; FGMRES takes hierarchies whose coarsest level fits the LDS-resident solvers (<= %d rows)", what, h->A[h->nlevels - 1]->M, sk::CG_MAXN);
    auto local = [&](const sgpu_op *op) {
        if (op && (op->has_remote || op->recvSize))
            return fail(SGPU_ERR_ARG, "%s: an operator has a remote part (%d halo entries); FGMRES takes single-rank operators only", what, op->recvSize);
        return (int)SGPU_OK;
    };
    for (int l = 0; l < h->nlevels; ++l) {
        CHK(local(h->A[l]));
        if (l < h->nlevels - 1) { CHK(local(h->P[l])); CHK(local(h->R[l])); }
    }
    return SGPU_OK;
}

// the hierarchy's FGMRES work space for this restart length: made at the first call, remade when the restart length changes
int amg_gmres(sgpu_amg *h, int restart, AmgGmres **out) {
    if (h->gm && h->gm->restart != restart) {
        HIPCHK(hipStreamSynchronize(g.cs));
        h->gm.reset();
    }
    if (!h->gm) {
        std::unique_ptr<AmgGmres> G(new AmgGmres());
        const size_t n = (size_t)h->A[0]->M;
        G->restart = restart;
        G->ld = std::max<size_t>(2, (n + 1) & ~(size_t)1);
        HIPCHK(alloc_vec(G->V, G->ld * (size_t)(restart + 1)));
        HIPCHK(alloc_vec(G->Z, G->ld * (size_t)restart));
        HIPCHK(alloc_vec(G->pin, G->ld)); HIPCHK(alloc_vec(G->pout, G->ld));
        HIPCHK(alloc_vec(G->coef, 2 * (size_t)(restart + 1) + 1));
        HIPCHK(alloc_vec(G->partials, (size_t)(restart + 1) * sk::GS_MAXBLK));
        HIPCHK(G->hcoef.alloc(2 * (size_t)(restart + 1) + 1));
        h->gm = std::move(G);
    }
    *out = h->gm.get();
    return SGPU_OK;
}

// pout = one V-cycle on pin from a zero iterate: vcycle0's capture and replay on the fixed pair, in a graph the scalar cache never sees
int gmres_precondition(sgpu_amg *h, AmgGmres &G) {
    if (!h->prm.use_graph) return vcycle0_eager(h, G.pout, G.pin, true);
    if (G.exec && G.graph_gen != g_plan_generation) {       // an operator was retuned since the capture
        HIPCHK(hipStreamSynchronize(g.cs));
        G.drop_graph();
    }
    if (!G.exec) {
        HIPCHK(hipStreamBeginCapture(g.cs, hipStreamCaptureModeThreadLocal));
        const int st = vcycle0_eager(h, G.pout, G.pin, true);
        const hipError_t e = hipStreamEndCapture(g.cs, &G.graph);
        if (st != SGPU_OK) { G.drop_graph(); return st; }
        if (e != hipSuccess) return fail(SGPU_ERR_HIP, "hipStreamEndCapture: %s", hipGetErrorString(e));
        HIPCHK(hipGraphInstantiate(&G.exec, G.graph, nullptr, nullptr, 0));
        G.graph_gen = g_plan_generation;
    }
    ++g_launches; HIPCHK(hipGraphLaunch(G.exec, g.cs));
    return SGPU_OK;
}

int gs_debug_args(const void *V, size_t ld, int ncols, const void *w, size_t n, const char *what) {
    CHK(need_ctx());
    if (!V || !w) return fail(SGPU_ERR_ARG, "%s: null argument", what);
    if (ncols < 1 || ncols > 65) return fail(SGPU_ERR_ARG, "%s: 1 to 65 columns (restart <= 64), got %d", what, ncols);
    if ((ld & 1) || ld < n) return fail(SGPU_ERR_ARG, "%s: the leading dimension (%zu) must be even and at least n (%zu)", what, ld, n);
    if (!gs_aligned(V) || !gs_aligned(w)) return fail(SGPU_ERR_ARG, "%s: V and w must be 16-byte aligned", what);
    return SGPU_OK;
}

} // namespace

extern "C" {

// ---- tests (include/saena_gpu_debug.h): the solver's own launch helpers on the caller's arrays ----
int sgpu_debug_gs_dots(const value_t *V, size_t ld, int ncols, const value_t *w, size_t n, value_t *out_host) {
    CHK(gs_debug_args(V, ld, ncols, w, n, "debug_gs_dots"));
    if (!out_host) return fail(SGPU_ERR_ARG, "debug_gs_dots: null argument");
    DevArr<double> partials, out;
    CHK(dev_alloc(partials, (size_t)ncols * sk::GS_MAXBLK)); CHK(dev_alloc(out, (size_t)ncols));
    CHK(gs_dots(V, ld, ncols, w, n, partials, out));
    HIPCHK(hipMemcpyAsync(out_host, out, (size_t)ncols * sizeof(double), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    return SGPU_OK;
}

int sgpu_debug_gs_update(const value_t *V, size_t ld, int ncols, const value_t *h_host, value_t *w, size_t n, value_t *norm2_out_host) {
    CHK(gs_debug_args(V, ld, ncols, w, n, "debug_gs_update"));
    if (!h_host) return fail(SGPU_ERR_ARG, "debug_gs_update: null argument");
    DevArr<double> partials, coef;
    CHK(dev_alloc(partials, sk::GS_MAXBLK)); CHK(dev_alloc(coef, (size_t)ncols + 1));
    HIPCHK(hipMemcpyAsync(coef, h_host, (size_t)ncols * sizeof(double), hipMemcpyHostToDevice, g.cs));
    CHK(gs_update(V, ld, ncols, coef, w, n, partials, norm2_out_host ? coef + ncols : nullptr));
    if (norm2_out_host) HIPCHK(hipMemcpyAsync(norm2_out_host, coef + ncols, sizeof(double), hipMemcpyDeviceToHost, g.cs));
    HIPCHK(hipStreamSynchronize(g.cs));
    return SGPU_OK;
}

// measurement (tests/perf_gmres.py): `reps` back-to-back runs of one helper between two events; kind 0: the dots of ncols columns,
// 1: the update by ncols columns with the fused norm (coefficients zero: w keeps its values)
int sgpu_debug_time_gs(int kind, const value_t *V, size_t ld, int ncols, value_t *w, size_t n, int reps, float *ms) {
    CHK(gs_debug_args(V, ld, ncols, w, n, "debug_time_gs"));
    if (!ms || reps < 1 || (kind != 0 && kind != 1)) return fail(SGPU_ERR_ARG, "debug_time_gs: bad argument");
    DevArr<double> partials, coef;
    CHK(dev_alloc(partials, (size_t)ncols * sk::GS_MAXBLK)); CHK(dev_alloc(coef, (size_t)ncols + 1));
    CHK(sgpu_vec_fill(coef, 0.0, (size_t)ncols + 1));
    auto once = [&]() { return kind == 0 ? gs_dots(V, ld, ncols, w, n, partials, coef) : gs_update(V, ld, ncols, coef, w, n, partials, coef + ncols); };
    if (kind == 1) CHK(once());                                // (after it the coefficients are still zero: the dots are not run)
    return time_reps(reps, ms, once);
}

// Restarted flexible GMRES.  Per inner iteration j: z = M v_j (one V-cycle from zero through the fixed pair, or z = v_j), w = A z,
// classical Gram-Schmidt twice against v_0 .. v_j, ONE host synchronisation (both coefficient sets and ||w||^2), then on the host the
// Hessenberg column, its Givens rotations and the residual estimate |g_{j+1}|.  The estimate is tested before v_{j+1} is formed.  At
// the end of a cycle: y from the triangular system, u += Z y, r = rhs - A u and its dot recomputed; only that recomputed dot
// declares convergence.
int sgpu_solve_FGMRES(sgpu_amg *h, value_t *u, const value_t *rhs, int restart, int precond, int *iters, value_t *hist, int cap, value_t *true_res) {
    CHK(need_ctx());
    if (!h || !u || !rhs) return fail(SGPU_ERR_ARG, "null argument");
    if (h->null_space == 1) return fail(SGPU_ERR_ARG, "solve_FGMRES: the hierarchy knows the constant null space; symmetric solvers only (a nonsymmetric operator's left null vector need not be constant): sgpu_solve_pCG, sgpu_solve_CG, sgpu_solve, sgpu_solve_smoother");
    if (restart < 1 || restart > 64) return fail(SGPU_ERR_ARG, "solve_FGMRES: the restart length must be in 1..64 (got %d)", restart);
    if (precond != 0 && precond != 1) return fail(SGPU_ERR_ARG, "solve_FGMRES: precond is 0 (none) or 1 (one V-cycle), got %d", precond);
    if (!gs_aligned(u)) return fail(SGPU_ERR_ARG, "solve_FGMRES: u must be 16-byte aligned");
    CHK(gmres_check(h, "solve_FGMRES"));
    AmgGmres *Gp = nullptr;
    CHK(amg_gmres(h, restart, &Gp));
    AmgGmres &G = *Gp;
    sgpu_op *A = h->A[0];
    const size_t sz = (size_t)A->M, ld = G.ld;
    const int m = restart, max_iter = h->prm.solver_max_iter;
    double *V = G.V, *Zp = precond ? G.Z : G.V;                    // without a preconditioner z_j is v_j
    auto fetch = [&](const double *dev, int k) -> int {
        HIPCHK(hipMemcpyAsync(G.hcoef, dev, (size_t)k * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        return SGPU_OK;
    };
    if (iters) *iters = 0;
    if (true_res) *true_res = 0.0;
    CHK(sgpu_vec_fill(u, 0.0, sz));
    CHK(sgpu_residual_negative(A, u, rhs, V));                     // r_0 = rhs - A 0, in column 0 of the basis
    CHK(gs_dots(V, ld, 1, V, sz, G.partials, G.coef));
    CHK(fetch(G.coef, 1));
    const double init_dot = G.hcoef[0];
    if (hist && cap > 0) hist[0] = std::sqrt(init_dot);
    if (true_res) *true_res = std::sqrt(init_dot);
    if (init_dot == 0.0) return SGPU_OK;                           // u = 0 is the solution
    if (!std::isfinite(init_dot)) return fail(SGPU_ERR_NOCONV, "solve_FGMRES: non-finite residual at iteration 0");   // u = 0, nothing more is launched
    const double thr = init_dot * h->prm.solver_tol * h->prm.solver_tol;
    std::vector<double> H((size_t)(m + 1) * m, 0.0), cs((size_t)m), sn((size_t)m), gv((size_t)m + 1), y((size_t)m);
    double cur_dot = init_dot;
    int k = 0;
    bool conv = false;
    while (k < max_iter) {
        CHK(gs_scale(G.coef, V, V, sz));                           // v_0 = r / ||r||  (coef[0] holds r . r)
        std::fill(gv.begin(), gv.end(), 0.0);
        gv[0] = std::sqrt(cur_dot);
        int jj = 0;                                                // columns of this cycle
        bool est_conv = false;
        for (int j = 0; j < m && k < max_iter; ++j) {
            double *vj = V + (size_t)j * ld, *w = V + (size_t)(j + 1) * ld;
            if (precond) {
                CHK(sgpu_vec_copy(G.pin, vj, sz));
                CHK(gmres_precondition(h, G));
                CHK(sgpu_spmv(A, G.pout, w));
                CHK(sgpu_vec_copy(G.Z + (size_t)j * ld, G.pout, sz));
            } else {
                CHK(sgpu_spmv(A, vj, w));
            }
            const int nc = j + 1;
            double *h1 = G.coef, *h2 = G.coef + nc, *nrm = G.coef + 2 * nc;
            CHK(gs_dots(V, ld, nc, w, sz, G.partials, h1));
            CHK(gs_update(V, ld, nc, h1, w, sz, G.partials, nullptr));
            CHK(gs_dots(V, ld, nc, w, sz, G.partials, h2));
            CHK(gs_update(V, ld, nc, h2, w, sz, G.partials, nrm));
            CHK(fetch(G.coef, 2 * nc + 1));
            const double nrm2 = G.hcoef[2 * nc];
            double *hc = H.data() + (size_t)j * (m + 1);
            for (int i = 0; i < nc; ++i) hc[i] = G.hcoef[i] + G.hcoef[nc + i];
            hc[nc] = std::sqrt(nrm2);
            for (int i = 0; i < j; ++i) {
                const double t = cs[i] * hc[i] + sn[i] * hc[i + 1];
                hc[i + 1] = cs[i] * hc[i + 1] - sn[i] * hc[i];
                hc[i] = t;
            }
            const double d = std::sqrt(hc[j] * hc[j] + hc[j + 1] * hc[j + 1]);
            if (!(d > 0.0) || !std::isfinite(d)) {
                if (iters) *iters = k;
                return fail(SGPU_ERR_NOCONV, "solve_FGMRES: breakdown at iteration %d (a Hessenberg column of norm %g): the operator or the preconditioner is singular on the Krylov space", k + 1, d);
            }
            cs[j] = hc[j] / d; sn[j] = hc[j + 1] / d;
            hc[j] = d; hc[j + 1] = 0.0;
            gv[j + 1] = -(sn[j] * gv[j]);
            gv[j] = cs[j] * gv[j];
            ++k; jj = j + 1;
            if (hist && k < cap) hist[k] = std::fabs(gv[j + 1]);
            if (gv[j + 1] * gv[j + 1] < thr) { est_conv = true; break; }   // tested before v_{j+1} is formed: a vanishing ||w|| here never divides
            if (j + 1 == m || k == max_iter) break;
            if (!(nrm2 > 0.0)) {
                if (iters) *iters = k;
                return fail(SGPU_ERR_NOCONV, "solve_FGMRES: ||w|| = 0 at iteration %d without convergence (estimate %g, threshold %g)", k, std::fabs(gv[j + 1]), std::sqrt(thr));
            }
            CHK(gs_scale(nrm, w, w, sz));                          // v_{j+1} = w / ||w||
        }
        (void)est_conv;
        for (int i = jj - 1; i >= 0; --i) {                        // R y = g
            double s = gv[i];
            for (int c = i + 1; c < jj; ++c) s -= H[(size_t)c * (m + 1) + i] * y[c];
            y[i] = s / H[(size_t)i * (m + 1) + i];
        }
        for (int i = 0; i < jj; ++i) G.hcoef[i] = -y[i];           // u += Z y is the update with negated coefficients
        HIPCHK(hipMemcpyAsync(G.coef, G.hcoef, (size_t)jj * sizeof(double), hipMemcpyHostToDevice, g.cs));
        CHK(gs_update(Zp, ld, jj, G.coef, u, sz, G.partials, nullptr));
        CHK(sgpu_residual_negative(A, u, rhs, V));                 // r = rhs - A u, recomputed
        CHK(gs_dots(V, ld, 1, V, sz, G.partials, G.coef));
        CHK(fetch(G.coef, 1));
        cur_dot = G.hcoef[0];
        if (true_res) *true_res = std::sqrt(cur_dot);
        if (cur_dot < thr) { conv = true; break; }                 // the estimate alone never ends the solve: another cycle starts
        if (!std::isfinite(cur_dot)) break;
    }
    if (iters) *iters = k;
    return conv ? SGPU_OK : SGPU_ERR_NOCONV;
}

} // extern "C"
