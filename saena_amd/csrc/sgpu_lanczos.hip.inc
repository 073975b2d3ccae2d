// sgpu_lanczos.hip.inc -- sgpu_op_eig_max (include/saena_gpu.h): the Chebyshev eigenvalue estimate of the host setup
// (amg_hierarchy::find_eig, host/amg_setup.cpp) with its recurrence on the device, and the hook that lets the one-rank setup and
// update1 / update2 take their estimates from it.  Part of sgpu_runtime.hip; kernels: kernels_lanczos.hip.h.
//
// What is restated here is the loop of find_eig and nothing else: the start vector and the tridiagonal eigenvalue are the host's own
// functions (lanczos_start_vector, lanczos_ritz_max), the product is the operator's current form through apply().  Nothing of the
// operator is touched that a plain sgpu_spmv does not touch: no plan, no plan-cache entry, no x-window mode, no captured graph.
// The scratch -- v, vprev, w, t, isd, two scalars and the partial sums -- is ONE allocation owned by the call; the solver's scalar
// slots and partial sums (g.dscalar, g.partials) are not written.  One host synchronisation per step: the host needs a and b for the
// tridiagonal matrix and takes find_eig's early exit on b.
namespace {

int lanczos_eig_max(sgpu_op *op, int steps, double *eig_max) {
    const size_t n = (size_t)op->M, ld = (n + 1) & ~(size_t)1;           // every vector starts on a 16-byte boundary
    const int m = (int)std::min<size_t>((size_t)steps, n), nb = dot_nblocks(n), nb2 = gs_nblocks(n);
    std::vector<double> start(n), alpha, beta;                            // (declared first: outlives the device arrays an upload may still read it for)
    DevArr<double> scratch;                                               // freed on every return below
    PinArr<double> hs;
    if (scratch.alloc(5 * ld + 2 + (size_t)g.n_partials) != hipSuccess) return fail(SGPU_ERR_NOMEM, "op_eig_max: hipMalloc of %zu doubles failed", 5 * ld + 2 + (size_t)g.n_partials);
    if (hs.alloc(2) != hipSuccess) return fail(SGPU_ERR_NOMEM, "op_eig_max: hipHostMalloc failed");
    double *v = scratch, *vprev = v + ld, *w = vprev + ld, *t = w + ld, *isd = t + ld, *S = isd + ld, *partials = S + 2;
    saena_host::lanczos_start_vector((index_t)n, start.data());
    HIPCHK(hipMemsetAsync(scratch, 0, scratch.bytes(), g.cs));           // vprev = 0
    HIPCHK(hipMemcpyAsync(v, start.data(), n * sizeof(double), hipMemcpyHostToDevice, g.cs));
    SGPU_LAUNCH(sk::k_lz_start, dim3(nb2), dim3(sk::BLOCK), 0, g.cs, (const double *)op->inv_diag, (const double *)v, isd, t, n);
    HIPCHK(hipGetLastError());
    double b = 0.0;
    for (int k = 0; k < m; ++k) {
        CHK(apply(op, sk::EPI_SPMV, t, w, EpiArgs()));                                                       // w = A (isd .* v)
        SGPU_LAUNCH(sk::k_lz_scale_dot, dim3(nb), dim3(sk::BLOCK), 0, g.cs, (const double *)isd, (const double *)v, w, n, partials);
        SGPU_LAUNCH(sk::k_reduce_partials, dim3(1), dim3(sk::BLOCK), 0, g.cs, (const double *)partials, nb, S);           // a = w . v
        SGPU_LAUNCH(sk::k_lz_update_dot, dim3(nb), dim3(sk::BLOCK), 0, g.cs, (const double *)S, b, (const double *)v, (const double *)vprev, w, n, partials);
        SGPU_LAUNCH(sk::k_reduce_partials, dim3(1), dim3(sk::BLOCK), 0, g.cs, (const double *)partials, nb, S + 1);       // w . w
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(hs, S, 2 * sizeof(double), hipMemcpyDeviceToHost, g.cs));
        HIPCHK(hipStreamSynchronize(g.cs));
        alpha.push_back(hs[0]);
        b = std::sqrt(hs[1]);
        if (k + 1 < m) beta.push_back(b);
        if (b < 1e-300 || k + 1 == m) break;
        SGPU_LAUNCH(sk::k_lz_shift, dim3(nb2), dim3(sk::BLOCK), 0, g.cs, (const double *)w, b, (const double *)isd, vprev, t, n);   // v_next into vprev's buffer
        HIPCHK(hipGetLastError());
        std::swap(v, vprev);                                                                                  // vprev <- v, v <- v_next
    }
    *eig_max = saena_host::lanczos_ritz_max(alpha, beta);
    return SGPU_OK;
}

// saena_host::g_eig_hook: a temporary one-rank operator on the heuristic plan (no autotune, no plan-cache entry), the estimate, destroy
int gpu_eig_hook(int n, const long *ptr, const int *col, const double *val, const double *inv_diag, int steps, double *eig_max) {
    if (!g.live || g.nranks > 1 || n <= 0 || !ptr || !inv_diag || !eig_max || ptr[n] >= INT32_MAX) return 1;
    std::vector<index_t> npr((size_t)n);
    for (int i = 0; i < n; ++i) npr[(size_t)i] = (index_t)(ptr[i + 1] - ptr[i]);
    sgpu_op_desc d = {};
    d.M = n; d.N_local = n; d.col_offset = 0;
    d.nnz_l_local = ptr[n]; d.nnzPerRow_local = npr.data(); d.col_local = col; d.val_local = val;
    d.inv_diag = inv_diag;
    sgpu_op *op = nullptr;
    if (sgpu_op_create(&d, &op) != SGPU_OK) return 1;
    const int st = sgpu_op_eig_max(op, steps, eig_max);
    sgpu_op_destroy(op);
    return st == SGPU_OK ? 0 : 1;
}

bool g_debug_capture_open = false;

} // namespace

extern "C" {

void sgpu_install_eig_hook(int on) { saena_host::g_eig_hook = on ? &gpu_eig_hook : nullptr; }

int sgpu_op_eig_max(sgpu_op *op, int steps, value_t *eig_max) {
    CHK(need_ctx());
    if (!op || !eig_max) return fail(SGPU_ERR_ARG, "op_eig_max: null argument");
    if (steps < 0 || steps > 64) return fail(SGPU_ERR_ARG, "op_eig_max: the number of Lanczos steps must be in 1..64, or 0 for the default of 20 (got %d)", steps);
    if (op->M == 0) return fail(SGPU_ERR_ARG, "op_eig_max: the operator has no rows (M == 0)");
    if (op->has_remote || op->recvSize || op->vIndexSize)
        return fail(SGPU_ERR_ARG, "op_eig_max: the operator has a remote part (%d halo entries, %d sent); the estimate takes single-rank operators only", op->recvSize, op->vIndexSize);
    if (g.nranks > 1) return fail(SGPU_ERR_ARG, "op_eig_max: runs on one rank only (this context has %d)", g.nranks);
    if (op->M != op->N_local) return fail(SGPU_ERR_ARG, "op_eig_max: the operator is not square (%d rows, %d columns)", op->M, op->N_local);
    if (!op->inv_diag) return fail(SGPU_ERR_ARG, "op_eig_max: the operator has no inv_diag");
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    HIPCHK(hipStreamIsCapturing(g.cs, &cap));
    if (cap != hipStreamCaptureStatusNone) return fail(SGPU_ERR_ARG, "op_eig_max: a capture is open on the compute stream (the estimate synchronises once per step)");
    return lanczos_eig_max(op, steps == 0 ? 20 : steps, eig_max);
}

// tests (include/saena_gpu_debug.h): open / close an empty capture on the compute stream
int sgpu_debug_capture(int begin) {
    CHK(need_ctx());
    if (begin) {
        if (g_debug_capture_open) return fail(SGPU_ERR_STATE, "debug_capture: a capture is already open");
        HIPCHK(hipStreamBeginCapture(g.cs, hipStreamCaptureModeThreadLocal));
        g_debug_capture_open = true;
        return SGPU_OK;
    }
    if (!g_debug_capture_open) return fail(SGPU_ERR_STATE, "debug_capture: no capture is open");
    g_debug_capture_open = false;
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamEndCapture(g.cs, &graph));
    if (graph) HIPCHK(hipGraphDestroy(graph));
    return SGPU_OK;
}

} // extern "C"
