// dense_eig.h -- the small dense problems of the Rayleigh-Ritz step of sgpu_eigs_LOBPCG (order <= 3 K = 24): Cholesky with a
// relative pivot test, cyclic Jacobi for the symmetric eigenproblem, and the generalised symmetric problem A v = w B v through
// L^-1 A L^-T.  No LAPACK.  Matrices are row-major, n x n, M[i * n + j]; only symmetric input makes sense (the callers symmetrise).
#pragma once

namespace saena_host {

constexpr int DENSE_EIG_MAXN = 24;
constexpr int JACOBI_MAX_SWEEPS = 30;

// A = L L^T, L lower triangular (its upper part is zeroed).  A pivot d_j = a_jj - sum_k l_jk^2 must exceed
// 256 n eps a_jj: column j then stands out of the span of the columns before it by more than rounding can fake.  -> false when
// a pivot does not (A is not numerically positive definite; L is left half written), or a diagonal entry is not positive / finite.
bool dense_cholesky(int n, const double *A, double *L);

// T = L^-T (upper triangular, the lower part zeroed): the columns of X T are orthonormal when L is the Cholesky factor of X^T X
void dense_inv_lower_transposed(int n, const double *L, double *T);

// eigenvalues ascending in w[n], eigenvectors orthonormal in the columns of V (V[i * n + k] = component i of vector k).
// Cyclic Jacobi by rows, until every off-diagonal entry is below eps sqrt(|a_ii a_jj|)-scale rounding.  -> sweeps used,
// -1 if JACOBI_MAX_SWEEPS did not suffice or an entry is not finite.  A is read only.
int dense_sym_eig(int n, const double *A, double *w, double *V);

// A v = w B v: w ascending, V^T B V = I.  -> sweeps of the Jacobi iteration (>= 0), -1 if B is not numerically positive definite,
// -2 if the Jacobi iteration failed, -3 if n is outside 1 .. DENSE_EIG_MAXN
int dense_sym_geig(int n, const double *A, const double *B, double *w, double *V);

} // namespace saena_host
