/* gficf_pca.h — C ABI of libgficf_pca.so: runPCA / runLSA / computePCADim of the reference (R/dimensinalityReduction.R:19-133,
 * 206-230, through rsvd::rpca / rsvd::rsvd) and the projection of embedNewCells (R/cellClassifier.R:50-64): the randomized SVD
 * of the GF-ICF matrix on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, transpose, scan, status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * RELAXED CONTRACT.  The algorithm is the Halko / Martinsson / Tropp randomized SVD as rsvd runs it; the contract is the
 * algorithm, not rsvd's bits.  A is the cells x genes matrix t(gficf), N x G, handed over as the genes x cells CSC matrix that
 * gficf() returns.  The work runs on the orientation with rows >= columns (A when N >= G, its transpose otherwise, as rsvd
 * does); n = min(N, G), l = k + p (rsvd: p = 10), q power iterations (rsvd: 2).  The test matrix Omega (n x l, column-major
 * f64) is an INPUT: the library holds no random number generator and the result is a function of the arguments.
 *     Y = A Omega;  q times: Y = orth(Y), Z = A' Y, Z = orth(Z), Y = A Z;  Q = orth(Y);  B' = A' Q (n x l);
 *     B = W diag(d) V';  U = Q W;  the k leading components are kept.
 * Outputs: d (k singular values, descending), genes = V (G x k), cells = U diag(d) (N x k: what runLSA forms and what rpca's
 * x holds); when the orientation was transposed the roles of U and V are swapped back.
 *   - orth and the final SVD go through the l x l Gram matrix and a symmetric eigen-solve on the device (parallel cyclic
 *     Jacobi, one workgroup): orth forms S = Y'Y = W L W' and sets Y <- Y W L^(-1/2), twice; the SVD of B takes d^2 and W from
 *     B B' and V = B' W diag(1/d).
 *   - Directions with lambda <= tau * lambda_max are dropped: their columns become zero and their d becomes 0, so a matrix of
 *     rank < l gives finite output.  tau = max(m, 1024) * 2^-52 for a Gram matrix over m rows: the worst-case rounding error
 *     of an m-term f64 dot product relative to lambda_max, and never below what the Jacobi sweeps themselves leave at l = 128.
 *   - centre != 0 never densifies: mu = the per-gene mean over the cells, (A - 1 mu')X = AX - 1 (mu'X) and
 *     (A - 1 mu')'Y = A'Y - mu (1'Y) as rank-one corrections; mu is returned for later projection.
 *   - sign rule: every component is signed so that the entry of largest magnitude of its genes column is positive (the first
 *     such entry on ties).
 *   - no floating-point atomics anywhere: columns are cut into fixed segments whose partial rows are added in a fixed order,
 *     Gram matrices and column sums are summed over fixed chunks in order.  The same input gives the same bits on every call.
 * Limits: 1 <= k <= l <= min(128, N, G), q >= 0 (GFICF_ERR_INVALID_ARG otherwise); a workspace that is too small is
 * GFICF_ERR_CAPACITY.  Deferred (through the status word at the head of the workspace, collected by gficf_rsvd_sync): a
 * non-finite value in x, Omega, X or Y is GFICF_ERR_BAD_VALUE; a row index out of range or a bad column pointer is
 * GFICF_ERR_BAD_CSC.  Matrices are column-major f64 at this boundary. */
#ifndef GFICF_PCA_H
#define GFICF_PCA_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_PCA_ABI_VERSION 1
#define GFICF_PCA_MAX_L 128

int gficf_pca_abi_version(void);

/* Y = A'X for the CSC matrix A (nrows x ncols; d_colptr: ncols + 1 int64, d_rowidx / d_x: nnz entries): X is nrows x l, Y is
 * ncols x l, 1 <= l <= 128.  The building block of the decomposition (both directions: on the genes x cells matrix and on its
 * transpose) and of the projection.  Only enqueues; gficf_rsvd_sync(ctx, ws) waits and collects the deferred errors. */
size_t gficf_csc_tmm_workspace_bytes(int64_t nrows, int64_t ncols, int64_t nnz, int l);
int gficf_csc_tmm_device(gficf_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                         int64_t nnz, const double* d_X, int l, void* ws, size_t ws_bytes, double* d_Y);
int gficf_csc_tmm_host(gficf_ctx* ctx, int64_t nrows, int64_t ncols, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                       const double* x, const double* X, int l, double* Y);

/* orth alone, in place on the m x l matrix d_Y (m >= l, 1 <= l <= 128): an orthonormal basis of its column range, the columns
 * of dropped directions zero (they come last: the columns are ordered by decreasing eigenvalue of the second pass). */
size_t gficf_orthonormalize_workspace_bytes(int64_t m, int l);
int gficf_orthonormalize_device(gficf_ctx* ctx, int64_t m, int l, double* d_Y, void* ws, size_t ws_bytes);

/* The decomposition.  Device form: the genes x cells CSC matrix as in gficf_cluster_markers_device, d_omega min(N, G) x l,
 * d_d k values, d_cells N x k, d_genes G x k, d_centre G values (mu; written only when centre != 0, may be NULL otherwise).
 * Only enqueues on the context's stream, no synchronisation inside. */
size_t gficf_rsvd_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int l);
int gficf_rsvd_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                      int centre, const double* d_omega, int k, int l, int q, void* ws, size_t ws_bytes, double* d_d, double* d_cells,
                      double* d_genes, double* d_centre);
/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws (a workspace of any *_device entry above). */
int gficf_rsvd_sync(gficf_ctx* ctx, const void* ws);
/* Host form, shaped like gficf_cluster_markers_host: colptr int32 or int64 (colptr_is_i64). */
int gficf_rsvd_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                    int centre, const double* omega, int k, int l, int q, double* d, double* cells, double* genes, double* centre_out);

/* x %*% data$pca$genes of embedNewCells for a genes x new-cells GF-ICF matrix: out (n_new x k) = (t(x) - 1 mu') genes, genes
 * G x k, centre = mu (G values) or NULL for no centring. */
int gficf_pca_project_host(gficf_ctx* ctx, int64_t G, int64_t n_new, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                           const double* x, const double* genes, int k, const double* centre, double* out);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_PCA_H */
