/* gficf_svds.h — C ABI of libgficf_svds.so: the exact truncated SVD behind randomized = FALSE of runPCA / runLSA /
 * computePCADim (reference R/dimensinalityReduction.R:57,124,213,216: RSpectra::svds, rsvd::rpca(rand = FALSE)) on the MI355X
 * (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links and nothing else: it takes that library's gficf_ctx and
 * uses its stream, device scratch, transpose, scan, status codes and gficf_last_error().  The kernels of libgficf_pca.so
 * (Y = A'X, the rank-one centring, the Gram matrix, the one-workgroup eigen-solve, orth, the sign rule) are shared with it as
 * text; include/gficf_pca.h states them and tau.  The core ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * CONTRACT.  The contract is the method below, not RSpectra's bits.  A = t(M), N x G, is handed over as the genes x cells CSC
 * matrix M that gficf() returns.  At = A - 1 mu' when centre != 0 (mu: the per-gene mean over the cells) and A otherwise; it
 * is never densified: (A - 1 mu')X = AX - 1 (mu'X) and (A - 1 mu')'Y = A'Y - mu (1'Y), the rank-one corrections of
 * gficf_pca.h.  The work runs on the short side, n = min(N, G): the operator is C = At'At (G <= N) or At At' (N < G), applied
 * as two Y = A'X products, one over the matrix and one over its transposed copy (what RSpectra's svds does).
 *
 * Method: block Lanczos with full reorthogonalisation, Rayleigh-Ritz and thick restart, for the k largest eigenpairs of C.
 * Arguments: k, the block width b, the basis capacity m, tol, max_cycles and a start block (n x b, column-major f64).  The
 * start block is an INPUT: the library holds no random number generator and the result is a function of the arguments.
 *   start   Q = orth(start), its width bw = the directions orth keeps (orth of gficf_pca.h: Gram + Jacobi, twice).
 *   cycle   a cycle is a run of steps.  One step:
 *             - Q (orthonormal, bw columns) is appended to the basis V; |V| is its column count;
 *             - W = C Q;  sigma = max(sigma, the largest column norm of W) (a lower bound of ||C||);
 *             - P = V'W goes into the explicit projected matrix H = V'C V, both triangles (the block's own bw x bw corner as
 *               (P + P') / 2);
 *             - W <- W - V (V'W), twice, the sums over fixed chunks of rows added in order;  R = W;
 *             - the cycle ends here if |V| = n, if a next block of min(b, n - |V|) columns does not fit under m, or if the
 *               cycle has taken as many steps as it would with blocks of full width;
 *             - otherwise Q = orth(W), where the first pass also drops every direction whose norm is <= tau * sigma (what is
 *               left of W once V spans the range it lies in is rounding error of that size).  Dropped directions narrow the
 *               block; an empty block ends the cycle: the space is exhausted.
 *           A cycle never discards columns of a block to make it fit: the residual estimate below holds only then.
 *   Ritz    H = Z diag(theta) Z' by the eigen-solve of gficf_pca.h in one workgroup (|V| <= 128), descending; directions with
 *           theta_i <= tau * theta_1 are dropped (zero column of Z, theta_i = 0).  The residual of pair i is
 *           rho_i = ||R Z[rows of the last block, i]||, computed on the device, and pair i has converged when
 *           rho_i <= max(tol * theta_i, tau * theta_1).  tau = max(N, G, 1024) * 2^-52, the rounding bound of gficf_pca.h: below
 *           it the cross product cannot go in f64.
 *   stop    when the k leading pairs have converged, or the space is exhausted (|V| = n or an empty block), or after
 *           max_cycles cycles (or after the first when m = n: that cycle spans the whole space).
 *   restart nk = min(k + b, |V| - b) Ritz vectors are kept: V <- V Z[:, :nk], H <- diag(theta[:nk]),
 *           sigma = max(sigma, theta_1); the next block is R, projected against the kept vectors (twice) and
 *           orthonormalised as above.  Its coupling to the kept vectors enters H through the V'W of the next step.
 *   finish  V_k = V Z[:, :k], then V_k <- V_k (3 I - V_k'V_k) / 2, one Newton-Schulz step: the kept vectors are rotated at
 *           every restart and not orthonormalised again, and this takes their accumulated rounding drift out without
 *           turning them within their span;  T = At V_k (At' V_k when N < G) on the long side;  d_i = ||T[:, i]|| (the
 *           column norm, not sqrt(theta_i)).  G <= N: genes = V_k, cells = T (that is U diag(d)).  N < G: the roles are
 *           swapped back, genes = T / d, cells = V_k diag(d).  Dropped directions and positions beyond an exhausted space get
 *           d = 0 and zero columns (rsvd's rule for rank < l).  The sign rule is that of gficf_pca.h.
 * Outputs: d (k, descending up to rounding), cells (N x k), genes (G x k), centre (mu, G values, with centre != 0),
 * residuals (k values rho_i / theta_i, 0 where theta_i = 0) and info (4 x int64): cycles, products (applications of C, two
 * sparse products each), n_converged (of the k leading pairs), exhausted (0 / 1).  n_converged < k with exhausted == 0 means
 * max_cycles was reached: the result is the current Ritz approximation, and residuals says how far it is.
 *
 * Synchronisation: one read-back of 5 integers per cycle (the info block and the status word), and none besides; between two
 * read-backs gficf_svds_device only enqueues on the context's stream.  Block widths, |V| and nk live on the device.
 * Determinism: no floating-point atomics anywhere; every sum over rows runs over fixed chunks added in order.  The same input
 * gives the same bits on every call.
 * Limits: 1 <= b <= 32, b <= m <= min(128, N, G), 1 <= k <= m, and k + 2 b <= m unless m = min(N, G) (with m = n any k <= n is
 * allowed: the cycle spans the whole space); max_cycles >= 1; tol >= 0 — GFICF_ERR_INVALID_ARG otherwise.  A workspace that is
 * too small is GFICF_ERR_CAPACITY.  Deferred (through the status word at the head of the workspace, collected by
 * gficf_svds_sync; the cycles stop at the first read-back that sees it): a non-finite value in x or in start is
 * GFICF_ERR_BAD_VALUE; a row index out of range or a bad column pointer is GFICF_ERR_BAD_CSC.
 * Limitation: one block adds at most b directions to an eigenspace per step, so an eigenvalue of C with multiplicity above b
 * is returned at most b times.  Matrices are column-major f64 at this boundary. */
#ifndef GFICF_SVDS_H
#define GFICF_SVDS_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_SVDS_ABI_VERSION 1
#define GFICF_SVDS_MAX_B 32
#define GFICF_SVDS_MAX_M 128

int gficf_svds_abi_version(void);

/* Bytes of device scratch of gficf_svds_device; 0 on arguments it would refuse. */
size_t gficf_svds_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int k, int b, int m);

/* Device form: the genes x cells CSC matrix as in gficf_rsvd_device, d_start min(N, G) x b, d_d k values, d_cells N x k,
 * d_genes G x k, d_centre G values (written only when centre != 0, may be NULL otherwise), d_residuals k values, d_info 4 x
 * int64.  Only enqueues between the per-cycle read-backs, on the context's stream. */
int gficf_svds_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                      int centre, const double* d_start, int k, int b, int m, double tol, int max_cycles, void* ws, size_t ws_bytes,
                      double* d_d, double* d_cells, double* d_genes, double* d_centre, double* d_residuals, int64_t* d_info);
/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_svds_sync(gficf_ctx* ctx, const void* ws);
/* Host form, shaped like gficf_rsvd_host: colptr int32 or int64 (colptr_is_i64). */
int gficf_svds_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                    int centre, const double* start, int k, int b, int m, double tol, int max_cycles, double* d, double* cells,
                    double* genes, double* centre_out, double* residuals, int64_t* info);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_SVDS_H */
