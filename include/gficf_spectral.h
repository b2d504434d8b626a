/* gficf_spectral.h — C ABI of libgficf_spectral.so: the connected components of a device-resident CSR graph and the leading
 * eigenvectors of its normalised Laplacian (uwot's init = "spectral" / "normlaplacian", the default start of uwot::umap and
 * uwot::tumap, which runReduction of the reference calls) on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device pool, status codes and gficf_last_error().  The core ABI is not changed.  The graph is the one
 * gficf_umap_graph_device (include/gficf_umap.h) leaves on the device: rowptr int64 (N + 1), col int32 0-based, val f32.
 *
 * 1. COMPONENTS.  An entry (i, j) joins i and j whether or not (j, i) is stored.  labels[i] is the SMALLEST vertex id of i's
 *    component, which makes the answer unique.  Scheme: hook and pointer-jump (Shiloach-Vishkin with full shortcutting).
 *    parent[i] = i; a round is (a) hook: every entry (u, w) with parent[u] != parent[w] does atomicMin(parent[max], min) on the
 *    two parents (integer: the fixed point does not depend on the order), (b) jump: parent[i] = the root of i's tree.  At the
 *    start of a round every tree is a star, so every root with a neighbouring tree of smaller root is hooked: on a path the
 *    trees at least halve per round (a min-label sweep would need N rounds).  The entry reads one "changed" word back per
 *    round and stops after the first round that hooked nothing.  info = {number of components, rounds}.
 *    A row pointer that does not start at 0, decreases or leaves [0, capacity] is GFICF_ERR_BAD_CSC, a column outside [0, N)
 *    GFICF_ERR_BAD_ID: both are found by a checking launch before any entry is followed, and returned by the entry itself
 *    (it synchronises; there is no deferred status here).
 *
 * 2. EIGEN-SOLVE.  Operator S = D^-1/2 P D^-1/2, P the f32 CSR graph taken as SYMMETRIC (P of gficf_umap_graph_device is, bit
 *    for bit), d_i = the sum of row i in f64 in column order, q0 = sqrt(d) / |sqrt(d)| its eigenvector at eigenvalue 1.  The
 *    entry returns the ndim eigenpairs of S with the largest eigenvalues theta in the complement of q0; the eigenvalues of the
 *    normalised Laplacian I - S are 1 - theta.  A value of P that is not positive and finite is GFICF_ERR_BAD_VALUE.
 *    The components are found first.  More than one (a zero-degree vertex is one of its own, and is never divided by): the
 *    entry returns GFICF_OK with info[0] = the count, info[1 .. 3] = 0, and leaves theta, residuals and vectors UNTOUCHED.
 *
 *    Method: a block Krylov subspace in f64 with block size b = ndim, full reorthogonalisation, Rayleigh-Ritz, thick restart.
 *      basis   V, at most mc = min(m, N - 1) orthonormal columns, all orthogonal to q0 (m: default 32, at most 64);
 *      block   W = S V_j for the newest block V_j; W is projected against q0 and every column of V, TWICE (c = [q0 V]' W,
 *              W -= [q0 V] c); the sums of the two coefficient sets are column block j of H = V' S V (its other triangle is
 *              taken by symmetry); then W is orthonormalised within itself, twice, through its b x b Gram matrix (G = W' W,
 *              Gram-Schmidt in the G inner product in a one-lane kernel, W <- W T) and becomes V_{j+1}.  A block is narrower
 *              than b only where the basis is capped by N - 1 (see cycle).  A column whose squared norm after the projection is
 *              <= 1e-24 x the one before it, or whose pivot is <= 1e-12 x its own squared norm, is DROPPED (a zero column,
 *              flagged): the Krylov space is exhausted there.  Dropped columns are left out of H on the host.
 *      cycle   ends when no further block fits.  Capped by m (mc = m < N - 1): at the last FULL block, so a cycle holds me <= mc
 *              columns, me = keep + b floor((mc - keep) / b) (keep = 0 in the first), and the columns past me stay unused: no
 *              column of a remainder is ever discarded, S V - V H stays confined to W_last, and the estimate and the restart
 *              block below are the true residuals.  (A narrower last block there discards b - bw columns of the remainder
 *              before it; the estimate is then too small and the iteration stalls: at ndim 3, m 32 at a relative residual
 *              of 9e-3.)  Capped by N - 1 (mc = N - 1 <= m): the last block takes the mc - nc < b columns that are left; the
 *              complement of q0 is exhausted, the columns left out are dependent, me = mc.  For ndim 1, and for ndim 2 with an
 *              even m, me = mc in every cycle.  Everything below reads me for the number of columns.
 *              The remainder W_last of the last block (projected, not normalised) stays, with its Gram
 *              matrix G_last.  ONE synchronisation per cycle: H, the flags and G_last are read back (8 KB + 0.8 KB at m = 32).
 *              The host solves H = Z diag(theta) Z' (cyclic Jacobi, fixed sweep order, theta descending).  The residual of
 *              Ritz pair l is W_last z_l (z_l: the rows of Z of the last block), its norm sqrt(z_l' G_last z_l).
 *      restart V <- V Z[:, :keep], keep = ndim + 2 (fewer if fewer columns live); the next block is the residuals
 *              W_last Z_last[:, :b] of the leading b pairs, projected and orthonormalised as above.  The kept columns are the
 *              leading keep Ritz vectors, except where a restarted cycle has room for ONE block only (mc - keep < 2 b, as at
 *              m = 2 ndim + 2): there, from the second restart on, the two beyond the leading b are the Ritz vectors l >= b
 *              with the largest sum over i < b of Z[i, l]^2 (the lowest l on ties; kept in ascending l), i.e. those that
 *              carry most of the previous cycle's leading b vectors.  Any set of Ritz vectors keeps S V - V H inside W_last;
 *              this set keeps the direction of the last step, the locally optimal recurrence of LOBPCG.  With the next
 *              Ritz pairs instead, a one-block cycle is a gradient step (connected blobs, ndim 3, m 8: 306 restarts, with
 *              this rule 70).
 *      stop    when the estimate of each of the leading ndim pairs is <= tol max(|theta|, eps^(2/3)) (eps = 2^-52), or after
 *              max_restarts restarts.  Then X = V Z[:, :ndim], each column signed so that its largest-magnitude entry is
 *              positive (lowest index on ties), and the residuals are RECOMPUTED from one more multiplication: the reported
 *              norms are |S x - theta x|_2, and converged = 1 iff each of them meets the bound.  (If the recomputed ones miss it
 *              although the estimate did not, and restarts remain, the iteration goes on.)
 *    Defaults of the mirror: tol = 1e-4 (uwot's), m = 32, max_restarts = 200.
 *    The block size is what returns a doubly degenerate eigenvalue as a plane: on a ring a single-vector Lanczos returns one
 *    vector of the top plane and then one of the next.
 *    Launches: degree (one lane per row), S x block (8 lanes per row, rows longer than 256 entries by a whole wave from a hub
 *    list; the block is row-interleaved and pre-scaled by d^-1/2, so a neighbour costs one load of b doubles), the tall-skinny
 *    products [q0 V]' W over 128 fixed row chunks and their fixed-order sum, W -= [q0 V] c, the b x b kernel, W <- W T, and
 *    the rotation V <- V Z.
 *    Determinism: no floating-point atomics; every dot product and norm is added over fixed chunks in a fixed order; a row's
 *    sum by a fixed lane pattern.  The same input gives the same bits on every call.
 *    Differences from uwot: RSpectra's solver is a single-vector implicitly restarted Lanczos with its own random start;
 *    here the block form above, and the start block is an INPUT (N x ndim f64 row-major), as Omega is for gficf_rsvd_*.
 *
 * Arguments: N < 1, a negative capacity or a NULL pointer is GFICF_ERR_INVALID_ARG; for the solve also N <= ndim, ndim
 * outside [1, GFICF_SPECTRAL_MAX_NDIM], m < 2 ndim + 2 or m > GFICF_SPECTRAL_MAX_M, tol not positive and finite, max_restarts < 0,
 * N >= 2^31.  A workspace that is too small is GFICF_ERR_CAPACITY. */
#ifndef GFICF_SPECTRAL_H
#define GFICF_SPECTRAL_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_SPECTRAL_ABI_VERSION 1
#define GFICF_SPECTRAL_MAX_NDIM 8
#define GFICF_SPECTRAL_MAX_M 64

int gficf_spectral_abi_version(void);

/* Components.  d_rowptr N + 1, d_col `capacity` entries of which d_rowptr[N] are in use; d_labels N int32; d_info two int64 on
 * the device: {components, rounds}.  Synchronises once per round. */
size_t gficf_graph_components_workspace_bytes(int64_t N);
int gficf_graph_components_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, int64_t capacity, int32_t* d_labels,
                                  int64_t* d_info, void* ws, size_t ws_bytes);

/* Eigen-solve.  d_start: N x ndim f64 row-major, read only.  Outputs on the device: d_theta and d_resid ndim f64 each,
 * d_vectors N x ndim f64 row-major (unit columns), d_info four int64: {components, restarts, multiplications by S, converged}.
 * Synchronises once per cycle, and once for the recomputed residuals. */
size_t gficf_spectral_workspace_bytes(int64_t N, int64_t capacity, int ndim, int m);
int gficf_spectral_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity, int ndim,
                          const double* d_start, double tol, int m, int max_restarts, void* ws, size_t ws_bytes, double* d_theta, double* d_resid,
                          double* d_vectors, int64_t* d_info);

/* Host form: CSR in host memory (nnz = rowptr[N] entries).  Components first; the solve only when there is one.  labels: N
 * int32 or NULL; info as above, its four int64 in host memory; theta, resid, vectors untouched when info[0] > 1. */
int gficf_spectral_host(gficf_ctx* ctx, int64_t N, const int64_t* rowptr, const int32_t* col, const float* val, int ndim, const double* start,
                        double tol, int m, int max_restarts, int32_t* labels, double* theta, double* resid, double* vectors, int64_t* info);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_SPECTRAL_H */
