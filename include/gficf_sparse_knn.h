/* gficf_sparse_knn.h — C ABI of libgficf_sparse_knn.so: the exact k-nearest-neighbour search over the sparse cells of a
 * GF-ICF matrix on the MI355X (gfx950).  It is what the data$pca-less branch of the reference's runReduction needs
 * (R/dimensinalityReduction.R:179-187 embeds t(data$gficf) directly): every other search of the library is dense with d <= 128
 * (gficf_knn_dpad), and a cell of a GF-ICF matrix is a sparse vector in thousands of genes.
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links and nothing else: it takes that library's gficf_ctx and
 * uses its stream, device scratch, status codes, metrics (gficf_knn_metric), GFICF_KNN_MAX_K and gficf_last_error().  The core
 * ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * INPUT.  M, genes x cells (G x N), CSC: the column pointer int64 on the device (int32 or int64 at the host entry), row ids
 * int32, STRICTLY ascending within a column, values f64.  OUTPUT.  The table of gficf_knn_host: idx, n_q x k int32, 1-based,
 * column-major with leading dimension ld_out, and dist alike in f64: for every query cell the k smallest (key, id) pairs over
 * ALL N cells, the query itself included, ties broken by the smaller id.
 *
 * CONTRACT.  The contract is the method below.  The values are rounded to f32 once, in a prepare pass.  Every distance is a
 * function of ONE sum over the genes both cells store, plus per-cell scalars of the prepare pass (G: the number of genes):
 *
 *   metric       pair sum over the shared genes      distance
 *   euclidean    S = sum a b                         sqrt(max(0, na + nb - 2 S)),                 na = sum a^2
 *   manhattan    T = sum (|a| + |b| - |a - b|)       max(0, la + lb - T),                         la = sum |a|
 *   cosine       S                                   1 - S / (sqrt(na) sqrt(nb));  1 when either norm is 0
 *   correlation  S                                   1 - (S - G ma mb) / (sqrt(na - G ma^2) sqrt(nb - G mb^2)),   ma = sum a / G;
 *                                                    1 when either centred norm is 0
 *
 *   - The pair sums and the per-cell scalars are accumulated in f64 from the f32 values, every operation rounded as written.
 *     A product of two f32 values is exact in f64, so S += a b takes one rounding whether the kernel fuses it or not (it does:
 *     one multiply-add instruction); nothing else is fused.
 *   - The summation order is fixed and there are no floating-point atomics.  A sum over the stored entries e = 0, 1, ... of a
 *     column runs in GFICF_SPARSE_KNN_LANES chains, chain l adding the entries l, l + LANES, l + 2 LANES, ... in order, and
 *     the chains are added in a fixed tree (chain l with chain l ^ 8, then ^ 4, ^ 2, ^ 1).  The pair sum of (query, candidate)
 *     runs over the CANDIDATE's stored entries against the query's values (0 where the query stores nothing, which adds an
 *     exact 0); it does not depend on the tile the query is in nor on the slice the candidate is in.
 *   - The distance is formed in f64; cosine and correlation are then clamped at 0 from below (Cauchy-Schwarz bounds them there
 *     in exact arithmetic; rounding alone takes the distance of two identical cells to -1e-16), and the result is rounded once
 *     to f32 for the key  sortable(d) << 32 | id  (sortable: the order-preserving map of the f32 bits to uint32).
 *   - The pair (i, i) gets the key of the distance 0 without arithmetic: a self distance computed as 1 - S / (r r) is 1e-16,
 *     not 0, and that noise, not the neighbours, would otherwise decide column 0.
 *   - The k smallest of a set of distinct keys is unique: the order in which the waves of a workgroup hand candidates to a
 *     query's list varies between runs, the result does not.  The same input gives the same bits on every call, and the
 *     ranges [0, a) and [a, N) give the bits of [0, N).
 *   dist holds the f32 value of the key, widened.
 *
 * KERNELS.  (1) prepare: one 16-lane group per cell: the f32 copy of the values, na, la and sum a of the cell, and the deferred
 * checks.  (2) tiles: a workgroup holds a tile of TQ query cells as a dense f32 [G][TQ] array in LDS (zero-filled, scattered
 * from their columns) and streams the candidate columns of its slice through once: a 16-lane group per candidate reads its
 * (row, value) pairs coalesced (several entries of a chain ahead of their use; the adds stay in order), gathers the TQ query values of that gene from LDS, keeps TQ f64 sums, reduces them across its
 * lanes; only a candidate that beats a query's current k-th key reaches that query's list (kept sorted in LDS by one wave).
 * TQ is the largest of {8, 4, 2, 1} with G * TQ <= GFICF_SPARSE_KNN_LDS_FLOATS (128 KiB of the 160 KiB of a CU; the lists
 * and the hand-over slots take the rest), so G <= GFICF_SPARSE_KNN_LDS_FLOATS: more genes are GFICF_ERR_UNSUPPORTED.  The
 * candidates are cut into `slices` equal ranges when ceil(N / TQ) workgroups would not fill the chip.  (3) merge: one wave per
 * query merges the slices' lists and writes the table.  gficf_sparse_knn_shape states TQ, slices and the gene limit.
 *
 * Limits: 1 <= k <= min(GFICF_KNN_MAX_K, N) (k > GFICF_KNN_MAX_K: GFICF_ERR_UNSUPPORTED; k > N: GFICF_ERR_INVALID_ARG, as in
 * gficf_knn_host), N < 2^31.  Deferred (the status word at the head of the workspace, collected by gficf_sparse_knn_sync): a
 * row id outside [0, G) or not strictly ascending within its column, or a column pointer that decreases or leaves [0, nnz], is
 * GFICF_ERR_BAD_CSC; a non-finite value (after the rounding to f32) is GFICF_ERR_BAD_VALUE.  The kernels read and write
 * inside their buffers whatever the input holds; the table of such a call is not meaningful. */
#ifndef GFICF_SPARSE_KNN_H
#define GFICF_SPARSE_KNN_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_SPARSE_KNN_ABI_VERSION 1
#define GFICF_SPARSE_KNN_LANES 16
#define GFICF_SPARSE_KNN_LDS_FLOATS 32768

int gficf_sparse_knn_abi_version(void);

/* The decomposition for G genes, N cells and k neighbours, a host query: tile_queries (TQ), slices, and max_genes (the
 * largest G the search takes, whatever G is).  G > max_genes: GFICF_ERR_UNSUPPORTED, with max_genes still written. */
int gficf_sparse_knn_shape(int64_t G, int64_t N, int k, int* tile_queries, int* slices, int64_t* max_genes);

/* Bytes of device scratch of gficf_sparse_knn_device for n_queries = q_end - q_begin; 0 on arguments it would refuse. */
size_t gficf_sparse_knn_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int k, int64_t n_queries);

/* Device form: the queries [q_begin, q_end) against all N cells.  d_idx (and d_dist, which may be NULL): n_q x k column-major
 * with leading dimension ld_out >= n_q.  Only enqueues, on the context's stream. */
int gficf_sparse_knn_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                            int64_t nnz, int k, int metric, int64_t q_begin, int64_t q_end, void* ws, size_t ws_bytes, int32_t* d_idx,
                            double* d_dist, int64_t ld_out);
/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_sparse_knn_sync(gficf_ctx* ctx, const void* ws);
/* Host form, shaped like gficf_knn_host: colptr int32 or int64 (colptr_is_i64); idx N x k column-major int32 (1-based), dist
 * N x k column-major doubles or NULL. */
int gficf_sparse_knn_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                          const double* x, int k, int metric, int32_t* idx, double* dist);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_SPARSE_KNN_H */
