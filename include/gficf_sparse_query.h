/* gficf_sparse_query.h — C ABI of libgficf_sparse_query.so: the exact k nearest TRAINING cells of every QUERY cell, both sparse
 * columns of GF-ICF matrices over the same genes, on the MI355X (gfx950).  It is the search behind embedding and classifying new
 * cells without PCA: what gficf_transform_search_device is to the dense cells of data$pca, this is to the sparse cells a model of
 * runReductionSparse was trained on.
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links and nothing else; the core ABI is not changed.  Its kernels
 * are those of libgficf_sparse_knn.so as text (gficf_amd/csrc/sparse_knn_tiles.h), instantiated with the queries taken from a
 * second matrix.
 *
 * INPUT.  Two CSC matrices with the same number of rows G: the training cells, G x N, and the queries, G x M.  Each follows the
 * input rules of include/gficf_sparse_knn.h: the column pointer int64 on the device (int32 or int64 at the host entry), row ids
 * int32, STRICTLY ascending within a column, values f64.  OUTPUT.  idx, M x k int32, 1-based ids of TRAINING cells, column-major
 * with leading dimension ld_out; dist alike in f64 and / or f32: for every query the k smallest (key, id) pairs over all N
 * training cells, ties broken by the smaller id.
 *
 * CONTRACT.  The method of include/gficf_sparse_knn.h, word for word: the values of both matrices are rounded to f32 once, in a
 * prepare pass each; the per-cell scalars and the pair sums are accumulated in f64 in GFICF_SPARSE_KNN_LANES (16) chains added
 * in the fixed tree (l with l ^ 8, ^ 4, ^ 2, ^ 1); the pair sum of (query, training cell) runs over the stored entries of the
 * CANDIDATE, which is the training cell, against the query's dense values (0 where the query stores nothing); the distance is
 * that header's table with the QUERY's scalars first (a) and the training cell's second (b), plus 0.0, rounded once to f32 for
 * the key  sortable(d) << 32 | training id.  What differs:
 *
 *   - No self rule: a query is no column of the training matrix and no pair is special.  A query equal to a training cell gets
 *     exactly 0 under euclidean and manhattan: S is then the same chain as na, so (na + na) - 2 S = 0, and T = 2 la bit for
 *     bit.  Under cosine and correlation the same pair gets a value in [0, 2^-51], not necessarily 0: 1 - S / (r r) with
 *     r = sqrt(na) is 0 or 2.2e-16 depending on how r r rounds against S (a NumPy restatement of the method gave 2.2e-16 for
 *     8 of 40 such pairs); the square search writes its diagonal without arithmetic for this reason, and here there is no
 *     diagonal to write.  Among several training cells equal to the query, such noise and then the id decide the order.
 *   - A query's row of the table depends on that query, the training matrix and k only: not on the tile it is in, not on
 *     the slice count (which follows from M), not on the other queries.  Any split of the queries gives the bits of the whole.
 *
 * KERNELS.  Two prepare launches (training, queries), the tile kernel over ceil(M / TQ) x slices workgroups, the merge.  TQ
 * and the slices follow the rule of gficf_sparse_knn_shape for M queries against N candidates; gficf_sparse_query_shape states them.
 *
 * Limits: 1 <= k <= min(GFICF_KNN_MAX_K, N) (k > GFICF_KNN_MAX_K: GFICF_ERR_UNSUPPORTED; k > N: GFICF_ERR_INVALID_ARG), M >= 0
 * (M = 0 runs the prepare passes and writes nothing), G <= GFICF_SPARSE_KNN_LDS_FLOATS (more: GFICF_ERR_UNSUPPORTED), N and
 * M < 2^31.  The status codes are those of the square search, and so are the deferred checks (gficf_sparse_query_sync), applied
 * to each matrix: GFICF_ERR_BAD_CSC, GFICF_ERR_BAD_VALUE.  The kernels read and write inside their buffers whatever the input
 * holds; the table of such a call is not meaningful. */
#ifndef GFICF_SPARSE_QUERY_H
#define GFICF_SPARSE_QUERY_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_sparse_knn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_SPARSE_QUERY_ABI_VERSION 1

int gficf_sparse_query_abi_version(void);

/* The decomposition for G genes, N training cells, M queries and k neighbours, a host query: tile_queries (TQ), slices, and
 * max_genes (written whatever G is).  G > max_genes: GFICF_ERR_UNSUPPORTED. */
int gficf_sparse_query_shape(int64_t G, int64_t N, int64_t M, int k, int* tile_queries, int* slices, int64_t* max_genes);

/* Bytes of device scratch of gficf_sparse_query_device; 0 on arguments it would refuse. */
size_t gficf_sparse_query_workspace_bytes(int64_t G, int64_t N, int64_t nnz_train, int64_t M, int64_t nnz_query, int k);

/* Device form: the M queries (d_q_*) against the N training cells (d_t_*).  d_idx: M x k column-major with leading dimension
 * ld_out >= M; d_dist (f64) and d_dist_f32 alike, each may be NULL.  Only enqueues, on the context's stream. */
int gficf_sparse_query_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_t_colptr, const int32_t* d_t_rowidx, const double* d_t_x,
                              int64_t nnz_train, int64_t M, const int64_t* d_q_colptr, const int32_t* d_q_rowidx, const double* d_q_x,
                              int64_t nnz_query, int k, int metric, void* ws, size_t ws_bytes, int32_t* d_idx, double* d_dist,
                              float* d_dist_f32, int64_t ld_out);
/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_sparse_query_sync(gficf_ctx* ctx, const void* ws);
/* Host form: each colptr int32 or int64 (its *_is_i64); idx M x k column-major int32 (1-based), dist M x k column-major
 * doubles or NULL. */
int gficf_sparse_query_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* t_colptr, int t_colptr_is_i64, const int32_t* t_rowidx,
                            const double* t_x, int64_t M, const void* q_colptr, int q_colptr_is_i64, const int32_t* q_rowidx,
                            const double* q_x, int k, int metric, int32_t* idx, double* dist);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_SPARSE_QUERY_H */
