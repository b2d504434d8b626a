/* gficf_umap.h — C ABI of libgficf_umap.so: runReduction of the reference (R/dimensinalityReduction.R:157-192, whose default is
 * uwot::tumap(data$pca$cells)): the UMAP / t-UMAP embedding of the cells on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, neighbour search, radix sort, scan, status codes and gficf_last_error().  The core ABI is not changed.
 *
 * RELAXED CONTRACT.  The algorithm and its objective are UMAP's (McInnes, Healy, Melville 2018) as uwot runs them; the random
 * bits and the update order are not uwot's.  Three stages, each an entry of its own, and one chained host entry.
 *
 * 1. FUZZY GRAPH from the N x k neighbour table of the search (column-major, 1-based ids, column 0 the nearest point; the ids
 *    of a row are distinct; a negative distance, which the search's cosine and correlation metrics can round to, counts as 0).
 *    Per point i, with c = local_connectivity >= 1, f = floor(c), r = c - f and nz the positive
 *    distances of columns 1 .. k-1 in order:
 *      rho_i   = nz[f-1] (+ r (nz[f] - nz[f-1]) when r > 0 and nz[f] exists) if len(nz) >= f, max(nz) if 0 < len(nz) < f, else 0;
 *      sigma_i solves sum_{j=1..k-1} exp(-max(0, d_ij - rho_i) / sigma) = log2(k): at most 64 bisections from sigma = 1,
 *              lo = 0, hi = inf (doubling while hi is infinite), stopped at |sum - target| < 1e-5; then floored at
 *              1e-3 x the mean of the row's k distances (rho_i > 0) or 1e-3 x the mean of all N k distances (rho_i = 0);
 *      w_ij    = 0 where idx_ij = i; 1 where d_ij - rho_i <= 0 or sigma_i = 0; else exp(-(d_ij - rho_i) / sigma_i)   (f32).
 *    P = m (W + W' - W o W') + (1 - m) (W o W'), m = set_op_mix_ratio, as CSR (= CSC: P is symmetric): rowptr int64 (N + 1),
 *    col int32 0-based ASCENDING within a row, val f32; zero entries dropped, no diagonal; capacity 2 N k, nnz on the device.
 *    P[i,j] and P[j,i] are the same bits (both evaluate the formula on (min, max) of the two memberships).
 * 2. LAYOUT, epochs [epoch_begin, epoch_end) of n_epochs, in place on Y (N x 2 f32 row-major).
 *    Schedule, stateless and integer: wmax = the largest value of P, q_e = min(floor((double)w_e / wmax * 2^32), 2^32 - 1);
 *    entry e is due in epoch n (0-based) iff ((n + 1) q_e >> 32) > (n q_e >> 32) in u64.  An entry with n_epochs q_e < 2^32
 *    never fires (uwot's pruning of w < wmax / n_epochs).  Running [0, a) then [a, n) gives the bits of [0, n).
 *    Update, owner computes: vertex v alone writes its next position.  It walks its row in column order with its running
 *    position y_v; every other position is read from the epoch-start buffer.  Per due entry (v, j), alpha = learning_rate
 *    (1 - n / n_epochs):
 *      twice in succession (the second stands for uwot's move of the tail of the mirrored entry (j, v), due in the same
 *      epochs): diff = y_v - y_j, d2 = |diff|^2, coef = -2ab d2^(b-1) / (a d2^b + 1) (0 at d2 = 0), y_v += alpha clip(coef diff, +-4);
 *      then negative_sample_rate times, s = 0 ..: key = mix(mix(mix(seed + n) + e) + s), mix the splitmix64 finaliser, e the
 *      entry's position in col; j = ((key >> 32) N) >> 32, skipped if j = v; coef = 2 gamma b / ((0.001 + d2)(a d2^b + 1)),
 *      y_v += alpha clip(coef diff, +-4), the clipped step being +4 on both coordinates at d2 = 0.
 *    a = b = 1 (t-UMAP) takes a path without pow.  All arithmetic is f32, unfused.  One launch per epoch.
 * 3. CHAIN (gficf_umap_host): prepare -> search with distances -> graph -> layout, device-resident.  The initial coordinates
 *    are an INPUT: the library holds no generator beyond the counter hash above.
 * No floating-point atomics anywhere: sums and maxima run over fixed chunks in a fixed order, and no result depends on how the
 * work was mapped to lanes.  The same input gives the same bits on every call.
 *
 * Limits: 2 <= k <= GFICF_KNN_MAX_K, k <= N, N k < 2^31, local_connectivity >= 1, 0 <= set_op_mix_ratio <= 1, a, b > 0,
 * n_epochs >= 1, 0 <= epoch_begin <= epoch_end <= n_epochs, negative_sample_rate >= 0 (GFICF_ERR_INVALID_ARG otherwise); a
 * workspace or an output that is too small is GFICF_ERR_CAPACITY.  Deferred (through the status word at the head of the
 * workspace, collected by gficf_umap_sync): a non-finite distance, a non-finite initial coordinate or a value of P
 * that is not positive and finite is GFICF_ERR_BAD_VALUE; a neighbour id outside [1, N] or a column of P outside [0, N) is
 * GFICF_ERR_BAD_ID; a row pointer of P that decreases or leaves [0, capacity] is GFICF_ERR_BAD_CSC. */
#ifndef GFICF_UMAP_H
#define GFICF_UMAP_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_UMAP_ABI_VERSION 1

int gficf_umap_abi_version(void);

/* Stage 1.  d_idx / d_dist: exactly what gficf_knn_search_device writes (leading dimension ld >= N).  d_rowptr N + 1, d_col and
 * d_val `capacity` >= 2 N k entries, d_nnz one int64; d_sigma / d_rho: N f32 each or NULL; d_w: the memberships W before the symmetrisation,
 * N x k f32 column-major with leading dimension N, or NULL (the seam the graph's properties are tested at).  Only enqueues. */
size_t gficf_umap_graph_workspace_bytes(int64_t N, int k);
int gficf_umap_graph_device(gficf_ctx* ctx, const int32_t* d_idx, const float* d_dist, int64_t N, int k, int64_t ld, double local_connectivity,
                            double set_op_mix_ratio, void* ws, size_t ws_bytes, int64_t* d_rowptr, int32_t* d_col, float* d_val, int64_t capacity,
                            int64_t* d_nnz, float* d_sigma, float* d_rho, float* d_w);

/* Stage 2.  P as stage 1 wrote it (the entries in use are d_rowptr[N]; `capacity` is the length of d_col / d_val); d_Y: N x 2
 * f32 row-major, updated in place.  Only enqueues: one launch per epoch. */
size_t gficf_umap_layout_workspace_bytes(int64_t N, int64_t capacity);
int gficf_umap_layout_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity, float a,
                             float b, float gamma, float learning_rate, int negative_sample_rate, int n_epochs, int epoch_begin, int epoch_end,
                             uint64_t seed, float* d_Y, void* ws, size_t ws_bytes);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws (a workspace of either *_device entry above). */
int gficf_umap_sync(gficf_ctx* ctx, const void* ws);

/* Stage 3, host form.  X: N x d column-major f64 (ld >= N, d <= 128); metric: a gficf_knn_metric; n_neighbors counts the point
 * itself; init and embedding: N x 2 column-major f64.  On request (each NULL or given): the graph — rowptr N + 1 int64, col and
 * val 2 N n_neighbors entries, *nnz the entries in use — and the neighbour table — idx N x n_neighbors int32 1-based, dist f32,
 * both column-major. */
int gficf_umap_host(gficf_ctx* ctx, const double* X, int64_t N, int d, int64_t ld, int metric, int n_neighbors, double local_connectivity,
                    double set_op_mix_ratio, double a, double b, double gamma, double learning_rate, int negative_sample_rate, int n_epochs,
                    const double* init, uint64_t seed, double* embedding, int64_t* rowptr, int32_t* col, float* val, int64_t* nnz, int32_t* idx,
                    float* dist);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_UMAP_H */
