/* gficf_transform.h — C ABI of libgficf_transform.so: embedNewCells and classify.cells of the reference (R/cellClassifier.R:15-95,
 * through uwot::umap_transform and class::knn): new cells placed into a trained UMAP / t-UMAP plane and labelled by their trained
 * neighbours, on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, gficf_knn_prepare_device, status codes and gficf_last_error().  The core ABI is not changed.
 *
 * RELAXED CONTRACT, in the sense of gficf_umap.h: the algorithm is UMAP's transform (McInnes, Healy, Melville 2018) as umap-learn
 * and uwot run it; the random bits and the schedule are this library's.  Nothing here claims their bits.  The differences:
 *   - the floor of sigma uses the row's own mean distance (umap-learn: the mean of the whole batch when rho = 0);
 *   - the schedule's maximum is the row's own largest membership (uwot: the largest of the whole batch);
 *   both so that the result for one new cell does not depend on which other cells were submitted with it;
 *   - one attraction per due entry (gficf_umap.h applies two, for its mirrored entry; trained cells do not move, there is none);
 *   - the vote breaks ties by the order of the row, never at random, and does not widen k to the points tied at the k-th
 *     distance (class::knn does both).
 * Notation: N trained cells, M new cells, d <= 128 dimensions, k neighbours.
 *
 * 1. SEARCH of the M query rows against the N training rows, both as gficf_knn_prepare_device writes them (row-major f32, pitch
 *    gficf_knn_dpad(d), same metric).  Per query the k smallest (distance, index) pairs over all N training rows, ties by the
 *    smaller index; d_idx M x k int32, 1-based TRAINING ids, column-major, column 0 the nearest; d_dist f32 alike.  The arithmetic
 *    is that of gficf_knn_search_device, and so are the bits: f32 accumulated in dimension order over the padded row; manhattan
 *    acc + |a - b|; euclidean ranked on the chain fma(a - b, a - b, acc), sqrtf of it returned; cosine and correlation
 *    1.0f - acc with acc = fma(a, b, acc) over the prepared rows.  With the training rows as queries the table is that of
 *    gficf_knn_search_device bit for bit.  The candidate range is split S ways, S chosen from M (gficf_transform_search_split).
 * 2. MEMBERSHIPS from that table.  There is no self column: all k columns count.  A distance below 0 counts as 0.  With
 *    c' = max(0, local_connectivity - 1), f = floor(c'), r = c' - f and nz the row's positive distances in order:
 *      rho_i   = for f >= 1: nz[f-1] (+ r (nz[f] - nz[f-1]) when r > 0 and nz[f] exists) if len(nz) >= f, max(nz) if 0 < len(nz) < f,
 *                else 0; for f = 0: r nz[0], or 0 with no positive distance (local_connectivity = 1: rho = 0 everywhere);
 *      sigma_i solves sum_{c=0..k-1} exp(-max(0, d_ic - rho_i) / sigma) = log2(k): at most 64 bisections from sigma = 1, lo = 0,
 *                hi = inf (doubling while hi is infinite), stopped at |sum - target| < 1e-5, f32, the sum in column order; then
 *                floored at 1e-3 x the mean of the row's k distances, whatever rho_i is;
 *      w_ic    = 1 where d_ic - rho_i <= 0 or sigma_i = 0, else expf(-(d_ic - rho_i) / sigma_i).
 *    No symmetrisation: the table is the graph; its rows are new cells, its heads trained cells.
 * 3. INITIAL POSITION  y_i = sum_c w_ic Y_train[idx_ic] / sum_c w_ic, f32, the sums in column order; the plain mean of the k
 *    positions when sum_c w_ic = 0.  Y_train: N x 2 f32 row-major, read only.
 * 4. LAYOUT, epochs [epoch_begin, epoch_end) of n_epochs, in place on Y (M x 2 f32 row-major).
 *    Schedule, per row: q_ic = min(floor((double)w_ic / wmax_i * 2^32), 2^32 - 1), wmax_i = max_c w_ic; entry (i, c) is due in
 *    epoch n (0-based) iff ((n + 1) q >> 32) > (n q >> 32) in u64.
 *    Update: cell i walks its k entries in column order with its running position; alpha = learning_rate (1 - n / n_epochs).
 *    Per due entry (i, c): ONE attraction towards Y_train[idx_ic - 1]: diff = y - y_j, d2 = |diff|^2,
 *      coef = -2ab d2^(b-1) / (a d2^b + 1) (0 at d2 = 0), y += alpha clip(coef diff, +-4);
 *    then negative_sample_rate repulsions, s = 0 ..: e = (query_offset + i) k + c, key = mix(mix(mix(seed + n) + e) + s), mix the
 *      splitmix64 finaliser, j = ((key >> 32) N) >> 32, never skipped (a trained cell is never the new cell itself);
 *      coef = 2 gamma b / ((0.001 + d2)(a d2^b + 1)), y += alpha clip(coef diff, +-4), the clipped step +4 on both coordinates at
 *      d2 = 0.  a = b = 1 (t-UMAP) takes a path without pow.  All arithmetic is f32, unfused.
 *    ONE launch for the whole epoch range: a cell belongs to one group of lanes for the whole launch, its position stays in
 *    registers between epochs, and nothing is written but Y, once at the end.  Running [0, a) then [a, n) gives the bits of
 *    [0, n).  The result for cell i depends on row i, the model and query_offset + i only: two halves of a batch run with the
 *    right offsets give the bits of the whole.
 * 5. VOTE: pred_i = the class with the most votes among labels[idx_ic - 1], c = 0 .. k-1; among classes that tie, the one whose
 *    first member comes first in the row.
 * No atomics on data anywhere (the status word only); no result depends on how the work was mapped to lanes.  The same input
 * gives the same bits on every call.
 *
 * Limits: 1 <= k <= min(N, GFICF_KNN_MAX_K), M >= 0, N k < 2^31, 1 <= d <= 128, 1 <= local_connectivity <= GFICF_KNN_MAX_K,
 * a, b > 0, n_epochs >= 1, 0 <= epoch_begin <= epoch_end <= n_epochs, negative_sample_rate >= 0, query_offset >= 0,
 * (query_offset + M) k < 2^63, C >= 1, leading dimensions >= M (GFICF_ERR_INVALID_ARG otherwise); a workspace that is too small
 * is GFICF_ERR_CAPACITY.  Deferred (through the status word at the head of the workspace, collected by gficf_transform_sync):
 * a non-finite distance, membership or coordinate is GFICF_ERR_BAD_VALUE; a neighbour id outside [1, N] or a label outside
 * [0, C) is GFICF_ERR_BAD_ID.  A non-finite coordinate of the rows handed to gficf_knn_prepare_device is that entry's
 * GFICF_ERR_BAD_VALUE, collected by gficf_ctx_sync (which gficf_transform_sync calls). */
#ifndef GFICF_TRANSFORM_H
#define GFICF_TRANSFORM_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_TRANSFORM_ABI_VERSION 1

int gficf_transform_abi_version(void);

/* Every workspace below begins with the status word of its entry (zeroed by the entry).  All *_device entries only enqueue. */

/* Stage 1.  d_train: N prepared rows; d_query: M prepared rows; d_idx / d_dist (or NULL): M x k column-major, ld_out >= M.
 * gficf_transform_search_split: the number of slices S the candidate range is cut into for M queries against N rows. */
int gficf_transform_search_split(gficf_ctx* ctx, int64_t M, int64_t N);
size_t gficf_transform_search_workspace_bytes(int64_t M, int64_t N, int k);
int gficf_transform_search_device(gficf_ctx* ctx, const float* d_train, int64_t N, const float* d_query, int64_t M, int d, int k, int metric,
                                  void* ws, size_t ws_bytes, int32_t* d_idx, float* d_dist, int64_t ld_out);

/* Stage 2.  d_idx / d_dist: the table of stage 1 (ld >= M).  d_w: M x k f32 column-major, ld_w >= M; d_sigma / d_rho: M f32 or NULL. */
size_t gficf_transform_weights_workspace_bytes(int64_t M, int k);
int gficf_transform_weights_device(gficf_ctx* ctx, const int32_t* d_idx, const float* d_dist, int64_t N, int64_t M, int k, int64_t ld,
                                   double local_connectivity, void* ws, size_t ws_bytes, float* d_w, int64_t ld_w, float* d_sigma, float* d_rho);

/* Stage 3.  d_Y: M x 2 f32 row-major, written. */
size_t gficf_transform_init_workspace_bytes(int64_t M, int k);
int gficf_transform_init_device(gficf_ctx* ctx, const int32_t* d_idx, int64_t ld, const float* d_w, int64_t ld_w, const float* d_Y_train, int64_t N,
                                int64_t M, int k, void* ws, size_t ws_bytes, float* d_Y);

/* Stage 4.  d_Y: M x 2 f32 row-major, updated in place.  One launch for the epoch range. */
size_t gficf_transform_layout_workspace_bytes(int64_t M, int k);
int gficf_transform_layout_device(gficf_ctx* ctx, const int32_t* d_idx, int64_t ld, const float* d_w, int64_t ld_w, const float* d_Y_train, int64_t N,
                                  int64_t M, int k, float a, float b, float gamma, float learning_rate, int negative_sample_rate, int n_epochs,
                                  int epoch_begin, int epoch_end, uint64_t seed, int64_t query_offset, float* d_Y, void* ws, size_t ws_bytes);

/* Vote.  d_labels: int32[N] in [0, C); d_pred: int32[M]; d_votes: M x C int32 row-major, or NULL. */
size_t gficf_transform_vote_workspace_bytes(int64_t M, int k);
int gficf_transform_vote_device(gficf_ctx* ctx, const int32_t* d_idx, int64_t ld, const int32_t* d_labels, int64_t N, int64_t M, int k, int C,
                                void* ws, size_t ws_bytes, int32_t* d_pred, int32_t* d_votes);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws (a workspace of any *_device entry above). */
int gficf_transform_sync(gficf_ctx* ctx, const void* ws);

/* Host forms.  X_train: N x d, Q: M x d, column-major f64 (ld_x >= N, ld_q >= M); metric: a gficf_knn_metric.
 * gficf_transform_search_host: prepare x 2 -> search.  idx: M x k int32 1-based, dist: M x k f64 or NULL, both column-major. */
int gficf_transform_search_host(gficf_ctx* ctx, const double* X_train, int64_t N, int64_t ld_x, const double* Q, int64_t M, int64_t ld_q, int d,
                                int k, int metric, int32_t* idx, double* dist);

/* prepare x 2 -> search -> memberships -> initial position -> layout, device-resident.  Y_train: N x 2, init (or NULL: stage 3)
 * and embedding: M x 2, column-major f64.  On request (each NULL or given), column-major: idx M x k int32, dist and w M x k f32,
 * sigma and rho M f32, y0 M x 2 f64 (the positions the layout started from). */
int gficf_transform_host(gficf_ctx* ctx, const double* X_train, int64_t N, int64_t ld_x, const double* Y_train, const double* Q, int64_t M,
                         int64_t ld_q, int d, int metric, int k, double local_connectivity, double a, double b, double gamma, double learning_rate,
                         int negative_sample_rate, int n_epochs, int epoch_begin, int epoch_end, const double* init, uint64_t seed,
                         int64_t query_offset, double* embedding, int32_t* idx, float* dist, float* w, float* sigma, float* rho, double* y0);

/* prepare x 2 -> search -> vote.  labels: int32[N] in [0, C); pred: int32[M]. */
int gficf_transform_classify_host(gficf_ctx* ctx, const double* X_train, int64_t N, int64_t ld_x, const double* Q, int64_t M, int64_t ld_q, int d,
                                  int k, int metric, const int32_t* labels, int C, int32_t* pred);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_TRANSFORM_H */
