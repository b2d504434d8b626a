/* gficf_tsne.h — C ABI of libgficf_tsne.so: the "tsne" reduction of the reference (R/dimensinalityReduction.R:175-177,
 * Rtsne::Rtsne(X = data$pca$cells, dims = 2, pca = F, max_iter = 1000)): the t-SNE embedding of the cells on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, neighbour search, radix sort, scan, status codes and gficf_last_error().  The core ABI is not changed.
 *
 * RELAXED CONTRACT.  The algorithm and its objective are van der Maaten's (2008, 2014) as Rtsne runs them; the random bits are
 * not Rtsne's (the initial coordinates are an INPUT), and the repulsion is EXACT (all N^2 pairs) where Rtsne's default is
 * Barnes-Hut at theta = 0.5.  Three stages, each an entry of its own, and one chained host entry.
 *
 * 1. AFFINITIES from the N x k neighbour table of the search: euclidean, column-major, 1-based ids, column 0 the point itself,
 *    K = k - 1 = floor(3 perplexity).  Per row, in f64, with d2_m the squared distances of the columns 1 .. K whose id is not
 *    the row itself and d2min the smallest of them:
 *      p_m ~ exp(-beta (d2_m - d2min)),   H = beta sum_m (d2_m - d2min) p_m / sum_m p_m + log sum_m p_m;
 *    beta is bisected from 1 until |H - log(perplexity)| < 1e-5 or 200 evaluations: H too large raises beta (doubled while there
 *    is no upper bound, else the mean with it), H too small lowers it (halved while there is no lower bound): bhtsne's loop.
 *    Pc_m = p_m / sum p at the last beta EVALUATED (the beta returned), rounded to f32; an entry whose id is the row itself
 *    gets Pc = 0.  A row whose distances are all equal gets the same value, 1 / their number, on every entry (whatever beta).
 *    DIFFERENCE from bhtsne: the shift by d2min is ours.  It gives the same entropy and the same normalised p in exact
 *    arithmetic and avoids rows whose exponentials all underflow.
 *    P = (Pc + Pc') / (2 N) as CSR (= CSC: P is symmetric): rowptr int64 (N + 1), col int32 0-based ASCENDING within a row,
 *    val f32; no diagonal, zero entries dropped; capacity 2 N K, nnz on the device.  P[i,j] and P[j,i] carry the same bits:
 *    both evaluate (float)(((double)lo + (double)hi) / (2 N)) on (lo, hi) = (min, max) of the two conditionals.
 * 2. GRADIENT, Rtsne's Barnes-Hut form at theta = 0.  With q_ij = 1 / (1 + |y_i - y_j|^2):
 *      Z      = sum_{i != j} q_ij
 *      rep_i  = sum_{j != i} q_ij^2 (y_i - y_j)
 *      attr_i = sum_{j in row i of P} P_ij q_ij (y_i - y_j)
 *      dC_i   = x attr_i - rep_i / Z,      x the exaggeration in force.
 *    There is NO FACTOR 4, as in Rtsne's code: the true gradient of the KL divergence is 4 dC, and eta = 200 is tuned to this
 *    form.  KL = sum over the stored entries of P_ij log(P_ij Z / q_ij), un-exaggerated, in f64.
 *    Arithmetic.  The repulsive field is f32: per pair dx = y_i.x - y_j.x, dy alike, s = fma(dx, dx, fma(dy, dy, 1)),
 *    q = rcp(s) (v_rcp_f32, 1 ulp, exact on powers of two), z += q, rx = fma(q q, dx, rx), ry alike.  The j = i pair adds a
 *    zero vector by itself and a 1 to z; N is taken off the sum of all z in f64.  A lane adds at most GFICF_TSNE_TILE = 128
 *    pairs in f32 (the longest f32 accumulation chain, T); every tile's sums are added in f64, tile after tile, slice after
 *    slice, row block after row block: fixed chunks in a fixed order.  attr, the combination x attr - rep / Z and KL are f64;
 *    dC is rounded to f32 once.
 * 3. LAYOUT, iterations [iter_begin, iter_end) of max_iter on three N x 2 f32 row-major arrays: Y, uY (the velocity) and
 *    gains.  Per iteration n (0-based), per coordinate, in f32, unfused:
 *      x    = exaggeration_factor if n < stop_lying_iter, else 1;   mu = momentum if n < mom_switch_iter, else final_momentum;
 *      gain = gain + 0.2 where sign(dC) != sign(uY), else gain * 0.8 (sign(0) = 0); floored at 0.01;
 *      uY   = mu uY - (eta gain) dC;   Y += uY;   then the column means of Y, summed in f64, are subtracted (one rounding).
 *    Exaggeration is a factor in the attractive sum: P is never rescaled in place, and nothing carries between iterations but
 *    Y, uY and gains.  So running [0, a) then [a, n) gives the bits of [0, n) in all three arrays, and the same input gives the
 *    same bits on every call.  DIFFERENCE from Rtsne: it switches one iteration later (at iter == stop_lying_iter, after that
 *    iteration's update, and likewise the momentum).  Rtsne's defaults: perplexity 30, max_iter 1000, stop_lying_iter and
 *    mom_switch_iter 250 (0 when initial coordinates are given), momentum 0.5, final_momentum 0.8, eta 200, exaggeration 12.
 *    Duplicate rows of X are not checked for (Rtsne refuses them): they are harmless here.
 * 4. CHAIN (gficf_tsne_host): prepare -> search with distances -> affinities -> layout, device-resident.
 * No floating-point atomics anywhere: Z, the means, KL and the per-slice partial fields are summed over fixed chunks in a fixed
 * order, and the decomposition (gficf_tsne_shape) depends on N only, not on the device.
 *
 * Limits (GFICF_ERR_INVALID_ARG unless stated): perplexity > 0; N - 1 >= 3 perplexity (Rtsne's check); k = floor(3 perplexity)
 * + 1 <= GFICF_KNN_MAX_K, that is perplexity < 42.34 (GFICF_ERR_UNSUPPORTED beyond); N k < 2^31; max_iter >= 0 and
 * 0 <= iter_begin <= iter_end <= max_iter; a workspace or an output that is too small is GFICF_ERR_CAPACITY.  Deferred
 * (through the status word at the head of the workspace, collected by gficf_tsne_sync): a non-finite distance, coordinate or
 * value of P (or a negative one) is GFICF_ERR_BAD_VALUE; a neighbour id outside [1, N] or a column of P outside [0, N) is
 * GFICF_ERR_BAD_ID; a row pointer of P that decreases or leaves [0, capacity] is GFICF_ERR_BAD_CSC. */
#ifndef GFICF_TSNE_H
#define GFICF_TSNE_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_TSNE_ABI_VERSION 1
#define GFICF_TSNE_TILE 128 /* T: the longest f32 accumulation chain of the repulsion kernel */

int gficf_tsne_abi_version(void);

/* Stage 1.  d_idx / d_dist: exactly what gficf_knn_search_device writes for k = floor(3 perplexity) + 1 columns (leading
 * dimension ld >= N).  d_rowptr N + 1, d_col and d_val `capacity` >= 2 N (k - 1) entries, d_nnz one int64; d_beta: N f64 or
 * NULL; d_pc: the conditionals Pc before the symmetrisation, N x (k - 1) f32 column-major with leading dimension N (column m
 * belongs to column m + 1 of the table), or NULL (the seam the properties are tested at).  Only enqueues. */
size_t gficf_tsne_affinities_workspace_bytes(int64_t N, int k);
int gficf_tsne_affinities_device(gficf_ctx* ctx, const int32_t* d_idx, const float* d_dist, int64_t N, int k, int64_t ld, double perplexity,
                                 void* ws, size_t ws_bytes, int64_t* d_rowptr, int32_t* d_col, float* d_val, int64_t capacity, int64_t* d_nnz,
                                 double* d_beta, float* d_pc);

/* The decomposition of the repulsion kernel for N points, a pure host query that depends on N only: a workgroup owns
 * *rows_per_block rows i and one of *slices contiguous ranges of j, which it walks in tiles of *tile (= GFICF_TSNE_TILE)
 * positions.  Any pointer may be NULL. */
int gficf_tsne_shape(int64_t N, int* rows_per_block, int* tile, int* slices);

/* Stage 2.  P as stage 1 wrote it (the entries in use are d_rowptr[N]; `capacity` is the length of d_col / d_val); d_Y: N x 2
 * f32 row-major.  For the exaggeration x: d_dC N x 2 f32; d_rep N x 2 f32 (un-normalised) or NULL; d_Z one f64; d_kl one f64
 * or NULL.  ws: a workspace of gficf_tsne_layout_workspace_bytes.  One iteration's first half, and the seam the field is
 * tested at.  Only enqueues. */
int gficf_tsne_gradient_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity,
                               const float* d_Y, double exaggeration, void* ws, size_t ws_bytes, float* d_dC, float* d_rep, double* d_Z,
                               double* d_kl);

/* Stage 3.  d_Y, d_uY, d_gains: N x 2 f32 row-major, updated in place (a fresh run starts from uY = 0, gains = 1); d_kl: the
 * KL divergence of the coordinates left behind (one more evaluation of the field), one f64, or NULL.  Only enqueues: three
 * launches per iteration. */
size_t gficf_tsne_layout_workspace_bytes(int64_t N, int64_t capacity);
int gficf_tsne_layout_device(gficf_ctx* ctx, int64_t N, const int64_t* d_rowptr, const int32_t* d_col, const float* d_val, int64_t capacity,
                             int max_iter, int iter_begin, int iter_end, int stop_lying_iter, int mom_switch_iter, double momentum,
                             double final_momentum, double eta, double exaggeration_factor, float* d_Y, float* d_uY, float* d_gains, void* ws,
                             size_t ws_bytes, double* d_kl);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws (a workspace of any *_device entry above). */
int gficf_tsne_sync(gficf_ctx* ctx, const void* ws);

/* Stage 4, host form.  X: N x d column-major f64 (ld >= N, d <= 128); init and embedding: N x 2 column-major f64; *kl: the final
 * KL divergence (or NULL).  On request (each NULL or given): P — rowptr N + 1 int64, col and val 2 N floor(3 perplexity)
 * entries, *nnz the entries in use — and the neighbour table — idx N x (floor(3 perplexity) + 1) int32 1-based, dist f32, both
 * column-major. */
int gficf_tsne_host(gficf_ctx* ctx, const double* X, int64_t N, int d, int64_t ld, double perplexity, int max_iter, int stop_lying_iter,
                    int mom_switch_iter, double momentum, double final_momentum, double eta, double exaggeration_factor, const double* init,
                    double* embedding, double* kl, int64_t* rowptr, int32_t* col, float* val, int64_t* nnz, int32_t* idx, float* dist);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_TSNE_H */
