/* gficf_harmony.h — C ABI of libgficf_harmony.so: Harmony (Korsunsky et al. 2019, Nat. Methods 16:1289), the batch correction of
 * the PCA cells between runPCA and runReduction / clustcells, on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) and every other add-on are not changed.
 *
 * The contract is the method, stage by stage, not harmony's random bits: the library never draws a random number, the start
 * centroids and the order of the cells within a clustering round are inputs (gficf_rsvd_* treats omega the same way).
 *
 * Inputs.
 *   Z       N x d row-major f64, 1 <= d <= 128: the cells.
 *   levels  V x N int32: V categorical variables as 0-based GLOBAL level ids.  Variable v owns the contiguous ids
 *           [var_start[v], var_start[v + 1]), var_start[0] = 0, var_start[V] = B, every variable at least one level;
 *           1 <= V <= 4, 1 <= B <= 64.  var_start is a HOST array of V + 1 int32.  A level may have no cell.
 *           Phi is the implied B x N one-hot matrix (V ones a column), Pr[b] the mean of its row b, Phi* is Phi under a row of ones.
 *   theta, lambda   B f64 each, on the device, per level.  sigma > 0.
 *   K       clusters, 1 <= K <= 100, K <= N.     Y0  K x d f64: the start centroids (the Python layer draws K distinct cells).
 *   perm    rounds x N int32: one permutation of [0, N) per clustering round, consumed in order over the whole run.
 *           An entry outside [0, N) is never followed (GFICF_ERR_INVALID_ARG at the sync); a row that repeats a cell is the
 *           caller's error and is not detected.
 *   R is K x N row-major (R[k, i] = R[k * N + i]), O and E are K x B, Y is K x d, all f64.
 *
 * Stages.  All arithmetic is f64, every operation rounded as written (harmony.hip is compiled with -ffp-contract=off), sums
 * in fixed orders: no floating-point atomics, the same input gives the same bits on every call, and no launch shape depends
 * on the device (only on N, K, d, B, V).  "ascending" below means a left-to-right sum starting from 0.
 *
 * 1 Normalise (gficf_harmony_normalise_device).  Zc[i] = Z[i] / sqrt(sum_j Z[i,j]^2) (j ascending).  A zero row stays zero
 *   and is counted (info[0] of the sync); a row whose norm is not finite is GFICF_ERR_BAD_VALUE at the sync.
 *
 * 2 Start (gficf_harmony_start_device).  init_iter >= 0 hard Lloyd iterations under cosine from Y = Y0 (Y0 is used as given):
 *   cell i goes to the k of largest Y[k] . Zc[i] (j ascending; the lowest k wins a tie); then Y[k] = s / |s| with
 *   s = the sum of its cells (below); a cluster whose sum has norm 0 (an empty one) keeps its previous centroid.
 *   labels (N int32) are the assignments of the last iteration (all 0 for init_iter = 0).
 *
 *   Sums over cells with d columns (here, the soft centroids of stage 4, the moments of stage 6): the cells are cut into chunks
 *   of 1024 consecutive cells, a chunk is summed ascending, the chunk sums are added ascending.
 *
 * 3 Assign (gficf_harmony_assign_device).  dist[k,i] = 2 (1 - Y[k] . Zc[i]);  m_i = min_k dist[k,i];
 *   e[k,i] = exp(-(dist[k,i] - m_i) / sigma);  R[k,i] = e[k,i] / sum_k e[k,i] (k ascending).
 *   O = R Phi^T;  E[k,b] = S[k] Pr[b] with S[k] = sum_i R[k,i].
 *
 *   Sums over cells by level (O, the counts behind Pr, the block terms of stage 4, the Gram entries of stage 6): a list of cells
 *   is cut into chunks of 1024 consecutive list positions, a chunk into 4 quarters of 256; a quarter is summed in a fixed rotated
 *   order, the quarters as (q0 + q1) + (q2 + q3), the chunk sums ascending.  S[k] is the ascending sum of O[k,b] over the levels
 *   of variable 0 (every cell has exactly one).  Pr[b] = count_b / N, one division.
 *
 * 4 Clustering round (gficf_harmony_round_device).  Y[k] = s / |s|, s = sum_i R[k,i] Zc[i] (norm 0 keeps the Y handed in), dist
 *   as in 3.  The round's permutation is cut into n_blocks contiguous blocks as numpy.array_split does (the first N mod n_blocks
 *   are one longer; an empty block is a no-op), visited in order.  For block T, with R_T the block's columns:
 *       O -= R_T Phi_T^T,  E[k,b] -= S_T[k] Pr[b]                                        (the block's own terms out)
 *       R[k,i] = e[k,i] prod_{b active in i} pow((E[k,b] + 1) / (O[k,b] + 1), theta[b]), normalised over k as in 3, i in T
 *       O += R_T Phi_T^T,  E[k,b] += S_T[k] Pr[b]                                        (and back in)
 *   the product over the variables ascending, multiplied into e one factor at a time.  The blocks depend on each other through
 *   O and E; they run one after the other on the stream, with no host synchronisation inside a round.
 *
 * 5 Objective (gficf_harmony_objective_device), for the Y of the round (dist is recomputed from it):
 *       sum_i sum_k ( R dist + sigma R log R + sigma R sum_{b active in i} theta[b] log((O[k,b] + 1) / (E[k,b] + 1)) ),  0 log 0 = 0.
 *   The list of objectives of a run starts with the one after stage 3 and gets one entry a round.  The clustering of an outer
 *   iteration stops after its round t >= 3 when (old - new) / |old| < epsilon_cluster, old and new the sums of the three entries
 *   ending one before the last and at the last; or after max_iter_kmeans rounds.  The host reads one f64 a round: the only
 *   synchronisation.
 *
 * 6 Correct (gficf_harmony_correct_device).  For every cluster k
 *       A_k = Phi* diag(R[k]) Phi*^T + diag(0, lambda)      (B + 1)^2
 *       W_k = A_k^-1 Phi* diag(R[k]) Z                      (B + 1) x d, then W_k[0, :] = 0
 *       Zcorr[i] = Z[i] - sum_k R[k,i] sum_{b active in i} W_k[1 + b]      (k ascending, the variables ascending inside)
 *   always from the Z handed in (the ORIGINAL cells), never from a previous correction.  The row of ones of the moments is the
 *   ascending sum of variable 0's rows.  A_k is factored by Cholesky (one workgroup a cluster, no pivoting); a pivot that is not
 *   positive (a cluster without mass, or an empty level with lambda = 0) makes W_k = 0, so that cluster contributes nothing; such
 *   clusters are counted (info[1] of the sync), never a NaN.
 *
 * 7 Outer loop (gficf_harmony_device): 1, 2, 3, the objective; then for it = 1 .. max_iter_harmony: rounds of 4 each followed
 *   by 5 until 5's rule stops them; 6 from Z; Zc = 1 of Zcorr; stop after it >= 2 when (h[it-1] - h[it]) / |h[it-1]| <
 *   epsilon_harmony, h[it] the last objective of iteration it.  It is exactly the stage entries called one after the other.
 *
 * Differences from harmony, stated: one start of the initial k-means from given centroids (harmony: kmeans(nstart = 10)); the
 * exponentials are shifted by the cell's smallest distance (the normalised R is the same in exact arithmetic and no column
 * underflows at small sigma); the block order comes from given permutations; lambda estimation, reference_values,
 * cluster_prior and do_pca are not provided.
 *
 * Rejected before any launch: a size outside the limits above that the library could in principle grow to (d > 128, K > 100,
 * B > 64, V > 4, N > 2^31 - 1) GFICF_ERR_UNSUPPORTED; anything else (a size below 1, K > N, var_start not as stated, sigma not
 * positive and finite, n_blocks < 1, negative iteration limits, too few rounds of perm, a NULL pointer, a workspace too small)
 * GFICF_ERR_INVALID_ARG.  Deferred to gficf_harmony_sync: a level id outside its variable's range or a perm entry outside
 * [0, N) (GFICF_ERR_INVALID_ARG; such an entry is skipped, nothing is read or written out of bounds), a non-finite row norm
 * (GFICF_ERR_BAD_VALUE). */
#ifndef GFICF_HARMONY_H
#define GFICF_HARMONY_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_HARMONY_ABI_VERSION 1
#define GFICF_HARMONY_MAX_D 128
#define GFICF_HARMONY_MAX_K 100
#define GFICF_HARMONY_MAX_B 64
#define GFICF_HARMONY_MAX_V 4

int gficf_harmony_abi_version(void);

/* Device scratch of every entry below (one block serves them all; its first 16 bytes are the status word and the two counters).
 * 0 for sizes the entries reject. */
size_t gficf_harmony_workspace_bytes(int64_t N, int64_t d, int64_t K, int64_t V, int64_t B);

/* Stage 1.  Zeroes the status word and the counters first: it is the first stage of a run.  Z and Zc may be the same block. */
int gficf_harmony_normalise_device(gficf_ctx* ctx, int64_t N, int64_t d, const double* d_Z, double* d_Zc, void* ws, size_t ws_bytes);
/* Stage 2.  d_Y0 and d_Y may be the same block. */
int gficf_harmony_start_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, const double* d_Zc, const double* d_Y0, int32_t init_iter,
                               double* d_Y, int32_t* d_labels, void* ws, size_t ws_bytes);
/* Stage 3. */
int gficf_harmony_assign_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                                const double* d_Zc, const int32_t* d_levels, const double* d_Y, double sigma, double* d_R, double* d_O,
                                double* d_E, void* ws, size_t ws_bytes);
/* Stage 4: one round.  d_perm: the round's N int32.  d_R, d_O, d_E and d_Y are read and written. */
int gficf_harmony_round_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                               const double* d_Zc, const int32_t* d_levels, const double* d_theta, double sigma, const int32_t* d_perm,
                               int32_t n_blocks, double* d_R, double* d_O, double* d_E, double* d_Y, void* ws, size_t ws_bytes);
/* Stage 5.  d_obj: one f64 on the device. */
int gficf_harmony_objective_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                                   const double* d_Zc, const int32_t* d_levels, const double* d_Y, const double* d_R, const double* d_O,
                                   const double* d_E, const double* d_theta, double sigma, double* d_obj, void* ws, size_t ws_bytes);
/* Stage 6.  d_W (may be NULL): K x (B + 1) x d f64, the W_k. */
int gficf_harmony_correct_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start,
                                 const double* d_Z, const int32_t* d_levels, const double* d_R, const double* d_lambda, double* d_Zcorr,
                                 double* d_W, void* ws, size_t ws_bytes);
/* Stage 7: the chain.  rounds: the rows of d_perm, at least max_iter_harmony * max_iter_kmeans.  Device outputs: d_Zcorr and
 * d_Zc (N x d), d_R, d_Y, d_O, d_E.  Host outputs: objective (1 + rounds f64: the list of stage 5), iter_rounds
 * (max_iter_harmony int32: the rounds of each outer iteration) and info (4 int64: outer iterations run, rounds run, 1 if the
 * outer rule stopped the run else 0, 0).  Waits once a round for the objective; the deferred errors are gficf_harmony_sync's. */
int gficf_harmony_device(gficf_ctx* ctx, int64_t N, int64_t d, int64_t K, int64_t V, int64_t B, const int32_t* var_start, const double* d_Z,
                         const int32_t* d_levels, const double* d_theta, const double* d_lambda, double sigma, const double* d_Y0,
                         const int32_t* d_perm, int64_t rounds, int32_t init_iter, int32_t max_iter_harmony, int32_t max_iter_kmeans,
                         int32_t n_blocks, double epsilon_cluster, double epsilon_harmony, double* d_Zcorr, double* d_Zc, double* d_R,
                         double* d_Y, double* d_O, double* d_E, double* objective, int32_t* iter_rounds, int64_t* info, void* ws,
                         size_t ws_bytes);
/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws.  info (may be NULL): 2 int64, the zero rows the
 * last normalisation met and the clusters the last correction left out. */
int gficf_harmony_sync(gficf_ctx* ctx, const void* ws, int64_t* info);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_HARMONY_H */
