/* gficf_nmf.h — C ABI of libgficf_nmf.so: non-negative matrix factorisation of the GF-ICF matrix on the MI355X (gfx950),
 * by alternating non-negative least squares; the step people put between gficf() and clustcells() when they want
 * parts-based, non-negative gene programmes instead of a signed SVD.
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links and nothing else: it takes that library's gficf_ctx and
 * uses its stream, device scratch, transpose, scan, status codes and gficf_last_error().  The sparse product Y = A'X, the
 * chunked Gram matrix and the chunked column sum are those of libgficf_pca.so, shared as text (include/gficf_pca.h states
 * them).  The core ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * CONTRACT.  The contract is the method below, not RcppML's or scikit-learn's bits.
 * Model: A ~ W diag(d) H.  A is G x N, CSC, non-negative f64 (the genes x cells matrix gficf() returns); W is G x k and its
 * columns sum to 1; H is k x N and its rows sum to 1; 1 <= k <= GFICF_NMF_MAX_K.  The start W0 (G x k, non-negative) is an
 * INPUT: the library draws nothing.  All arithmetic is f64 in fixed orders with no floating-point atomics: the same input
 * gives the same bits on every call.
 *
 * Layout.  Dense operands on the device are ROW-major with the pitch ld = GFICF_NMF_LD(k) (k rounded up to 8), one row per
 * gene (W: G x ld) or per cell (H is held as its transpose: N x ld, row i = column i of H); columns k .. ld are padding:
 * ignored on input, zero on output.  A Gram matrix S has the pitch lp = GFICF_NMF_LP(k) (16, 32, 64 or 128).
 *
 * One iteration of gficf_nmf_device:
 *   1. S = W'W (fixed chunks of rows, added in order), S[j][j] += ridge;  B = A'W - L1_h (one row per cell).
 *   2. H <- nnls(S, B), warm-started from diag(d) H of the previous iteration, from zero in the first.
 *   3. d[j] = sum_i H[j][i] (fixed chunks, added in order), then H[j][:] /= d[j].  A factor with d[j] = 0 is dead: its row
 *      stays zero and d[j] = 0; dead factors are counted and never produce a NaN.
 *   4. S = H H' + ridge;  B = A H' - L1_w, the same product over the transposed copy of A (made once per run).
 *   5. W <- nnls(S, B), warm-started from W diag(d);  d[j] = sum_g W[g][j];  W[:][j] /= d[j].
 *   6. delta = 1 - cor(W, W_previous), Pearson over all G k entries from five sums in a fixed chunked order (delta = 1 when a
 *      variance is not positive).  Stop when delta < tol or after maxit iterations.  The host reads one small block per
 *      iteration (delta, the loss when tracked, the status word, the counts): the only synchronisation.
 * Steps 1 - 3 (and 4 - 5, on the transposed matrix) are gficf_nmf_half_device; the chain is exactly its stage entries
 * called one after the other.
 *
 * The solve, gficf_nnls_device.  For each of M rows b of B, minimise h'S h / 2 - b'h over h >= 0 by cyclic coordinate descent
 * on a maintained gradient g.  Every product below is rounded, then every sum: no fused multiply-add.
 *   inv[j] = 1 / S[j][j] if S[j][j] > 0, else 0; a coordinate with inv[j] = 0 starts at 0 and is never visited.
 *   start   g = -b;  then, for j ascending with h0[j] != 0:  g[l] = g[l] + h0[j] * S[l][j] for every l.
 *   sweep   for j = 0 .. k-1 in order:  x = h[j] - g[j] * inv[j];  hn = x > 0 ? x : 0;  D = hn - h[j];  if D != 0:
 *           g[l] = g[l] + D * S[l][j] for every l, h[j] = hn.  The sweep's measure is the maximum of |D| / (hn + 1e-15)
 *           over the coordinates that moved (0 when none did).
 *   stop    after the sweep whose measure is < cd_tol, or after cd_maxit sweeps.  (cd_tol = 0 always runs to the cap.)
 * A maximum does not depend on an order, nothing in a sweep is a sum over lanes, and every row is independent: each row's
 * result and sweep count are the same for any split of the rows.  The sweep counts are an output (int32 per row).
 *
 * The loss ||A - W diag(d) H||_F^2, gficf_nmf_loss_device, without densifying:
 *   ||A||^2 - 2 sum_i sum_j (A'W)[i][j] d[j] H[j][i] + sum_jl (d[j] (W'W)[j][l] d[l]) (H H')[j][l],
 * every sum over fixed chunks added in order.  With track_loss the chain records it once per iteration.  It is never part
 * of the stop rule: it cancels against ||A||^2, so its last digits mean nothing once the fit is good.
 *
 * New cells, gficf_nmf_project_device: S = W'W + ridge, B = A_new'W, H_new = nnls(S, B) from zero; row i is cell i in the
 * units of (diag(d) H)', the cells of the training run.
 *
 * Workspace and deferred errors.  The first word of a workspace is its status word: zero before the first entry that uses
 * it (gficf_nmf_sync reads it behind everything enqueued and clears it; the host entries do both themselves).  Deferred:
 * a row index out of range or a bad column pointer (GFICF_ERR_BAD_CSC), a non-finite value of A, W or H, and a negative
 * entry of A or of a start (GFICF_ERR_BAD_VALUE).  The chain stops at the first read-back that sees the status word set.
 * Refused at the call: GFICF_ERR_UNSUPPORTED for k > GFICF_NMF_MAX_K and for G or N > 2^31 - 1; GFICF_ERR_INVALID_ARG for
 * sizes below 1, k > min(G, N) in the chain, negative or NaN limits, NULL pointers, a workspace that is too small. */
#ifndef GFICF_NMF_H
#define GFICF_NMF_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_NMF_ABI_VERSION 1
#define GFICF_NMF_MAX_K 128
#define GFICF_NMF_LD(k) (((k) + 7) & ~7)
#define GFICF_NMF_LP(k) ((k) <= 16 ? 16 : (k) <= 32 ? 32 : (k) <= 64 ? 64 : 128)
#define GFICF_NMF_NNLS_WS_BYTES 1024

int gficf_nmf_abi_version(void);

/* Bytes of device scratch of every entry below on a G x N matrix (or N x G: the size is symmetric) of nnz entries; 0 on
 * sizes every entry refuses.  gficf_nnls_device alone needs GFICF_NMF_NNLS_WS_BYTES. */
size_t gficf_nmf_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int k);

/* The solve.  d_S: k x k, row pitch ld_s >= k;  d_B, d_H0 (or NULL: from zero), d_H: M x GFICF_NMF_LD(k);  d_sweeps: M
 * int32.  d_H may be d_H0.  Only enqueues. */
int gficf_nnls_device(gficf_ctx* ctx, int64_t M, int k, const double* d_S, int ld_s, const double* d_B, const double* d_H0, double cd_tol,
                      int cd_maxit, double* d_H, int32_t* d_sweeps, void* ws, size_t ws_bytes);

/* One half-step (steps 1 - 3) on a CSC matrix of n_in rows and n_out columns: from the factor d_X (n_in x ld) to the factor
 * d_Y (n_out x ld, normalised) and d_d (k).  warm != 0: d_Y and d_d hold the previous factor and scaling on entry, and the
 * solve starts from their product.  Optional outputs (NULL: not wanted): d_S (lp x lp), d_B (n_out x ld), d_sweeps (n_out
 * int32), d_counts (2 int64: dead factors, rows whose solve ended at cd_maxit above cd_tol).  Only enqueues. */
int gficf_nmf_half_device(gficf_ctx* ctx, int64_t n_in, int64_t n_out, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                          int64_t nnz, int k, const double* d_X, double* d_Y, double* d_d, int warm, double l1, double ridge, double cd_tol,
                          int cd_maxit, double* d_S, double* d_B, int32_t* d_sweeps, int64_t* d_counts, void* ws, size_t ws_bytes);

/* d_loss: 4 f64: the loss, ||A||^2, the cross term and the quadratic term.  Only enqueues. */
int gficf_nmf_loss_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                          int k, const double* d_W, const double* d_d, const double* d_H, double* d_loss, void* ws, size_t ws_bytes);

/* The chain.  d_W0, d_W: G x ld (may be the same);  d_d: k;  d_H: N x ld.  Host outputs: h_delta (maxit f64), h_loss (maxit
 * f64, written with track_loss != 0; may be NULL otherwise), h_info (4 int64: iterations, 1 if tol stopped it, dead
 * factors, rows whose solve ended at cd_maxit in the last iteration). */
int gficf_nmf_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                     int k, const double* d_W0, double tol, int maxit, double l1_w, double l1_h, double ridge, double cd_tol, int cd_maxit,
                     int track_loss, double* d_W, double* d_d, double* d_H, double* h_delta, double* h_loss, int64_t* h_info, void* ws,
                     size_t ws_bytes);

/* New cells against a trained W (G x ld): d_H n_new x ld.  Optional outputs as in the half-step.  Only enqueues. */
int gficf_nmf_project_device(gficf_ctx* ctx, int64_t G, int64_t n_new, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                             int64_t nnz, int k, const double* d_W, double ridge, double cd_tol, int cd_maxit, double* d_H, double* d_S,
                             double* d_B, int32_t* d_sweeps, void* ws, size_t ws_bytes);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws; clears the status word. */
int gficf_nmf_sync(gficf_ctx* ctx, void* ws);

/* Host forms: colptr int32 or int64 (colptr_is_i64); dense matrices ROW-major without padding: W0, w G x k; h N x k (the
 * transpose of H); delta, loss (or NULL), info as above. */
int gficf_nmf_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x, int k,
                   const double* W0, double tol, int maxit, double l1_w, double l1_h, double ridge, double cd_tol, int cd_maxit, int track_loss,
                   double* w, double* d, double* h, double* delta, double* loss, int64_t* info);
/* w: G x k; h: n_new x k; sweeps: n_new int32 or NULL. */
int gficf_nmf_project_host(gficf_ctx* ctx, int64_t G, int64_t n_new, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                           const double* x, int k, const double* w, double ridge, double cd_tol, int cd_maxit, double* h, int32_t* sweeps);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_NMF_H */
