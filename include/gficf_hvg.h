/* gficf_hvg.h — C ABI of libgficf_hvg.so: the highly variable genes of findVarGenes() (reference R/deGenes.R:72-164, the scVEGs
 * procedure of Chen et al., BMC Genomics 2016), the gene selection behind findClusterMarkers(hvg = TRUE), on the MI355X (gfx950)
 * from the sparse matrix: nothing is densified.
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, radix sort, transpose, status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * All arithmetic is f64, written out operation by operation; hvg.hip is compiled with -ffp-contract=off and without fast-math.
 * There are no floating-point atomics and every sum has a fixed order: the same input gives the same bits on every call.
 *   A "wave sum" over a list: lane l of 64 adds the terms l, l + 64, ... in turn, then the 64 partial sums are combined by the
 *   butterfly l with l ^ 32, then ^ 16, ... ^ 1 (every lane ends with the same bits).
 *   A "folded sum": thread t of 256 adds the terms t, t + 256, ... in turn, then the 256 partial sums are folded pairwise
 *   (t with t + 128, then + 64, ... + 1).
 *
 * Input: the normalised counts, G genes x N cells (N >= 2), CSC: colptr (N + 1 offsets), rowidx (int32, each row at most once per
 * column), x (f64).  A bad row index or offset is GFICF_ERR_BAD_CSC at the sync.
 *
 * 1. Moments (device; k_hv_moments, one wave per gene over the gene-major view of gficf_csc_transpose_device).
 *      nobs = the gene's stored x != 0;  mean = (wave sum of x) / N;
 *      ss   = (wave sum of (x - mean) * (x - mean) over the stored x != 0) + (N - nobs) * (mean * mean)      (two passes, as R's sd)
 *      var  = ss / (N - 1);  sd = sqrt(var);  cv = sd / mean;  lx = log10(mean);  ly = log10(cv).
 *    A gene is VALID where lx and ly are finite (R drops only NA; a constant row, ly = -Inf, would make locfit fail).  Invalid
 *    genes get NaN in fit, weights, cvDist and P and take part in nothing below, except that G counts them in step 3.
 *    n = the number of valid genes, k = floor(0.2 * n); k < 4 (n < 20) is refused with GFICF_ERR_UNSUPPORTED.
 *
 * 2. Robust local regression (device), locfit.robust(ly ~ lp(lx, nn = .2)) at its defaults deg = 2, tricube kernel, iter = 3.
 *    The valid genes are sorted by lx with the library's stable radix sort (the order-preserving 64-bit image of the double,
 *    two 32-bit passes; equal lx stay in gene order).  The fit at a point x (k_hv_locfit, one wave per point):
 *      h = the k-th smallest |lx_i - x| over all valid genes, whatever their weights (lx is sorted: the k nearest are a window
 *          found by binary search, h the larger of its two end distances);
 *      u_i = (lx_i - x) / h;  W(u) = (1 - |u|^3)^3 where |u| < 1, else 0 (a point at distance exactly h weighs nothing);
 *      S_j = wave sum of w_i W u_i^j (j = 0 .. 4),  T_j = wave sum of w_i W u_i^j ly_i (j = 0 .. 2), over the window |lx_i - x| <= h;
 *      the value is beta0 of the weighted quadratic in u, by elimination without pivoting:
 *        l1 = S1 / S0, l2 = S2 / S0;  p1 = S2 - l1 S1;  a12 = S3 - l1 S2;  a22 = S4 - l2 S2;  r1 = T1 - l1 T0;  r2 = T2 - l2 T0;
 *        p1 < 1e-10 S0:  beta0 = T0 / S0                                                                   (degree 0)
 *        else m = a12 / p1, p2 = a22 - m a12;  p2 < 1e-10 S0:  b1 = r1 / p1, beta0 = (T0 - S1 b1) / S0        (degree 1)
 *        else b2 = (r2 - m r1) / p2, b1 = (r1 - a12 b2) / p1, beta0 = (T0 - S1 b1 - S2 b2) / S0               (degree 2)
 *      h = 0: the w-weighted mean of ly over the points at x.  S0 = 0: NaN (an error in the whole procedure).
 *    Cleveland's robustness iterations: four fits at the valid genes, w = 1 at the first.  After each of the first three:
 *      res = ly - fit;  s = median |res| (R's median: the mean of the two middle values where n is even);
 *      w = max(1 - (res / (6 s))^2, 0)^2.  s = 0 leaves the weights (and so every later fit) as they are; the s of the later
 *      rounds is then 0 again.  The fourth fit's weights serve every later evaluation.
 *    STATED DIFFERENCE: locfit fits at the vertices of a kd-tree and interpolates cubically between them, residuals
 *    included.  Here every value is a direct fit.
 *
 * 3. Trusted range.  seq(a, b, by) is a + i * by for i = 0 .. floor((b - a) / by + 1e-10).
 *      g5 = seq(min lx, max lx, 0.005);  gap_i = #{valid genes: g5_i - 0.05 <= lx < g5_i + 0.05}, the bounds formed as
 *      written, counted by two searches in the sorted lx (device);  ySeq = the fit at g5 (device; R goes through
 *      log10(10^g5), here the grid value itself is used).
 *      Host: cdx0 = the first (0-based) i with gap_i > 0.005 * G (all G rows, as R's m);  j0 = the first j with
 *      ySeq[j + 1] - ySeq[j] > 0 and g5[j + 1] > 0, or len - 2 where there is none;  the points used are the indices
 *      cdx0 + 1 .. j0 + 1 (R's cdx[1]:ix[1] + 1).  No such i, cdx0 > j0 or fewer than 3 points: GFICF_ERR_BAD_VALUE,
 *      "the variance-mean trend cannot be fitted" (R would fail in nls).
 *
 * 4. Curve (host), nls(y ~ 0.5 * log10(b / x + a), start b = 1, a = 0) on x = 10^g5 of those points: Gauss-Newton with R's
 *    defaults.  Each round: the residuals r and the Jacobian J (n x 2), its QR by modified Gram-Schmidt, q = Q^T r,
 *    the relative offset sqrt(|q|^2 / (|r|^2 - |q|^2)); converged below 1e-5 (or where |r|^2 <= 1e-26 (sum y^2 + n): an exact
 *    fit, where R's ratio is 0 / 0).  Else the increment R^-1 q is tried at the step factor f (1 at the start): accepted
 *    where b / x + a > 0 everywhere and |r|^2 does not grow, then f = min(2 f, 1); else f is halved, down to 1 / 1024.
 *    At most 500 rounds.  No convergence, a singular Jacobian or f < 1 / 1024: GFICF_ERR_BAD_VALUE.
 *
 * 5. Distances (device).  g1 = seq(min lx, max lx, 0.001);  yf = 0.5 * log10(b / 10^g1 + a).  For each valid gene (one wave),
 *    over the grid points with g1 >= lx - 0.2 and g1 < lx + 0.2 (as written; two searches):  d = sqrt((g1 - lx)^2 + (yf - ly)^2),
 *    the first minimum wins.  Sign, the reference's overwritten branch kept: g1* > lx: -d;  else +d where yf* < ly, otherwise -d.
 *    cvDist = log2(10^(+-d)).  (The two lists are read through the cache, not staged in LDS: a gene reads 400 of their points.)
 *
 * 6. Mode (device), density(cvDist, kernel = "gaussian").  bw = bw.nrd0 = 0.9 * min(sd, IQR / 1.34) * n^(-1/5): sd with the
 *    n - 1 denominator (folded sums), the type-7 quartiles of the sorted cvDist ((1 - h) x_lo + h x_hi), R's fall-backs
 *    (min = 0 -> sd -> |x_1| -> 1).  grid_j = lo + j * ((hi - lo) / 511), grid_511 = hi, with lo = min - 3 bw, hi = max + 3 bw.
 *    dens_j = folded sum over i of exp(-0.5 * z * z), z = (grid_j - cvDist_i) / bw;  distMid = the grid point of the first maximum.
 *    STATED DIFFERENCE: R bins the data onto 1 024 cells, convolves by FFT and interpolates; here the sums are exact.
 *
 * 7. p-values (host).  d2 = cvDist - distMid;  tmp = c(d2[d2 <= 0], |d2[d2 < 0]|) + distMid;  mu = mean(tmp);
 *    sigma = sqrt(mean((tmp - mu)^2)) (fitdistr's MLE);  P = 0.5 * erfc((cvDist - mu) / (sigma * sqrt(2))).  The FDR
 *    (p.adjust over the valid genes) is left to the caller. */
#ifndef GFICF_HVG_H
#define GFICF_HVG_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_HVG_ABI_VERSION 1
/* points of the density grid of step 6 */
#define GFICF_HVG_KDE_N 512
/* the longest grids of steps 3 and 5 that finite positive doubles can ask for (lx in [-324, 309]) */
#define GFICF_HVG_GRID5_MAX 126601
#define GFICF_HVG_GRID1_MAX 633001
/* entries of the scalar block the host entries return (all f64; counts and indices are whole numbers):
 *   0 n, 1 k, 2-4 s of the three robustness rounds, 5 len(g5), 6 cdx0, 7 j0, 8 b, 9 a, 10 Gauss-Newton rounds, 11 len(g1),
 *   12 bw, 13 distMid, 14 mu, 15 sigma */
#define GFICF_HVG_SCALARS 16

int gficf_hvg_abi_version(void);

/* Device scratch of every device entry below (one layout serves all) for lists of up to G values, the gene-major view of a
 * G x N matrix of nnz stored entries (N = 0, nnz = 0: none, for the entries that take no matrix) and grids of up to grid_pts
 * points.  0 for sizes the entries reject. */
size_t gficf_hvg_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int64_t grid_pts);

/* Step 1, device-resident.  d_colptr: N + 1 int64.  d_mean, d_sd, d_var, d_lx, d_ly: G f64; d_nobs, d_valid: G int32.
 * Clears the status word of ws.  Only enqueues on the context's stream. */
int gficf_hvg_moments_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                             void* ws, size_t ws_bytes, double* d_mean, double* d_sd, double* d_var, int32_t* d_nobs, double* d_lx, double* d_ly,
                             int32_t* d_valid);

/* The order of step 2: d_perm (n int32) lists the positions of d_key (n f64) by ascending key, equal keys by position, the
 * positions with d_valid[i] == 0 last (d_valid NULL: all count); d_count: one int32, how many count. */
int gficf_hvg_order_device(gficf_ctx* ctx, int64_t n, const double* d_key, const int32_t* d_valid, void* ws, size_t ws_bytes, int32_t* d_perm,
                           int32_t* d_count);

/* The local fit of step 2 at m points d_at, from n points d_xs (ascending: a decrease is GFICF_ERR_INVALID_ARG at the sync),
 * d_ys and weights d_w (NULL: ones), over the k nearest (1 <= k <= n).  d_fit, d_h: m f64 (d_h may be NULL). */
int gficf_hvg_locfit_device(gficf_ctx* ctx, int64_t n, const double* d_xs, const double* d_ys, const double* d_w, int64_t k, int64_t m,
                            const double* d_at, void* ws, size_t ws_bytes, double* d_fit, double* d_h);

/* Cleveland's loop of step 2: iters + 1 fits at the data, the weights starting at 1 (d_w_in NULL) or at d_w_in.  d_w, d_fit: n
 * f64, the last round's weights and fit; d_s: iters f64. */
int gficf_hvg_robust_device(gficf_ctx* ctx, int64_t n, const double* d_xs, const double* d_ys, const double* d_w_in, int64_t k, int32_t iters,
                            void* ws, size_t ws_bytes, double* d_w, double* d_fit, double* d_s);

/* The counts of step 3 on the grid x0 + i * step, i < len: d_grid (len f64) and d_gap (len int32), the points of the
 * ascending d_xs in [grid_i - half, grid_i + half). */
int gficf_hvg_gap_device(gficf_ctx* ctx, int64_t n, const double* d_xs, double x0, double step, double half, int64_t len, void* ws, size_t ws_bytes,
                         double* d_grid, int32_t* d_gap);

/* Step 5 for n points (any order) against the curve (b, a) on the grid x0 + i * 0.001, i < len (len <= the workspace's
 * grid_pts).  d_cvdist: n f64; d_index (may be NULL): n int32, the nearest grid point, -1 where the window holds none. */
int gficf_hvg_curve_distance_device(gficf_ctx* ctx, int64_t n, const double* d_lx, const double* d_ly, double b, double a, double x0, int64_t len,
                                    void* ws, size_t ws_bytes, double* d_cvdist, int32_t* d_index);

/* Step 6 for n >= 2 values.  d_stats: 8 f64 (bw, distMid, grid lo, grid hi, sd, first and third quartile, mean); d_dens:
 * GFICF_HVG_KDE_N f64; d_argmax: one int32. */
int gficf_hvg_kde_device(gficf_ctx* ctx, int64_t n, const double* d_v, void* ws, size_t ws_bytes, double* d_stats, double* d_dens, int32_t* d_argmax);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_hvg_sync(gficf_ctx* ctx, const void* ws);

/* Steps 2 - 7 from host arrays mean and cv of G genes.  Per gene (G each): lx, ly, fit, weights, cvdist, P (f64; NaN at an
 * invalid gene) and valid (int32).  scalars: GFICF_HVG_SCALARS f64.  g5, yseq (f64) and gap (int32): GFICF_HVG_GRID5_MAX
 * entries each, len(g5) of them written.  Every output but P, valid and scalars may be NULL. */
int gficf_hvg_trend_host(gficf_ctx* ctx, int64_t G, const double* mean, const double* cv, double* lx, double* ly, int32_t* valid, double* fit,
                         double* weights, double* cvdist, double* P, double* scalars, double* g5, int32_t* gap, double* yseq);

/* The whole procedure from the CSC matrix on the host: step 1 (mean, sd, var: G f64, nobs: G int32, each may be NULL), then
 * as gficf_hvg_trend_host.  only_moments != 0 stops after step 1 (P and scalars may then be NULL too). */
int gficf_hvg_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                   int32_t only_moments, double* mean, double* sd, double* var, int32_t* nobs, double* lx, double* ly, int32_t* valid, double* fit,
                   double* weights, double* cvdist, double* P, double* scalars, double* g5, int32_t* gap, double* yseq);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_HVG_H */
