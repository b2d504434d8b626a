/* gficf_od.h — C ABI of libgficf_od.so: the overdispersed genes of findOverDispersed() (reference
 * R/dimensinalityReduction.R:235-308, after pagoda2), the gene selection (use.odgenes) and variance scaling (var.scale) of
 * runPCA() / runLSA(), on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links together with libgficf_hvg.so (for
 * gficf_hvg_moments_device): it takes that library's gficf_ctx and uses its stream, device scratch, radix sort, status codes and
 * gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) and the ABI of every other add-on are not changed.
 *
 * All arithmetic is f64; od.hip is compiled with -ffp-contract=off and without fast-math.  There are no floating-point atomics
 * and every sum has a fixed order ("folded sum": gficf_hvg.h): the same input gives the same bits on every call.
 *
 * STATED DIFFERENCE, the basis.  The reference fits mgcv::gam(v ~ s(m, k = gam.k)), whose default basis is the thin-plate
 * regression spline: an eigen-truncation of an n x n radial matrix, taken above 2 000 genes on a random subsample of 2 000
 * knots.  It is neither reproducible nor worth a device eigen-solve.  This library fits the same model on mgcv's other standard
 * basis, the cubic regression spline: gam(v ~ s(m, k = gam.k, bs = "cr")) with the smoothing parameter chosen by GCV.  The two
 * bases span nearly the same smooth functions at k = 5.  There is no R where this library is built: how far the two fits are
 * apart has NOT been measured.
 *
 * Inputs, per gene g: m_g (the ICF weight), var_g and nobs_g of the raw counts over all N cells, zeros included, with the n - 1
 * denominator (step 1 of gficf_hvg.h).  v_g = log(var_g).  Gene g is VALID iff v_g is finite and nobs_g >= min_gene_cells (and
 * m_g is finite).  n = the number of valid genes.
 *
 * 1. Fit.  n < 1.5 * gam_k (or gam_k < 2): the straight line v ~ m by least squares (the reference's lm branch).  Otherwise
 *    x_0 < ... < x_{u-1} are the distinct m of the valid genes (stable radix sort, then a scan); knot j (j = 0 .. k - 1) sits at
 *    sorted position t = j (u - 1) / (k - 1), linearly interpolated between x_floor(t) and x_ceil(t) (mgcv's place.knots).
 *    u < k: the straight line (STATED DIFFERENCE: mgcv stops).  The straight line is the same code with the two knots x_0 and
 *    x_{u-1} and no penalty; u = 1: the mean.
 *    The basis is the natural cubic spline in its value-at-knots form (Wood, Generalized Additive Models, 4.1.2): spacings h_j,
 *    D the (k - 2) x k second-difference matrix, B the (k - 2) x (k - 2) tridiagonal one, F = B^-1 D padded with a zero first
 *    and last row, the penalty S = D^T B^-1 D.  The design row of an m in [kn_j, kn_{j+1}] is
 *      a- e_j + a+ e_{j+1} + c- F_j + c+ F_{j+1},   a- = (kn_{j+1} - m) / h_j,   a+ = (m - kn_j) / h_j,
 *      c- = ((kn_{j+1} - m)^3 / h_j - h_j (kn_{j+1} - m)) / 6,   c+ = ((m - kn_j)^3 / h_j - h_j (m - kn_j)) / 6.
 *    The rows sum to 1, so fitted values and GCV score are those of beta = argmin |v - X beta|^2 + lambda beta^T S beta
 *    (mgcv's intercept and sum-to-zero constraint reparameterise the same space).
 *
 * 2. lambda.  GCV(lambda) = n RSS / (n - tr A)^2.  X^T X = L L^T, L^-1 S L^-T = U diag(s) U^T (cyclic Jacobi), the two smallest
 *    s_i set to exactly 0 (the penalty's null space), z = U^T L^-1 X^T (v - vbar):
 *      tr A = sum 1 / (1 + lambda s_i),   RSS = sum (v - vbar)^2 - sum z_i^2 (2 / (1 + lambda s_i) - 1 / (1 + lambda s_i)^2).
 *    The search is fixed: rho = ln lambda on the 97 grid points ln(10) (-12 + j / 4), the first smallest, then 60 golden-section
 *    steps on [rho_{j-1}, rho_{j+1}] (c = hi - phi (hi - lo), d = lo + phi (hi - lo); GCV(c) < GCV(d) keeps [lo, d], else
 *    [c, hi]; the midpoint of the last bracket); at an end of the grid, that end.  sp >= 0 fixes lambda instead (mgcv's sp).
 *    The device takes the sums in a fixed order: vbar, then X^T X, X^T (v - vbar), sum (v - vbar)^2 (workgroup b of nb adds the
 *    genes b 256 + t, + nb 256, ... in thread t; folded sums; the nb partial sums folded again).  The k x k stage runs on the
 *    host in plain f64 C++ inside this library: gficf_od_fit_device waits for some 60 doubles between two launches.
 *
 * 3. res_g = v_g - fit_g for valid genes, -Inf otherwise.  lp_g = pf(exp(res_g), nobs_g, nobs_g, lower.tail = FALSE,
 *    log.p = TRUE): with a = nobs_g / 2 and z = 1 / (1 + e^res) this is log I_z(a, a), formed in log space.  res >= 0:
 *      lp = a (log z + log(1 - z)) - log a - (2 lgamma(a) - lgamma(2a)) + log CF,   log z = -softplus(res), log(1 - z) = -softplus(-res),
 *    CF the modified-Lentz continued fraction of the incomplete beta.  res < 0, by symmetry: log1p(-exp(lp(-res))).
 *    res = -Inf: 0.  nobs = 0: NaN (R's pf at df 0).  STATED DIFFERENCE: where exp(res) overflows R returns -Inf; here lp stays finite.
 *
 * 4. lpa = bh.adjust(lp, log = TRUE), literally, over the non-NaN lp: ordered ascending (stable: ties by row),
 *    q_i = lp_(i) + log(n' / i), the running minimum from the end, scattered back; NaN stays NaN.  log(n' / i) is taken on the
 *    host by the C library: gficf_od_bh_log_device waits for n' (one int32).
 *
 * 5. qv_g = qchisq(lp_g, N - 1, lower.tail = FALSE, log.p = TRUE) / N: the x with log Q((N - 1) / 2, x / 2) = lp_g, by Newton in
 *    log space (bracketed) from a Wilson-Hilferty start; Q from the series of P where x / 2 < a + 1, from the Legendre
 *    continued fraction above.  lp = 0: 0.  lp = -Inf: +Inf.  lp > 0, NaN or df <= 0: NaN.
 *    Every iteration has a cap (200 000 terms, 200 Newton steps): a value that hits one raises GFICF_ERR_BAD_VALUE at gficf_od_sync.
 *
 * 6. gsf_g = sqrt(min(max(qv_g, min_adjusted_variance), max_adjusted_variance) / exp(v_g)); NaN goes through the clip, as R's
 *    pmax / pmin; a gsf that is not finite becomes 0.
 *
 * The status word.  The first 4 bytes of a workspace hold the deferred errors; the caller zeroes them before the first entry
 * on a fresh workspace, gficf_od_sync clears them after reading.  The host entries do both themselves. */
#ifndef GFICF_OD_H
#define GFICF_OD_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_OD_ABI_VERSION 1
/* the most knots of the spline (gam_k: below 2 the straight line, 3 .. GFICF_OD_K_MAX the spline; 2 is refused) */
#define GFICF_OD_K_MAX 8
/* entries of the info block of a fit (all f64): 0 n, 1 u, 2 the basis size used (0 no valid gene, 1 the mean, 2 the straight
 * line, else gam_k), 3 lambda, 4 the GCV score, 5 tr A, 6 vbar, 7 RSS, 8 .. 15 the knots (NaN beyond the basis size) */
#define GFICF_OD_INFO 16

int gficf_od_abi_version(void);

/* Device scratch of every device entry below (one layout) for lists of up to G values and, for gficf_od_select_scale_device,
 * N columns (else N = 0).  0 for sizes the entries reject. */
size_t gficf_od_workspace_bytes(int64_t G, int64_t N);

/* Steps 1 - 3 up to res.  d_m, d_var: G f64, d_nobs: G int32.  d_v, d_fit (NaN at an invalid gene), d_res: G f64; d_valid: G
 * int32.  info (host, GFICF_OD_INFO f64, may be NULL).  sp < 0 (or NaN): the GCV search.  Waits for the stream once, for the
 * host stage; d_fit and d_res are then only enqueued.  A singular X^T X is GFICF_ERR_BAD_VALUE. */
int gficf_od_fit_device(gficf_ctx* ctx, int64_t G, const double* d_m, const double* d_var, const int32_t* d_nobs, int32_t gam_k, int32_t min_gene_cells,
                        double sp, void* ws, size_t ws_bytes, double* d_v, int32_t* d_valid, double* d_fit, double* d_res, double* info);

/* Step 3 over arrays: d_lp[i] = log I_z(a_i, a_i), z = 1 / (1 + exp(res_i)).  Only enqueues. */
int gficf_od_logpf_device(gficf_ctx* ctx, int64_t n, const double* d_res, const double* d_a, void* ws, size_t ws_bytes, double* d_lp);

/* Step 5 over an array: d_x[i] = qchisq(lp_i, df, lower.tail = FALSE, log.p = TRUE).  Only enqueues. */
int gficf_od_logqchisq_device(gficf_ctx* ctx, int64_t n, const double* d_lp, double df, void* ws, size_t ws_bytes, double* d_x);

/* Steps 3, 5, 6 per gene from d_res, d_nobs, d_v and the number of cells N: d_lp, d_qv, d_gsf (G f64).  Only enqueues. */
int gficf_od_scores_device(gficf_ctx* ctx, int64_t G, const double* d_res, const int32_t* d_nobs, const double* d_v, int64_t N, double min_adjusted_variance,
                           double max_adjusted_variance, void* ws, size_t ws_bytes, double* d_lp, double* d_qv, double* d_gsf);

/* Step 4.  Waits for the stream once (the count of the non-NaN lp); d_lpa is then only enqueued. */
int gficf_od_bh_log_device(gficf_ctx* ctx, int64_t G, const double* d_lp, void* ws, size_t ws_bytes, double* d_lpa);

/* Rows selected and scaled: from the G x N CSC (d_colptr N + 1 int64, d_rowidx int32, d_x f64, nnz entries), a row mask
 * (d_mask, G int32, non-zero selects) and a scale per row (d_scale, G f64; NULL: 1) to the CSC of the selected rows, renumbered
 * in ascending order and multiplied by their scale: d_out_colptr (N + 1 int64), d_out_rowidx and d_out_x (room for nnz
 * entries), d_nsel (one int32: the rows selected).  A count pass, a scan, a write pass; an entry whose scale is 0 stays stored,
 * as 0.  d_mask NULL: only d_out_x is written (nnz values, the structure is shared; the other outputs may be NULL).  A row index
 * or column pointer out of range is GFICF_ERR_BAD_CSC at gficf_od_sync; nothing is written outside the outputs.  Only enqueues. */
int gficf_od_select_scale_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                                 const int32_t* d_mask, const double* d_scale, void* ws, size_t ws_bytes, int64_t* d_out_colptr, int32_t* d_out_rowidx,
                                 double* d_out_x, int32_t* d_nsel);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws (cleared once read). */
int gficf_od_sync(gficf_ctx* ctx, const void* ws);

/* Steps 1 - 6 from host arrays m, var (f64) and nobs (int32) of G genes and the number of cells N >= 2.  Per gene (G each): v,
 * fit, res, lp, lpa, qv, gsf (f64) and valid (int32); info: GFICF_OD_INFO f64.  Every output may be NULL. */
int gficf_od_from_moments_host(gficf_ctx* ctx, int64_t G, int64_t N, const double* m, const double* var, const int32_t* nobs, int32_t gam_k,
                               int32_t min_gene_cells, double min_adjusted_variance, double max_adjusted_variance, double sp, double* v, int32_t* valid,
                               double* fit, double* res, double* lp, double* lpa, double* qv, double* gsf, double* info);

/* The whole procedure from the raw counts on the host (G x N CSC; colptr int32 or int64) and m: the moments
 * (gficf_hvg_moments_device; var f64 and nobs int32, G each), then as gficf_od_from_moments_host. */
int gficf_od_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x, const double* m,
                  int32_t gam_k, int32_t min_gene_cells, double min_adjusted_variance, double max_adjusted_variance, double sp, double* var, int32_t* nobs,
                  double* v, int32_t* valid, double* fit, double* res, double* lp, double* lpa, double* qv, double* gsf, double* info);

/* gficf_od_select_scale_device from and to host arrays (mask and scale may each be NULL).  out_rowidx and out_x: room for the
 * input's entries, out_colptr[N] of them written.  A mask that selects no row is GFICF_ERR_INVALID_ARG. */
int gficf_od_select_scale_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                               const int32_t* mask, const double* scale, int64_t* out_colptr, int32_t* out_rowidx, double* out_x, int32_t* out_nsel);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_OD_H */
