/* gficf_gsea.h — C ABI of libgficf_gsea.so: gene-set enrichment of every cluster's gene ranking, the per-cluster fgsea call of
 * runGSEA() (reference R/pathwayAnalisys.R:65-96, fgsea at gseaParam = 0), for all clusters and pathways in one call, on the
 * MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, scan, radix sort, status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * Inputs.  stats: G x C column-major f64 (data$cluster.gene.rnk: one column per cluster).  Pathways in CSR form: ptr holds
 * P + 1 int64 offsets, members the int32 rows of stats.  nsim >= 1 permutations, a 32-bit seed, min_size, max_size.
 *
 * Rejected, all deferred to gficf_gsea_sync: a NaN or infinite statistic (GFICF_ERR_BAD_VALUE); a member outside [0, G) and a
 * member repeated within a tested pathway (GFICF_ERR_INVALID_ARG; the repeat shows as popcount(mask) != length).  At once:
 * G > GFICF_GSEA_MAX_G = 131 072 (the gene mask of a set is G bits of LDS: 16 KiB), G * C or P * C beyond 2^31 - 1
 * (GFICF_ERR_UNSUPPORTED).
 *
 * Order.  Per cluster c the genes are ordered by decreasing statistic; -0.0 equals 0.0; ties are broken by ascending row
 * (fgsea leaves ties to R's order() and warns; cluster.gene.rnk always has a tail of equal zeros, so the order is fixed here).
 * r_c(g) is the 0-based position of gene g.
 *
 * Tested pathways.  Pathway p of size m = ptr[p + 1] - ptr[p] is tested iff min_size <= m <= min(max_size, G - 1) (and m >= 1).
 * An untested pathway has 0 in every output (the reference's Matrix(0)); its members are not looked at.
 *
 * Enrichment score: fgsea's calcGseaStat at gseaParam = 0 (every weight |r|^0 = 1), scoreType "std", in f64.  For a set with
 * ascending 1-based positions S_1 < ... < S_m among G:
 *     top_i    = i / m - (S_i - i) / (G - m)
 *     bottom_i = top_i - 1 / m
 *     maxP = max top_i,  minP = min bottom_i
 *     ES = maxP if maxP > -minP;  minP if maxP < -minP;  else 0.0
 * Each quotient is one correctly rounded f64 division of exactly converted integers, each difference one f64 subtraction
 * (gsea.hip is compiled with -ffp-contract=off); max and min do not depend on the order.  ES is bit-reproducible.
 *
 * Permutations.  mix32(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16  (uint32, wrapping).
 *     c_j      = mix32(j + mix32(seed))          (wrapping add)
 *     key_j(g) = mix32(g ^ c_j)
 *     pi_j     = the positions [0, G) sorted by key_j ascending (mix32 is a bijection: no two keys tie)
 * The random set of size m of permutation j is {pi_j(0), ..., pi_j(m - 1)}: the sizes share a permutation by prefix, as fgsea's
 * sampler does.  null[d][j] is the ES of that set for the d-th distinct tested size.  A null value depends on (seed, j, G, m)
 * only: not on nsim, not on the other sizes or pathways, not on how the permutations are batched.
 *
 * Statistics of pathway p in cluster c, x running over the nsim null values of p's size (fgseaSimple's estimator):
 *     nGeEs = #{x >= ES}, nLeEs = #{x <= ES}, nGeZero = #{x >= 0}, nLeZero = #{x <= 0}
 *     geZeroMean = sum max(x, 0) / nGeZero,  leZeroMean = sum min(x, 0) / nLeZero
 *     NES  = ES / (ES > 0 ? geZeroMean : |leZeroMean|)     (NaN or Inf when that side of the null is empty, as in fgsea)
 *     pval = min((1 + nLeEs) / (1 + nLeZero), (1 + nGeEs) / (1 + nGeZero))      (integers converted to f64)
 * The two sums are taken in a fixed order: thread t of 256 adds x_t, x_(t + 256), ... in turn, then the 256 partial sums are
 * folded pairwise (t with t + 128, then + 64, ... + 1).  The same input gives the same bits on every call.
 *
 * Relaxed contract.  ES and NES are fgsea's.  The p-value is fgseaSimple's with nsim permutations, not the multilevel-splitting
 * estimate of fgseaMultilevel: it cannot go below 1 / (nsim + 1); raise nsim for a lower floor.  The random bits are this
 * library's.  All clusters share one null per size (the null of a set depends on (G, m) only when every weight is 1).
 *
 * Outputs es, nes, pval are P x C, column-major f64; null is D x nsim, row d the null of the d-th distinct tested size. */
#ifndef GFICF_GSEA_H
#define GFICF_GSEA_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_GSEA_ABI_VERSION 1
#define GFICF_GSEA_MAX_G 131072

int gficf_gsea_abi_version(void);

/* Permutations made per batch: B = min(nsim, 1024, floor(2^22 / G)), at least 1.  The rows pi_j of a batch and their sort
 * buffers take 24 B per (permutation, gene), so the scratch of the permutations stays below 96 MiB whatever nsim is; 1024 bounds
 * the null grid of one launch.  G <= GFICF_GSEA_MAX_G leaves B >= 32.  0 for G < 1 or nsim < 1. */
int64_t gficf_gsea_perm_batch(int64_t G, int64_t nsim);

/* Device scratch of gficf_gsea_device: 12 B per statistic (key, rank), 24 B of sort buffers per element of the larger of the
 * G * C statistics and the B * G entries of one batch of B = gficf_gsea_perm_batch(G, nsim) permutations, the sort's histograms,
 * 32 B per size and the D x nsim null table.  0 for sizes gficf_gsea_device rejects. */
size_t gficf_gsea_workspace_bytes(int64_t G, int32_t C, int64_t P, int64_t n_members, int32_t D, int64_t nsim);

/* Device-resident form.  d_stats: G x C; d_ptr: P + 1; d_members: n_members = d_ptr[P]; d_sizes: the D distinct tested sizes,
 * ascending, each in [1, G - 1]; d_size_idx: per pathway the index of its size in d_sizes, or -1 if it is not tested (an index
 * whose size is not the pathway's length is GFICF_ERR_INVALID_ARG at sync).  d_es, d_nes, d_pval: P x C; d_null: D x nsim or NULL.
 * Only enqueues on the context's stream; call gficf_gsea_sync with the same workspace to wait and collect the deferred errors. */
int gficf_gsea_device(gficf_ctx* ctx, int64_t G, int32_t C, const double* d_stats, int64_t P, const int64_t* d_ptr, const int32_t* d_members,
                      int64_t n_members, int32_t D, const int32_t* d_sizes, const int32_t* d_size_idx, int64_t nsim, uint32_t seed, void* ws,
                      size_t ws_bytes, double* d_es, double* d_nes, double* d_pval, double* d_null);
/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_gsea_sync(gficf_ctx* ctx, const void* ws);

/* Host form: host arrays in and out.  Sizes, D and the tested mask are derived from ptr, min_size and max_size.  null: NULL, or
 * null_rows x nsim with null_rows equal to the number of distinct tested sizes (anything else is GFICF_ERR_INVALID_ARG). */
int gficf_gsea_host(gficf_ctx* ctx, int64_t G, int32_t C, const double* stats, int64_t P, const int64_t* ptr, const int32_t* members, int64_t nsim,
                    uint32_t seed, int64_t min_size, int64_t max_size, double* es, double* nes, double* pval, double* null, int64_t null_rows);

/* pi_j alone (G int32 into out): a probe for tests and for callers who want the sampler. */
int gficf_gsea_permutation_host(gficf_ctx* ctx, int64_t G, uint32_t seed, int64_t j, int32_t* out);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_GSEA_H */
