/* gficf_gsea_exact.h — C ABI of libgficf_gsea_exact.so: the exact one-sided tail of the enrichment score that libgficf_gsea.so
 * computes (include/gficf_gsea.h: fgsea's calcGseaStat at gseaParam = 0), on the MI355X (gfx950).  It has no permutation floor.
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) and libgficf_gsea.so are not changed.
 *
 * At gseaParam = 0 every weight is 1, so the null of a set of m genes among G is uniform over the m-subsets of the G positions
 * and depends on (G, m) only.  The share of subsets whose running sum reaches x is a lattice-path count.
 *
 * Input.  G, and n pairs (m_q, x_q): m_q an int32 set size in [1, G - 1], x_q an f64 enrichment score exactly as gficf_gsea_*
 * returns it.  Output tail_q, f64.  In the arithmetic of include/gficf_gsea.h, with i the 1-based hit index and j the number of
 * misses before that hit,
 *     top(i, j)    = fl(fl(i / m) - fl(j / (G - m)))
 *     bottom(i, j) = fl(top(i, j) - fl(1 / m))
 * and for a set with ascending 1-based positions S_1 < ... < S_m
 *     x > 0:   tail = P(maxP >= x): the share of the m-subsets with some top(i, S_i - i) >= x
 *     x < 0:   tail = P(minP <= x): the share with some bottom(i, S_i - i) <= x
 *     x == 0:  tail = 1.0
 * The comparisons are made on the same f64 expressions as the ES kernel's, so a set always counts itself: for the ES of a set,
 * tail >= 1 / C(G, m).  For an x that no set reaches the tail is 0.
 *
 * Recurrence, first-passage form (1 - survivors would cancel; here every term is positive).  A(i, j) is the probability that a
 * random subset's first t = i + j positions hold i hits and j misses and that no hit so far was blocked.  A(0, 0) = 1.  With
 * inv_t = fl(1 / (G - t)), one correctly rounded division per step t, out of state (i, j):
 *     a miss carries  fl(A * fl((G - m - j) * inv_t))  to (i, j + 1)
 *     a hit  carries  fl(A * fl((m - i) * inv_t))      to (i + 1, j), unless that hit is blocked;
 *     the mass of a blocked hit is added to the tail and goes no further
 *     A(i, j) of step t + 1 = fl(miss mass + hit mass), two roundings (gsea_exact.hip is compiled with -ffp-contract=off).
 * x > 0: hit i + 1 after j misses is blocked iff top(i + 1, j) >= x.  x < 0: the walk runs over the mirrored set (position S
 * read as G + 1 - S, which maps the m-subsets onto themselves): its hit i' after j' misses is the set's hit i = m - i' + 1 after
 * j = G - m - j' misses, and it is blocked iff bottom(i, j) <= x, the comparison being made on the set's own (i, j).  Either way
 * top and bottom are monotone in j, so hit i' is blocked exactly for j' <= J(i') (a staircase, J found by bisection on j' with
 * the expression above, -1 if never), no mass lies at or under the staircase, and the tail has at most G terms.  The sweep
 * ends with the last step that can block a hit, t = max over i' of J(i') + i' - 1.
 *
 * Order of the additions (fixed: no floating-point atomics; a pair's result does not depend on the batch it is in, and the same
 * input gives the same bits on every call).  R is the smallest power of two with 64 R >= m + 1.  One wave computes a pair; lane l
 * of 64 holds the hit indices [l R, (l + 1) R) and one partial sum.  In step t the lane adds the blocked mass out of its
 * indices l R + R - 1, l R + R - 2, ..., l R in that order to its partial sum (an index that blocks nothing adds +0.0).  After
 * the last step the 64 partial sums are folded as lane l += lane (l xor d) for d = 32, 16, 8, 4, 2, 1.
 *
 * Accuracy.  A path factor takes 4 roundings per step (inv_t, the count times inv_t, the product with A, the sum), at most G
 * steps, and the tail is a sum of at most G positive terms: relative error at most (2 G + G / 2) 2^-52 to first order against
 * the exact rational.  The contract is 4 G 2^-52 whenever that rational is >= 1e-290.  Below 1e-290 the result may lose
 * digits or come out 0 (subnormal products); it is never negative, NaN or above the true value by more than the bound.
 *
 * Rejected, deferred to gficf_gsea_tail_sync: m outside [1, G - 1] (GFICF_ERR_INVALID_ARG); x not finite or |x| > 1
 * (GFICF_ERR_BAD_VALUE); the tail of such a pair is NaN.  At once: G < 2 or n < 0 (GFICF_ERR_INVALID_ARG), G > 131 072 or
 * n > 2^31 - 1 (GFICF_ERR_UNSUPPORTED).  A size above GFICF_GSEA_EXACT_MAX_SIZE = 4095 (64 lanes of at most 64 registers) gets
 * tail = NaN: that is not an error.
 *
 * What the Python layer makes of it (gficf_amd.gsea(..., exact=True)), with nGeZero and nLeZero of the pathway's size from
 * the sampled null of gficf_gsea_*:
 *     pval_exact = min(1, tail * (nsim + 1) / (n0 + 1)),  n0 = nGeZero if ES > 0, nLeZero if ES < 0;  1 if ES == 0
 * the exact one-sided tail divided by a sampled probability of the sign.  The numerator of fgseaSimple's estimator converges to
 * P(ES >= x) = P(maxP >= x) - P(maxP >= x, -minP >= maxP), so pval_exact is at least the limit of the simple estimator; the
 * difference is negligible once p is small.  The sign is not a fair coin in f64: mathematically tied sets split by the last
 * bit (at G = 12, m = 6 there are 478 positive and 400 negative sets). */
#ifndef GFICF_GSEA_EXACT_H
#define GFICF_GSEA_EXACT_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_GSEA_EXACT_ABI_VERSION 1
#define GFICF_GSEA_EXACT_MAX_G 131072
#define GFICF_GSEA_EXACT_MAX_SIZE 4095

int gficf_gsea_exact_abi_version(void);

/* Device scratch of gficf_gsea_tail_device: the status word and the G reciprocals inv_t.  0 for sizes it rejects at once. */
size_t gficf_gsea_tail_workspace_bytes(int64_t G, int64_t n);

/* Device-resident form.  d_size: n int32; d_es: n f64; d_tail: n f64.  Only enqueues on the context's stream; call
 * gficf_gsea_tail_sync with the same workspace to wait and collect the deferred errors. */
int gficf_gsea_tail_device(gficf_ctx* ctx, int64_t G, int64_t n, const int32_t* d_size, const double* d_es, double* d_tail, void* ws,
                           size_t ws_bytes);
/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_gsea_tail_sync(gficf_ctx* ctx, const void* ws);

/* Host form: host arrays in and out. */
int gficf_gsea_tail_host(gficf_ctx* ctx, int64_t G, int64_t n, const int32_t* size, const double* es, double* tail);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_GSEA_EXACT_H */
