/* gficf_markers.h — C ABI of libgficf_markers.so: marker genes, the one-vs-rest Mann-Whitney U test of findClusterMarkers()
 * (reference R/deGenes.R:15-60) for every cluster in one call, on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) is not changed by it.
 *
 * What is computed, for gene g and cluster c (n1 = cells of c, n2 = N - n1), with the reference's arithmetic
 * (src/rcpp_parallel_mann_whitney.cpp:40-104, src/mann_whitney.cpp), its quirks included:
 *   - average ranks over all N cells of the gene, ties by exact f64 equality; -0.0 equals 0.0; every zero (implicit, stored,
 *     -0.0) is one tie group; negative values rank below it;
 *   - U1 = R_c - n1(n1+1)/2, U2 = R_rest - n2(n2+1)/2, exact (2 x rank sums are kept as int64);
 *   - mu = floor(n1 n2 / 2)  (the reference divides a size_t);
 *   - z = (U1 < U2 ? U1 - mu : U2 - mu), then z < 0 ? z + 0.5 : z - 0.5, then z / sigma: so U1 == U2 gives p < 1;
 *   - sigma = sqrt((n1 n2 / 12) ((n1 + n2 + 1) - T / ((n1 + n2)(n1 + n2 - 1)))) in f64, in this order, without fused
 *     multiply-adds; T = sum over the tie groups (the zero group included) of t^3 - t, exact as an int64 for N <= 2 097 151
 *     (larger N is GFICF_ERR_UNSUPPORTED); converted to f64 once, which equals the reference's running f64 sum for N <= 208 063
 *     (N^3 < 2^53), beyond that it is the correctly rounded exact value;
 *   - p = erfc(|z| / sqrt(2)) (= 2 gsl_cdf_gaussian_P(z) for z < 0, 2 Q(z) otherwise); p = 1 exactly when the gene holds one
 *     distinct value;
 *   - log2FC = log2(((S_c + n1) / n1) / ((S_rest + n2) / n2)), S = sum of the values (the reference's avg(v + 1)); the sums are
 *     accumulated as 128-bit fixed-point integers, so the result does not depend on the order of the additions: the same input
 *     gives the same bits on every call, and permuting the cells together with their labels changes nothing.  A gene whose
 *     largest |value| would push the fixed-point scale below 2^64 (|v| >= 2^(61 - bit_width(N))) sums in f64 instead, in its
 *     sorted order and with the rest's sum built without subtraction: as accurate as the reference's f64 sums, just as
 *     deterministic, and slower (one thread walks such a gene).
 * Rejected: a NaN or infinite value (GFICF_ERR_BAD_VALUE), C < 2, an empty cluster, a label outside [0, C)
 * (GFICF_ERR_INVALID_ARG), a malformed CSC (GFICF_ERR_BAD_CSC).
 * Outputs are G x C, column-major f64: column c belongs to label c (callers number labels in base::unique order). */
#ifndef GFICF_MARKERS_H
#define GFICF_MARKERS_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_MARKERS_ABI_VERSION 1

int gficf_markers_abi_version(void);

/* Device scratch of gficf_cluster_markers_device for G genes, N cells, nnz stored entries and C clusters.  About
 * 60 B per stored entry plus 32 B per (gene, cluster) pair. */
size_t gficf_cluster_markers_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int32_t C);

/* Device-resident form: the genes x cells CSC matrix (d_colptr: N + 1 int64, d_rowidx / d_x: nnz = d_colptr[N] entries),
 * d_cluster: one label in [0, C) per cell; d_p, d_lfc: G x C column-major.  Only enqueues on the context's stream; call
 * gficf_cluster_markers_sync with the same workspace to wait and to collect the deferred input errors. */
int gficf_cluster_markers_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                                 int64_t nnz, const int32_t* d_cluster, int32_t C, void* ws, size_t ws_bytes, double* d_p, double* d_lfc);
/* gficf_ctx_sync, then the deferred errors of the marker kernels that wrote into ws. */
int gficf_cluster_markers_sync(gficf_ctx* ctx, const void* ws);

/* Host form, shaped like gficf_cluster_signatures_host: colptr int32 or int64 (colptr_is_i64), p and lfc G x C. */
int gficf_cluster_markers_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                               const double* x, const int32_t* cluster, int32_t C, double* p, double* lfc);

/* rcpp_parallel_WMU_test(matX, matY) (src/rcpp_parallel_mann_whitney.cpp:107-129): X is G x n1, Y is G x n2, column-major f64;
 * out is G x 2, column-major: [p, log2FC] of X against Y. */
int gficf_cluster_markers_dense_host(gficf_ctx* ctx, int64_t G, int64_t n1, const double* X, int64_t n2, const double* Y, double* out);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_MARKERS_H */
