/* gficf_gsva.h — C ABI of libgficf_gsva.so: GSVA scores of every cell within its cluster and the per-(pathway, cluster) sums
 * of the limma contrasts, the method = "GSVA" branch of runGSEA() (reference R/pathwayAnalisys.R:97-138: per cluster
 * GSVA::gsva(gficf[, cells], pathways, kcdf = "Gaussian", method = "gsva"), then limma on the score matrix), for all clusters
 * and pathways in one call, on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, radix sort, status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * Inputs.  The GF-ICF matrix, G genes x N cells, f64, stored zeros allowed, in two sparse forms of the same nnz entries:
 *   gene-major, grouped:  seg_ptr holds G * C + 1 int64 offsets; segment s = g * C + c holds the stored entries of gene g in
 *                         the cells of cluster c (cell[e], x[e]), each cell at most once;
 *   cell-major:           colptr holds N + 1 int64 offsets; the entries of cell j are row[e] (strictly ascending genes) and
 *                         src[e], the index of the same entry in the gene-major arrays.
 * cluster[N]: int32 in [0, C).  Pathways in CSR form (the gficf_gsea_* form): ptr holds P + 1 int64 offsets, members the int32
 * rows.  min_size, max_size.
 *
 * Rejected, all deferred to gficf_gsva_sync: a NaN or infinite value or density (GFICF_ERR_BAD_VALUE); a cluster id outside
 * [0, C), a member outside [0, G), a member repeated within a pathway, an entry in a segment that is not its cluster's, more
 * entries in a segment than its cluster has cells, a cell or src index out of range, rows of a cell that do not ascend, offsets
 * that leave [0, nnz] or [0, n_members] (GFICF_ERR_INVALID_ARG).  At once: G > GFICF_GSVA_MAX_G = 131 072 (the position mask of
 * a set is G bits of LDS), a cell with more than GFICF_GSVA_MAX_CELL_NZ = 4 096 stored entries (the two sorted lists of a
 * cell's stored genes take 20 B of LDS per entry, padded to a power of two), G * C, P * C beyond 2^31 - 1 (GFICF_ERR_UNSUPPORTED).
 *
 * The stages are per cluster c with n = n_c cells: GSVA's method = "gsva" at kcdf = "Gaussian", tau = 1, mx.diff = TRUE,
 * abs.ranking = FALSE.  All arithmetic is f64, written out operation by operation; gsva.hip is compiled with
 * -ffp-contract=off.  A "folded sum" over a segment is: thread t of 256 adds the terms t, t + 256, ... in turn, then the 256
 * partial sums are folded pairwise (t with t + 128, then + 64, ... + 1).  nz is the segment's length, z = n - nz its zeros.
 *
 * 1. Gene filter.  mean = (folded sum of x_i) / n;  ss = (folded sum of (x_i - mean) * (x_i - mean)) + z * (mean * mean);
 *    sd = sqrt(ss / (n - 1)).  Gene g is kept in cluster c iff n >= 2 and sd >= 1e-10 (GSVA's constant-gene filter).  G_c is
 *    the number of kept genes; they keep their row order.  sd is 0 where n < 2.
 *
 * 2. Density.  r = 0.7071067811865476 / (sd / 4)  (the bandwidth is sd / 4; r = 1 / (bw * sqrt 2)).
 *    Phi((a - b) / bw) is evaluated as 0.5 * erfc((b - a) * r), exactly, where GSVA reads a 10 000-step table clipped at
 *    |v| > 10 (the stated relaxation).
 *      stored entry j:  L_j = (sum_i 0.5 * erfc((x_i - x_j) * r)  +  z * (0.5 * erfc(-x_j * r))) / n
 *                       the sum runs over the segment's nz entries in their stored order i = 0, 1, ..., one addition each
 *                       (i = j included: 0.5);
 *      zero cells:      L0 = ((folded sum of 0.5 * erfc(x_i * r)) + 0.5 * z) / n   when z > 0
 *      d = -log((1 - L) / L).
 *    L lies in [0.5 / n, 1 - 0.5 / n], so d is finite.  d_nz (per stored entry) and d0 (per gene and cluster) are 0 where the
 *    gene is not kept; d0 is 0 where z = 0 (no cell reads it).  The sparse form equals the dense all-pairs sum: the z zeros
 *    of a gene are one group.  No floating-point atomics: the same input gives the same bits on every call.
 *
 * 3. Order.  Per cell the kept genes of its cluster are ordered by decreasing d (d_nz where the cell stores the gene, d0
 *    elsewhere); -0.0 equals 0.0; ties are broken by ascending row (R's order(decreasing = TRUE) is stable).  The gene at
 *    1-based position S has rank score w = |(G_c - S + 1) - G_c / 2|.
 *
 * 4. Tested pathways.  m_pc counts the members of pathway p kept in cluster c.  p is tested in c iff
 *    min_size <= m_pc <= min(max_size, G_c - 1) and m_pc >= 1.  An untested pathway is 0 in every cell of c (the reference's
 *    Matrix(0)).
 *
 * 5. Score.  With the ascending positions S_1 < ... < S_m of the kept members, their weights w_i and W = sum w_i:
 *      top_i    = (sum_{t <= i} w_t) / W - (S_i - i) / (G_c - m)
 *      bottom_i = (sum_{t <  i} w_t) / W - (S_i - i) / (G_c - m)
 *      ES = max(0, max top_i) + min(0, min bottom_i)
 *    The prefix sums are exact (multiples of 0.5 far below 2^53, so their order does not matter); each quotient is one rounded
 *    division, each difference one subtraction: ES is bit-reproducible.  This is the closed form of GSVA's sequential walk,
 *    from which it differs by that walk's rounding (some 1e-15).  W = 0 happens only for m = 1 on the middle gene of an even
 *    G_c (S = G_c / 2 + 1): ES is NaN there, as in GSVA.
 *
 * Sums for the limma step.  sum[p, c] and sumsq[p, c]: the sum of es[p, j] and of es[p, j] * es[p, j] over the cells j of
 * cluster c in ascending j, one addition each.  The contrasts are finished on the host from them (gficf_amd.gsva_de_pathways):
 * limma's lmFit / eBayes / topTable in the non-robust form without the B column, which needs limma's tmixture prior and is
 * not provided.
 *
 * Outputs.  es: P x N column-major f64.  tested: P x C, kept: G x C (int32 0 / 1, column-major).  sd, d0: G x C column-major.
 * d_nz: one f64 per stored entry, in the gene-major order.  sum, sumsq: P x C column-major. */
#ifndef GFICF_GSVA_H
#define GFICF_GSVA_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_GSVA_ABI_VERSION 1
#define GFICF_GSVA_MAX_G 131072
#define GFICF_GSVA_MAX_CELL_NZ 4096
/* the density kernel: x_i per LDS tile and x_j per pass of a workgroup (one per lane); x_j of one workgroup.  A segment of
 * more than GFICF_GSVA_JSPLIT entries takes several workgroups, each with its own range of j. */
#define GFICF_GSVA_TILE 256
#define GFICF_GSVA_JSPLIT 1024

int gficf_gsva_abi_version(void);

/* Device scratch of the two device entries (one layout serves both): the status word, 8 B per cluster, 44 B per
 * (gene, cluster) for the order of the d0 (keys, sort buffers, ranks), the sort's histograms and 4 B per (pathway, cluster).
 * 0 for sizes the entries reject. */
size_t gficf_gsva_workspace_bytes(int64_t G, int64_t N, int32_t C, int64_t P);

/* Stages 1-2, device-resident.  max_seg: an upper bound of the longest segment (it sizes the grid).  Clears the status word
 * of ws.  Only enqueues on the context's stream. */
int gficf_gsva_density_device(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* d_cluster, const int64_t* d_seg_ptr,
                              const int32_t* d_cell, const double* d_x, int64_t nnz, int64_t max_seg, void* ws, size_t ws_bytes, double* d_sd,
                              double* d_d0, int32_t* d_kept, double* d_dnz);

/* Stages 3-5 and the sums, device-resident, from given densities.  max_cell_nz: an upper bound of the longest cell (it sizes
 * the LDS lists).  fresh != 0 clears the status word of ws first; 0 keeps what gficf_gsva_density_device left there. */
int gficf_gsva_scores_device(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* d_cluster, const int64_t* d_colptr, const int32_t* d_row,
                             const int64_t* d_src, int64_t nnz, int64_t max_cell_nz, const double* d_dnz, const double* d_d0, const int32_t* d_kept,
                             int64_t P, const int64_t* d_ptr, const int32_t* d_members, int64_t n_members, int64_t min_size, int64_t max_size,
                             int32_t fresh, void* ws, size_t ws_bytes, double* d_es, int32_t* d_tested, double* d_sum, double* d_sumsq);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_gsva_sync(gficf_ctx* ctx, const void* ws);

/* Host form of the whole call: host arrays in and out; the score matrix stays on the device between the stages.  sd, d0 and
 * dnz may be NULL. */
int gficf_gsva_host(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* cluster, const int64_t* seg_ptr, const int32_t* cell,
                    const double* x, const int64_t* colptr, const int32_t* row, const int64_t* src, int64_t P, const int64_t* ptr,
                    const int32_t* members, int64_t min_size, int64_t max_size, double* es, int32_t* tested, int32_t* kept, double* sd, double* d0,
                    double* dnz, double* sum, double* sumsq);

/* Host form of stages 3-5 and the sums alone: dnz holds nnz densities, src indexes it. */
int gficf_gsva_scores_host(gficf_ctx* ctx, int64_t G, int64_t N, int32_t C, const int32_t* cluster, const int64_t* colptr, const int32_t* row,
                           const int64_t* src, int64_t nnz, const double* dnz, const double* d0, const int32_t* kept, int64_t P, const int64_t* ptr,
                           const int32_t* members, int64_t min_size, int64_t max_size, double* es, int32_t* tested, double* sum, double* sumsq);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_GSVA_H */
