/* gficf_tmm.h — C ABI of libgficf_tmm.so: edgeR's TMM library-size factors and counts per million, the normalize = TRUE
 * branch of gficf() and of normCounts() (reference R/gficf.R:43-47: cpm(calcNormFactors(DGEList(counts = M)))), for all cells
 * in one call, on the MI355X (gfx950), from the sparse matrix: nothing is densified.
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device scratch, status codes and gficf_last_error().  The core ABI (GFICF_HIP_ABI_VERSION) is not changed.
 *
 * Input.  The count matrix, G genes x N cells, CSC: colptr (N + 1 int32 or int64 offsets), rowidx (int32, each row at most once
 * per column), x (f64 >= 0; stored zeros allowed, they count as zeros).  Rejected, deferred to gficf_tmm_sync: a negative, NaN
 * or infinite x (GFICF_ERR_INVALID_ARG: DGEList refuses them), a row outside [0, G) or offsets that decrease or leave [0, nnz]
 * (GFICF_ERR_BAD_CSC), more cells beyond the LDS capacity than announced (GFICF_ERR_INVALID_ARG).
 *
 * All arithmetic is f64, written out operation by operation; tmm.hip is compiled with -ffp-contract=off and without fast-math.
 * There are no floating-point atomics: the same input gives the same bits on every call.  A "folded sum" over a cell is: thread
 * t of 256 adds the terms of the stored entries t, t + 256, ... of the column in turn (an entry without a term is passed over),
 * then the 256 partial sums are folded pairwise (t with t + 128, then + 64, ... + 1).
 *
 * Stage 1, column statistics (edgeR's .calcFactorQuantile and the sums behind its choice of the reference column).
 *   G' is the number of rows with any x > 0 (calcNormFactors drops the all-zero rows first).
 *   lib[c] = folded sum of x;  sq[c] = folded sum of sqrt(x).
 *   f75[c]: R's type-7 quantile at p = 0.75 of the column's G' values, zeros included:  idx = (G' - 1) * 0.75, lo = floor(idx),
 *   hi = ceil(idx), q = x_(lo); where idx > lo and x_(hi) != q, q = (1 - h) * q + h * x_(hi) with h = idx - lo;  f75 = q / lib.
 *   With z = G' - (the column's x > 0) zeros, the order statistic x_(k) (0-based) is 0 for k < z and else the (k - z)-th of the
 *   sorted positive values.  The two order statistics are returned too.  Where lib[c] = 0 (an empty column), f75 is 0 (R's 0 / 0
 *   would stop calcNormFactors at its if(); the stated relaxation).
 *
 * The reference column (host; gficf_tmm_host, or the caller of the device entries): where median(f75) < 1e-20 the first
 * argmax of sq, else the first argmin of |f75 - mean(f75)|, the mean being the exactly rounded sum (Python's math.fsum) / N.
 *
 * Stage 2, TMM factors (edgeR's .calcFactorTMM).  For cell c against the reference column r, with nO = lib[c], nR = lib[r], over
 * the n common entries (obs > 0 and ref > 0; obs = x of the cell, ref = x of the reference column in the same row):
 *   logR = log2((obs / nO) / (ref / nR));   v = (nO - obs) / nO / obs + (nR - ref) / nR / ref.
 *
 *   THE TIE RULE.  edgeR trims on the average ranks of logR and of absE = (log2(obs / nO) + log2(ref / nR)) / 2.  On integer counts
 *   mathematically tied genes (the pairs (1,1), (2,2), (3,3) for logR; (1,4), (2,2) for absE) are tied or split by the rounding of
 *   those operations, the tie groups are big, and a group across a trim boundary goes in or out as a whole: a log2 that differs
 *   in its last bit changes the kept set.  This library ranks on keys that take one correctly rounded operation and are equal
 *   exactly when the genes are mathematically tied:
 *     rank of logR := average rank of q = obs / ref     (one f64 division: 3/6 and 1/2 are the same double)
 *     rank of absE := average rank of s = obs * ref     (one f64 multiplication, exact for counts below 2^26)
 *   logR and absE are monotone in q and s within a cell, so on data without ties this is edgeR's kept set and its factor, bit for
 *   bit (checked on 800 x 40 continuous values).  On integer counts the literal port (rankdata of logR and absE as computed)
 *   deviates from this rule: on synth.counts_csc(2000, 300, 0.07) it changes the kept set of 5 of the 300 cells and a factor
 *   by up to 8.8 % (tests/test_tmm_cpu.py records it).
 *
 *   The average rank of an entry is #less + (#equal + 1) / 2 (itself among the equal).  An entry is kept where
 *   loL <= rank_q <= hiL and loS <= rank_s <= hiS, with loL = floor(n * logratioTrim) + 1, hiL = n + 1 - loL,
 *   loS = floor(n * sumTrim) + 1, hiS = n + 1 - loS, the products taken in f64 as written (10 * 0.3 is 3.0000000000000004).
 *   doWeighting != 0:  f = (folded sum of logR / v) / (folded sum of 1 / v) over the kept entries, a NaN term dropped from its
 *   own sum (na.rm);  doWeighting == 0:  f = (folded sum of logR) / (the number of kept entries whose logR is not NaN).
 *   The factor is 2^f; it is 1 where f is NaN, where n = 0 and where max |logR| over the n common entries < 1e-6.
 *   Acutoff is not an argument: at its default (-1e10) it excludes nothing finite.
 *   Outputs per cell: the factor, n and the number of kept entries (int32).
 *
 *   A cell whose n common entries fit the LDS capacity (max_lds_n, 0 = GFICF_TMM_LDS_N) is ranked from its two sorted key
 *   lists in LDS by binary search; a longer cell is ranked by a second kernel that counts over the keys in global workspace,
 *   O(n^2).  Both form the same ranks and add the same terms in the same order: the same bits.  (The LDS kernel runs in two
 *   tiers where a cell may be longer than 2 048: lists of 2 048 keys for every cell, so that several workgroups share a CU, then
 *   lists of the full capacity for the cells that did not fit.)  Stage 1 sorts a cell's positive values in LDS under the same
 *   capacity and selects by counting beyond it.
 *
 *   The factors are normalised on the host:  f / exp(mean(log f)).
 *
 * Stage 3, cpm.  out = x / (1e-6 * (lib[c] * f[c])): two multiplications and a division, one rounding each, into a CSC matrix
 * of the input's structure. */
#ifndef GFICF_TMM_H
#define GFICF_TMM_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_TMM_ABI_VERSION 1
/* the LDS capacity in keys of a cell: two u64 lists of 8 192 keys are 128 KiB of the CU's 160 KiB */
#define GFICF_TMM_LDS_N 8192

int gficf_tmm_abi_version(void);

/* Device scratch of the device entries (one layout serves all): the status word, the counters, 4 B per gene (the rows that hold
 * a count), 8 B per gene (the reference column as a dense table), 4 B per cell (the cells the first tier of the factor kernel
 * hands on), 4 B per big cell and 16 B per big entry.  big_cells,
 * big_entries: the number of cells with more stored entries than the LDS capacity, and their stored entries together (upper
 * bounds; a cell's common entries are at most its stored ones).  0 for sizes the entries reject. */
size_t gficf_tmm_workspace_bytes(int64_t G, int64_t N, int64_t big_cells, int64_t big_entries);

/* Stage 1, device-resident.  max_cell_nz: an upper bound of the longest column (it sizes the LDS list).  Clears the status
 * word of ws.  d_lib, d_sq, d_f75: N f64; d_ostat: 2 * N f64, x_(lo) of cell c at [c] and x_(hi) at [N + c]; d_gprime: one
 * int32, G'.  Only enqueues on the context's stream. */
int gficf_tmm_stats_device(gficf_ctx* ctx, int64_t G, int64_t N, const void* d_colptr, int colptr_is_i64, const int32_t* d_rowidx, const double* d_x,
                           int64_t nnz, int64_t max_cell_nz, int64_t max_lds_n, void* ws, size_t ws_bytes, double* d_lib, double* d_sq,
                           double* d_f75, double* d_ostat, int32_t* d_gprime);

/* Stage 2, device-resident, from given library sizes.  ref_col in [0, N).  fresh != 0 clears the status word of ws first; 0
 * keeps what gficf_tmm_stats_device left there.  d_factor: N f64 (not yet normalised); d_n, d_kept: N int32. */
int gficf_tmm_factors_device(gficf_ctx* ctx, int64_t G, int64_t N, const void* d_colptr, int colptr_is_i64, const int32_t* d_rowidx, const double* d_x,
                             int64_t nnz, int64_t max_cell_nz, int64_t ref_col, const double* d_lib, double logratio_trim, double sum_trim,
                             int32_t do_weighting, int64_t max_lds_n, int64_t big_cells, int64_t big_entries, int32_t fresh, void* ws,
                             size_t ws_bytes, double* d_factor, int32_t* d_n, int32_t* d_kept);

/* Stage 3, device-resident: d_out holds nnz f64.  Reads colptr only (checked: offsets that leave [0, nnz] write nothing and
 * raise the status word of ws). */
int gficf_tmm_cpm_device(gficf_ctx* ctx, int64_t N, const void* d_colptr, int colptr_is_i64, const double* d_x, int64_t nnz, const double* d_lib,
                         const double* d_factor, void* ws, size_t ws_bytes, double* d_out);

/* gficf_ctx_sync, then the deferred errors of the kernels that wrote into ws. */
int gficf_tmm_sync(gficf_ctx* ctx, const void* ws);

/* Host form of the whole call: stats, the reference column (ref_col < 0: chosen as stated above; else the caller's), the
 * factors, their normalisation and, where cpm is not NULL, the counts per million (nnz f64).  ostat, sq, f75, factor_raw, n and
 * kept may be NULL.  With factor_in not NULL only stage 3 runs, on the caller's factor_in and lib_in; where lib_in is NULL the
 * library sizes are stage 1's (cpm's lib.size = colSums), returned in lib if that is not NULL. */
int gficf_tmm_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x, int64_t ref_col,
                   double logratio_trim, double sum_trim, int32_t do_weighting, int64_t max_lds_n, const double* lib_in, const double* factor_in,
                   double* lib, double* sq, double* f75, double* ostat, int32_t* gprime, int64_t* ref_out, double* factor_raw, double* factor,
                   int32_t* n, int32_t* kept, double* cpm);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_TMM_H */
