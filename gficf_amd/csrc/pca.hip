// pca.hip — runPCA / runLSA / computePCADim: the randomized SVD of the GF-ICF matrix (reference R/dimensinalityReduction.R:19-133,
// 206-230 through rsvd::rpca / rsvd::rsvd) and the projection of embedNewCells (R/cellClassifier.R:50-64).  Built into
// libgficf_pca.so, which links libgficf_hip.so and uses its context, pool, transpose, scan and error plumbing
// (include/gficf_pca.h states the algorithm and what is relaxed).
//
// Dense operands are kept ROW-major with a padded pitch ld = l rounded up to 8 (columns l .. ld - 1 hold zeros), so a gathered
// row is one coalesced read with lanes mapped to columns; the ABI's column-major matrices are converted at the boundary.  The
// small l x l matrices have the pitch LP = 16, 32, 64 or 128 (the smallest that holds l).  Launches:
//   k_pca_in         column-major -> row-major, non-finite values flagged
//   k_pca_nseg       segments of every column (PCA_SEG entries each, at least one); bad column pointers flagged; (scan)
//   k_pca_spmm       Y = A'X: one wave per (column, segment); 64 entries' indices and values are loaded at once and handed round
//                    by shuffles, the lanes of a group (8 .. 64 lanes, two columns per lane beyond 64) read one dense row; the
//                    groups' sums are added in a fixed order; a one-segment column is written straight to the result
//   k_pca_spmm_sum   the columns of several segments: their partial rows added in segment order
//   k_pca_colsum(+_fin), k_pca_rank1   w'X over fixed chunks, summed in order; Y -= a v'  (centring, never densified)
//   k_pca_gram(+_fin)   Y'Y over fixed chunks of rows, the chunks summed in order
//   k_pca_eig        l x l symmetric eigen-solve in ONE workgroup: parallel cyclic Jacobi, the matrix in LDS, the vectors behind it
//                    (l <= 90) or in global memory; sorted, the dropped directions zeroed; W L^-1/2, W L^1/2 and W come out
//   k_pca_apply      Y <- Y M for such an l x l matrix M
//   k_pca_sign, k_pca_out   the sign rule; row-major -> column-major, the k leading columns
// No floating-point atomic anywhere (the status word takes integer ORs): the same input gives the same bits on every call.
#include <cmath>
#include <vector>

#include "addon_status.h"
#include "common.h"
#include "gficf_pca.h"
#include "pca_kernels.h"                   // the kernels and launchers listed above: shared as text with svds.hip

namespace {

static_assert(PCA_MAX_L == GFICF_PCA_MAX_L, "pca_kernels.h and gficf_pca.h disagree on the widest operand");

// ------------------------------------------------------------------------------------------------ workspaces
struct PcaTmmWs {               // gficf_csc_tmm_device, the projection
  uint32_t* status;
  int64_t* seg;
  double *part, *Xrm, *Yrm;
  PcaSmall sm;
};

size_t pca_carve_tmm(char* base, int64_t nrows, int64_t ncols, int64_t nnz, int l, PcaTmmWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t ld = (size_t)pca_ld(l);
  w.status = cv.take<uint32_t>(1);
  w.seg = cv.take<int64_t>((size_t)ncols + 1);
  w.part = cv.take<double>((size_t)pca_max_units(ncols, nnz) * ld);
  w.Xrm = cv.take<double>((size_t)nrows * ld);
  w.Yrm = cv.take<double>((size_t)ncols * ld);
  pca_carve_small(cv, 1, l, w.sm);
  return cv.total();
}

struct PcaOrthWs {
  uint32_t* status;
  double *a, *b;
  PcaSmall sm;
};

size_t pca_carve_orth(char* base, int64_t m, int l, PcaOrthWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.status = cv.take<uint32_t>(1);
  w.a = cv.take<double>((size_t)m * (size_t)pca_ld(l));
  w.b = cv.take<double>((size_t)m * (size_t)pca_ld(l));
  pca_carve_small(cv, m, l, w.sm);
  return cv.total();
}

struct PcaWs {
  uint32_t* status;
  void* tr_ws;
  size_t tr_bytes;
  int64_t* tptr;
  int32_t* tidx;
  double* tx;
  int64_t *segM, *segT;
  double *part, *cells0, *cells1, *genes0, *genes1, *mu;
  PcaSmall sm;
};

size_t pca_carve(char* base, int64_t G, int64_t N, int64_t nnz, int l, PcaWs& w) {
  gficf_carver cv;
  cv.base = base;
  const size_t n1 = (size_t)(nnz > 0 ? nnz : 1), ld = (size_t)pca_ld(l);
  w.status = cv.take<uint32_t>(1);
  w.tr_bytes = gficf_csc_transpose_workspace_bytes(G, N);
  w.tr_ws = cv.take<char>(w.tr_bytes);
  w.tptr = cv.take<int64_t>((size_t)G + 1);
  w.tidx = cv.take<int32_t>(n1);
  w.tx = cv.take<double>(n1);
  w.segM = cv.take<int64_t>((size_t)N + 1);
  w.segT = cv.take<int64_t>((size_t)G + 1);
  w.part = cv.take<double>((size_t)pca_max_units(G > N ? G : N, nnz) * ld);
  w.cells0 = cv.take<double>((size_t)N * ld);             // N-row operands (pitch at least 8: the column of ones behind mu)
  w.cells1 = cv.take<double>((size_t)N * ld);
  w.genes0 = cv.take<double>((size_t)G * ld);
  w.genes1 = cv.take<double>((size_t)G * ld);
  w.mu = cv.take<double>((size_t)G);
  pca_carve_small(cv, G > N ? G : N, l, w.sm);
  return cv.total();
}

int pca_check_l(int l) {
  if (l < 1 || l > PCA_MAX_L) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "l = %d is outside [1, %d]", l, PCA_MAX_L);
  return GFICF_OK;
}

int pca_check_rsvd(int64_t G, int64_t N, int64_t nnz, int k, int l, int q) {
  if (G < 1 || N < 1 || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld, nnz = %lld: the matrix needs a row and a column", (long long)G, (long long)N, (long long)nnz);
  if (G > INT32_MAX || N > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 genes or cells");
  const int64_t n = G < N ? G : N;
  if (k < 1 || k > l || l > PCA_MAX_L || l > n)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d, l = %d: 1 <= k <= l <= min(%d, N, G) = %lld is required", k, l, PCA_MAX_L, (long long)(n < PCA_MAX_L ? n : PCA_MAX_L));
  if (q < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "q = %d: the number of power iterations cannot be negative", q);
  return GFICF_OK;
}

// Y (ncols x l, column-major) = A'X - 1 (centre'X), through the workspace's row-major copies
int pca_tmm_core(gficf_ctx* ctx, const PcaTmmWs& w, PcaCsc A, const double* d_X, int l, const double* d_centre, double* d_Y) {
  const int ld = pca_ld(l);
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_pca_in, dim3(pca_grid(A.nrows * ld)), dim3(256), 0, st, A.nrows, l, ld, d_X, w.Xrm, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  A.segptr = w.seg;
  A.max_units = pca_max_units(A.ncols, A.nnz);
  int rc = pca_csc_prepare(ctx, A, w.status);
  if (!rc) rc = pca_spmm(ctx, A, w.Xrm, l, w.Yrm, w.part, w.status);
  if (!rc && d_centre) rc = pca_centre(ctx, w.Xrm, A.nrows, d_centre, w.Yrm, A.ncols, nullptr, ld, w.sm.cpart, w.sm.cvec);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pca_out, dim3(pca_grid(A.ncols * l)), dim3(256), 0, st, A.ncols, l, ld, (const double*)w.Yrm, (const double*)nullptr, d_Y);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int pca_check_tmm(int64_t nrows, int64_t ncols, int64_t nnz, int l) {
  if (nrows < 1 || ncols < 0 || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "nrows = %lld, ncols = %lld, nnz = %lld", (long long)nrows, (long long)ncols, (long long)nnz);
  if (nrows > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 rows");
  return pca_check_l(l);
}

// the host form of Y = A'X - 1 (centre'X): gficf_csc_tmm_host and gficf_pca_project_host
int pca_tmm_host(gficf_ctx* ctx, const char* entry, int64_t nrows, int64_t ncols, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                 const double* x, const double* X, int l, const double* centre, double* Y) {
  if (nrows < 1 || ncols < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "nrows = %lld, ncols = %lld", (long long)nrows, (long long)ncols);
  if (!colptr || !X || (ncols > 0 && !Y)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  int rc = gficf_host_colptr(colptr, colptr_is_i64, ncols, "colptr", cp, &nnz);
  if (rc) return rc;
  rc = pca_check_tmm(nrows, ncols, nnz, l);
  if (rc) return rc;
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1);
  PcaTmmWs w;
  const size_t wsb = pca_carve_tmm(nullptr, nrows, ncols, nnz, l, w);
  gficf_host_io io{ctx, entry};
  gficf_carver cv;
  int64_t* d_cp; int32_t* d_ri; double *d_x, *d_X, *d_c, *d_Y; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)ncols + 1); d_ri = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_X = cv.take<double>((size_t)nrows * (size_t)l); d_c = cv.take<double>((size_t)nrows); d_Y = cv.take<double>((size_t)ncols * (size_t)l);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * cp.size());
  io.up(d_ri, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  io.up(d_X, X, sizeof(double) * (size_t)nrows * (size_t)l);
  if (centre) io.up(d_c, centre, sizeof(double) * (size_t)nrows);
  if (io.ok()) {
    pca_carve_tmm(d_ws, nrows, ncols, nnz, l, w);
    PcaCsc A{nrows, ncols, nnz, d_cp, d_ri, d_x, nullptr, 0};
    rc = pca_tmm_core(ctx, w, A, d_X, l, centre ? d_c : nullptr, d_Y);
    if (!rc) io.down(Y, d_Y, sizeof(double) * (size_t)ncols * (size_t)l);
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_rsvd_sync(ctx, d_ws);
}

}  // namespace

extern "C" {

int gficf_pca_abi_version(void) { return GFICF_PCA_ABI_VERSION; }

size_t gficf_csc_tmm_workspace_bytes(int64_t nrows, int64_t ncols, int64_t nnz, int l) {
  if (nrows < 0 || ncols < 0 || nnz < 0 || l < 1 || l > PCA_MAX_L) return 0;
  PcaTmmWs w;
  return pca_carve_tmm(nullptr, nrows, ncols, nnz, l, w);
}

int gficf_csc_tmm_device(gficf_ctx* ctx, int64_t nrows, int64_t ncols, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                         int64_t nnz, const double* d_X, int l, void* ws, size_t ws_bytes, double* d_Y) {
  GFICF_CTX_ENTER(ctx);
  int rc = pca_check_tmm(nrows, ncols, nnz, l);
  if (rc) return rc;
  if (!d_colptr || !d_X || !ws || (ncols > 0 && !d_Y) || (nnz > 0 && (!d_rowidx || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  PcaTmmWs w;
  const size_t need = pca_carve_tmm(nullptr, nrows, ncols, nnz, l, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  pca_carve_tmm((char*)ws, nrows, ncols, nnz, l, w);
  PcaCsc A{nrows, ncols, nnz, d_colptr, d_rowidx, d_x, nullptr, 0};
  return pca_tmm_core(ctx, w, A, d_X, l, nullptr, d_Y);
}

int gficf_csc_tmm_host(gficf_ctx* ctx, int64_t nrows, int64_t ncols, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                       const double* x, const double* X, int l, double* Y) {
  GFICF_CTX_ENTER(ctx);
  return pca_tmm_host(ctx, "gficf_csc_tmm_host", nrows, ncols, colptr, colptr_is_i64, rowidx, x, X, l, nullptr, Y);
}

int gficf_pca_project_host(gficf_ctx* ctx, int64_t G, int64_t n_new, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                           const double* x, const double* genes, int k, const double* centre, double* out) {
  GFICF_CTX_ENTER(ctx);
  return pca_tmm_host(ctx, "gficf_pca_project_host", G, n_new, colptr, colptr_is_i64, rowidx, x, genes, k, centre, out);
}

size_t gficf_orthonormalize_workspace_bytes(int64_t m, int l) {
  if (m < 0 || l < 1 || l > PCA_MAX_L) return 0;
  PcaOrthWs w;
  return pca_carve_orth(nullptr, m, l, w);
}

int gficf_orthonormalize_device(gficf_ctx* ctx, int64_t m, int l, double* d_Y, void* ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  int rc = pca_check_l(l);
  if (rc) return rc;
  if (m < l) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "m = %lld rows cannot hold l = %d orthonormal columns", (long long)m, l);
  if (!d_Y || !ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  PcaOrthWs w;
  const size_t need = pca_carve_orth(nullptr, m, l, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  pca_carve_orth((char*)ws, m, l, w);
  const int ld = pca_ld(l);
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_pca_in, dim3(pca_grid(m * ld)), dim3(256), 0, st, m, l, ld, (const double*)d_Y, w.a, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = pca_orth(ctx, w.sm, w.a, w.b, m, l);
  if (rc) return rc;
  hipLaunchKernelGGL(k_pca_out, dim3(pca_grid(m * l)), dim3(256), 0, st, m, l, ld, (const double*)w.a, (const double*)nullptr, d_Y);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

size_t gficf_rsvd_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int l) {
  if (G < 0 || N < 0 || nnz < 0 || l < 1 || l > PCA_MAX_L) return 0;
  PcaWs w;
  return pca_carve(nullptr, G, N, nnz, l, w);
}

int gficf_rsvd_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int64_t nnz,
                      int centre, const double* d_omega, int k, int l, int q, void* ws, size_t ws_bytes, double* d_d, double* d_cells,
                      double* d_genes, double* d_centre) {
  GFICF_CTX_ENTER(ctx);
  int rc = pca_check_rsvd(G, N, nnz, k, l, q);
  if (rc) return rc;
  if (!d_colptr || !d_omega || !ws || !d_d || !d_cells || !d_genes || (centre && !d_centre) || (nnz > 0 && (!d_rowidx || !d_x)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  PcaWs w;
  const size_t need = pca_carve(nullptr, G, N, nnz, l, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  pca_carve((char*)ws, G, N, nnz, l, w);
  const int ld = pca_ld(l);
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  // the gene-major view: M (genes x cells CSC) gives A X = M'X, its transpose T gives A'X = T'X
  rc = gficf_csc_transpose_device(ctx, G, N, d_colptr, d_rowidx, d_x, nnz, w.tptr, w.tidx, w.tx, w.tr_ws, w.tr_bytes);
  if (rc) return rc;
  const PcaCsc M{G, N, nnz, d_colptr, d_rowidx, d_x, w.segM, pca_max_units(N, nnz)};
  const PcaCsc T{N, G, nnz, w.tptr, w.tidx, w.tx, w.segT, pca_max_units(G, nnz)};
  rc = pca_csc_prepare(ctx, M, w.status);
  if (!rc) rc = pca_csc_prepare(ctx, T, w.status);
  if (rc) return rc;
  const double* mu = nullptr;
  if (centre) {                                            // mu = A'1 / N
    hipLaunchKernelGGL(k_pca_ones, dim3(pca_grid(N * 8)), dim3(256), 0, st, N, 8, w.cells0);
    GFICF_HIP_CHECK(hipGetLastError());
    rc = pca_spmm(ctx, T, w.cells0, 1, w.genes0, w.part, w.status);
    if (rc) return rc;
    hipLaunchKernelGGL(k_pca_copy, dim3(pca_grid(G)), dim3(256), 0, st, G, (const double*)w.genes0, 1.0 / (double)N, (int64_t)8, w.mu);
    hipLaunchKernelGGL(k_pca_copy, dim3(pca_grid(G)), dim3(256), 0, st, G, (const double*)w.mu, 1.0, (int64_t)1, d_centre);
    GFICF_HIP_CHECK(hipGetLastError());
    mu = w.mu;
  }
  // to_cells(X: G rows) = (A - 1 mu')X, to_genes(X: N rows) = (A - 1 mu')'X
  auto to_cells = [&](const double* X, double* out) {
    int r = pca_spmm(ctx, M, X, l, out, w.part, w.status);
    if (!r && mu) r = pca_centre(ctx, X, G, mu, out, N, nullptr, ld, w.sm.cpart, w.sm.cvec);
    return r;
  };
  auto to_genes = [&](const double* X, double* out) {
    int r = pca_spmm(ctx, T, X, l, out, w.part, w.status);
    if (!r && mu) r = pca_centre(ctx, X, N, nullptr, out, G, mu, ld, w.sm.cpart, w.sm.cvec);
    return r;
  };
  const bool tr = N < G;                                   // the tall side: cells when N >= G, genes otherwise
  double *big0 = tr ? w.genes0 : w.cells0, *big1 = tr ? w.genes1 : w.cells1, *sm0 = tr ? w.cells0 : w.genes0, *sm1 = tr ? w.cells1 : w.genes1;
  const int64_t mb = tr ? G : N, ms = tr ? N : G;
  auto to_big = [&](const double* X, double* out) { return tr ? to_genes(X, out) : to_cells(X, out); };
  auto to_small = [&](const double* X, double* out) { return tr ? to_cells(X, out) : to_genes(X, out); };
  hipLaunchKernelGGL(k_pca_in, dim3(pca_grid(ms * ld)), dim3(256), 0, st, ms, l, ld, d_omega, sm0, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = to_big(sm0, big0);
  for (int it = 0; it < q && !rc; ++it) {
    rc = pca_orth(ctx, w.sm, big0, big1, mb, l);
    if (!rc) rc = to_small(big0, sm0);
    if (!rc) rc = pca_orth(ctx, w.sm, sm0, sm1, ms, l);
    if (!rc) rc = to_big(sm0, big0);
  }
  if (!rc) rc = pca_orth(ctx, w.sm, big0, big1, mb, l);    // Q
  if (!rc) rc = to_small(big0, sm0);                       // B' = A'Q
  if (!rc) rc = pca_gram_eig(ctx, w.sm, sm0, ms, l);       // B B' = W diag(d^2) W'
  // tall side cells: cells = U d = Q W d, genes = V = B'W / d;  tall side genes: genes = Q W, cells = B'W
  if (!rc) rc = pca_apply(ctx, big0, mb, l, tr ? w.sm.Mkeep : w.sm.Mfwd, big1);
  if (!rc) rc = pca_apply(ctx, sm0, ms, l, tr ? w.sm.Mkeep : w.sm.Minv, sm1);
  if (rc) return rc;
  const double *cells = tr ? sm1 : big1, *genes = tr ? big1 : sm1;
  hipLaunchKernelGGL(k_pca_sign, dim3((unsigned)k), dim3(256), 0, st, genes, G, ld, w.sm.sgn);
  hipLaunchKernelGGL(k_pca_out, dim3(pca_grid(G * k)), dim3(256), 0, st, G, k, ld, genes, (const double*)w.sm.sgn, d_genes);
  hipLaunchKernelGGL(k_pca_out, dim3(pca_grid(N * k)), dim3(256), 0, st, N, k, ld, cells, (const double*)w.sm.sgn, d_cells);
  hipLaunchKernelGGL(k_pca_copy, dim3(1), dim3(256), 0, st, (int64_t)k, (const double*)w.sm.dv, 1.0, (int64_t)1, d_d);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_rsvd_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  const int rc = gficf_addon_read_status(ctx, ws, &st);
  if (rc) return rc;
  if (st & PCA_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row index out of range or a bad column pointer");
  if (st & PCA_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a NaN or an infinite value in the matrix or in a dense operand");
  return GFICF_OK;
}

int gficf_rsvd_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx, const double* x,
                    int centre, const double* omega, int k, int l, int q, double* d, double* cells, double* genes, double* centre_out) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: the matrix needs a row and a column", (long long)G, (long long)N);
  if (!colptr || !omega || !d || !cells || !genes || (centre && !centre_out)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  int rc = gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz);
  if (rc) return rc;
  rc = pca_check_rsvd(G, N, nnz, k, l, q);
  if (rc) return rc;
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1), n = (size_t)(G < N ? G : N);
  const size_t wsb = gficf_rsvd_workspace_bytes(G, N, nnz, l);
  gficf_host_io io{ctx, "gficf_rsvd_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t* d_ri; double *d_x, *d_om, *d_dd, *d_ce, *d_ge, *d_mu; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_ri = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_om = cv.take<double>(n * (size_t)l); d_dd = cv.take<double>((size_t)k); d_ce = cv.take<double>((size_t)N * (size_t)k);
    d_ge = cv.take<double>((size_t)G * (size_t)k); d_mu = cv.take<double>((size_t)G);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * cp.size());
  io.up(d_ri, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  io.up(d_om, omega, sizeof(double) * n * (size_t)l);
  if (io.ok()) {
    rc = gficf_rsvd_device(ctx, G, N, d_cp, d_ri, d_x, nnz, centre, d_om, k, l, q, d_ws, wsb, d_dd, d_ce, d_ge, d_mu);
    if (!rc) {
      io.down(d, d_dd, sizeof(double) * (size_t)k);
      io.down(cells, d_ce, sizeof(double) * (size_t)N * (size_t)k);
      io.down(genes, d_ge, sizeof(double) * (size_t)G * (size_t)k);
      if (centre) io.down(centre_out, d_mu, sizeof(double) * (size_t)G);
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_rsvd_sync(ctx, d_ws);
}

}  // extern "C"
