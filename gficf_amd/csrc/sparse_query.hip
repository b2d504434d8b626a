// sparse_query.hip — libgficf_sparse_query.so: the exact k nearest training cells of every query cell, both sparse
// (include/gficf_sparse_query.h states the contract by reference to include/gficf_sparse_knn.h).  The kernels are sparse_knn.hip's
// as text (sparse_knn_tiles.h), instantiated with SELF = false and the query side pointed at the second matrix.  Four launches
// per call: prepare (training), prepare (queries), tiles, merge.
#include "gficf_sparse_query.h"

#include "sparse_knn_tiles.h"

namespace {

int sq_check(int64_t G, int64_t N, int64_t nnz_t, int64_t M, int64_t nnz_q, int k, int metric) {
  if (G < 1 || N < 1 || nnz_t < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld, nnz = %lld: the training matrix needs a row and a column", (long long)G, (long long)N, (long long)nnz_t);
  if (M < 0 || nnz_q < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "M = %lld, nnz = %lld: a negative size of the query matrix", (long long)M, (long long)nnz_q);
  if (N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N = %lld exceeds int32 ids", (long long)N);
  if (M > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "M = %lld exceeds int32 ids", (long long)M);
  if (G > SK_MAX_G) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld genes exceed the %lld one query cell's dense copy may hold in LDS", (long long)G, (long long)SK_MAX_G);
  if (k < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d: at least one neighbour", k);
  if (k > GFICF_KNN_MAX_K) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "k = %d exceeds GFICF_KNN_MAX_K = %d", k, GFICF_KNN_MAX_K);
  if (k > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d neighbours asked of N = %lld training cells", k, (long long)N);
  if (!gficf_knn_metric_ok(metric)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "unknown metric %d", metric);
  return GFICF_OK;
}

// ---------------------------------------------------------------- workspace
struct SqWs {
  uint32_t* status;
  float *t_xf, *q_xf;        // the values of each matrix rounded to f32
  double *t_p0, *t_p1;       // N: the per-cell scalars of the training cells (k_sk_prepare)
  double *q_p0, *q_p1;       // M: those of the queries
  u64* part;                 // M x slices x k keys, ascending within a list
};

size_t sq_carve(char* base, int64_t N, int64_t nnz_t, int64_t M, int64_t nnz_q, int k, int slices, SqWs& w) {
  gficf_carver cv{base};
  const size_t m1 = (size_t)(M > 0 ? M : 1);
  w.status = cv.take<uint32_t>(1);
  w.t_xf = cv.take<float>((size_t)(nnz_t > 0 ? nnz_t : 1));
  w.t_p0 = cv.take<double>((size_t)N);
  w.t_p1 = cv.take<double>((size_t)N);
  w.q_xf = cv.take<float>((size_t)(nnz_q > 0 ? nnz_q : 1));
  w.q_p0 = cv.take<double>(m1);
  w.q_p1 = cv.take<double>(m1);
  w.part = cv.take<u64>(m1 * (size_t)slices * (size_t)k);
  return cv.total();
}

// one matrix's prepare pass; a matrix without columns still gets its (empty) launch
int sq_prepare(gficf_ctx* ctx, int64_t G, int64_t n, int64_t nnz, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x, int metric,
               float* xf, double* p0, double* p1, uint32_t* status) {
  const int64_t blocks = gficf_ceil_div(n, 256 / SK_LANES);
  hipLaunchKernelGGL(k_sk_prepare, dim3((unsigned)(blocks > 0 ? blocks : 1)), dim3(256), 0, ctx->stream, G, n, nnz, d_colptr, d_rowidx, d_x, metric, xf,
                     p0, p1, status);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_sparse_query_abi_version(void) { return GFICF_SPARSE_QUERY_ABI_VERSION; }

int gficf_sparse_query_shape(int64_t G, int64_t N, int64_t M, int k, int* tile_queries, int* slices, int64_t* max_genes) {
  if (!tile_queries || !slices || !max_genes) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  *max_genes = SK_MAX_G;
  *tile_queries = 0;
  *slices = 0;
  GFICF_RC(sq_check(G, N, 0, M, 0, k, GFICF_KNN_EUCLIDEAN));
  *tile_queries = sk_tile_queries(G);
  *slices = sk_slices(M, N, *tile_queries);
  return GFICF_OK;
}

size_t gficf_sparse_query_workspace_bytes(int64_t G, int64_t N, int64_t nnz_train, int64_t M, int64_t nnz_query, int k) {
  if (G < 1 || G > SK_MAX_G || N < 1 || N > 0x7FFFFFFFll || nnz_train < 0 || M < 0 || M > 0x7FFFFFFFll || nnz_query < 0 || k < 1 ||
      k > GFICF_KNN_MAX_K)
    return 0;
  SqWs w;
  return sq_carve(nullptr, N, nnz_train, M, nnz_query, k, sk_slices(M, N, sk_tile_queries(G)), w);
}

int gficf_sparse_query_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_t_colptr, const int32_t* d_t_rowidx, const double* d_t_x,
                              int64_t nnz_train, int64_t M, const int64_t* d_q_colptr, const int32_t* d_q_rowidx, const double* d_q_x,
                              int64_t nnz_query, int k, int metric, void* ws, size_t ws_bytes, int32_t* d_idx, double* d_dist,
                              float* d_dist_f32, int64_t ld_out) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(sq_check(G, N, nnz_train, M, nnz_query, k, metric));
  if (!d_t_colptr || !d_q_colptr || !ws || (M > 0 && !d_idx) || (nnz_train > 0 && (!d_t_rowidx || !d_t_x)) ||
      (nnz_query > 0 && (!d_q_rowidx || !d_q_x)))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ld_out < M) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld_out = %lld < number of queries %lld", (long long)ld_out, (long long)M);
  const int tq = sk_tile_queries(G), slices = sk_slices(M, N, tq);
  SqWs w;
  const size_t need = sq_carve(nullptr, N, nnz_train, M, nnz_query, k, slices, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  sq_carve((char*)ws, N, nnz_train, M, nnz_query, k, slices, w);
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  GFICF_RC(sq_prepare(ctx, G, N, nnz_train, d_t_colptr, d_t_rowidx, d_t_x, metric, w.t_xf, w.t_p0, w.t_p1, w.status));
  GFICF_RC(sq_prepare(ctx, G, M, nnz_query, d_q_colptr, d_q_rowidx, d_q_x, metric, w.q_xf, w.q_p0, w.q_p1, w.status));
  if (M == 0) return GFICF_OK;
  SkArgs a{};
  a.G = G; a.N = N; a.nnz = nnz_train; a.colptr = d_t_colptr; a.rowidx = d_t_rowidx; a.xf = w.t_xf; a.p0 = w.t_p0; a.p1 = w.t_p1;
  a.q_nnz = nnz_query; a.q_colptr = d_q_colptr; a.q_rowidx = d_q_rowidx; a.q_xf = w.q_xf; a.q_p0 = w.q_p0; a.q_p1 = w.q_p1;
  a.k = k; a.metric = metric; a.slices = slices; a.q_begin = 0; a.q_end = M; a.per_slice = gficf_ceil_div(N, slices); a.part = w.part;
  const int64_t tiles = gficf_ceil_div(M, tq);
  GFICF_RC((metric == GFICF_KNN_MANHATTAN ? sk_launch_tq<true, false>(ctx, a, tq, tiles) : sk_launch_tq<false, false>(ctx, a, tq, tiles)));
  hipLaunchKernelGGL(k_sk_merge, dim3((unsigned)gficf_ceil_div(M, SK_MERGE_THREADS / 64)), dim3(SK_MERGE_THREADS), 0, st, (const u64*)w.part, M, slices,
                     k, d_idx, d_dist, d_dist_f32, ld_out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_sparse_query_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  GFICF_RC(gficf_addon_read_status(ctx, ws, &st));
  if (st & SK_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row id out of range or not strictly ascending within its column, or a bad column pointer, in the training or the query matrix");
  if (st & SK_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a NaN or an infinite value in the training or the query matrix (after rounding to f32)");
  return GFICF_OK;
}

int gficf_sparse_query_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* t_colptr, int t_colptr_is_i64, const int32_t* t_rowidx,
                            const double* t_x, int64_t M, const void* q_colptr, int q_colptr_is_i64, const int32_t* q_rowidx,
                            const double* q_x, int k, int metric, int32_t* idx, double* dist) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || N < 1 || M < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld, M = %lld: the training matrix needs a row and a column", (long long)G, (long long)N, (long long)M);
  if (!t_colptr || !q_colptr || (M > 0 && !idx)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> tcp, qcp;
  int64_t nt = 0, nq = 0;
  GFICF_RC(gficf_host_colptr(t_colptr, t_colptr_is_i64, N, "the training colptr", tcp, &nt));
  GFICF_RC(gficf_host_colptr(q_colptr, q_colptr_is_i64, M, "the query colptr", qcp, &nq));
  GFICF_RC(sq_check(G, N, nt, M, nq, k, metric));
  if ((nt > 0 && (!t_rowidx || !t_x)) || (nq > 0 && (!q_rowidx || !q_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t tsz = (size_t)(nt > 0 ? nt : 1), qsz = (size_t)(nq > 0 ? nq : 1), ob = (size_t)(M > 0 ? M : 1) * (size_t)k;
  const size_t wsb = gficf_sparse_query_workspace_bytes(G, N, nt, M, nq, k);
  gficf_host_io io{ctx, "gficf_sparse_query_host"};
  gficf_carver cv;
  int64_t *d_tcp, *d_qcp; int32_t *d_tri, *d_qri, *d_idx; double *d_tx, *d_qx, *d_dist; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_tcp = cv.take<int64_t>((size_t)N + 1); d_tri = cv.take<int32_t>(tsz); d_tx = cv.take<double>(tsz);
    d_qcp = cv.take<int64_t>((size_t)M + 1); d_qri = cv.take<int32_t>(qsz); d_qx = cv.take<double>(qsz);
    d_idx = cv.take<int32_t>(ob); d_dist = cv.take<double>(ob);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_tcp, tcp.data(), sizeof(int64_t) * tcp.size());
  io.up(d_tri, t_rowidx, sizeof(int32_t) * (size_t)nt);
  io.up(d_tx, t_x, sizeof(double) * (size_t)nt);
  io.up(d_qcp, qcp.data(), sizeof(int64_t) * qcp.size());
  io.up(d_qri, q_rowidx, sizeof(int32_t) * (size_t)nq);
  io.up(d_qx, q_x, sizeof(double) * (size_t)nq);
  int rc = GFICF_OK;
  if (io.ok()) {
    rc = gficf_sparse_query_device(ctx, G, N, d_tcp, d_tri, d_tx, nt, M, d_qcp, d_qri, d_qx, nq, k, metric, d_ws, wsb, d_idx, dist ? d_dist : nullptr,
                                   nullptr, M > 0 ? M : 1);
    if (!rc && M > 0) {
      io.down(idx, d_idx, (size_t)M * (size_t)k * sizeof(int32_t));
      if (dist) io.down(dist, d_dist, (size_t)M * (size_t)k * sizeof(double));
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_sparse_query_sync(ctx, d_ws);
}

}  // extern "C"
