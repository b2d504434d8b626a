// sparse_knn.hip — libgficf_sparse_knn.so: exact kNN over the sparse cells of a GF-ICF matrix (include/gficf_sparse_knn.h states
// the method: the contract).  Three launches per call: prepare (f32 values, per-cell scalars, deferred checks), tiles (dense
// queries in LDS, sparse candidates streamed), merge (the slices' lists into the table).  The kernels are text this object shares
// with sparse_query.hip (sparse_knn_tiles.h); here the queries are columns of the candidates' own matrix, SELF = true.
#include "gficf_sparse_knn.h"

#include "sparse_knn_tiles.h"

namespace {

int sk_check(int64_t G, int64_t N, int64_t nnz, int k, int metric) {
  if (G < 1 || N < 1 || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld, nnz = %lld: the matrix needs a row and a column", (long long)G, (long long)N, (long long)nnz);
  if (N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N = %lld exceeds int32 ids", (long long)N);
  if (G > SK_MAX_G) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld genes exceed the %lld one query cell's dense copy may hold in LDS", (long long)G, (long long)SK_MAX_G);
  if (k < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d: at least one neighbour", k);
  if (k > GFICF_KNN_MAX_K) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "k = %d exceeds GFICF_KNN_MAX_K = %d", k, GFICF_KNN_MAX_K);
  if (k > N) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "k = %d neighbours asked of N = %lld points", k, (long long)N);
  if (!gficf_knn_metric_ok(metric)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "unknown metric %d", metric);
  return GFICF_OK;
}

// ---------------------------------------------------------------- workspace
struct SkWs {
  uint32_t* status;
  float* xf;          // nnz: the values rounded to f32
  double* p0;         // N: na (euclidean), la (manhattan), sqrt(na) (cosine), the centred norm (correlation)
  double* p1;         // N: ma (correlation)
  u64* part;          // n_q x slices x k keys, ascending within a list
};

size_t sk_carve(char* base, int64_t N, int64_t nnz, int k, int64_t n_q, int slices, SkWs& w) {
  gficf_carver cv{base};
  w.status = cv.take<uint32_t>(1);
  w.xf = cv.take<float>((size_t)(nnz > 0 ? nnz : 1));
  w.p0 = cv.take<double>((size_t)N);
  w.p1 = cv.take<double>((size_t)N);
  w.part = cv.take<u64>((size_t)(n_q > 0 ? n_q : 1) * (size_t)slices * (size_t)k);
  return cv.total();
}

}  // namespace

extern "C" {

int gficf_sparse_knn_abi_version(void) { return GFICF_SPARSE_KNN_ABI_VERSION; }

int gficf_sparse_knn_shape(int64_t G, int64_t N, int k, int* tile_queries, int* slices, int64_t* max_genes) {
  if (!tile_queries || !slices || !max_genes) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  *max_genes = SK_MAX_G;
  *tile_queries = 0;
  *slices = 0;
  GFICF_RC(sk_check(G, N, 0, k, GFICF_KNN_EUCLIDEAN));
  *tile_queries = sk_tile_queries(G);
  *slices = sk_slices(N, N, *tile_queries);
  return GFICF_OK;
}

size_t gficf_sparse_knn_workspace_bytes(int64_t G, int64_t N, int64_t nnz, int k, int64_t n_queries) {
  if (G < 1 || G > SK_MAX_G || N < 1 || N > 0x7FFFFFFFll || nnz < 0 || k < 1 || k > GFICF_KNN_MAX_K || n_queries < 0 || n_queries > N) return 0;
  const int tq = sk_tile_queries(G);
  SkWs w;
  return sk_carve(nullptr, N, nnz, k, n_queries, sk_slices(n_queries, N, tq), w);
}

int gficf_sparse_knn_device(gficf_ctx* ctx, int64_t G, int64_t N, const int64_t* d_colptr, const int32_t* d_rowidx, const double* d_x,
                            int64_t nnz, int k, int metric, int64_t q_begin, int64_t q_end, void* ws, size_t ws_bytes, int32_t* d_idx,
                            double* d_dist, int64_t ld_out) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(sk_check(G, N, nnz, k, metric));
  if (q_begin < 0 || q_end < q_begin || q_end > N)
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "query range [%lld, %lld) outside [0, %lld]", (long long)q_begin, (long long)q_end, (long long)N);
  const int64_t n_q = q_end - q_begin;
  if (!d_colptr || !ws || (n_q > 0 && !d_idx) || (nnz > 0 && (!d_rowidx || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ld_out < n_q) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "ld_out = %lld < number of queries %lld", (long long)ld_out, (long long)n_q);
  const int tq = sk_tile_queries(G), slices = sk_slices(n_q, N, tq);
  SkWs w;
  const size_t need = sk_carve(nullptr, N, nnz, k, n_q, slices, w);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  sk_carve((char*)ws, N, nnz, k, n_q, slices, w);
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  hipLaunchKernelGGL(k_sk_prepare, dim3((unsigned)gficf_ceil_div(N, 256 / SK_LANES)), dim3(256), 0, st, G, N, nnz, d_colptr, d_rowidx, d_x, metric,
                     w.xf, w.p0, w.p1, w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  if (n_q == 0) return GFICF_OK;
  SkArgs a{};
  a.G = G; a.N = N; a.nnz = nnz; a.colptr = d_colptr; a.rowidx = d_rowidx; a.xf = w.xf; a.p0 = w.p0; a.p1 = w.p1;
  a.q_nnz = nnz; a.q_colptr = d_colptr; a.q_rowidx = d_rowidx; a.q_xf = w.xf; a.q_p0 = w.p0; a.q_p1 = w.p1;   // the queries: columns of the same matrix
  a.k = k; a.metric = metric; a.slices = slices; a.q_begin = q_begin; a.q_end = q_end; a.per_slice = gficf_ceil_div(N, slices); a.part = w.part;
  const int64_t tiles = gficf_ceil_div(n_q, tq);
  GFICF_RC((metric == GFICF_KNN_MANHATTAN ? sk_launch_tq<true, true>(ctx, a, tq, tiles) : sk_launch_tq<false, true>(ctx, a, tq, tiles)));
  hipLaunchKernelGGL(k_sk_merge, dim3((unsigned)gficf_ceil_div(n_q, SK_MERGE_THREADS / 64)), dim3(SK_MERGE_THREADS), 0, st, (const u64*)w.part, n_q,
                     slices, k, d_idx, d_dist, (float*)nullptr, ld_out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_sparse_knn_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  GFICF_RC(gficf_addon_read_status(ctx, ws, &st));
  if (st & SK_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "a row id out of range or not strictly ascending within its column, or a bad column pointer");
  if (st & SK_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "a NaN or an infinite value in the matrix (after rounding to f32)");
  return GFICF_OK;
}

int gficf_sparse_knn_host(gficf_ctx* ctx, int64_t G, int64_t N, const void* colptr, int colptr_is_i64, const int32_t* rowidx,
                          const double* x, int k, int metric, int32_t* idx, double* dist) {
  GFICF_CTX_ENTER(ctx);
  if (G < 1 || N < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, N = %lld: the matrix needs a row and a column", (long long)G, (long long)N);
  if (!colptr || !idx) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> cp;
  int64_t nnz = 0;
  GFICF_RC(gficf_host_colptr(colptr, colptr_is_i64, N, "colptr", cp, &nnz));
  GFICF_RC(sk_check(G, N, nnz, k, metric));
  if (nnz > 0 && (!rowidx || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1), ob = (size_t)N * (size_t)k;
  const size_t wsb = gficf_sparse_knn_workspace_bytes(G, N, nnz, k, N);
  gficf_host_io io{ctx, "gficf_sparse_knn_host"};
  gficf_carver cv;
  int64_t* d_cp; int32_t *d_ri, *d_idx; double *d_x, *d_dist; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_cp = cv.take<int64_t>((size_t)N + 1); d_ri = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_idx = cv.take<int32_t>(ob); d_dist = cv.take<double>(ob);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_cp, cp.data(), sizeof(int64_t) * cp.size());
  io.up(d_ri, rowidx, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  int rc = GFICF_OK;
  if (io.ok()) {
    rc = gficf_sparse_knn_device(ctx, G, N, d_cp, d_ri, d_x, nnz, k, metric, 0, N, d_ws, wsb, d_idx, dist ? d_dist : nullptr, N);
    if (!rc) {
      io.down(idx, d_idx, ob * sizeof(int32_t));
      if (dist) io.down(dist, d_dist, ob * sizeof(double));
    }
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_sparse_knn_sync(ctx, d_ws);
}

}  // extern "C"
