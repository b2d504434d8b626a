// slm.hip — smart local moving (algorithm 3 of the reference's RunModularityClustering, src/ModularityOptimizer.cpp:651-690) on
// the level loop of leiden.hip.  Built into libgficf_slm.so, which links libgficf_hip.so; include/gficf_slm.h states the contract.
// What it shares with leiden.hip is leiden_kernels.h, as text; new here are the fenced instantiations of k_ld_move / k_ld_apply
// (through ld_local_moving<true>), the canonical labels of a level, the iteration, the early stop, the starts and the entries.
//
// Launches (n vertices of a level; "w/b" as in leiden.hip):
//   once per call    k_ld_fix, k_ld_check_labels
//   per start        k_ld_first + k_ld_canon or k_comm_iota (the start partition)
//   per iteration    a copy of the start, k_comm_iota (the vertex map)
//     per level      k_ld_accum, local moving (leiden.hip's list: 3 copies, 4 x (k_ld_move w/b, k_ld_apply), quality, per pass),
//                    k_ld_flag_size + scan (the communities)
//       sub-moving   k_sl_init (singletons), local moving again with the fence (k_ld_move<., true> w/b, k_ld_apply<true>),
//                    k_comm_fill + k_ld_first + k_ld_canon + a copy (canonical sub-labels), k_ld_flag_ref + scan (their number)
//       aggregation  leiden.hip's (ld_aggregate)
//     at its end     k_ld_gather, canon, k_sl_differ (did it return its start?); 64 bytes read back
//   per start        k_ld_accum + quality (Q of its result); the best start's canonical labels kept
//   at the end       k_ld_accum + quality + the numbering by size of community_ops.h
// No floating-point atomics.
#include "leiden_kernels.h"
#include "gficf_slm.h"

namespace {

constexpr uint32_t SL_SUB_SEED = 0x27D4EB2Fu;      // the sub-moving hashes its classes with seed ^ this

__global__ __launch_bounds__(256) void k_sl_init(int64_t n, const u64* __restrict__ kv, int32_t* __restrict__ sub, int32_t* __restrict__ ssize,
                                                 u64* __restrict__ Ks) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) { sub[v] = (int32_t)v; ssize[v] = 1; Ks[v] = kv[v]; }
}

__global__ __launch_bounds__(256) void k_sl_differ(int64_t n, const int32_t* __restrict__ a, const int32_t* __restrict__ b, u64* __restrict__ scal) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n && a[v] != b[v]) *(uint32_t*)(scal + LD_S_CHANGED) = 1u;
}

// the buffers of LdWs the refinement does not use here
int32_t* sl_best(LdWs& w) { return w.prop; }                 // canonical labels of the best start so far
int32_t* sl_tmp(LdWs& w) { return (int32_t*)w.ext; }         // canonical labels on their way
int32_t* sl_start(LdWs& w) { return (int32_t*)w.ec; }        // what the iteration started from

// out[v] = the smallest member of lab[v]'s community, for the n vertices of a level (out is not lab)
void sl_canon(LdRun& R, int64_t n, const int32_t* lab, int32_t* out) {
  const unsigned gb = gficf_grid_capped(n, 256, 1u << 30);
  hipLaunchKernelGGL(k_comm_fill<int32_t>, dim3(gb), dim3(256), 0, R.st(), n, INT32_MAX, R.w.first);
  hipLaunchKernelGGL(k_ld_first, dim3(gb), dim3(256), 0, R.st(), n, lab, R.w.first);
  hipLaunchKernelGGL(k_ld_canon, dim3(gb), dim3(256), 0, R.st(), n, lab, (const int32_t*)R.w.first, out);
}

// step 3: local moving from singletons inside the communities of `fence`; canonical sub-labels in w.ref, their scan in w.newid
int sl_submove(LdRun& R, const LdG& g, bool big, int level, uint32_t seed, const int32_t* fence, int* passes, int64_t* n_sub) {
  LdWs& w = R.w;
  const unsigned gv = gficf_grid_capped(g.n, 256, 1u << 30);
  hipLaunchKernelGGL(k_sl_init, dim3(gv), dim3(256), 0, R.st(), g.n, g.kv, w.ref, w.rsize, w.Kr);
  double q_sub = 0.0;
  GFICF_RC(ld_local_moving<true>(R, g, big, level, seed ^ SL_SUB_SEED, LdPart{w.ref, w.Kr, w.rsize}, fence, passes, &q_sub));
  sl_canon(R, g.n, w.ref, sl_tmp(w));
  GFICF_HIP_CHECK(hipMemcpyAsync(w.ref, sl_tmp(w), sizeof(int32_t) * (size_t)g.n, hipMemcpyDeviceToDevice, R.st()));
  hipLaunchKernelGGL(k_ld_flag_ref, dim3(gficf_grid_capped(g.n + 1, 256, 1u << 30)), dim3(256), 0, R.st(), g.n, (const int32_t*)w.ref, w.newid);
  GFICF_RC(ld_scan_count(R, w.newid, g.n, n_sub));
  return GFICF_OK;
}

// one iteration from the canonical labels in w.comm (N entries); the finest vertices' labels come out in w.lab
int sl_iteration(LdRun& R, uint32_t seed, int start, int it, int* levels) {
  LdWs& w = R.w;
  const unsigned gN = gficf_grid_capped(R.N, 256, 1u << 30);
  hipLaunchKernelGGL(k_comm_iota, dim3(gN), dim3(256), 0, R.st(), R.N, w.top);
  LdG g = R.g0;
  bool big = R.big0;
  const bool debug = getenv("GFICF_SLM_DEBUG") != nullptr;         // per-level trace on stderr
  *levels = 0;
  for (int level = 0; level < LD_MAX_LEVELS; ++level) {
    ++*levels;
    GFICF_RC(ld_accum(R, g, w.comm));
    int passes = 0, sub_passes = -1;
    double q_level = 0.0;
    GFICF_RC(ld_local_moving<false>(R, g, big, level, seed, LdPart{w.comm, w.K, w.size}, nullptr, &passes, &q_level));
    int64_t n_comm = 0, n2 = -1;
    hipLaunchKernelGGL(k_ld_flag_size, dim3(gficf_grid_capped(g.n + 1, 256, 1u << 30)), dim3(256), 0, R.st(), g.n, (const int32_t*)w.size, w.flag);
    GFICF_RC(ld_scan_count(R, w.flag, g.n, &n_comm));
    const int64_t n = g.n;
    const bool lone = n_comm == n;                         // every community is a single vertex of the level
    if (!lone) GFICF_RC(sl_submove(R, g, big, level, seed, w.comm, &sub_passes, &n2));
    if (debug) fprintf(stderr, "[slm] start=%d iter=%d level=%d vertices=%lld long=%d passes=%d q=%.9f communities=%lld sub_passes=%d sub=%lld\n", start, it,
                       level, (long long)n, big ? 1 : 0, passes, q_level, (long long)n_comm, sub_passes, (long long)n2);
    if (lone || n2 == n) break;                            // or the sub-moving merged nothing
    GFICF_RC(ld_aggregate(R, &g, &big, level, n2));
  }
  hipLaunchKernelGGL(k_ld_gather, dim3(gN), dim3(256), 0, R.st(), R.N, (const int32_t*)w.top, (const int32_t*)w.comm, w.lab);
  return GFICF_OK;
}

int sl_device_args(int64_t N, int64_t nnz, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, const void* d_out, const void* d_ws,
                   size_t ws_bytes) {
  if (!d_indptr || !d_out || !d_ws || (nnz > 0 && (!d_indices || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  const size_t need = ld_carve(nullptr, nullptr, N, nnz);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_slm_abi_version(void) { return GFICF_SLM_ABI_VERSION; }

size_t gficf_slm_workspace_bytes(int64_t N, int64_t nnz) {
  if (N < 0 || nnz < 0) return 0;
  return ld_carve(nullptr, nullptr, N, nnz);
}

int gficf_slm_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz, double resolution,
                     int n_start, int n_iter, uint32_t seed, const int32_t* d_init_or_null, void* d_ws, size_t ws_bytes, int32_t* d_labels,
                     gficf_slm_info* info) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (n_start < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_start = %d: must be at least 1", n_start);
  if (n_iter < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_iter = %d: must be at least 1", n_iter);
  if (!info) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "info is NULL");
  *info = gficf_slm_info{};
  if (N == 0) return GFICF_OK;
  GFICF_RC(sl_device_args(N, nnz, d_indptr, d_indices, d_x, d_labels, d_ws, ws_bytes));
  LdRun R;
  R.ctx = ctx; R.N = N; R.nnz = nnz; R.resolution = resolution;
  ld_carve(&R.w, d_ws, N, nnz);
  LdWs& w = R.w;
  hipStream_t st = ctx->stream;
  bool no_edges = false;
  GFICF_RC(ld_setup(R, d_indptr, d_indices, d_x, d_init_or_null, &no_edges));
  const unsigned gN = gficf_grid_capped(N, 256, 1u << 30);
  if (no_edges) {                                          // every vertex is its own cluster, Q = 0
    hipLaunchKernelGGL(k_comm_iota, dim3(gN), dim3(256), 0, st, N, d_labels);
    GFICF_HIP_CHECK(hipStreamSynchronize(st));
    info->n_clusters = N;
    return GFICF_OK;
  }
  const size_t lab_b = sizeof(int32_t) * (size_t)N;
  u64 h[LD_S_N];
  double q_best = 0.0;
  for (int s = 0; s < n_start; ++s) {
    const uint32_t sd = seed + (uint32_t)s;
    if (d_init_or_null) ld_canon(R, d_init_or_null, w.comm);
    else hipLaunchKernelGGL(k_comm_iota, dim3(gN), dim3(256), 0, st, N, w.comm);
    int iters = 0, levels = 0;
    for (int it = 0; it < n_iter; ++it) {
      ++iters;
      GFICF_HIP_CHECK(hipMemcpyAsync(sl_start(w), w.comm, lab_b, hipMemcpyDeviceToDevice, st));
      GFICF_RC(sl_iteration(R, sd, s, it, &levels));
      ld_canon(R, w.lab, w.comm);                          // the next iteration's start, and the spelling the result is numbered from
      GFICF_HIP_CHECK(hipMemsetAsync(w.scal + LD_S_CHANGED, 0, sizeof(u64), st));
      hipLaunchKernelGGL(k_sl_differ, dim3(gN), dim3(256), 0, st, N, (const int32_t*)w.comm, (const int32_t*)sl_start(w), w.scal);
      GFICF_RC(ld_read_scal(R, h));
      if (!(uint32_t)h[LD_S_CHANGED]) break;               // it returned its own start: every further iteration would
    }
    double q = 0.0;
    int64_t nc = 0;
    GFICF_RC(ld_finish(R, nullptr, &nc, &q));
    if (s == 0 || q > q_best) {
      q_best = q;
      info->start = s; info->iterations = iters; info->levels = levels;
      GFICF_HIP_CHECK(hipMemcpyAsync(sl_best(w), w.comm, lab_b, hipMemcpyDeviceToDevice, st));
    }
  }
  GFICF_HIP_CHECK(hipMemcpyAsync(w.comm, sl_best(w), lab_b, hipMemcpyDeviceToDevice, st));
  GFICF_RC(ld_finish(R, d_labels, &info->n_clusters, &info->modularity));
  return GFICF_OK;
}

int gficf_slm_submove_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz,
                             double resolution, const int32_t* d_labels_in, uint32_t seed, int level, void* d_ws, size_t ws_bytes, int32_t* d_sub_out,
                             gficf_slm_submove_info* info) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (level < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "level = %d: must not be negative", level);
  if (!info) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "info is NULL");
  *info = gficf_slm_submove_info{};
  if (N == 0) return GFICF_OK;
  if (!d_labels_in) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  GFICF_RC(sl_device_args(N, nnz, d_indptr, d_indices, d_x, d_sub_out, d_ws, ws_bytes));
  LdRun R;
  R.ctx = ctx; R.N = N; R.nnz = nnz; R.resolution = resolution;
  ld_carve(&R.w, d_ws, N, nnz);
  bool no_edges = false;
  GFICF_RC(ld_setup(R, d_indptr, d_indices, d_x, d_labels_in, &no_edges));
  if (no_edges) {
    hipLaunchKernelGGL(k_comm_iota, dim3(gficf_grid_capped(N, 256, 1u << 30)), dim3(256), 0, ctx->stream, N, d_sub_out);
    GFICF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    info->n_sub = N;
    return GFICF_OK;
  }
  int passes = 0;
  int64_t n_sub = 0;
  GFICF_RC(sl_submove(R, R.g0, R.big0, level, seed, d_labels_in, &passes, &n_sub));
  GFICF_HIP_CHECK(hipMemcpyAsync(d_sub_out, R.w.ref, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
  GFICF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  GFICF_HIP_CHECK(hipGetLastError());
  info->n_sub = n_sub;
  info->passes = passes;
  return GFICF_OK;
}

// the staging of both host entries: the matrix, one label array in (or none), one out, the workspace
static int sl_host(gficf_ctx* ctx, const char* name, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz,
                   const int32_t* lab_in, int32_t* lab_out, int (*run)(void*, const int64_t*, const int32_t*, const double*, const int32_t*, void*, size_t, int32_t*),
                   void* arg) {
  if (!indptr || !lab_out || (nnz > 0 && (!indices || !x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> ptr;
  int64_t m = 0;
  GFICF_RC(gficf_host_colptr(indptr, 1, N, "indptr", ptr, &m));
  if (m != nnz) GFICF_FAIL(GFICF_ERR_BAD_CSC, "indptr[N] = %lld, nnz = %lld", (long long)m, (long long)nnz);
  const size_t ws_b = gficf_slm_workspace_bytes(N, nnz), e = (size_t)(nnz > 0 ? nnz : 1);
  gficf_host_io io{ctx, name};
  gficf_carver cv;
  int64_t* d_ptr; int32_t *d_idx, *d_in, *d_out; double* d_x; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_ptr = cv.take<int64_t>((size_t)N + 1); d_idx = cv.take<int32_t>(e); d_x = cv.take<double>(e); d_in = cv.take<int32_t>((size_t)N);
    d_out = cv.take<int32_t>((size_t)N); d_ws = cv.take<char>(ws_b);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_ptr, indptr, sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_idx, indices, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (lab_in) io.up(d_in, lab_in, sizeof(int32_t) * (size_t)N);
  if (!io.ok()) return io.drain(GFICF_OK);
  const int rc = run(arg, d_ptr, d_idx, d_x, lab_in ? d_in : nullptr, d_ws, ws_b, d_out);
  if (rc) return io.drain(rc);
  io.down(lab_out, d_out, sizeof(int32_t) * (size_t)N);
  return io.drain(GFICF_OK);
}

struct SlHostRun { gficf_ctx* ctx; int64_t N, nnz; double resolution; int n_start, n_iter; uint32_t seed; gficf_slm_info* info; };
struct SlHostSub { gficf_ctx* ctx; int64_t N, nnz; double resolution; uint32_t seed; int level; gficf_slm_submove_info* info; };

int gficf_slm_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz, double resolution, int n_start,
                   int n_iter, uint32_t seed, const int32_t* init_or_null, int32_t* labels, gficf_slm_info* info) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (n_start < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_start = %d: must be at least 1", n_start);
  if (n_iter < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_iter = %d: must be at least 1", n_iter);
  if (!info) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "info is NULL");
  *info = gficf_slm_info{};
  if (N == 0) return GFICF_OK;
  SlHostRun a{ctx, N, nnz, resolution, n_start, n_iter, seed, info};
  return sl_host(ctx, "gficf_slm_host", N, indptr, indices, x, nnz, init_or_null, labels,
                 [](void* p, const int64_t* d_ptr, const int32_t* d_idx, const double* d_x, const int32_t* d_in, void* d_ws, size_t ws_b, int32_t* d_out) {
                   SlHostRun& a = *(SlHostRun*)p;
                   return gficf_slm_device(a.ctx, a.N, d_ptr, d_idx, d_x, a.nnz, a.resolution, a.n_start, a.n_iter, a.seed, d_in, d_ws, ws_b, d_out, a.info);
                 },
                 &a);
}

int gficf_slm_submove_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz, double resolution,
                           const int32_t* labels_in, uint32_t seed, int level, int32_t* sub_out, gficf_slm_submove_info* info) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (level < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "level = %d: must not be negative", level);
  if (!info) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "info is NULL");
  *info = gficf_slm_submove_info{};
  if (N == 0) return GFICF_OK;
  if (!labels_in) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  SlHostSub a{ctx, N, nnz, resolution, seed, level, info};
  return sl_host(ctx, "gficf_slm_submove_host", N, indptr, indices, x, nnz, labels_in, sub_out,
                 [](void* p, const int64_t* d_ptr, const int32_t* d_idx, const double* d_x, const int32_t* d_in, void* d_ws, size_t ws_b, int32_t* d_out) {
                   SlHostSub& a = *(SlHostSub*)p;
                   return gficf_slm_submove_device(a.ctx, a.N, d_ptr, d_idx, d_x, a.nnz, a.resolution, d_in, a.seed, a.level, d_ws, ws_b, d_out, a.info);
                 },
                 &a);
}

}  // extern "C"
