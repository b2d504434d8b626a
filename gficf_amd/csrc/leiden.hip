// leiden.hip — Leiden community detection on the Jaccard graph (clustcells(community.algo = "leiden"), reference
// R/clustCells.R:100-107).  Built into libgficf_leiden.so, which links libgficf_hip.so and uses its context, scan, radix sort and
// error plumbing (include/gficf_leiden.h states the contract, the conflict rule of the refinement and every threshold).
// Here: the refinement, the iteration and the entries; what slm.hip runs too — the level graph, local moving, the quality
// launches, aggregation, the scans — is in leiden_kernels.h, where k_ld_move / k_ld_apply take a fence that Leiden leaves out.
//
// Launches (n vertices of a level; "w/b" = a wave-per-vertex launch for rows up to 128 entries and, only where the level has a
// longer row, a workgroup-per-vertex launch for those):
//   once             k_ld_fix (fixed-point weights, diagonal zeroed, vertex weights, 2W, validation), k_ld_check_labels
//   per iteration    k_ld_first + k_ld_canon (a community's label = its smallest member), k_comm_iota (the vertex map)
//   per level        k_ld_accum (totals and sizes of the start partition), the quality launches (below)
//     per pass       3 copies (the undo snapshot); per sub-round (4): k_ld_move w/b, k_ld_apply; then the quality launches
//                    k_ld_inw (internal weight, per-block integer partial sums), k_ld_sq (sum K^2 over fixed chunks),
//                    k_ld_qfin (both added up in a fixed order); 64 bytes read back (moved?, internal weight, sum K^2)
//     count          k_ld_flag_size + scan: the communities of the level; 8 bytes read back
//     refinement     k_rf_init, k_rf_ext (e(v, C - v) and E(r, C - r)); per round: k_rf_propose w/b, k_rf_commit, 8 bytes read
//                    back (committed?), k_rf_ext again if so
//     aggregation    k_ld_flag_ref + scan (new ids), k_ag_vertex (k, row capacities, community of a new vertex), scan (row
//                    starts), k_ag_emit w/b, k_ag_finish, k_ag_comm, k_ag_top
//   at the end       k_ld_gather (labels of the finest vertices), canon, k_ld_accum + quality (Q of the result),
//                    the numbering by size of community_ops.h (k_comm_size_keys, radix sort, k_comm_rank, k_comm_final)
// No floating-point atomics; the integer atomics are on per-community totals (distinct addresses); "something moved" is a word
// every mover stores 1 into, not a counter.
#include "leiden_kernels.h"
#include "gficf_leiden.h"

namespace {

// ---------------------------------------------------------------- refinement
__global__ __launch_bounds__(256) void k_rf_init(int64_t n, const u64* __restrict__ kv, int32_t* __restrict__ ref, int32_t* __restrict__ rsize,
                                                 u64* __restrict__ Kr) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) { ref[v] = (int32_t)v; rsize[v] = 1; Kr[v] = kv[v]; }
}

// a wave per vertex: the weight from v into its community outside its refined community.  first: every refined community is a
// singleton, so this is e(v, C - v) (kept in ec) and E(r, C - r) at once; later rounds add into ext (zeroed before)
__global__ __launch_bounds__(256) void k_rf_ext(LdG g, int first, const int32_t* __restrict__ comm, const int32_t* __restrict__ ref, u64* __restrict__ ec,
                                                u64* __restrict__ ext) {
  const int lane = threadIdx.x & 63;
  for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < g.n; v += (int64_t)gridDim.x * 4) {
    const int32_t cv = comm[v], rv = ref[v];
    u64 s = 0;
    for (int64_t e = g.beg[v] + lane; e < g.end[v]; e += 64) {
      const int32_t u = g.nbr[e];
      if (u != v && comm[u] == cv && ref[u] != rv) s += g.wt[e];
    }
    s = gficf_wave_sum(s);
    if (lane == 0) {
      if (first) { ec[v] = s; ext[v] = s; }
      else if (s) atomicAdd(&ext[rv], s);
    }
  }
}

template <bool BLK>
__global__ __launch_bounds__(256) void k_rf_propose(LdG g, double r, const int32_t* __restrict__ comm, const u64* __restrict__ K,
                                                    const int32_t* __restrict__ ref, const int32_t* __restrict__ rsize, const u64* __restrict__ Kr,
                                                    const u64* __restrict__ ext, const u64* __restrict__ ec, int32_t* __restrict__ prop,
                                                    u64* __restrict__ scal) {
  using SH = LdShape<BLK>;
  __shared__ int32_t s_key[SH::TABLE];
  __shared__ u64 s_val[SH::TABLE];
  __shared__ double red_g[4];
  __shared__ int32_t red_c[4];
  __shared__ u64 red_s[4];
  int32_t* const key = BLK ? s_key : s_key + (threadIdx.x >> 6) * LD_SMALL_SLOTS;
  u64* const val = BLK ? s_val : s_val + (threadIdx.x >> 6) * LD_SMALL_SLOTS;
  const int tid = ld_tid<BLK>();
  for (int64_t v = ld_first_vertex<BLK>(); v < g.n; v += ld_vertex_stride<BLK>()) {
    const int64_t lo = g.beg[v], hi = g.end[v];
    if ((hi - lo > LD_SMALL_DEG) != BLK) continue;
    const int32_t cv = comm[v];
    const u64 kvv = g.kv[v], Kc = K[cv];
    // alone in its refined community (whose label is then v) and well connected to its community
    const bool eligible = rsize[ref[v]] == 1 && (double)ec[v] >= r * (double)kvv * (double)(Kc - kvv);
    if (!eligible) {
      if (tid == 0) prop[v] = -1;
      continue;
    }
    const int P = ld_passes<BLK>(hi - lo, g.n);
    double bg = 0.0;
    int32_t bc = -1;
    u64 none = 0;
    for (int p = 0; p < P; ++p) {
      ld_clear<BLK>(key, val);
      ld_sync<BLK>();
      for (int64_t e = lo + tid; e < hi; e += SH::NT) {
        const int32_t u = g.nbr[e];
        const u64 w = g.wt[e];
        if (u == v || w == 0 || comm[u] != cv) continue;
        const int32_t ru = ref[u];
        if (!ld_in_pass(ru, P, p)) continue;
        bool own;      // (who claimed the slot: not needed here)
        if (gficf_comm_insert<SH::SLOTS>(key, val, ru, w, &own) < 0) atomicOr((uint32_t*)(scal + LD_S_STATUS), LD_ST_DENSE);
      }
      ld_sync<BLK>();
      for (int i = tid; i < SH::SLOTS; i += SH::NT) {
        const int32_t c = key[i];
        if (c < 0) continue;
        if (!(rsize[c] > 1 || c < (int32_t)v)) continue;                          // a singleton of larger id proposes to v, not v to it
        const u64 kr = Kr[c];
        if (!((double)ext[c] >= r * (double)kr * (double)(Kc - kr))) continue;    // the target must be well connected
        const double gain = (double)val[i] - r * (double)kvv * (double)kr;
        if (gain >= 0.0 && ld_better(gain, c, bg, bc)) { bg = gain; bc = c; }
      }
      ld_sync<BLK>();
    }
    ld_reduce<BLK>(bg, bc, none, red_g, red_c, red_s);
    if (tid == 0) prop[v] = bc;
  }
}

// a proposal commits iff its target had more than one member at the start of the round or its single member proposed nothing.
// rsize[p] read while others add to it: a target with prop[p] >= 0 is joined by nobody and stays at 1 or drops to 0, one with
// prop[p] < 0 accepts either way — the outcome does not depend on the order.
__global__ __launch_bounds__(256) void k_rf_commit(int64_t n, const u64* __restrict__ kv, const int32_t* __restrict__ prop, int32_t* __restrict__ ref,
                                                   int32_t* rsize, u64* __restrict__ Kr, u64* __restrict__ scal) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int32_t p = prop[v];
  if (p < 0) return;
  if (!(prop[p] < 0 || __hip_atomic_load(&rsize[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > 1)) return;
  ref[v] = p;
  atomicAdd(&rsize[p], 1);
  rsize[v] = 0;
  if (kv[v]) atomicAdd(&Kr[p], kv[v]);
  Kr[v] = 0;
  *(uint32_t*)(scal + LD_S_CHANGED) = 1u;
}

// the refinement of (comm, K) on g into w.ref (labels: a member of the refined community, whose ref is itself)
int ld_refine(LdRun& R, const LdG& g, bool big, int64_t* rounds) {
  LdWs& w = R.w;
  const unsigned gw = gficf_grid_capped(g.n, 4, LD_GRID), gb = gficf_grid_capped(g.n, 1, LD_GRID_BIG), gv = gficf_grid_capped(g.n, 256, 1u << 30);
  hipLaunchKernelGGL(k_rf_init, dim3(gv), dim3(256), 0, R.st(), g.n, g.kv, w.ref, w.rsize, w.Kr);
  hipLaunchKernelGGL(k_rf_ext, dim3(gw), dim3(256), 0, R.st(), g, 1, (const int32_t*)w.comm, (const int32_t*)w.ref, w.ec, w.ext);
  u64 h[LD_S_N];
  *rounds = 0;
  for (int64_t round = 0; round <= g.n; ++round) {         // a round that commits shrinks the singletons: at most n of them
    ++*rounds;
    GFICF_HIP_CHECK(hipMemsetAsync(w.scal + LD_S_CHANGED, 0, sizeof(u64), R.st()));
    hipLaunchKernelGGL(k_rf_propose<false>, dim3(gw), dim3(256), 0, R.st(), g, R.r, (const int32_t*)w.comm, (const u64*)w.K, (const int32_t*)w.ref,
                       (const int32_t*)w.rsize, (const u64*)w.Kr, (const u64*)w.ext, (const u64*)w.ec, w.prop, w.scal);
    if (big)
      hipLaunchKernelGGL(k_rf_propose<true>, dim3(gb), dim3(256), 0, R.st(), g, R.r, (const int32_t*)w.comm, (const u64*)w.K, (const int32_t*)w.ref,
                         (const int32_t*)w.rsize, (const u64*)w.Kr, (const u64*)w.ext, (const u64*)w.ec, w.prop, w.scal);
    hipLaunchKernelGGL(k_rf_commit, dim3(gv), dim3(256), 0, R.st(), g.n, g.kv, (const int32_t*)w.prop, w.ref, w.rsize, w.Kr, w.scal);
    GFICF_RC(ld_read_scal(R, h));
    GFICF_RC(ld_dense_check(h));
    if (!(uint32_t)h[LD_S_CHANGED]) break;
    GFICF_HIP_CHECK(hipMemsetAsync(w.ext, 0, sizeof(u64) * (size_t)g.n, R.st()));
    hipLaunchKernelGGL(k_rf_ext, dim3(gw), dim3(256), 0, R.st(), g, 0, (const int32_t*)w.comm, (const int32_t*)w.ref, w.ec, w.ext);
  }
  return GFICF_OK;
}

// one iteration from the canonical labels in w.comm (N entries); the finest vertices' labels come out in w.lab
int ld_iteration(LdRun& R, int seed) {
  LdWs& w = R.w;
  const unsigned gN = gficf_grid_capped(R.N, 256, 1u << 30);
  hipLaunchKernelGGL(k_comm_iota, dim3(gN), dim3(256), 0, R.st(), R.N, w.top);
  LdG g = R.g0;
  bool big = R.big0;
  const bool debug = getenv("GFICF_LEIDEN_DEBUG") != nullptr;      // per-level trace on stderr
  for (int level = 0; level < LD_MAX_LEVELS; ++level) {
    GFICF_RC(ld_accum(R, g, w.comm));
    int passes = 0;
    int64_t rounds = 0;
    double q_level = 0.0;
    GFICF_RC(ld_local_moving<false>(R, g, big, level, (uint32_t)seed, LdPart{w.comm, w.K, w.size}, nullptr, &passes, &q_level));
    const unsigned gv = gficf_grid_capped(g.n + 1, 256, 1u << 30);
    int64_t n_comm = 0, n2 = 0;
    hipLaunchKernelGGL(k_ld_flag_size, dim3(gv), dim3(256), 0, R.st(), g.n, (const int32_t*)w.size, w.flag);
    GFICF_RC(ld_scan_count(R, w.flag, g.n, &n_comm));
    if (debug) fprintf(stderr, "[leiden] level %d: %lld vertices%s, %d passes of local moving, Q %.9f, %lld communities\n", level, (long long)g.n,
                       big ? " (long rows)" : "", passes, q_level, (long long)n_comm);
    if (n_comm == g.n) break;                              // every community is a single vertex of the level
    GFICF_RC(ld_refine(R, g, big, &rounds));
    hipLaunchKernelGGL(k_ld_flag_ref, dim3(gv), dim3(256), 0, R.st(), g.n, (const int32_t*)w.ref, w.newid);
    GFICF_RC(ld_scan_count(R, w.newid, g.n, &n2));
    if (debug) fprintf(stderr, "[leiden]          %lld refinement rounds, %lld refined communities\n", (long long)rounds, (long long)n2);
    if (n2 == g.n) break;                                  // the refinement merged nothing
    GFICF_RC(ld_aggregate(R, &g, &big, level, n2));         // by the refined partition
  }
  hipLaunchKernelGGL(k_ld_gather, dim3(gN), dim3(256), 0, R.st(), R.N, (const int32_t*)w.top, (const int32_t*)w.comm, w.lab);
  return GFICF_OK;
}

}  // namespace

extern "C" {

int gficf_leiden_abi_version(void) { return GFICF_LEIDEN_ABI_VERSION; }

size_t gficf_leiden_workspace_bytes(int64_t N, int64_t nnz) {
  if (N < 0 || nnz < 0) return 0;
  return ld_carve(nullptr, nullptr, N, nnz);
}
size_t gficf_leiden_refine_workspace_bytes(int64_t N, int64_t nnz) { return gficf_leiden_workspace_bytes(N, nnz); }

int gficf_leiden_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz, double resolution,
                        int n_iterations, int seed, const int32_t* d_init_or_null, int32_t* d_labels, int64_t* n_clusters, double* modularity, void* d_ws,
                        size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (n_iterations < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_iterations = %d: must be at least 1", n_iterations);
  if (!n_clusters) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_clusters is NULL");
  *n_clusters = 0;
  if (modularity) *modularity = 0.0;
  if (N == 0) return GFICF_OK;
  if (!d_indptr || !d_labels || !d_ws || (nnz > 0 && (!d_indices || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  const size_t need = ld_carve(nullptr, nullptr, N, nnz);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
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
    *n_clusters = N;
    return GFICF_OK;
  }
  if (d_init_or_null) ld_canon(R, d_init_or_null, w.comm);
  else hipLaunchKernelGGL(k_comm_iota, dim3(gN), dim3(256), 0, st, N, w.comm);
  for (int it = 0; it < n_iterations; ++it) {
    GFICF_RC(ld_iteration(R, seed));
    ld_canon(R, w.lab, w.comm);                            // the next iteration's start, and the spelling the result is numbered from
  }
  // Q of the result, its clusters by decreasing size (ties: the smaller canonical label = the first vertex)
  double q = 0.0;
  int64_t nc = 0;
  GFICF_RC(ld_finish(R, d_labels, &nc, &q));
  *n_clusters = nc;
  if (modularity) *modularity = q;
  return GFICF_OK;
}

int gficf_leiden_refine_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz,
                               double resolution, const int32_t* d_labels_in, int32_t* d_refined_out, int64_t* n_refined, void* d_ws, size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (!n_refined) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_refined is NULL");
  *n_refined = 0;
  if (N == 0) return GFICF_OK;
  if (!d_indptr || !d_labels_in || !d_refined_out || !d_ws || (nnz > 0 && (!d_indices || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  const size_t need = ld_carve(nullptr, nullptr, N, nnz);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_CAPACITY, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  LdRun R;
  R.ctx = ctx; R.N = N; R.nnz = nnz; R.resolution = resolution;
  ld_carve(&R.w, d_ws, N, nnz);
  LdWs& w = R.w;
  bool no_edges = false;
  GFICF_RC(ld_setup(R, d_indptr, d_indices, d_x, d_labels_in, &no_edges));
  const unsigned gN = gficf_grid_capped(N, 256, 1u << 30);
  if (no_edges) {
    hipLaunchKernelGGL(k_comm_iota, dim3(gN), dim3(256), 0, ctx->stream, N, d_refined_out);
    GFICF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
    *n_refined = N;
    return GFICF_OK;
  }
  GFICF_HIP_CHECK(hipMemcpyAsync(w.comm, d_labels_in, sizeof(int32_t) * (size_t)N, hipMemcpyDeviceToDevice, ctx->stream));
  GFICF_RC(ld_accum(R, R.g0, w.comm));
  int64_t rounds = 0;
  GFICF_RC(ld_refine(R, R.g0, R.big0, &rounds));
  int64_t n2 = 0;
  hipLaunchKernelGGL(k_ld_flag_ref, dim3(gficf_grid_capped(N + 1, 256, 1u << 30)), dim3(256), 0, ctx->stream, N, (const int32_t*)w.ref, w.newid);
  GFICF_RC(ld_scan_count(R, w.newid, N, &n2));
  ld_canon(R, w.ref, d_refined_out);                       // one spelling: the smallest member
  GFICF_HIP_CHECK(hipStreamSynchronize(ctx->stream));
  GFICF_HIP_CHECK(hipGetLastError());
  *n_refined = n2;
  return GFICF_OK;
}

int gficf_leiden_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz, double resolution,
                      int n_iterations, int seed, const int32_t* init_or_null, int32_t* labels, int64_t* n_clusters, double* modularity) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (n_iterations < 1) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_iterations = %d: must be at least 1", n_iterations);
  if (!n_clusters) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_clusters is NULL");
  *n_clusters = 0;
  if (modularity) *modularity = 0.0;
  if (N == 0) return GFICF_OK;
  if (!indptr || !labels || (nnz > 0 && (!indices || !x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> ptr;
  int64_t m = 0;
  GFICF_RC(gficf_host_colptr(indptr, 1, N, "indptr", ptr, &m));
  if (m != nnz) GFICF_FAIL(GFICF_ERR_BAD_CSC, "indptr[N] = %lld, nnz = %lld", (long long)m, (long long)nnz);
  const size_t ws_b = gficf_leiden_workspace_bytes(N, nnz), e = (size_t)(nnz > 0 ? nnz : 1);
  gficf_host_io io{ctx, "gficf_leiden_host"};
  gficf_carver cv;
  int64_t* d_ptr; int32_t *d_idx, *d_init, *d_lab; double* d_x; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_ptr = cv.take<int64_t>((size_t)N + 1); d_idx = cv.take<int32_t>(e); d_x = cv.take<double>(e); d_init = cv.take<int32_t>((size_t)N);
    d_lab = cv.take<int32_t>((size_t)N); d_ws = cv.take<char>(ws_b);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_ptr, indptr, sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_idx, indices, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (init_or_null) io.up(d_init, init_or_null, sizeof(int32_t) * (size_t)N);
  if (!io.ok()) return io.drain(GFICF_OK);
  const int rc = gficf_leiden_device(ctx, N, d_ptr, d_idx, d_x, nnz, resolution, n_iterations, seed, init_or_null ? d_init : nullptr, d_lab, n_clusters,
                                     modularity, d_ws, ws_b);
  if (rc) return io.drain(rc);
  io.down(labels, d_lab, sizeof(int32_t) * (size_t)N);
  return io.drain(GFICF_OK);
}

int gficf_leiden_refine_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz, double resolution,
                             const int32_t* labels_in, int32_t* refined_out, int64_t* n_refined) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(ld_check_args(N, nnz, resolution));
  if (!n_refined) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_refined is NULL");
  *n_refined = 0;
  if (N == 0) return GFICF_OK;
  if (!indptr || !labels_in || !refined_out || (nnz > 0 && (!indices || !x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> ptr;
  int64_t m = 0;
  GFICF_RC(gficf_host_colptr(indptr, 1, N, "indptr", ptr, &m));
  if (m != nnz) GFICF_FAIL(GFICF_ERR_BAD_CSC, "indptr[N] = %lld, nnz = %lld", (long long)m, (long long)nnz);
  const size_t ws_b = gficf_leiden_refine_workspace_bytes(N, nnz), e = (size_t)(nnz > 0 ? nnz : 1);
  gficf_host_io io{ctx, "gficf_leiden_refine_host"};
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
  io.up(d_in, labels_in, sizeof(int32_t) * (size_t)N);
  if (!io.ok()) return io.drain(GFICF_OK);
  const int rc = gficf_leiden_refine_device(ctx, N, d_ptr, d_idx, d_x, nnz, resolution, d_in, d_out, n_refined, d_ws, ws_b);
  if (rc) return io.drain(rc);
  io.down(refined_out, d_out, sizeof(int32_t) * (size_t)N);
  return io.drain(GFICF_OK);
}

}  // extern "C"
