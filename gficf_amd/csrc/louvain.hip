// louvain.hip — community detection on the Jaccard graph ("next" row N4 of the scope table).
//
// What clustcells() runs on the adjacency matrix of the kNN -> Jaccard graph:
//   RunModularityClustering(igraph::as_adjacency_matrix(g, attr = "weight", sparse = T), 1, resolution, 1 | 2, n.start,
//                           n.iter, seed, verbose)                                         (reference R/clustCells.R:80,86)
// -> RunModularityClusteringCpp (src/RModularityOptimizer.cpp:25-181) -> VOSClusteringTechnique::runLouvainAlgorithm
// (src/ModularityOptimizer.cpp:594-612): local moving (:484-592), network reduction, recursion; quality function
// calcQualityFunction (:461-482) = standard modularity with a resolution parameter,
//   Q = (1 / 2W) * [ sum_ij A_ij delta(c_i, c_j)  -  resolution * sum_c K_c^2 / 2W ],   K_c = sum of the degrees in c,
// over the strict lower triangle of the matrix (the driver skips the diagonal, src/RModularityOptimizer.cpp:73-75).
//
// RELAXED PARITY CONTRACT.  The reference is a sequential, seed-exact algorithm: vertices move one at
// a time in the order of a java.util.Random permutation.  A device form cannot follow that order and stay parallel, so
// this is NOT label-for-label parity: the contract is the same objective (the Q above, same resolution semantics, same
// diagonal handling, clusters numbered by decreasing size as Clustering::orderClustersByNNodes :132-158 does), a
// modularity within a stated tolerance of the reference's own result on the same graph (tests/test_louvain_gpu.py
// compares against a build of the reference's ModularityOptimizer.cpp, oracle/_ref/), and bit-reproducible output.
//
// Device algorithm (deterministic parallel Louvain), per start:
//   * weights in 2^-32 fixed point (u64): every sum — a vertex's weight towards a community, the community totals —
//     is an integer sum, so atomics commute and the result does not depend on scheduling or on the order of a row's entries;
//   * local moving, synchronous within a sub-round: every vertex reads the same snapshot (labels, community totals and
//     sizes), accumulates its edge weight per neighbouring community in an LDS hash table (one wave per vertex up to 128
//     entries, one workgroup beyond), takes the community with the best gain
//       gain(v -> c) = w(v, c) - k_v * K_c(without v) * resolution / 2W         (reference :540, ties: smaller id :541)
//     if that beats staying; two singletons never swap (only the larger id moves).  The vertices are split into S
//     hash classes that move one after the other (S grows as the graph gets small, where simultaneous moves hurt most);
//     totals are applied between sub-rounds.  An iteration that lowers Q is undone and ends the level;
//   * reduction: communities renumbered by a scan; every vertex sums its entries per neighbouring community (the same LDS
//     table) and appends one entry per community to the row of its own community in the coarse graph.  The coarse graph is
//     a MULTIGRAPH in pointerB / pointerE form (a row may name a neighbour once per member vertex; every consumer sums
//     per community anyway); no sort anywhere;
//   * n_iter > 1 restarts from the finest graph with the labels found so far, as the reference's iterations do;
//   * algorithm 2 (runLouvainAlgorithmWithMultilevelRefinement, :629-649): after the descent, back up through the levels
//     with one more local moving on each, seeded with the labels found below it; a level's graph is rebuilt from the
//     finest one through its saved vertex map rather than kept.
//   * a vertex whose every option has a negative gain leaves for an unused cluster (:546-550): its own id, if free.
//   * n_start "random starts": each start varies the seed of the class hash (the only arbitrary choice there is); the best
//     modularity wins, as in the reference.  Start 0 with seed 0 is the plain run.
//   * the alternative modularity function (2): unit node weights, the resolution as given — a context option.
// Algorithm 3 is refused by these entries: it is slm.hip's, an add-on of its own (include/gficf_slm.h).
//
// Round 6 — the starts in ONE launch set, the iterations without host round trips:
//   * the n_start starts are independent problems on one graph.  They run as ONE problem on the disjoint union of B copies
//     ("components"; B = as many starts as the workspace holds, at most 16): union vertex b * N + v, labels / totals / sizes
//     per union vertex, every quantity that decides something (Q, moved vertices, sub-round count, seed) per component.
//     Level 0 never materialises the copies: a wave loads a vertex's row ONCE and evaluates it for every component.  Coarse
//     levels are one graph whose vertex ids are the scan's new ids (contiguous per component).  A component whose descent
//     or whole run has ended idles (its kernels skip it) while the others go on; its results are those of running that start
//     alone (tests/test_louvain_gpu.py: batched == one by one);
//   * convergence and undo are decided on the device (k_lv_decide: one small block per iteration): the move kernel of an
//     iteration's first sub-round also sums the internal weight of the labels it READS, i.e. the previous iteration's
//     result, so the quality check costs no pass of its own; an iteration's kernels look at the component's action flag and
//     do nothing once its level has ended.  The host enqueues one iteration AHEAD and waits for the previous one's event:
//     the stream is never drained inside a level; per level there is one synchronisation (the sizes of the next level);
//   * counters that every moving vertex used to hit with one global atomic (a single address: 150-220 us of the 158-226 us
//     a level-0 sub-round took while most vertices still moved) are per-block partial sums in fixed slots, added up by
//     k_lv_decide; the vertex kernels are persistent grids striding over the vertices.
#include <cstdlib>
#include <cstring>

#include <atomic>
#include <vector>

#include "louvain_shared.h"
#include "louvain_move.h"
#include "louvain_reduce.h"

namespace {

// ---- level 0: fixed-point weights, validation
__global__ __launch_bounds__(256) void k_lv_fix(int64_t N, int64_t nnz, const int32_t* __restrict__ nbr, const double* __restrict__ x,
                                                u64* __restrict__ wt, u64* __restrict__ max_wt, uint32_t* __restrict__ status) {
  __shared__ u64 s_max[4];
  u64 mx = 0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < nnz; e += (int64_t)gridDim.x * 256) {
    const double v = x[e];
    const int32_t u = nbr[e];
    const bool ok = u >= 0 && u < N && v >= 0.0 && v <= 1048576.0;      // NaN fails the comparisons
    if (!ok) atomicOr(status, u >= 0 && u < N ? GFICF_ST_BAD_VALUE : GFICF_ST_BAD_CSC);
    const u64 f = ok ? (u64)llrint(v * GFICF_COMM_SCALE) : 0ull;
    wt[e] = f;
    mx = f > mx ? f : mx;
  }
  for (int d = 32; d > 0; d >>= 1) { const u64 o = __shfl_down(mx, d); mx = o > mx ? o : mx; }
  if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {                                        // the largest weight bounds every later sum (checked by the host)
    for (int t = 1; t < 4; ++t) mx = s_max[t] > mx ? s_max[t] : mx;
    if (mx) atomicMax(max_wt, mx);
  }
}

// vertex weights (the row sums without the diagonal) and 2W: a wave per vertex, the row read by consecutive lanes; one atomic per workgroup
__global__ __launch_bounds__(256) void k_lv_vertex_weight(int64_t n, int64_t m, const int64_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                         const u64* __restrict__ wt, u64* __restrict__ kv, u64* __restrict__ two_w,
                                                         uint32_t* __restrict__ status) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 total = 0;                                       // lane 0: the sum over this wave's vertices
  for (int64_t v = (int64_t)blockIdx.x * 4 + wave; v < n; v += (int64_t)gridDim.x * 4) {
    int64_t lo = ptr[v], hi = ptr[v + 1];
    if (lo < 0 || hi < lo || hi > m) { if (lane == 0) atomicOr(status, GFICF_ST_BAD_CSC); lo = hi = 0; }
    u64 s = 0;
    for (int64_t e = lo + lane; e < hi; e += 64) {
      const int32_t u = nbr[e];
      if (u != v && u >= 0 && u < n) s += wt[e];
    }
    for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d);
    if (lane == 0) { kv[v] = s; total += s; }
  }
  __shared__ u64 s_sum[4];
  if (lane == 0) s_sum[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    if (t) atomicAdd(two_w, t);
  }
}

// ---- control kernels (one small block; thread b = component b)
// A batch begins: the seeds of its starts, nothing found yet.
__global__ void k_lv_ctl_batch(LvCtl* ctl, int B, int first_start, int seed) {
  const int b = threadIdx.x;
  if (b == 0) { ctl->B = B; ctl->n_mid = ctl->n_large = 0; ctl->n_union2 = 0; }
  if (b >= LV_MAX_B) return;
  LvComp& C = ctl->c[b];
  const int start = first_start + b;
  C.seed = start == 0 && seed == 0 ? 0u : gficf_comm_hash((uint32_t)seed * 0x9E3779B1u + (uint32_t)start + 1u);
  C.finished = b < B ? 0 : 1;
  C.any_move = 1;
  C.n_labels = 0;
  C.q_prev = C.q_final = 0.0;
  C.self_w = C.in_w = 0;
  C.live = C.cont = 0;
  C.n_saved = 0;
  C.v0 = C.n = C.n2 = C.newbase = 0;
}

// A level begins.  mode 0: level 0 of a pass (v0 = b * N, n = N; pass > 0: seeded with the labels found so far, a start whose last
// pass moved nothing has finished).  mode 1: the level below was renumbered and reduced (v0 = newbase, n = n2 for the
// components that go on).  mode 2: a refinement level of algorithm 2 (the participants and sizes were set by k_lv_ctl_refine).
__global__ void k_lv_ctl_level(LvCtl* ctl, int mode, int pass, int64_t N, int s_env) {
  __shared__ int64_t s_nl[LV_MAX_B];
  const int b = threadIdx.x;
  const int B = ctl->B;
  if (b < LV_MAX_B) {
    LvComp& C = ctl->c[b];
    if (mode == 0) {
      if (pass > 0 && !C.any_move) C.finished = 1;
      C.live = b < B && !C.finished;
      C.v0 = b < B ? (int64_t)b * N : 0;                 // (a slot beyond the batch: an empty range, never an index past the union)
      C.n = b < B ? N : 0;
      C.self_w = 0;
      C.any_move = 0;
      C.n_saved = 0;
      C.seed_base = C.v0;
    } else if (mode == 1) {
      C.live = C.cont;
      C.v0 = C.newbase; C.n = C.n2;
      C.seed_base = C.v0;
    }
    C.cont = 0;
    C.S = lv_sub_rounds_of(C.n, s_env);
    C.level_done = C.live ? 0 : 1;
    C.action = LV_IDLE;
    C.iter = 0;
    C.level_moved = 0;
    C.in_run = 0;
    s_nl[b] = b < B && C.live ? C.n_labels : 0;
  }
  __syncthreads();
  if (b < LV_MAX_B) {
    int64_t base = 0;
    for (int t = 0; t < b; ++t) base += s_nl[t];
    ctl->c[b].lab_base = base;
  }
}

// Labels (seed == NULL: singletons), totals and sizes of the level.  A seeded start leaves totals and sizes at zero for
// k_lv_accum.  The vertices of a component that does not take part are dead: own label, size 0 (they vanish at the next renumbering).
__global__ __launch_bounds__(256) void k_lv_init(LvG g, const LvCtl* __restrict__ ctl, const int32_t* __restrict__ seed, int32_t* __restrict__ comm,
                                                 u64* __restrict__ K, int32_t* __restrict__ size, int32_t* __restrict__ mark_r, int32_t* __restrict__ mark_w,
                                                 u64* __restrict__ iw) {
  for (int64_t gv = (int64_t)blockIdx.x * 256 + threadIdx.x; gv < g.n; gv += (int64_t)gridDim.x * 256) {
    mark_r[gv] = 0; mark_w[gv] = 0; iw[gv] = 0ull;
    const int64_t b = g.rep > 1 ? gv / g.nb : 0;
    const int64_t v = gv - b * g.nb;
    const int comp = g.vcomp ? (int)g.vcomp[gv] : (int)b;
    const LvComp& C = ctl->c[comp];
    if (!C.live) { comm[gv] = (int32_t)gv; K[gv] = 0ull; size[gv] = 0; continue; }
    if (seed) { comm[gv] = (int32_t)(C.seed_base + seed[gv]); K[gv] = 0ull; size[gv] = 0; }
    else { comm[gv] = (int32_t)gv; K[gv] = g.kv[v]; size[gv] = 1; }
  }
}

// Totals and member counts of the communities comm[] names (K, size zeroed before).  With few labels every vertex would hit the
// same few addresses: when all components' labels fit LV_ACC_BINS bins (bin = lab_base + label - seed_base) they are summed in
// LDS first, one global atomic per label and block.
__global__ __launch_bounds__(256) void k_lv_accum(LvG g, const LvCtl* __restrict__ ctl, int binned, const int32_t* __restrict__ comm,
                                                  u64* __restrict__ K, int32_t* __restrict__ size) {
  __shared__ u64 s_k[LV_ACC_BINS];
  __shared__ int32_t s_n[LV_ACC_BINS];
  __shared__ int32_t s_c[LV_ACC_BINS];
  if (binned) {
    for (int t = threadIdx.x; t < LV_ACC_BINS; t += 256) { s_k[t] = 0ull; s_n[t] = 0; s_c[t] = -1; }
    __syncthreads();
  }
  for (int64_t gv = (int64_t)blockIdx.x * 256 + threadIdx.x; gv < g.n; gv += (int64_t)gridDim.x * 256) {
    const int64_t b = g.rep > 1 ? gv / g.nb : 0;
    const int comp = g.vcomp ? (int)g.vcomp[gv] : (int)b;
    const LvComp& C = ctl->c[comp];
    if (!C.live) continue;
    const int32_t c = comm[gv];
    const u64 k = g.kv[gv - b * g.nb];
    if (binned) {
      const int bin = (int)(C.lab_base + ((int64_t)c - C.seed_base));
      s_c[bin] = c;
      atomicAdd(&s_k[bin], k);
      atomicAdd(&s_n[bin], 1);
    } else {
      atomicAdd(&K[c], k);
      atomicAdd(&size[c], 1);
    }
  }
  if (binned) {
    __syncthreads();
    for (int t = threadIdx.x; t < LV_ACC_BINS; t += 256) {
      if (s_n[t]) { atomicAdd(&size[s_c[t]], s_n[t]); if (s_k[t]) atomicAdd(&K[s_c[t]], s_k[t]); }
    }
  }
}

// the vertices of the workgroup path: middle degrees from the front of the list, large ones from its end
__global__ __launch_bounds__(256) void k_lv_list_big(LvG g, const int64_t* __restrict__ n_dev, int32_t* __restrict__ big, unsigned* __restrict__ n_mid_large) {
  const int64_t nb = n_dev ? *n_dev : g.nb;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nb; v += (int64_t)gridDim.x * 256) {
    const int64_t deg = g.end[v] - g.beg[v];
    if (deg > LV_MID_DEG) big[nb - 1 - atomicAdd(n_mid_large + 1, 1u)] = (int32_t)v;
    else if (deg > LV_SMALL_DEG) big[atomicAdd(n_mid_large, 1u)] = (int32_t)v;
  }
}

// the list counts of the next level's graph, where the host reads them after the level's one synchronisation
__global__ void k_lv_ctl_publish(const LvCtl* __restrict__ ctl, LvHost* __restrict__ host) {
  if (threadIdx.x == 0) { host->n_mid = ctl->n_mid; host->n_large = ctl->n_large; __threadfence_system(); }
}

// ---- algorithm 2: the levels on the way back up
// The participants of refinement level `level` (starts that moved in this pass and saved that level), their vertex ranges (prefix of
// the saved sizes), and — level >= 1 — the base their level vertices get as labels of the finest graph (seed_base).
__global__ void k_lv_ctl_refine(LvCtl* ctl, int level, int64_t N) {
  __shared__ int64_t s_n[LV_MAX_B];
  const int b = threadIdx.x;
  const int B = ctl->B;
  if (b < LV_MAX_B) {
    LvComp& C = ctl->c[b];
    C.live = b < B && !C.finished && C.any_move && C.n_saved >= level;
    s_n[b] = C.live ? (level ? C.saved_n[level] : N) : 0;
  }
  __syncthreads();
  if (b < LV_MAX_B) {
    LvComp& C = ctl->c[b];
    int64_t base = 0;
    for (int t = 0; t < b; ++t) base += s_n[t];
    if (level == 0) { C.v0 = b < B ? (int64_t)b * N : 0; C.n = b < B ? N : 0; }
    else { C.v0 = base; C.n = s_n[b]; }
    C.seed_base = C.v0;
    C.self_w = 0;                          // level 0: nothing is folded into the vertices; a rebuilt level: set by k_lv_ctl_self
    C.newbase = C.v0; C.n2 = C.n;          // the level's vertices ARE the new ids of the rebuilding reduction
    C.cont = C.live;                       // ... which every participant takes part in
    if (b == LV_MAX_B - 1) ctl->n_union2 = base + s_n[b];
  }
}

// internal weight of given labels on the level's graph, per component (per-block partial sums in the slots of the small path)
__global__ __launch_bounds__(256) void k_lv_internal(LvG g, const LvCtl* __restrict__ ctl, const int32_t* __restrict__ comm, u64* __restrict__ part_in) {
  __shared__ u64 s_acc[4][LV_MAX_B];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  u64 acc = 0;
  for (int64_t v = (int64_t)blockIdx.x * 4 + wave; v < g.nb; v += (int64_t)gridDim.x * 4) {
    for (int b = 0; b < g.rep; ++b) {
      const int comp = g.vcomp ? (int)g.vcomp[v] : b;
      if (!ctl->c[comp].live) continue;
      const int64_t base = (int64_t)b * g.nb;
      const int32_t cv = comm[base + v];
      u64 s = 0;
      for (int64_t e = g.beg[v] + lane; e < g.end[v]; e += 64) {
        const int32_t u = g.nbr[e];
        if (u != v && comm[base + u] == cv) s += g.wt[e];
      }
      s = lv_wave_sum(s);
      if (lane == comp) acc += s;
    }
  }
  if (lane < LV_MAX_B) s_acc[wave][lane] = acc;
  __syncthreads();
  if (threadIdx.x < LV_MAX_B) part_in[(size_t)blockIdx.x * LV_MAX_B + threadIdx.x] = s_acc[0][threadIdx.x] + s_acc[1][threadIdx.x] + s_acc[2][threadIdx.x] + s_acc[3][threadIdx.x];
}

// self_w of the refinement level = the sum of those partial sums
__global__ __launch_bounds__(256) void k_lv_ctl_self(LvCtl* ctl, const u64* __restrict__ part_in, int nb) {
  __shared__ u64 s_in[4][LV_MAX_B];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int b = 0; b < LV_MAX_B; ++b) {
    u64 a = 0;
    for (int r = tid; r < nb; r += 256) a += part_in[(size_t)r * LV_MAX_B + b];
    a = lv_wave_sum(a);
    if (lane == 0) s_in[wave][b] = a;
  }
  __syncthreads();
  if (tid < LV_MAX_B) ctl->c[tid].self_w = ctl->c[tid].live ? s_in[0][tid] + s_in[1][tid] + s_in[2][tid] + s_in[3][tid] : 0ull;
}

// seedl[x] = the label of the original vertices that make up level vertex x (they all carry the same one)
__global__ __launch_bounds__(256) void k_lv_seed(int64_t N, const LvCtl* __restrict__ ctl, const int32_t* __restrict__ top, const int32_t* __restrict__ lab,
                                                 int32_t* __restrict__ seedl) {
  const int b = blockIdx.y;
  const LvComp& C = ctl->c[b];
  if (!C.live) return;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < N; v += (int64_t)gridDim.x * 256) {
    const size_t at = (size_t)b * (size_t)N + (size_t)v;
    seedl[C.v0 + top[at]] = lab[at];
  }
}

__global__ __launch_bounds__(256) void k_lv_iota(int64_t n, int64_t* __restrict__ out) {
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v <= n; v += (int64_t)gridDim.x * 256) out[v] = v;
}

// members of every label of the best start: the counts the final numbering (community_ops.h) sorts by
__global__ __launch_bounds__(256) void k_lv_count(int64_t n, int64_t C, const int32_t* __restrict__ lab, int32_t* __restrict__ cnt) {
  __shared__ int32_t s_n[LV_ACC_BINS];
  const bool binned = C <= LV_ACC_BINS;
  if (binned) {
    for (int t = threadIdx.x; t < C; t += 256) s_n[t] = 0;
    __syncthreads();
  }
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < n; v += (int64_t)gridDim.x * 256) {
    if (binned) atomicAdd(&s_n[lab[v]], 1);
    else atomicAdd(&cnt[lab[v]], 1);
  }
  if (binned) {
    __syncthreads();
    for (int t = threadIdx.x; t < C; t += 256)
      if (s_n[t]) atomicAdd(&cnt[t], s_n[t]);
  }
}

// ---- host side
struct LvLevel {          // a coarse graph's arrays (capacity: the union's entries)
  int64_t* beg; int64_t* end; int32_t* nbr; u64* wt; u64* kv; uint8_t* vcomp; int32_t* big;
};

struct LvWs {
  u64* wt0; u64* kv0; int32_t* big0;
  LvLevel lvl[2];
  int32_t *comm, *next, *snapc[2], *size, *snapS[2], *cur, *lab, *seedl, *tops, *best, *cnt, *rank, *mark_r, *mark_w;
  u64 *K, *snapK[2], *iw;
  int64_t* flag;            // n_union + 1 entries: the renumbering scan
  gficf_comm_sort_bufs sort;      // final numbering
  LvParts pt;
  LvCtl* ctl;
  u64* scalars;             // [0] 2W, [5] largest weight
};

// the workspace of B starts run together
static size_t lv_carve(LvWs* w, void* base, int64_t N, int64_t nnz, int B) {
  gficf_carver b{(char*)base};
  const size_t n = (size_t)(N > 0 ? N : 1), m = (size_t)(nnz > 0 ? nnz : 1);
  const size_t nu = n * (size_t)B, mu = m * (size_t)B;
  LvWs d;
  d.wt0 = b.take<u64>(m); d.kv0 = b.take<u64>(n); d.big0 = b.take<int32_t>(n);
  for (int i = 0; i < 2; ++i) {
    d.lvl[i].beg = b.take<int64_t>(nu + 1); d.lvl[i].end = b.take<int64_t>(nu + 1); d.lvl[i].nbr = b.take<int32_t>(mu); d.lvl[i].wt = b.take<u64>(mu);
    d.lvl[i].kv = b.take<u64>(nu); d.lvl[i].vcomp = b.take<uint8_t>(nu); d.lvl[i].big = b.take<int32_t>(nu);
  }
  d.comm = b.take<int32_t>(nu); d.next = b.take<int32_t>(nu); d.size = b.take<int32_t>(nu); d.cur = b.take<int32_t>(nu);
  d.lab = b.take<int32_t>(nu); d.seedl = b.take<int32_t>(nu);
  for (int i = 0; i < 2; ++i) { d.snapc[i] = b.take<int32_t>(nu); d.snapS[i] = b.take<int32_t>(nu); d.snapK[i] = b.take<u64>(nu); }
  d.tops = b.take<int32_t>(nu * LV_MAX_SAVED);
  d.best = b.take<int32_t>(n); d.cnt = b.take<int32_t>(n); d.rank = b.take<int32_t>(n);
  d.K = b.take<u64>(nu); d.iw = b.take<u64>(nu);
  d.mark_r = b.take<int32_t>(nu); d.mark_w = b.take<int32_t>(nu);
  d.flag = b.take<int64_t>(nu + 1);
  d.sort.take(b, n, N);
  d.pt.in_small = b.take<u64>((size_t)LV_GRID * LV_MAX_B); d.pt.in_mid = b.take<u64>((size_t)LV_GRID_BIG * LV_MAX_B);
  d.pt.in_large = b.take<u64>((size_t)LV_GRID_BIG * LV_MAX_B);
  for (int i = 0; i < 2; ++i) {
    d.pt.mv_small[i] = b.take<unsigned>((size_t)LV_GRID * LV_MAX_B); d.pt.mv_mid[i] = b.take<unsigned>((size_t)LV_GRID_BIG * LV_MAX_B);
    d.pt.mv_large[i] = b.take<unsigned>((size_t)LV_GRID_BIG * LV_MAX_B);
  }
  d.pt.sq = b.take<double>((size_t)LV_MAX_B * LV_SQ_BLOCKS);
  d.ctl = b.take<LvCtl>(1);
  d.scalars = b.take<u64>(8);
  if (w) *w = d;
  return b.total();
}

// an integer of the environment, if it is there and within [lo, hi]
static int lv_env_int(const char* name, int lo, int hi, int otherwise) {
  if (const char* e = getenv(name)) { const int v = atoi(e); if (v >= lo && v <= hi) return v; }
  return otherwise;
}

// Starts run together: as many as a workspace of ws_bytes holds, at most LV_MAX_B (GFICF_LOUVAIN_BATCH in the environment: at most
// that many — 1 = one after the other); union vertex ids are int32.
static int lv_batch(int64_t N, int64_t nnz, int n_start, size_t ws_bytes) {
  int B = n_start < 1 ? 1 : n_start > LV_MAX_B ? LV_MAX_B : n_start;
  const int lim = lv_env_int("GFICF_LOUVAIN_BATCH", 1, LV_MAX_B, LV_MAX_B);
  if (B > lim) B = lim;
  while (B > 1 && ((int64_t)B * N > (int64_t)INT32_MAX || lv_carve(nullptr, nullptr, N, nnz, B) > ws_bytes)) --B;
  return B;
}

// ---- the driver: a run, and one function per step.  g = a level's union graph, L = its workgroup-path lists.
struct LvLists { const int32_t* big; unsigned n_mid, n_large; };      // middle degrees from the front of big, large ones from its end

struct LvRun {
  gficf_ctx* ctx; hipStream_t st;
  int64_t N, nnz;
  LvWs w;
  LvHost* host;              // the pinned block the control kernels report into
  hipEvent_t ev[2];          // of the one-iteration-ahead loop, by iteration parity
  double r, q_coef, two_w;
  int s_env, Bmax, algorithm;
  bool debug;                // GFICF_LOUVAIN_DEBUG: per-level trace on stderr
  LvG g0;                    // the finest graph, one copy (lv_union0: B of them)
  LvLists L0;                // its lists: the same for every start, level-0 pass and batch
};

// What the host knows of one start.  The device owns the state machine (LvComp, moved on by the control kernels); these are the
// fields that decide what is enqueued next, brought up to date where a comment names the control kernel that is mirrored.
struct LvStart {
  bool finished, any_move, live;
  int64_t n, n_labels;       // its vertices at the current level; the labels of its last renumbering
  double q_final;
  int n_saved; int64_t saved_n[LV_MAX_SAVED + 1];
};

// the union of B copies of the finest graph, never materialised
static LvG lv_union0(const LvRun& R, int B) { LvG g = R.g0; g.n = (int64_t)B * R.N; g.rep = B; return g; }

// The grids over g: the persistent grid of the wave-per-vertex kernels, and those of the workgroup path over its listed (vertex,
// copy) items.  k_lv_move_mid packs two middle-degree items into a workgroup (a wave each), k_lv_emit_big<LV_EMIT_SLOTS> takes one.
constexpr int LV_MOVE_MID_PER_WG = 2, LV_EMIT_MID_PER_WG = 1;
struct LvGrids { unsigned small, mid, large; };
static LvGrids lv_grids(const LvG& g, const LvLists& L, int mid_per_wg) {
  return LvGrids{gficf_grid_capped(g.nb, 4, LV_GRID), L.n_mid ? gficf_grid_capped((int64_t)L.n_mid * g.rep, mid_per_wg, LV_GRID_BIG) : 0u,
                 L.n_large ? gficf_grid_capped((int64_t)L.n_large * g.rep, 1, LV_GRID_BIG) : 0u};
}

// the pinned block and the two events, made on a context's first run (ctx.hip releases them)
static int lv_host_get(LvRun& R) {
  gficf_ctx* ctx = R.ctx;
  if (!ctx->lv_host) {
    GFICF_HIP_CHECK(hipHostMalloc(&ctx->lv_host, sizeof(LvHost), hipHostMallocMapped | hipHostMallocCoherent));
    memset(ctx->lv_host, 0, sizeof(LvHost));
    for (int i = 0; i < 2; ++i) GFICF_HIP_CHECK(hipEventCreateWithFlags(&ctx->lv_ev[i], hipEventDisableTiming));
  }
  R.host = (LvHost*)ctx->lv_host; R.ev[0] = ctx->lv_ev[0]; R.ev[1] = ctx->lv_ev[1];
  return GFICF_OK;
}

// The argument checks, then level 0: fixed-point weights, vertex weights, 2W, the vertices of the workgroup path.  *done: there is
// nothing to run (no vertex; or no edge: every vertex is its own cluster, Q = 0) and the results are written.
static int lv_setup(LvRun& R, gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz, double resolution,
                    int algorithm, int n_start, int n_iter, int32_t* d_labels, int64_t* n_clusters, double* modularity, void* d_ws, size_t ws_bytes, bool* done) {
  if (N < 0 || nnz < 0 || n_iter < 1 || n_start < 1 || !(resolution >= 0.0))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size, n_start < 1, n_iter < 1 or a negative resolution");
  if (algorithm != 1 && algorithm != 2) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "algorithm must be 1 (Louvain) or 2 (Louvain with multilevel refinement)");
  if (!n_clusters) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "n_clusters is NULL");
  *n_clusters = 0;
  if (modularity) *modularity = 0.0;
  *done = true;
  if (N == 0) return GFICF_OK;
  if (!d_indptr || !d_labels || !d_ws || (nnz > 0 && (!d_indices || !d_x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (N > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 vertices");
  if (ws_bytes < gficf_louvain_workspace_bytes(N, nnz, 1))
    GFICF_FAIL(GFICF_ERR_INVALID_ARG, "workspace too small: %zu < %zu bytes", ws_bytes, gficf_louvain_workspace_bytes(N, nnz, 1));
  const int Bmax = lv_batch(N, nnz, n_start, ws_bytes);      // (gficf_louvain_workspace_bytes(N, nnz, n_start) sizes the workspace for all the starts)
  static std::atomic<bool> attr_set[64];                 // per device: the attribute belongs to the device's copy of the kernel
  if (!attr_set[ctx->device & 63]) {
    GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_lv_move_big<LV_BIG_SLOTS, true>, hipFuncAttributeMaxDynamicSharedMemorySize, LV_BIG_SLOTS * 12));
    GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_lv_move_big<LV_BIG_SLOTS, false>, hipFuncAttributeMaxDynamicSharedMemorySize, LV_BIG_SLOTS * 12));
    GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_lv_emit_big<LV_BIG_SLOTS>, hipFuncAttributeMaxDynamicSharedMemorySize, LV_BIG_SLOTS * 12));
    attr_set[ctx->device & 63] = true;
  }
  R.ctx = ctx; R.st = ctx->stream; R.N = N; R.nnz = nnz; R.Bmax = Bmax; R.algorithm = algorithm;
  LvWs& w = R.w;
  hipStream_t st = R.st;
  lv_carve(&w, d_ws, N, nnz, Bmax);
  GFICF_RC(lv_host_get(R));
  GFICF_HIP_CHECK(hipMemsetAsync(w.scalars, 0, 8 * sizeof(u64), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.ctl, 0, sizeof(LvCtl), st));
  if (nnz > 0) hipLaunchKernelGGL(k_lv_fix, dim3(gficf_grid_capped(nnz, 256, 2048)), dim3(256), 0, st, N, nnz, d_indices, d_x, w.wt0, w.scalars + 5, ctx->d_status);
  hipLaunchKernelGGL(k_lv_vertex_weight, dim3(gficf_grid_capped(N, 4, 2048)), dim3(256), 0, st, N, nnz, d_indptr, d_indices, w.wt0, w.kv0, w.scalars, ctx->d_status);
  u64 h_sc[6] = {0, 0, 0, 0, 0, 0};
  GFICF_HIP_CHECK(hipMemcpyAsync(h_sc, w.scalars, sizeof(h_sc), hipMemcpyDeviceToHost, st));
  GFICF_RC(gficf_ctx_sync(ctx));                   // also reports a malformed matrix before anything follows it
  const u64 two_w_fix = h_sc[0];
  if ((double)h_sc[5] * (double)nnz >= 9.0e18)     // the u64 sums (2W, community totals) could wrap
    GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "edge weights too large for the 2^-32 fixed-point sums (largest weight x entries >= 2^31): scale the matrix");
  const double two_w = (double)two_w_fix;
  if (two_w_fix == 0) {                            // no edges
    hipLaunchKernelGGL(k_comm_iota, dim3(gficf_grid_capped(N, 256, 1u << 30)), dim3(256), 0, st, N, d_labels);
    GFICF_HIP_CHECK(hipStreamSynchronize(st));
    *n_clusters = N;
    return GFICF_OK;
  }
  // standard modularity: node weight = degree, gain coefficient resolution / 2W, Q's second term resolution * sum K^2 / (2W)^2;
  // alternative (modularity function 2): node weight = 1 (2^32 in fixed point), coefficient = the resolution itself
  const bool alt = ctx->lv_modularity_fn == 2;
  if (alt && resolution > 1.0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "error: resolution<1 for alternative modularity");
  if (alt) hipLaunchKernelGGL(k_comm_fill<u64>, dim3(gficf_grid_capped(N, 256, 1u << 30)), dim3(256), 0, st, N, (u64)GFICF_COMM_SCALE, w.kv0);
  R.two_w = two_w; R.r = alt ? resolution / GFICF_COMM_SCALE : resolution / two_w;
  R.q_coef = alt ? resolution / (GFICF_COMM_SCALE * two_w) : resolution / (two_w * two_w);
  R.s_env = lv_env_int("GFICF_LOUVAIN_SUBROUNDS", 1, 64, 0); R.debug = getenv("GFICF_LOUVAIN_DEBUG") != nullptr;

  // the finest graph's workgroup-path vertices
  R.g0 = LvG{N, N, 1, d_indptr, d_indptr + 1, d_indices, w.wt0, w.kv0, nullptr};
  hipLaunchKernelGGL(k_lv_list_big, dim3(gficf_grid_capped(N, 256, 1024)), dim3(256), 0, st, R.g0, (const int64_t*)nullptr, w.big0, &w.ctl->n_mid);
  hipLaunchKernelGGL(k_lv_ctl_publish, dim3(1), dim3(64), 0, st, (const LvCtl*)w.ctl, R.host);
  GFICF_HIP_CHECK(hipStreamSynchronize(st));
  R.L0 = LvLists{w.big0, R.host->n_mid, R.host->n_large};
  *done = false;
  return GFICF_OK;
}

// the labels as given (seed == NULL: singletons), totals, sizes
static void lv_start_level(LvRun& R, const LvG& g, const int32_t* seed, bool binned) {
  LvWs& w = R.w;
  hipLaunchKernelGGL(k_lv_init, dim3(gficf_grid_capped(g.n, 256, 2048)), dim3(256), 0, R.st, g, (const LvCtl*)w.ctl, seed, w.comm, w.K, w.size, w.mark_r, w.mark_w, w.iw);
  if (seed) hipLaunchKernelGGL(k_lv_accum, dim3(gficf_grid_capped(g.n, 256, 1024)), dim3(256), 0, R.st, g, (const LvCtl*)w.ctl, binned ? 1 : 0, (const int32_t*)w.comm, w.K, w.size);
}

// one sub-round's move kernels, a launch per degree class; FIRST: sub-round 0 (they also sum the internal weight of the labels they read)
template <bool FIRST>
static void lv_launch_moves(LvRun& R, const LvG& g, const LvLists& L, const LvGrids& G, const LvMove& mv, int par) {
  LvWs& w = R.w;
  const LvCtl* ctl = w.ctl;
  const int32_t *comm = w.comm, *size = w.size, *mark_r = w.mark_r;
  const u64* K = w.K;
  hipLaunchKernelGGL(k_lv_move_small<FIRST>, dim3(G.small), dim3(256), 0, R.st, g, ctl, mv, comm, K, size, w.next, mark_r, w.mark_w, w.iw, w.pt.in_small, w.pt.mv_small[par]);
  if (G.mid) hipLaunchKernelGGL(k_lv_move_mid<FIRST>, dim3(G.mid), dim3(128), 0, R.st, g, ctl, mv, (int64_t)L.n_mid, L.big, comm, K, size, w.next, mark_r, w.mark_w, w.iw,
                                w.pt.in_mid, w.pt.mv_mid[par], R.ctx->d_status);
  if (G.large) hipLaunchKernelGGL((k_lv_move_big<LV_BIG_SLOTS, FIRST>), dim3(G.large), dim3(256), LV_BIG_SLOTS * 12, R.st, g, ctl, mv, 1, (int64_t)L.n_large, L.big, comm, K,
                                  size, w.next, mark_r, w.mark_w, w.iw, w.pt.in_large, w.pt.mv_large[par], R.ctx->d_status);
}

// Local moving until every component's level has ended.  The host enqueues iteration `it` and only then waits for the event of
// iteration it - 1, whose decision (k_lv_decide, on the device) it reads: one iteration ahead, the stream is never drained.
static int lv_local_moving(LvRun& R, const LvG& g, const LvLists& L, int S_max) {
  LvWs& w = R.w;
  hipStream_t st = R.st;
  const LvGrids G = lv_grids(g, L, LV_MOVE_MID_PER_WG);
  const unsigned ga = gficf_grid_capped(g.n, 256, 2048);
  for (int it = 0; it <= LV_MAX_ITERS + 1; ++it) {
    const int par = it & 1;
    hipLaunchKernelGGL(k_lv_pre, dim3(LV_SQ_BLOCKS, (unsigned)R.Bmax), dim3(256), 0, st, (const LvCtl*)w.ctl, par, (const u64*)w.K, (const int32_t*)w.size,
                       w.snapK[par], w.snapS[par], w.pt.sq);
    for (int s = 0; s < S_max; ++s) {
      const LvMove mv{R.r, s, it * S_max + s + 1, it * S_max + s + 1 - S_max};
      if (s == 0) {
        lv_launch_moves<true>(R, g, L, G, mv, par);
        hipLaunchKernelGGL(k_lv_decide, dim3(1), dim3(1024), 0, st, w.ctl, w.pt, (int)G.small, (int)G.mid, (int)G.large, it, R.two_w, R.q_coef, R.host);
      } else lv_launch_moves<false>(R, g, L, G, mv, par);
      hipLaunchKernelGGL(k_lv_apply, dim3(ga), dim3(256), 0, st, g, (const LvCtl*)w.ctl, s, par, w.comm, (const int32_t*)w.next, w.K, w.size, w.snapc[0],
                         w.snapc[1], (const u64*)w.snapK[par ^ 1], (const int32_t*)w.snapS[par ^ 1], w.mark_r, (const int32_t*)w.mark_w);
    }
    GFICF_HIP_CHECK(hipEventRecord(R.ev[par], st));
    if (it >= 1) {                                 // the decision of the iteration BEFORE the one just enqueued
      GFICF_HIP_CHECK(hipEventSynchronize(R.ev[par ^ 1]));
      if (R.debug) {
        fprintf(stderr, "[louvain]   n=%lld iter %d: %d component(s) go on;", (long long)g.n, it - 1, R.host->n_cont[it - 1]);
        for (int b = 0; b < R.Bmax; ++b) fprintf(stderr, " %.9f (%u moved)", R.host->q_iter[b], R.host->mv_iter[b]);
        fprintf(stderr, "\n");
      }
      if (R.host->n_cont[it - 1] == 0) break;      // every level has ended: the iteration just enqueued does nothing
    }
  }
  return GFICF_OK;
}

// the communities in use numbered 0 .. (w.flag = old id -> new id, contiguous per component); lab = new local id of comm[src] (src NULL: the vertex)
static int lv_renumber(LvRun& R, const LvG& g, const int32_t* src, bool seeded, bool refine, int level) {
  LvWs& w = R.w;
  hipLaunchKernelGGL(k_lv_used, dim3(gficf_grid_capped(g.n + 1, 256, 2048)), dim3(256), 0, R.st, g.n, (const int32_t*)w.size, w.flag);
  GFICF_RC(gficf_exclusive_scan_i64(R.ctx, w.flag, g.n + 1));
  hipLaunchKernelGGL(k_lv_ctl_renumbered, dim3(1), dim3(64), 0, R.st, w.ctl, (const int64_t*)w.flag, g.n, seeded ? 1 : 0, refine ? 1 : 0, R.algorithm, level, R.host);
  hipLaunchKernelGGL(k_lv_relabel, dim3(gficf_grid_capped(R.N, 256, 512), (unsigned)R.Bmax), dim3(256), 0, R.st, R.N, (const LvCtl*)w.ctl, src, (const int32_t*)w.comm,
                     (const int64_t*)w.flag, w.lab);
  return GFICF_OK;
}

// g reduced by the labels newid[comm[.]] (the components with `cont` set) into the arrays of nl, and the workgroup-path lists of the result
static int lv_reduce(LvRun& R, const LvG& g, const LvLists& L, const int64_t* newid, LvLevel& nl) {
  LvWs& w = R.w;
  hipStream_t st = R.st;
  const LvCtl* ctl = w.ctl;
  const LvGrids G = lv_grids(g, L, LV_EMIT_MID_PER_WG);
  const unsigned gv = gficf_grid_capped(g.n, 256, 1024);
  GFICF_HIP_CHECK(hipMemsetAsync(nl.beg, 0, sizeof(int64_t) * (size_t)(g.n + 1), st));
  GFICF_HIP_CHECK(hipMemsetAsync(w.cur, 0, sizeof(int32_t) * (size_t)g.n, st));
  hipLaunchKernelGGL(k_lv_rowcap, dim3(gv), dim3(256), 0, st, g, ctl, (const int32_t*)w.comm, newid, (const u64*)w.K, (const int32_t*)w.size, nl.beg, nl.kv, nl.vcomp);
  GFICF_RC(gficf_exclusive_scan_i64(R.ctx, nl.beg, g.n + 1));
  hipLaunchKernelGGL(k_lv_emit_small, dim3(G.small), dim3(256), 0, st, g, ctl, (const int32_t*)w.comm, newid, (const int64_t*)nl.beg, w.cur, nl.nbr, nl.wt);
  if (G.mid) hipLaunchKernelGGL(k_lv_emit_big<LV_EMIT_SLOTS>, dim3(G.mid), dim3(256), LV_EMIT_SLOTS * 12, st, g, ctl, 0, (int64_t)L.n_mid, L.big, (const int32_t*)w.comm,
                                newid, (const int64_t*)nl.beg, w.cur, nl.nbr, nl.wt, R.ctx->d_status);
  if (G.large) hipLaunchKernelGGL(k_lv_emit_big<LV_BIG_SLOTS>, dim3(G.large), dim3(256), LV_BIG_SLOTS * 12, st, g, ctl, 1, (int64_t)L.n_large, L.big, (const int32_t*)w.comm,
                                  newid, (const int64_t*)nl.beg, w.cur, nl.nbr, nl.wt, R.ctx->d_status);
  hipLaunchKernelGGL(k_lv_finish_rows, dim3(gv), dim3(256), 0, st, (const int64_t*)&w.ctl->n_union2, (const int64_t*)nl.beg, (const int32_t*)w.cur, nl.end);
  // the next level's lists (its vertex count is on the device: n_union2)
  GFICF_HIP_CHECK(hipMemsetAsync(&w.ctl->n_mid, 0, 2 * sizeof(unsigned), st));
  const LvG g2{g.n, g.n, 1, nl.beg, nl.end, nl.nbr, nl.wt, nl.kv, nl.vcomp};
  hipLaunchKernelGGL(k_lv_list_big, dim3(gv), dim3(256), 0, st, g2, (const int64_t*)&w.ctl->n_union2, nl.big, &w.ctl->n_mid);
  hipLaunchKernelGGL(k_lv_ctl_publish, dim3(1), dim3(64), 0, st, ctl, R.host);
  return GFICF_OK;
}

static int lv_sync_level(LvRun& R) {                // the level's ONE synchronisation
  GFICF_HIP_CHECK(hipGetLastError());
  GFICF_HIP_CHECK(hipStreamSynchronize(R.st));
  return GFICF_OK;
}

// the sub-rounds the host enqueues per iteration: the most any start that takes part cuts its own into (k_lv_ctl_level sets C.S)
static int lv_s_max(const LvRun& R, const LvStart* S, int B) {
  int m = 1;
  for (int b = 0; b < B; ++b)
    if (S[b].live) { const int s = lv_sub_rounds_of(S[b].n, R.s_env); m = s > m ? s : m; }
  return m;
}

// A pass begins (mirrors k_lv_ctl_level, mode 0): a start whose last pass moved nothing has finished; the others are live with N
// vertices each.  Returns the live starts.
static int lv_begin_pass(const LvRun& R, LvStart* S, int B, int pass) {
  int n_live = 0;
  for (int b = 0; b < B; ++b) {
    if (pass > 0 && !S[b].any_move) S[b].finished = true;
    S[b].live = !S[b].finished; S[b].n = R.N; S[b].any_move = false; S[b].n_saved = 0;
    n_live += S[b].live ? 1 : 0;
  }
  return n_live;
}

// After a descent level's synchronisation (mirrors k_lv_ctl_renumbered, refine == 0, through the LvHostComp it wrote): labels, Q,
// and whether the start goes on to the next level, whose size is saved for algorithm 2's way back.  Returns the starts that go on.
static int lv_read_descent_level(const LvRun& R, LvStart* S, int B, int first, int level) {
  int n_cont = 0;
  for (int b = 0; b < B; ++b) {
    if (!S[b].live) continue;
    const LvHostComp& H = R.host->c[b];
    S[b].n_labels = H.n2; S[b].q_final = H.q_prev; S[b].any_move = H.any_move != 0;
    if (H.cont) {
      if (R.algorithm == 2 && S[b].n_saved == level && level < LV_MAX_SAVED) S[b].saved_n[++S[b].n_saved] = H.n2;
      S[b].n = H.n2; ++n_cont;
    } else {
      S[b].live = false;
    }
    if (R.debug) fprintf(stderr, "[louvain]   start %d: %lld communities, Q %.9f, %s\n", first + b, (long long)H.n2, H.q_prev, H.cont ? "goes on" : "descent done");
  }
  return n_cont;
}

// After a refinement level's synchronisation (mirrors k_lv_ctl_renumbered, refine == 1): the participants' labels and Q.
static void lv_read_refine_level(const LvRun& R, LvStart* S, int B) {
  for (int b = 0; b < B; ++b)
    if (S[b].live) { S[b].n_labels = R.host->c[b].n2; S[b].q_final = R.host->c[b].q_prev; }
}

// One pass's way down: local moving, renumbering and reduction level by level until no start's graph shrinks any more.
static int lv_descent(LvRun& R, LvStart* S, int B, int first, int pass) {
  LvWs& w = R.w;
  LvG g = lv_union0(R, B);
  LvLists L = R.L0;
  int64_t tot_labels = 0;
  for (int b = 0; b < B; ++b) tot_labels += S[b].live ? S[b].n_labels : 0;
  for (int level = 0;; ++level) {
    const bool seeded = level == 0 && pass > 0;
    if (R.debug) fprintf(stderr, "[louvain] starts %d..%d pass %d level %d: union n=%lld\n", first, first + B - 1, pass, level, (long long)g.n);
    hipLaunchKernelGGL(k_lv_ctl_level, dim3(1), dim3(64), 0, R.st, w.ctl, level == 0 ? 0 : 1, pass, R.N, R.s_env);
    lv_start_level(R, g, seeded ? w.lab : nullptr, tot_labels <= LV_ACC_BINS);
    GFICF_RC(lv_local_moving(R, g, L, lv_s_max(R, S, B)));
    GFICF_RC(lv_renumber(R, g, level == 0 ? nullptr : w.lab, seeded, false, level));
    if (R.algorithm == 2 && level < LV_MAX_SAVED)       // the next level's vertices of every start that goes on: lab as it is now
      GFICF_HIP_CHECK(hipMemcpyAsync(w.tops + (size_t)level * (size_t)R.Bmax * (size_t)R.N, w.lab, sizeof(int32_t) * (size_t)B * (size_t)R.N, hipMemcpyDeviceToDevice, R.st));
    LvLevel& nl = w.lvl[level & 1];
    GFICF_RC(lv_reduce(R, g, L, w.flag, nl));           // (enqueued before the host knows whether anybody goes on: a small graph by then)
    GFICF_RC(lv_sync_level(R));
    if (!lv_read_descent_level(R, S, B, first, level)) break;
    const int64_t n2u = R.host->n_union2;
    g = LvG{n2u, n2u, 1, nl.beg, nl.end, nl.nbr, nl.wt, nl.kv, nl.vcomp};
    L = LvLists{nl.big, R.host->n_mid, R.host->n_large};
  }
  return GFICF_OK;
}

// Algorithm 2: back up through the levels, local moving on each with the labels found below it
// (runLouvainAlgorithmWithMultilevelRefinement, reference :629-649).  The graph of a level is rebuilt, not kept.
static int lv_refine_up(LvRun& R, LvStart* S, int B, int first, int pass) {
  LvWs& w = R.w;
  hipStream_t st = R.st;
  const LvCtl* ctl = w.ctl;
  const int64_t N = R.N;
  const LvG g0 = lv_union0(R, B);
  int top_level = -1;
  for (int b = 0; b < B; ++b)
    if (!S[b].finished && S[b].any_move) top_level = S[b].n_saved > top_level ? S[b].n_saved : top_level;
  for (int level = top_level; level >= 0; --level) {
    // the participants and their vertices at this level (mirrors k_lv_ctl_refine): starts that moved in this pass and saved the level
    int64_t n_un = 0, tot_lab = 0;
    for (int b = 0; b < B; ++b) {
      S[b].live = !S[b].finished && S[b].any_move && S[b].n_saved >= level;
      S[b].n = S[b].live ? (level ? S[b].saved_n[level] : R.N) : 0;
      n_un += S[b].n;
      tot_lab += S[b].live ? S[b].n_labels : 0;
    }
    const int32_t* top = level ? w.tops + (size_t)(level - 1) * (size_t)R.Bmax * (size_t)R.N : nullptr;
    hipLaunchKernelGGL(k_lv_ctl_refine, dim3(1), dim3(64), 0, R.st, w.ctl, level, R.N);
    LvG gl = g0;
    LvLists Ll = R.L0;
    if (level) {
      // the level's graph: the finest one reduced by the saved vertex map (labels seed_base + top, new ids = the labels themselves)
      LvLevel& nl = w.lvl[0];
      hipLaunchKernelGGL(k_lv_init, dim3(gficf_grid_capped(g0.n, 256, 2048)), dim3(256), 0, st, g0, ctl, top, w.comm, w.K, w.size, w.mark_r, w.mark_w, w.iw);
      hipLaunchKernelGGL(k_lv_accum, dim3(gficf_grid_capped(g0.n, 256, 1024)), dim3(256), 0, st, g0, ctl, 0, (const int32_t*)w.comm, w.K, w.size);
      hipLaunchKernelGGL(k_lv_internal, dim3(gficf_grid_capped(N, 4, LV_GRID)), dim3(256), 0, st, g0, ctl, (const int32_t*)w.comm, w.pt.in_small);
      hipLaunchKernelGGL(k_lv_seed, dim3(gficf_grid_capped(N, 256, 512), (unsigned)R.Bmax), dim3(256), 0, st, N, ctl, top, (const int32_t*)w.lab, w.seedl);
      hipLaunchKernelGGL(k_lv_iota, dim3(gficf_grid_capped(g0.n + 1, 256, 2048)), dim3(256), 0, st, g0.n, w.flag);
      // the vertex ranges of the level are fixed by k_lv_ctl_refine: v0 of the level, not of the finest graph — seed_base carried them
      // into the labels above; from here on v0 / n are the level's
      GFICF_RC(lv_reduce(R, g0, R.L0, w.flag, nl));
      hipLaunchKernelGGL(k_lv_ctl_self, dim3(1), dim3(256), 0, st, w.ctl, (const u64*)w.pt.in_small, (int)gficf_grid_capped(N, 4, LV_GRID));
      GFICF_RC(lv_sync_level(R));                         // the sizes of the lists
      gl = LvG{n_un, n_un, 1, nl.beg, nl.end, nl.nbr, nl.wt, nl.kv, nl.vcomp};
      Ll = LvLists{nl.big, R.host->n_mid, R.host->n_large};
    }
    if (R.debug) fprintf(stderr, "[louvain] starts %d..%d pass %d refinement level %d: union n=%lld\n", first, first + B - 1, pass, level, (long long)gl.n);
    hipLaunchKernelGGL(k_lv_ctl_level, dim3(1), dim3(64), 0, R.st, w.ctl, 2, pass, R.N, R.s_env);
    lv_start_level(R, gl, level ? w.seedl : w.lab, tot_lab <= LV_ACC_BINS);
    GFICF_RC(lv_local_moving(R, gl, Ll, lv_s_max(R, S, B)));
    GFICF_RC(lv_renumber(R, gl, top, false, true, level));
    GFICF_RC(lv_sync_level(R));
    lv_read_refine_level(R, S, B);
  }
  return GFICF_OK;
}

// a batch's starts against the best so far: strictly better wins, as the reference keeps the first of equals (:128)
static int lv_keep_best(LvRun& R, const LvStart* S, int B, int first, double* q_best, int64_t* n_best) {
  for (int b = 0; b < B; ++b) {
    if (R.debug) fprintf(stderr, "[louvain] start %d: Q %.9f, %lld clusters\n", first + b, S[b].q_final, (long long)S[b].n_labels);
    if (S[b].q_final > *q_best) {
      *q_best = S[b].q_final; *n_best = S[b].n_labels;
      GFICF_HIP_CHECK(hipMemcpyAsync(R.w.best, R.w.lab + (size_t)b * (size_t)R.N, sizeof(int32_t) * (size_t)R.N, hipMemcpyDeviceToDevice, R.st));
    }
  }
  return GFICF_OK;
}

}  // namespace

extern "C" {

size_t gficf_louvain_workspace_bytes(int64_t N, int64_t nnz, int n_start) {
  if (N < 0 || nnz < 0) return 0;
  return lv_carve(nullptr, nullptr, N, nnz, lv_batch(N, nnz, n_start, SIZE_MAX));
}

// Random starts (reference src/RModularityOptimizer.cpp:108-142): every start begins from singletons, runs up to n_iter
// passes and is kept if its modularity beats the best so far.  Nothing here is random; what a start varies is the seed
// of the hash that splits the vertices into sub-round classes (start 0 with seed 0 is the plain deterministic run).
int gficf_louvain_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz,
                         double resolution, int algorithm, int n_start, int n_iter, int seed, int32_t* d_labels, int64_t* n_clusters, double* modularity, void* d_ws,
                         size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  LvRun R;
  bool done = false;
  GFICF_RC(lv_setup(R, ctx, N, d_indptr, d_indices, d_x, nnz, resolution, algorithm, n_start, n_iter, d_labels, n_clusters, modularity, d_ws, ws_bytes, &done));
  if (done) return GFICF_OK;
  LvWs& w = R.w;
  double q_best = -INFINITY;
  int64_t n_best = 0;
  for (int first = 0; first < n_start; first += R.Bmax) {      // a batch: as many starts as run together
    const int B = n_start - first < R.Bmax ? n_start - first : R.Bmax;
    hipLaunchKernelGGL(k_lv_ctl_batch, dim3(1), dim3(64), 0, R.st, w.ctl, B, first, seed);
    LvStart S[LV_MAX_B];
    for (int b = 0; b < LV_MAX_B; ++b) S[b] = LvStart{b >= B, true, false, N, 0, 0.0, 0, {0}};      // (mirrors k_lv_ctl_batch)
    for (int pass = 0; pass < n_iter; ++pass) {
      if (!lv_begin_pass(R, S, B, pass)) break;
      GFICF_RC(lv_descent(R, S, B, first, pass));
      if (algorithm == 2) GFICF_RC(lv_refine_up(R, S, B, first, pass));
    }
    GFICF_RC(lv_keep_best(R, S, B, first, &q_best, &n_best));
  }
  *n_clusters = n_best;
  // clusters by decreasing size
  GFICF_HIP_CHECK(hipMemsetAsync(w.cnt, 0, sizeof(int32_t) * (size_t)n_best, R.st));
  hipLaunchKernelGGL(k_lv_count, dim3(gficf_grid_capped(N, 256, 1024)), dim3(256), 0, R.st, N, n_best, (const int32_t*)w.best, w.cnt);
  GFICF_RC(gficf_comm_number_by_size(ctx, n_best, N, w.cnt, w.best, w.sort, w.rank, d_labels));
  GFICF_HIP_CHECK(hipGetLastError());
  if (modularity) *modularity = q_best;
  return gficf_ctx_sync(ctx);
}

int gficf_louvain_host(gficf_ctx* ctx, int64_t N, const void* indptr, int indptr_is_i64, const int32_t* indices, const double* x,
                       double resolution, int algorithm, int n_start, int n_iter, int seed, int32_t* labels, int64_t* n_clusters, double* modularity) {
  GFICF_CTX_ENTER(ctx);
  if (N < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (n_clusters) *n_clusters = 0;
  if (modularity) *modularity = 0.0;
  if (N == 0) return GFICF_OK;
  if (!indptr || !labels || !n_clusters) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  std::vector<int64_t> h_ptr;
  int64_t nnz = 0;
  int rc = gficf_host_colptr(indptr, indptr_is_i64, N, "indptr", h_ptr, &nnz);
  if (rc) return rc;
  if (nnz > 0 && (!indices || !x)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t nsz = (size_t)(nnz > 0 ? nnz : 1), wsb = gficf_louvain_workspace_bytes(N, nnz, n_start);
  gficf_host_io io{ctx, "gficf_louvain_host"};
  gficf_carver cv;
  int64_t* d_ptr; int32_t *d_idx, *d_lab; double* d_x; void* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_ptr = cv.take<int64_t>((size_t)N + 1); d_idx = cv.take<int32_t>(nsz); d_x = cv.take<double>(nsz);
    d_lab = cv.take<int32_t>((size_t)N); d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_ptr, h_ptr.data(), sizeof(int64_t) * ((size_t)N + 1));
  io.up(d_idx, indices, sizeof(int32_t) * (size_t)nnz);
  io.up(d_x, x, sizeof(double) * (size_t)nnz);
  if (io.ok()) {
    rc = gficf_louvain_device(ctx, N, d_ptr, d_idx, d_x, nnz, resolution, algorithm, n_start, n_iter, seed, d_lab, n_clusters, modularity, d_ws, wsb);
    if (!rc) io.down(labels, d_lab, sizeof(int32_t) * (size_t)N);
  }
  return io.finish(rc);
}

}  // extern "C"
