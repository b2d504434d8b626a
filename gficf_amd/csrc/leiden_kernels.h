// leiden_kernels.h — what leiden.hip and slm.hip share, as text: the level graph, the workspace and run structs, the
// fixed-point / accumulate / quality kernels, local moving (k_ld_move, k_ld_apply: with or without a fence), aggregation and the scans.
#ifndef GFICF_LEIDEN_KERNELS_H
#define GFICF_LEIDEN_KERNELS_H

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "common.h"
#include "community_ops.h"

namespace {

typedef unsigned long long u64;

constexpr int LD_SMALL_DEG = 128;             // up to here: one wave per vertex, 256-slot table
constexpr int LD_SMALL_SLOTS = 256;
constexpr int LD_BIG_SLOTS = 4096;            // beyond: one workgroup per vertex, 16 KB keys + 32 KB sums
constexpr int LD_PASS_KEYS = 1024;            // communities a pass of the workgroup path is sized for (a quarter of its table)
constexpr int LD_SUB = 4;                     // sub-rounds (hash classes) of a pass of local moving
constexpr int LD_MAX_PASSES = 64;
constexpr int LD_MAX_LEVELS = 64;
constexpr int LD_GRID = 1536;                 // workgroups (4 waves) of the wave-per-vertex kernels
constexpr int LD_GRID_BIG = 1024;             // of the workgroup-per-vertex kernels
constexpr int LD_PARTS = 1024;                // fixed partial sums of the quality launches
constexpr uint32_t LD_ST_CSC = 1u, LD_ST_VALUE = 2u, LD_ST_ID = 4u, LD_ST_DENSE = 8u;
enum { LD_S_2W = 0, LD_S_MAXW = 1, LD_S_STATUS = 2, LD_S_CHANGED = 3, LD_S_BIG = 4, LD_S_INW = 5, LD_S_SQ = 6, LD_S_N = 8 };

// a level's graph: rows [beg[v], end[v]); a self-loop (nbr == v) is weight inside v, never an edge
struct LdG {
  int64_t n;
  const int64_t* beg;
  const int64_t* end;
  const int32_t* nbr;
  const u64* wt;
  const u64* kv;
};

// ---------------------------------------------------------------- the LDS table of a vertex's neighbouring communities
template <bool BLK> struct LdShape {
  static constexpr int SLOTS = BLK ? LD_BIG_SLOTS : LD_SMALL_SLOTS;
  static constexpr int NT = BLK ? 256 : 64;
  static constexpr int TABLE = BLK ? LD_BIG_SLOTS : 4 * LD_SMALL_SLOTS;      // entries of the workgroup's arrays
};
template <bool BLK> __device__ inline void ld_sync() {
  if (BLK) __syncthreads();
  else GFICF_WAVE_SYNC();
}
template <bool BLK> __device__ inline int ld_tid() { return BLK ? (int)threadIdx.x : (int)(threadIdx.x & 63); }
template <bool BLK> __device__ inline int64_t ld_first_vertex() { return BLK ? (int64_t)blockIdx.x : (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }
template <bool BLK> __device__ inline int64_t ld_vertex_stride() { return BLK ? (int64_t)gridDim.x : (int64_t)gridDim.x * 4; }
// passes over a long row: the distinct keys are at most min(entries, vertices of the level)
template <bool BLK> __device__ inline int ld_passes(int64_t deg, int64_t n) {
  if (!BLK) return 1;
  const int64_t d = deg < n ? deg : n;
  return (int)((d + LD_PASS_KEYS - 1) / LD_PASS_KEYS);
}
__device__ inline bool ld_in_pass(int32_t c, int P, int p) { return P == 1 || (int)((gficf_comm_hash((uint32_t)c) >> 12) % (uint32_t)P) == p; }

template <bool BLK> __device__ inline void ld_clear(int32_t* key, u64* val) {
  for (int i = ld_tid<BLK>(); i < LdShape<BLK>::SLOTS; i += LdShape<BLK>::NT) { key[i] = -1; val[i] = 0; }
}

__device__ inline bool ld_better(double g, int32_t c, double bg, int32_t bc) { return c >= 0 && (bc < 0 || g > bg || (g == bg && c < bc)); }
// best (gain, label) and a sum over the group, the same in every thread; red*: four entries each of the workgroup's LDS
template <bool BLK>
__device__ inline void ld_reduce(double& g, int32_t& c, u64& s, double* red_g, int32_t* red_c, u64* red_s) {
  for (int d = 32; d >= 1; d >>= 1) {
    const double og = __shfl_xor(g, d);
    const int32_t oc = __shfl_xor(c, d);
    if (ld_better(og, oc, g, c)) { g = og; c = oc; }
  }
  s = gficf_wave_sum(s);
  if (BLK) {
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { red_g[threadIdx.x >> 6] = g; red_c[threadIdx.x >> 6] = c; red_s[threadIdx.x >> 6] = s; }
    __syncthreads();
    g = red_g[0]; c = red_c[0]; s = red_s[0];
    for (int w = 1; w < 4; ++w) {
      if (ld_better(red_g[w], red_c[w], g, c)) { g = red_g[w]; c = red_c[w]; }
      s += red_s[w];
    }
  }
}

// ---------------------------------------------------------------- level 0
// a wave per vertex: fixed-point weights (the diagonal and everything invalid: 0), vertex weight, 2W, largest weight
__global__ __launch_bounds__(256) void k_ld_fix(int64_t N, int64_t nnz, const int64_t* __restrict__ ptr, const int32_t* __restrict__ nbr,
                                                const double* __restrict__ x, u64* __restrict__ wt, u64* __restrict__ kv, u64* __restrict__ scal) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t* const status = (uint32_t*)(scal + LD_S_STATUS);
  u64 total = 0, mx = 0;
  for (int64_t v = (int64_t)blockIdx.x * 4 + wave; v < N; v += (int64_t)gridDim.x * 4) {
    int64_t lo = ptr[v], hi = ptr[v + 1];
    if (lo < 0 || hi < lo || hi > nnz || (v == 0 && lo != 0)) { if (lane == 0) atomicOr(status, LD_ST_CSC); lo = hi = 0; }
    if (hi - lo > LD_SMALL_DEG && lane == 0) *(uint32_t*)(scal + LD_S_BIG) = 1u;
    u64 s = 0;
    for (int64_t e = lo + lane; e < hi; e += 64) {
      const int32_t u = nbr[e];
      const double w = x[e];
      const bool idok = u >= 0 && u < N, ok = idok && w >= 0.0 && w <= 1048576.0;      // NaN fails the comparisons
      if (!ok) atomicOr(status, idok ? LD_ST_VALUE : LD_ST_CSC);
      const u64 f = ok && u != v ? (u64)llrint(w * GFICF_COMM_SCALE) : 0ull;
      wt[e] = f;
      s += f;
      mx = f > mx ? f : mx;
    }
    s = gficf_wave_sum(s);
    if (lane == 0) { kv[v] = s; total += s; }
  }
  for (int d = 32; d >= 1; d >>= 1) { const u64 o = __shfl_xor(mx, d); mx = o > mx ? o : mx; }
  __shared__ u64 s_sum[4], s_max[4];
  if (lane == 0) { s_sum[wave] = total; s_max[wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const u64 t = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    for (int w = 1; w < 4; ++w) mx = s_max[w] > mx ? s_max[w] : mx;
    if (t) atomicAdd(scal + LD_S_2W, t);
    if (mx) atomicMax(scal + LD_S_MAXW, mx);
  }
}

__global__ __launch_bounds__(256) void k_ld_check_labels(int64_t N, const int32_t* __restrict__ lab, u64* __restrict__ scal) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < N && (lab[v] < 0 || lab[v] >= N)) atomicOr((uint32_t*)(scal + LD_S_STATUS), LD_ST_ID);
}

// first[c] = the smallest member of c (an integer minimum: the order does not matter)
__global__ __launch_bounds__(256) void k_ld_first(int64_t n, const int32_t* __restrict__ lab, int32_t* __restrict__ first) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) atomicMin(&first[lab[v]], (int32_t)v);
}
__global__ __launch_bounds__(256) void k_ld_canon(int64_t n, const int32_t* __restrict__ lab, const int32_t* __restrict__ first, int32_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) out[v] = first[lab[v]];
}
__global__ __launch_bounds__(256) void k_ld_gather(int64_t N, const int32_t* __restrict__ top, const int32_t* __restrict__ comm, int32_t* __restrict__ lab) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < N) lab[v] = comm[top[v]];
}

// totals and sizes of a partition (K and size zeroed before)
__global__ __launch_bounds__(256) void k_ld_accum(int64_t n, const int32_t* __restrict__ comm, const u64* __restrict__ kv, u64* __restrict__ K,
                                                  int32_t* __restrict__ size) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n) return;
  const int32_t c = comm[v];
  if (kv[v]) atomicAdd(&K[c], kv[v]);
  atomicAdd(&size[c], 1);
}

// ---------------------------------------------------------------- local moving
// FENCE: an entry (v, u) exists only if fence[u] == fence[v] (the sub-moving of slm.hip: fence = the parent communities);
// without it `fence` is not read
template <bool BLK, bool FENCE>
__global__ __launch_bounds__(256) void k_ld_move(LdG g, double r, int s, int t, uint32_t hseed, const int32_t* __restrict__ comm,
                                                 const u64* __restrict__ K, const int32_t* __restrict__ size, const int32_t* __restrict__ mark,
                                                 const int32_t* __restrict__ fence, int32_t* __restrict__ next, u64* __restrict__ scal) {
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
    const bool run = (int)(gficf_comm_hash((uint32_t)v ^ hseed) % (uint32_t)LD_SUB) == s && (t <= LD_SUB || mark[v] >= t - LD_SUB);
    if (!run) {
      if (tid == 0) next[v] = -1;
      continue;
    }
    const int32_t cv = comm[v];
    const u64 kvv = g.kv[v];
    const int32_t fv = FENCE ? fence[v] : 0;
    const int P = ld_passes<BLK>(hi - lo, g.n);
    double bg = 0.0;
    int32_t bc = -1;
    u64 stay = 0;
    for (int p = 0; p < P; ++p) {
      ld_clear<BLK>(key, val);
      ld_sync<BLK>();
      for (int64_t e = lo + tid; e < hi; e += SH::NT) {
        const int32_t u = g.nbr[e];
        const u64 w = g.wt[e];
        if (u == v || w == 0) continue;
        if (FENCE && fence[u] != fv) continue;
        const int32_t c = comm[u];
        if (c == cv) { if (p == 0) stay += w; continue; }
        if (!ld_in_pass(c, P, p)) continue;
        bool own;      // (who claimed the slot: not needed here)
        if (gficf_comm_insert<SH::SLOTS>(key, val, c, w, &own) < 0) atomicOr((uint32_t*)(scal + LD_S_STATUS), LD_ST_DENSE);
      }
      ld_sync<BLK>();
      for (int i = tid; i < SH::SLOTS; i += SH::NT) {
        const int32_t c = key[i];
        if (c < 0) continue;
        const double gain = (double)val[i] - r * (double)kvv * (double)K[c];
        if (ld_better(gain, c, bg, bc)) { bg = gain; bc = c; }
      }
      ld_sync<BLK>();
    }
    ld_reduce<BLK>(bg, bc, stay, red_g, red_c, red_s);
    if (tid == 0) {
      const double gs = (double)stay - r * (double)kvv * (double)(K[cv] - kvv);
      bool mv = bc >= 0 && (bg > gs || (bg == gs && bc < cv));
      if (mv && size[cv] == 1 && size[bc] == 1 && bc > cv) mv = false;      // two singletons never swap
      next[v] = mv ? bc : cv;
    }
  }
}

// a wave per vertex: the decided moves applied to labels, totals and sizes; the mover's neighbours (the targets of its entries of
// non-zero weight: a self-loop of a coarser level stamps the mover itself) stamped for another look
template <bool FENCE>
__global__ __launch_bounds__(256) void k_ld_apply(LdG g, int t, int32_t* __restrict__ comm, const int32_t* __restrict__ next, u64* __restrict__ K,
                                                  int32_t* __restrict__ size, int32_t* __restrict__ mark, const int32_t* __restrict__ fence,
                                                  u64* __restrict__ scal) {
  const int lane = threadIdx.x & 63;
  for (int64_t v = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); v < g.n; v += (int64_t)gridDim.x * 4) {
    const int32_t nx = next[v];
    if (nx < 0) continue;
    const int32_t old = comm[v];
    if (nx == old) continue;
    if (lane == 0) {
      const u64 k = g.kv[v];
      comm[v] = nx;
      atomicAdd(&K[nx], k);
      atomicAdd(&K[old], 0ull - k);
      atomicAdd(&size[nx], 1);
      atomicSub(&size[old], 1);
      *(uint32_t*)(scal + LD_S_CHANGED) = 1u;
    }
    const int32_t fv = FENCE ? fence[v] : 0;
    for (int64_t e = g.beg[v] + lane; e < g.end[v]; e += 64) {
      if (!g.wt[e]) continue;               // a stored zero, and the level-0 diagonal (k_ld_fix: 0), is no edge and carries no stamp
      const int32_t u = g.nbr[e];
      if (FENCE && fence[u] != fv) continue;                                  // nor does an entry across the fence
      mark[u] = t;
    }
  }
}

// ---------------------------------------------------------------- quality: internal weight and sum of K^2, fixed partial sums
__global__ __launch_bounds__(256) void k_ld_inw(LdG g, const int32_t* __restrict__ comm, u64* __restrict__ parts) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  u64 s = 0;
  for (int64_t v = (int64_t)blockIdx.x * 4 + wave; v < g.n; v += (int64_t)gridDim.x * 4) {
    const int32_t cv = comm[v];
    for (int64_t e = g.beg[v] + lane; e < g.end[v]; e += 64) {
      const int32_t u = g.nbr[e];
      if (u == v || comm[u] == cv) s += g.wt[e];
    }
  }
  s = gficf_wave_sum(s);
  __shared__ u64 s_sum[4];
  if (lane == 0) s_sum[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) parts[blockIdx.x] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

__global__ __launch_bounds__(256) void k_ld_sq(int64_t n, const u64* __restrict__ K, double* __restrict__ parts) {
  __shared__ double s_x[256];
  double x = 0.0;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.x * 256) {
    const double k = (double)K[c];
    x += k * k;
  }
  x = gficf_block_sum_f64(x, s_x);
  if (threadIdx.x == 0) parts[blockIdx.x] = x;
}

__global__ __launch_bounds__(256) void k_ld_qfin(int nb_in, const u64* __restrict__ pin, int nb_sq, const double* __restrict__ psq, u64* __restrict__ scal) {
  __shared__ double s_x[256];
  __shared__ u64 s_i[256];
  u64 a = 0;
  double x = 0.0;
  for (int i = threadIdx.x; i < nb_in; i += 256) a += pin[i];
  for (int i = threadIdx.x; i < nb_sq; i += 256) x += psq[i];
  s_i[threadIdx.x] = a;
  x = gficf_block_sum_f64(x, s_x);
  if (threadIdx.x == 0) {
    u64 t = 0;
    for (int i = 0; i < 256; ++i) t += s_i[i];
    scal[LD_S_INW] = t;
    scal[LD_S_SQ] = (u64)__double_as_longlong(x);
  }
}

__global__ __launch_bounds__(256) void k_ld_flag_size(int64_t n, const int32_t* __restrict__ size, int64_t* __restrict__ flag) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c <= n) flag[c] = c < n && size[c] > 0 ? 1 : 0;
}
__global__ __launch_bounds__(256) void k_ld_flag_ref(int64_t n, const int32_t* __restrict__ ref, int64_t* __restrict__ flag) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v <= n) flag[v] = v < n && ref[v] == (int32_t)v ? 1 : 0;
}

// ---------------------------------------------------------------- aggregation
// newid: exclusive scan of "v is the label of a refined community".  k of a new vertex, the capacity of its row (the entries of
// its members), the smallest new vertex of every community (its label on the next level)
__global__ __launch_bounds__(256) void k_ag_vertex(LdG g, const int32_t* __restrict__ ref, const int64_t* __restrict__ newid, const int32_t* __restrict__ comm,
                                                   u64* __restrict__ kv2, int64_t* __restrict__ rowcap, int32_t* __restrict__ cmin) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= g.n) return;
  const int64_t R = newid[ref[v]];
  if (g.kv[v]) atomicAdd(&kv2[R], g.kv[v]);
  const int64_t deg = g.end[v] - g.beg[v];
  if (deg) atomicAdd((u64*)&rowcap[R], (u64)deg);
  atomicMin(&cmin[comm[v]], (int32_t)R);
}

template <bool BLK>
__global__ __launch_bounds__(256) void k_ag_emit(LdG g, const int32_t* __restrict__ ref, const int64_t* __restrict__ newid, const int64_t* __restrict__ beg2,
                                                 u64* __restrict__ cur, int32_t* __restrict__ nbr2, u64* __restrict__ wt2, u64* __restrict__ scal) {
  using SH = LdShape<BLK>;
  __shared__ int32_t s_key[SH::TABLE];
  __shared__ u64 s_val[SH::TABLE];
  int32_t* const key = BLK ? s_key : s_key + (threadIdx.x >> 6) * LD_SMALL_SLOTS;
  u64* const val = BLK ? s_val : s_val + (threadIdx.x >> 6) * LD_SMALL_SLOTS;
  const int tid = ld_tid<BLK>(), lane = threadIdx.x & 63;
  const int wv = BLK ? (int)(threadIdx.x >> 6) : 0, nw = BLK ? 4 : 1;
  for (int64_t v = ld_first_vertex<BLK>(); v < g.n; v += ld_vertex_stride<BLK>()) {
    const int64_t lo = g.beg[v], hi = g.end[v];
    if ((hi - lo > LD_SMALL_DEG) != BLK || hi == lo) continue;
    const int64_t R = newid[ref[v]], row = beg2[R];
    const int P = ld_passes<BLK>(hi - lo, g.n);
    for (int p = 0; p < P; ++p) {
      ld_clear<BLK>(key, val);
      ld_sync<BLK>();
      for (int64_t e = lo + tid; e < hi; e += SH::NT) {
        const u64 w = g.wt[e];
        if (w == 0) continue;
        const int32_t c = (int32_t)newid[ref[g.nbr[e]]];
        if (!ld_in_pass(c, P, p)) continue;
        bool own;      // (who claimed the slot: not needed here)
        if (gficf_comm_insert<SH::SLOTS>(key, val, c, w, &own) < 0) atomicOr((uint32_t*)(scal + LD_S_STATUS), LD_ST_DENSE);
      }
      ld_sync<BLK>();
      // every wave places the slots of its 64-slot chunks: one reservation in the row per wave
      int cnt = 0;
      for (int ch = wv; ch < SH::SLOTS / 64; ch += nw) cnt += __popcll(__ballot(key[ch * 64 + lane] >= 0));
      u64 base = 0;
      if (lane == 0 && cnt) base = atomicAdd(&cur[R], (u64)cnt);
      base = __shfl(base, 0);
      for (int ch = wv; ch < SH::SLOTS / 64; ch += nw) {
        const int32_t c = key[ch * 64 + lane];
        const u64 mask = __ballot(c >= 0);
        if (c >= 0) {
          const int64_t at = row + (int64_t)base + __popcll(mask & ((1ull << lane) - 1ull));
          nbr2[at] = c;
          wt2[at] = val[ch * 64 + lane];
        }
        base += (u64)__popcll(mask);
      }
      ld_sync<BLK>();
    }
  }
}

__global__ __launch_bounds__(256) void k_ag_finish(int64_t n2, const int64_t* __restrict__ beg2, const u64* __restrict__ cur, int64_t* __restrict__ end2,
                                                   u64* __restrict__ scal) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v >= n2) return;
  end2[v] = beg2[v] + (int64_t)cur[v];
  if (cur[v] > (u64)LD_SMALL_DEG) *(uint32_t*)(scal + LD_S_BIG) = 1u;
}
__global__ __launch_bounds__(256) void k_ag_comm(int64_t n, const int32_t* __restrict__ ref, const int64_t* __restrict__ newid, const int32_t* __restrict__ comm,
                                                 const int32_t* __restrict__ cmin, int32_t* __restrict__ comm2) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) comm2[newid[ref[v]]] = cmin[comm[v]];      // the members of a refined community share a community: the same value
}
__global__ __launch_bounds__(256) void k_ag_top(int64_t N, int32_t* __restrict__ top, const int32_t* __restrict__ ref, const int64_t* __restrict__ newid) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < N) top[v] = (int32_t)newid[ref[top[v]]];
}

// ---------------------------------------------------------------- host side
struct LdLevel { int64_t* beg; int64_t* end; int32_t* nbr; u64* wt; u64* kv; };
struct LdWs {
  u64 *wt0, *kv0;
  LdLevel lvl[2];
  int32_t *comm, *comm2, *next, *size, *mark, *snapc, *snapS, *ref, *rsize, *prop, *top, *lab, *first, *rank;
  u64 *K, *snapK, *Kr, *ext, *ec, *cur;
  int64_t *flag, *newid;
  u64* pin; double* psq;
  gficf_comm_sort_bufs sort;
  u64* scal;
};

size_t ld_carve(LdWs* w, void* base, int64_t N, int64_t nnz) {
  gficf_carver b{(char*)base};
  const size_t n = (size_t)(N > 0 ? N : 1), m = (size_t)(nnz > 0 ? nnz : 1);
  LdWs d;
  d.wt0 = b.take<u64>(m); d.kv0 = b.take<u64>(n);
  for (int i = 0; i < 2; ++i) {
    d.lvl[i].beg = b.take<int64_t>(n + 1); d.lvl[i].end = b.take<int64_t>(n + 1); d.lvl[i].nbr = b.take<int32_t>(m); d.lvl[i].wt = b.take<u64>(m);
    d.lvl[i].kv = b.take<u64>(n);
  }
  int32_t** const i32[] = {&d.comm, &d.comm2, &d.next, &d.size, &d.mark, &d.snapc, &d.snapS, &d.ref, &d.rsize, &d.prop, &d.top, &d.lab, &d.first, &d.rank};
  for (int32_t** p : i32) *p = b.take<int32_t>(n);
  u64** const i64[] = {&d.K, &d.snapK, &d.Kr, &d.ext, &d.ec, &d.cur};
  for (u64** p : i64) *p = b.take<u64>(n);
  d.flag = b.take<int64_t>(n + 1); d.newid = b.take<int64_t>(n + 1);
  d.pin = b.take<u64>(LD_PARTS); d.psq = b.take<double>(LD_PARTS);
  d.sort.take(b, n, N > 0 ? N : 1);
  d.scal = b.take<u64>(LD_S_N);
  if (w) *w = d;
  return b.total();
}

struct LdRun {
  gficf_ctx* ctx;
  LdWs w;
  int64_t N, nnz;
  double resolution, two_w, r;
  LdG g0;
  bool big0;
  hipStream_t st() const { return ctx->stream; }
};

int ld_read_scal(LdRun& R, u64* h) {
  GFICF_HIP_CHECK(hipMemcpyAsync(h, R.w.scal, sizeof(u64) * LD_S_N, hipMemcpyDeviceToHost, R.st()));
  GFICF_HIP_CHECK(hipStreamSynchronize(R.st()));
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// fixed-point weights and validation of the matrix (and of `labels`, if given); fills two_w, r, g0, big0.  *no_edges: 2W == 0
int ld_setup(LdRun& R, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, const int32_t* d_labels, bool* no_edges) {
  LdWs& w = R.w;
  GFICF_HIP_CHECK(hipMemsetAsync(w.scal, 0, sizeof(u64) * LD_S_N, R.st()));
  hipLaunchKernelGGL(k_ld_fix, dim3(gficf_grid_capped(R.N, 4, 2048)), dim3(256), 0, R.st(), R.N, R.nnz, d_indptr, d_indices, d_x, w.wt0, w.kv0, w.scal);
  if (d_labels) hipLaunchKernelGGL(k_ld_check_labels, dim3(gficf_grid_capped(R.N, 256, 1u << 30)), dim3(256), 0, R.st(), R.N, d_labels, w.scal);
  u64 h[LD_S_N];
  GFICF_RC(ld_read_scal(R, h));
  const uint32_t status = (uint32_t)h[LD_S_STATUS];
  if (status & LD_ST_CSC) GFICF_FAIL(GFICF_ERR_BAD_CSC, "malformed matrix: a row pointer that is not monotone within [0, nnz] or an index outside [0, N)");
  if (status & LD_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "an edge weight that is not finite or outside [0, 2^20]");
  if (status & LD_ST_ID) GFICF_FAIL(GFICF_ERR_BAD_ID, "a label outside [0, N)");
  if ((double)h[LD_S_MAXW] * (double)R.nnz >= 9.0e18)
    GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "edge weights too large for the 2^-32 fixed-point sums (largest weight x entries >= 2^31): scale the matrix");
  R.two_w = (double)h[LD_S_2W];
  *no_edges = h[LD_S_2W] == 0;
  R.r = *no_edges ? 0.0 : R.resolution / R.two_w;
  R.big0 = (uint32_t)h[LD_S_BIG] != 0;
  R.g0 = LdG{R.N, d_indptr, d_indptr + 1, d_indices, w.wt0, w.kv0};
  return GFICF_OK;
}

// out[v] = the smallest member of lab[v]'s community (out may be lab)
void ld_canon(LdRun& R, const int32_t* lab, int32_t* out) {
  const unsigned gb = gficf_grid_capped(R.N, 256, 1u << 30);
  hipLaunchKernelGGL(k_comm_fill<int32_t>, dim3(gb), dim3(256), 0, R.st(), R.N, INT32_MAX, R.w.first);
  hipLaunchKernelGGL(k_ld_first, dim3(gb), dim3(256), 0, R.st(), R.N, lab, R.w.first);
  hipLaunchKernelGGL(k_ld_canon, dim3(gb), dim3(256), 0, R.st(), R.N, lab, (const int32_t*)R.w.first, out);
}

int ld_accum(LdRun& R, const LdG& g, const int32_t* comm) {
  GFICF_HIP_CHECK(hipMemsetAsync(R.w.K, 0, sizeof(u64) * (size_t)g.n, R.st()));
  GFICF_HIP_CHECK(hipMemsetAsync(R.w.size, 0, sizeof(int32_t) * (size_t)g.n, R.st()));
  hipLaunchKernelGGL(k_ld_accum, dim3(gficf_grid_capped(g.n, 256, 1u << 30)), dim3(256), 0, R.st(), g.n, comm, g.kv, R.w.K, R.w.size);
  return GFICF_OK;
}

// Q of (comm, K) on g; synchronises.  h: the scalar block as read (the "moved" word among it)
int ld_quality(LdRun& R, const LdG& g, const int32_t* comm, const u64* K, double* q, u64* h) {
  const unsigned gi = gficf_grid_capped(g.n, 4, LD_PARTS), gs = gficf_grid_capped(g.n, 256, LD_PARTS);
  hipLaunchKernelGGL(k_ld_inw, dim3(gi), dim3(256), 0, R.st(), g, comm, R.w.pin);
  hipLaunchKernelGGL(k_ld_sq, dim3(gs), dim3(256), 0, R.st(), g.n, K, R.w.psq);
  hipLaunchKernelGGL(k_ld_qfin, dim3(1), dim3(256), 0, R.st(), (int)gi, (const u64*)R.w.pin, (int)gs, (const double*)R.w.psq, R.w.scal);
  GFICF_RC(ld_read_scal(R, h));
  double sq;
  memcpy(&sq, &h[LD_S_SQ], sizeof(double));
  *q = (double)h[LD_S_INW] / R.two_w - R.resolution * sq / (R.two_w * R.two_w);
  return GFICF_OK;
}

int ld_dense_check(const u64* h) {
  if ((uint32_t)h[LD_S_STATUS] & LD_ST_DENSE)
    GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "a vertex touches more communities of one hash class than the 4096-slot table holds");
  return GFICF_OK;
}

// exclusive scan of flag[0 .. n] in place, its total (flag[n]) read back
int ld_scan_count(LdRun& R, int64_t* flag, int64_t n, int64_t* total) {
  GFICF_RC(gficf_exclusive_scan_i64(R.ctx, flag, n + 1));
  GFICF_HIP_CHECK(hipMemcpyAsync(total, flag + n, sizeof(int64_t), hipMemcpyDeviceToHost, R.st()));
  GFICF_HIP_CHECK(hipStreamSynchronize(R.st()));
  return GFICF_OK;
}

// the partition local moving works on: labels, totals and sizes of its communities (n entries each)
struct LdPart { int32_t* comm; u64* K; int32_t* size; };

// local moving on g from the partition p until nothing moves.  FENCE: only the entries inside one community of `fence` exist
template <bool FENCE>
int ld_local_moving(LdRun& R, const LdG& g, bool big, int level, uint32_t seed, const LdPart& p, const int32_t* fence, int* passes, double* q_out) {
  LdWs& w = R.w;
  const unsigned gw = gficf_grid_capped(g.n, 4, LD_GRID), gb = gficf_grid_capped(g.n, 1, LD_GRID_BIG);
  const uint32_t hseed = gficf_comm_hash(seed * 0x9E3779B1u + (uint32_t)level * 0x85EBCA77u + 0x165667B1u);
  GFICF_HIP_CHECK(hipMemsetAsync(w.mark, 0, sizeof(int32_t) * (size_t)g.n, R.st()));
  u64 h[LD_S_N];
  double q_prev = 0.0;
  GFICF_RC(ld_quality(R, g, p.comm, p.K, &q_prev, h));
  int t = 0;
  *passes = 0;
  for (int pass = 0; pass < LD_MAX_PASSES; ++pass) {
    ++*passes;
    GFICF_HIP_CHECK(hipMemcpyAsync(w.snapc, p.comm, sizeof(int32_t) * (size_t)g.n, hipMemcpyDeviceToDevice, R.st()));
    GFICF_HIP_CHECK(hipMemcpyAsync(w.snapS, p.size, sizeof(int32_t) * (size_t)g.n, hipMemcpyDeviceToDevice, R.st()));
    GFICF_HIP_CHECK(hipMemcpyAsync(w.snapK, p.K, sizeof(u64) * (size_t)g.n, hipMemcpyDeviceToDevice, R.st()));
    GFICF_HIP_CHECK(hipMemsetAsync(w.scal + LD_S_CHANGED, 0, sizeof(u64), R.st()));
    for (int s = 0; s < LD_SUB; ++s) {
      ++t;
      hipLaunchKernelGGL((k_ld_move<false, FENCE>), dim3(gw), dim3(256), 0, R.st(), g, R.r, s, t, hseed, (const int32_t*)p.comm, (const u64*)p.K,
                         (const int32_t*)p.size, (const int32_t*)w.mark, fence, w.next, w.scal);
      if (big)
        hipLaunchKernelGGL((k_ld_move<true, FENCE>), dim3(gb), dim3(256), 0, R.st(), g, R.r, s, t, hseed, (const int32_t*)p.comm, (const u64*)p.K,
                           (const int32_t*)p.size, (const int32_t*)w.mark, fence, w.next, w.scal);
      hipLaunchKernelGGL(k_ld_apply<FENCE>, dim3(gw), dim3(256), 0, R.st(), g, t, p.comm, (const int32_t*)w.next, p.K, p.size, w.mark, fence, w.scal);
    }
    double q = 0.0;
    GFICF_RC(ld_quality(R, g, p.comm, p.K, &q, h));
    GFICF_RC(ld_dense_check(h));
    if (!(uint32_t)h[LD_S_CHANGED]) break;
    if (q < q_prev) {                                      // a pass that lowers Q is undone and ends the level
      GFICF_HIP_CHECK(hipMemcpyAsync(p.comm, w.snapc, sizeof(int32_t) * (size_t)g.n, hipMemcpyDeviceToDevice, R.st()));
      GFICF_HIP_CHECK(hipMemcpyAsync(p.size, w.snapS, sizeof(int32_t) * (size_t)g.n, hipMemcpyDeviceToDevice, R.st()));
      GFICF_HIP_CHECK(hipMemcpyAsync(p.K, w.snapK, sizeof(u64) * (size_t)g.n, hipMemcpyDeviceToDevice, R.st()));
      break;
    }
    q_prev = q;
  }
  *q_out = q_prev;
  return GFICF_OK;
}

// aggregation of g by the partition ref (ref[label] == label, its n2 labels scanned into w.newid) into the level buffers `level & 1`:
// the new graph in *g (and whether it has a long row in *big), its vertices seeded in w.comm by their parent community, w.top followed
int ld_aggregate(LdRun& R, LdG* g_io, bool* big_io, int level, int64_t n2) {
  LdWs& w = R.w;
  const LdG g = *g_io;
  const bool big = *big_io;
  const LdLevel& L = w.lvl[level & 1];
  const unsigned gw = gficf_grid_capped(g.n, 4, LD_GRID), gb = gficf_grid_capped(g.n, 1, LD_GRID_BIG), g2 = gficf_grid_capped(n2, 256, 1u << 30);
  const unsigned gn = gficf_grid_capped(g.n, 256, 1u << 30), gN = gficf_grid_capped(R.N, 256, 1u << 30);
  GFICF_HIP_CHECK(hipMemsetAsync(L.kv, 0, sizeof(u64) * (size_t)n2, R.st()));
  GFICF_HIP_CHECK(hipMemsetAsync(L.beg, 0, sizeof(int64_t) * (size_t)(n2 + 1), R.st()));
  GFICF_HIP_CHECK(hipMemsetAsync(w.cur, 0, sizeof(u64) * (size_t)n2, R.st()));
  GFICF_HIP_CHECK(hipMemsetAsync(w.scal + LD_S_BIG, 0, sizeof(u64), R.st()));
  hipLaunchKernelGGL(k_comm_fill<int32_t>, dim3(gn), dim3(256), 0, R.st(), g.n, INT32_MAX, w.first);
  hipLaunchKernelGGL(k_ag_vertex, dim3(gn), dim3(256), 0, R.st(), g, (const int32_t*)w.ref, (const int64_t*)w.newid, (const int32_t*)w.comm, L.kv, L.beg,
                     w.first);
  GFICF_RC(gficf_exclusive_scan_i64(R.ctx, L.beg, n2 + 1));
  hipLaunchKernelGGL(k_ag_emit<false>, dim3(gw), dim3(256), 0, R.st(), g, (const int32_t*)w.ref, (const int64_t*)w.newid, (const int64_t*)L.beg, w.cur,
                     L.nbr, L.wt, w.scal);
  if (big)
    hipLaunchKernelGGL(k_ag_emit<true>, dim3(gb), dim3(256), 0, R.st(), g, (const int32_t*)w.ref, (const int64_t*)w.newid, (const int64_t*)L.beg, w.cur,
                       L.nbr, L.wt, w.scal);
  hipLaunchKernelGGL(k_ag_finish, dim3(g2), dim3(256), 0, R.st(), n2, (const int64_t*)L.beg, (const u64*)w.cur, L.end, w.scal);
  hipLaunchKernelGGL(k_ag_comm, dim3(gn), dim3(256), 0, R.st(), g.n, (const int32_t*)w.ref, (const int64_t*)w.newid, (const int32_t*)w.comm,
                     (const int32_t*)w.first, w.comm2);
  hipLaunchKernelGGL(k_ag_top, dim3(gN), dim3(256), 0, R.st(), R.N, w.top, (const int32_t*)w.ref, (const int64_t*)w.newid);
  GFICF_HIP_CHECK(hipMemcpyAsync(w.comm, w.comm2, sizeof(int32_t) * (size_t)n2, hipMemcpyDeviceToDevice, R.st()));
  u64 h[LD_S_N];
  GFICF_RC(ld_read_scal(R, h));
  GFICF_RC(ld_dense_check(h));
  *big_io = (uint32_t)h[LD_S_BIG] != 0;
  *g_io = LdG{n2, L.beg, L.end, L.nbr, L.wt, L.kv};
  return GFICF_OK;
}

int ld_check_args(int64_t N, int64_t nnz, double resolution) {
  if (N < 0 || nnz < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (!(resolution >= 0.0) || !std::isfinite(resolution)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "resolution = %g: must be finite and not negative", resolution);
  if (N > INT32_MAX - 1) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 2 vertices");
  return GFICF_OK;
}

// Q of the canonical labels in w.comm, their count, and the numbering by size (ties: the smaller canonical label = the first vertex)
int ld_finish(LdRun& R, int32_t* d_labels, int64_t* nc, double* q) {
  LdWs& w = R.w;
  u64 h[LD_S_N];
  GFICF_RC(ld_accum(R, R.g0, w.comm));
  GFICF_RC(ld_quality(R, R.g0, w.comm, w.K, q, h));
  hipLaunchKernelGGL(k_ld_flag_size, dim3(gficf_grid_capped(R.N + 1, 256, 1u << 30)), dim3(256), 0, R.st(), R.N, (const int32_t*)w.size, w.flag);
  GFICF_RC(ld_scan_count(R, w.flag, R.N, nc));
  if (d_labels) GFICF_RC(gficf_comm_number_by_size(R.ctx, R.N, R.N, w.size, w.comm, w.sort, w.rank, d_labels));      // every label in [0, N): the unused ones sort last
  GFICF_HIP_CHECK(hipStreamSynchronize(R.st()));
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

}  // namespace

#endif  // GFICF_LEIDEN_KERNELS_H

