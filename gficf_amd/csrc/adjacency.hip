// adjacency.hip — the Jaccard edge list as the symmetric weighted adjacency matrix (second half of "next" row N1).
//
// What clustcells() builds from the kept edges before community detection,
//   g <- igraph::graph.data.frame(relations, directed = FALSE)                       (reference R/clustCells.R:69)
//   igraph::as_adjacency_matrix(g, attr = "weight", sparse = T)                       (reference R/clustCells.R:80,86)
// i.e. A[i,j] = A[j,i] = sum of the weights of all edges between i and j (an i -> j and a j -> i edge are two
// edges of the undirected multigraph, so a mutual pair carries 2w), as a sparse matrix with sorted indices — the
// input of RunModularityClustering (src/RModularityOptimizer.cpp).  igraph is third-party (unpinned); the
// restatement is "A = W + W^T over the directed edge list W, duplicates summed, a self edge counted once".
// Vertices are the cells 1..N in cell order (igraph orders vertices by first appearance in the edge list, which is
// the same whenever every cell keeps at least one edge).
//
// Device path (round 6, second form).  Row r of A = the edges r -> * (half W) and the edges * -> r (half W^T).  The edge kernel emits
// W grouped by source cell, so half W needs no ordering at all: the run of every source is found where it lies.  Only the transposed
// half is ordered, and only by its row: ONE stable radix sort of E 8-byte elements (destination << 32 | edge number; b = bits of N
// significant: 17 at 100 k cells, two passes of 9 and 8 bits) — through round 5 the build sorted 2 E 64-bit keys row << 32 | col with
// a library sort over seven passes, in this round's first form over five.  The passes are the library's own radix sort (radix_sort.hip, which
// the kNN layout and Louvain's final numbering share; no library sort is called).  A wave then merges the two halves of a row: ranks
// its <= 128 entries by (column, emission position) in LDS, sums the runs of one column in that order (the order the full stable sort
// gave) and writes the row; longer rows take a wave of their own (<= 512 entries) or a workgroup.
//   1. k_adj_edges    validate, element = destination << 32 | e, (source, weight) packed for the gather of step 4, run of every source
//   2. radix passes   E elements over b bits, stable: within one destination the edges stay in emission order
//   3. k_adj_bounds   first sorted position of every destination (binary search), k_adj_caps + scan: room of every row, long rows listed
//   4. k_adj_rows(_mid, _big)  the merge above, rows written compacted at the start of their room
//   5. scan of the final lengths -> indptr, k_adj_compact: rows to their final place
// An edge list that is NOT grouped by source (any caller-made list is allowed) takes one more sort of the same kind, by source.
// Round 6's first attempt without any sort (row buckets filled by atomics) was slower: a device-scope atomic per edge for the
// transposed half — profiles/r06_adjacency_row_buckets.txt.
#include <atomic>
#include <cstring>
#include <vector>

#include "common.h"

namespace {

typedef unsigned long long u64;
constexpr uint32_t ADJ_NONE = 0xFFFFFFFFu;
constexpr int ADJ_WAVE_ROW = 128;            // entries a wave orders by ranking (two a lane)
constexpr int ADJ_MID_ROW = 512;             // entries a wave of its own orders by ranking (eight a lane)
constexpr int ADJ_WG_ROW = 4096;             // entries a workgroup orders in LDS

struct AdjPk { uint32_t src; uint32_t pad; double w; };      // what the transposed half gathers per entry: one 16 B read

__device__ inline bool adj_edge(const double* __restrict__ from, const double* __restrict__ to, int64_t e, int64_t N, int64_t* i, int64_t* j) {
  const double fi = from[e], fj = to[e];
  if (!(fi >= 1.0 && fi <= (double)N && fj >= 1.0 && fj <= (double)N && fi == trunc(fi) && fj == trunc(fj))) return false;
  *i = (int64_t)fi - 1; *j = (int64_t)fj - 1;
  return true;
}

// One thread per edge slot.  tkey = destination (ADJ_NONE: slot unused, bad ids, or a self edge — counted once, in half W), tval = e.
// The run of every source: its head writes rbeg, its tail rend; a source with two heads means the list is not grouped (*not_grouped).
__global__ __launch_bounds__(256) void k_adj_edges(const double* __restrict__ from, const double* __restrict__ to, const double* __restrict__ w,
                                                   int64_t cap, const int64_t* __restrict__ n_edges_p, int64_t N, u64* __restrict__ tkv,
                                                   AdjPk* __restrict__ pk, int32_t* __restrict__ rbeg,
                                                   int32_t* __restrict__ rend, int32_t* __restrict__ nruns, uint32_t* __restrict__ not_grouped,
                                                   int promised, uint32_t* __restrict__ status) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cap) return;
  const int64_t n_edges = n_edges_p ? (*n_edges_p < cap ? *n_edges_p : cap) : cap;
  uint32_t kt = ADJ_NONE;
  if (e < n_edges) {
    int64_t i, j;
    if (adj_edge(from, to, e, N, &i, &j)) {
      if (i != j) kt = (uint32_t)j;
      AdjPk q; q.src = (uint32_t)i; q.pad = 0u; q.w = w[e];
      pk[e] = q;
    } else {
      atomicOr(status, GFICF_ST_BAD_ID);
    }
    const double f = from[e];                               // (the runs count every edge whose source is a cell, whatever its destination)
    if (f >= 1.0 && f <= (double)N && f == trunc(f)) {
      const int64_t s = (int64_t)f - 1;
      if (e > 0 && from[e - 1] > f) not_grouped[1] = 1u;    // sources not ascending
      if (e == 0 || from[e - 1] != f) {
        rbeg[s] = (int32_t)e;
        if (atomicAdd(&nruns[s], 1) > 0) {
          *not_grouped = 1u;
          if (promised) atomicOr(status, GFICF_ST_NOT_GROUPED);
        }
      }
      if (e == n_edges - 1 || from[e + 1] != f) rend[s] = (int32_t)(e + 1);
    }
  }
  tkv[e] = ((u64)kt << 32) | (u64)e;                       // key above, edge number below: one 8 B element through the sort
}

// the list is not grouped: key = source for the second sort
__global__ __launch_bounds__(256) void k_adj_source_keys(const double* __restrict__ from, const double* __restrict__ to, int64_t cap,
                                                         const int64_t* __restrict__ n_edges_p, int64_t N, u64* __restrict__ skv) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cap) return;
  const int64_t n_edges = n_edges_p ? (*n_edges_p < cap ? *n_edges_p : cap) : cap;
  int64_t i, j;
  skv[e] = ((u64)((e < n_edges && adj_edge(from, to, e, N, &i, &j)) ? (uint32_t)i : ADJ_NONE) << 32) | (u64)e;
}

// L[r] = first position of the sorted keys holding a key >= r, r = 0 .. N (unused slots sort last: L[N] = number of real keys)
__global__ __launch_bounds__(256) void k_adj_bounds(const uint32_t* __restrict__ keys, int64_t M, int64_t N, int32_t* __restrict__ L) {
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (r > N) return;
  int64_t lo = 0, hi = M;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)keys[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  L[r] = (int32_t)lo;
}

// room of row r = its entries before equal columns are summed; rows too long for a wave of k_adj_rows are listed here (one device atomic
// per workgroup and list: 10 % of the rows of a kNN graph of real data at k = 50 are, and an atomic per row on one address costs more than the build)
__global__ __launch_bounds__(256) void k_adj_caps(int64_t N, const int32_t* __restrict__ rbeg, const int32_t* __restrict__ rend,
                                                  const int32_t* __restrict__ tL, const uint32_t* __restrict__ broken,
                                                  int64_t* __restrict__ start, int64_t* __restrict__ len2, int32_t* __restrict__ mid,
                                                  int32_t* __restrict__ big, unsigned* __restrict__ n_listed) {
  __shared__ unsigned s_n[2], s_base[2];
  const int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (threadIdx.x < 2) s_n[threadIdx.x] = 0u;
  __syncthreads();
  int64_t c = 0;
  if (r < N && !(broken && *broken)) {                     // (a list promised grouped that is not: its runs mean nothing — empty rows, the status says why)
    const int nw = rend[r] - rbeg[r];
    c = (nw > 0 ? nw : 0) + (tL[r + 1] - tL[r]);
  }
  if (r <= N) start[r] = c;
  if (r == N) len2[N] = 0;                                 // (the final lengths are scanned in place: N + 1 values)
  const int cls = c > ADJ_MID_ROW ? 1 : c > ADJ_WAVE_ROW ? 0 : -1;
  unsigned my = 0;
  if (cls >= 0) my = atomicAdd(&s_n[cls], 1u);
  __syncthreads();
  if (threadIdx.x < 2 && s_n[threadIdx.x]) s_base[threadIdx.x] = atomicAdd(&n_listed[threadIdx.x], s_n[threadIdx.x]);
  __syncthreads();
  if (cls >= 0) (cls ? big : mid)[s_base[cls] + my] = (int32_t)r;
}

struct AdjIn {
  const double* to; const double* w; const AdjPk* pk;
  const int32_t* rbeg; const int32_t* rend;       // half W: positions [rbeg, rend) of row r — edge numbers, or positions in `se` when the list was sorted by source
  const uint32_t* se;                             // NULL: the list is grouped by source
  const int32_t* tL; const uint32_t* te;          // half W^T: positions [tL[r], tL[r + 1]) of the edge numbers ordered by destination
  const uint32_t* unsorted;                       // device flag: some source is smaller than the one before it (half W^T then is not ordered by column)
};

__device__ inline u64 adj_key(uint32_t col, uint32_t pos) { return ((u64)col << 32) | pos; }

// entry t of a row whose half W holds nw entries starting at rb and whose half W^T starts at tb: key = (column, emission position), weight
__device__ inline void adj_load(const AdjIn& I, int rb, int nw, int tb, int64_t t, u64* key, double* wv) {
  if (t < nw) {
    const uint32_t e = I.se ? I.se[rb + t] : (uint32_t)(rb + t);
    *key = adj_key((uint32_t)((int64_t)I.to[e] - 1), 2u * e);
    *wv = I.w[e];
  } else {
    const uint32_t e = I.te[tb + (t - nw)];
    const AdjPk q = I.pk[e];
    *key = adj_key(q.src, 2u * e + 1u);
    *wv = q.w;
  }
}


// lower bound in a sorted run of distinct keys
__device__ inline int adj_lower_bound(const u64* a, int n, u64 key) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// One wave, one row of at most 64 * EPL entries (EPL a lane).  Every lane ranks its entries against the whole row read from LDS
// (broadcast reads; the keys are distinct: the position is), writes them at their rank, then the heads of the runs of one column add
// their run up in order and the row goes to the start of its room, compacted.  Returns the row's final length.
template <int EPL, bool MERGE>
__device__ inline int adj_wave_row(const AdjIn& I, int64_t row, int64_t lo, int n, int lane, u64* key, u64* skey, double* sw,
                                   int32_t* __restrict__ bcol, double* __restrict__ bw) {
  const int rb = I.rbeg[row], tb = I.tL[row];
  const int nw = n - (I.tL[row + 1] - tb);
  const bool tsorted = MERGE && I.se == nullptr && *I.unsorted == 0u;
  u64 k[EPL];
  double w[EPL];
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    k[s] = ~0ull; w[s] = 0.0;
    if (s * 64 + lane < n) adj_load(I, rb, nw, tb, s * 64 + lane, &k[s], &w[s]);
    key[s * 64 + lane] = k[s];
  }
  GFICF_WAVE_SYNC();
  int r[EPL];
#pragma unroll
  for (int s = 0; s < EPL; ++s) r[s] = 0;
  if (tsorted) {
    // half W^T arrived ordered (ascending sources): an entry's rank = its rank inside its own half + the entries of the other half below it.
    // Against half W (at most k entries, unordered): counted; against half W^T: its index there, or one binary search.
    for (int t = 0; t < nw; ++t) {
      const u64 kt = key[t];
#pragma unroll
      for (int s = 0; s < EPL; ++s) r[s] += kt < k[s] ? 1 : 0;
    }
#pragma unroll
    for (int s = 0; s < EPL; ++s) {
      const int t = s * 64 + lane;
      if (t < nw) r[s] += adj_lower_bound(key + nw, n - nw, k[s]);
      else r[s] += t - nw;
    }
  } else {
    for (int t = 0; t < n; ++t) {
      const u64 kt = key[t];
#pragma unroll
      for (int s = 0; s < EPL; ++s) r[s] += kt < k[s] ? 1 : 0;
    }
  }
#pragma unroll
  for (int s = 0; s < EPL; ++s)
    if (s * 64 + lane < n) { skey[r[s]] = k[s]; sw[r[s]] = w[s]; }
  GFICF_WAVE_SYNC();
  // heads of the runs of one column, their output positions (ranks among the heads), their sums
  int out[EPL];
  int total = 0;
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    const int e = s * 64 + lane;
    const bool head = e < n && (e == 0 || (skey[e] >> 32) != (skey[e - 1] >> 32));
    const u64 m = __ballot(head);
    out[s] = head ? total + __popcll(m & ((1ull << lane) - 1ull)) : -1;
    total += __popcll(m);
  }
#pragma unroll
  for (int s = 0; s < EPL; ++s) {
    const int e = s * 64 + lane;
    if (out[s] < 0) continue;
    const u64 c = skey[e] >> 32;
    double sum = sw[e];
    for (int t = e + 1; t < n && (skey[t] >> 32) == c; ++t) sum += sw[t];
    bcol[lo + out[s]] = (int32_t)c; bw[lo + out[s]] = sum;
  }
  GFICF_WAVE_SYNC();                                            // (the next row's loads overwrite key / skey / sw)
  return total;
}

// One wave per row of at most ADJ_WAVE_ROW entries; longer rows: up to ADJ_MID_ROW k_adj_rows_mid, beyond the workgroup kernel.
// len2[row] = the row's final length.
__global__ __launch_bounds__(256) void k_adj_rows(const AdjIn I, int64_t N, const int64_t* __restrict__ start, int32_t* __restrict__ bcol,
                                                  double* __restrict__ bw, int64_t* __restrict__ len2) {
  __shared__ u64 s_key[4][ADJ_WAVE_ROW];
  __shared__ u64 s_skey[4][ADJ_WAVE_ROW];
  __shared__ double s_sw[4][ADJ_WAVE_ROW];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N; row += (int64_t)gridDim.x * 4) {
    const int64_t lo = start[row];
    const int64_t n64 = start[row + 1] - lo;
    if (n64 > ADJ_WAVE_ROW) continue;                        // listed by k_adj_caps for k_adj_rows_mid / k_adj_rows_big
    const int n = (int)n64;
    const int total = n > 0 ? adj_wave_row<ADJ_WAVE_ROW / 64, true>(I, row, lo, n, lane, s_key[wave], s_skey[wave], s_sw[wave], bcol, bw) : 0;
    if (lane == 0) len2[row] = total;
  }
}

// One wave (a workgroup of its own: 12 KB of LDS) per listed row of ADJ_WAVE_ROW + 1 .. ADJ_MID_ROW entries — the tail of the in-degrees of
// a kNN graph of real data (10 % of the rows at k = 50, 40 % at k = 100): the same ranking, eight entries a lane.
__global__ __launch_bounds__(64) void k_adj_rows_mid(const AdjIn I, const int64_t* __restrict__ start, const int32_t* __restrict__ mid,
                                                     const unsigned* __restrict__ n_listed, int32_t* __restrict__ bcol, double* __restrict__ bw,
                                                     int64_t* __restrict__ len2) {
  __shared__ u64 s_key[ADJ_MID_ROW];
  __shared__ u64 s_skey[ADJ_MID_ROW];
  __shared__ double s_sw[ADJ_MID_ROW];
  const int lane = threadIdx.x;
  for (unsigned item = blockIdx.x; item < n_listed[0]; item += gridDim.x) {
    const int64_t row = mid[item], lo = start[row];
    const int n = (int)(start[row + 1] - lo);
    const int total = n <= 256 ? adj_wave_row<4, true>(I, row, lo, n, lane, s_key, s_skey, s_sw, bcol, bw)
                               : adj_wave_row<ADJ_MID_ROW / 64, true>(I, row, lo, n, lane, s_key, s_skey, s_sw, bcol, bw);
    if (lane == 0) len2[row] = total;
  }
}

// bitonic network over n2 (a power of two) elements held in arrays k / w
__device__ inline void adj_bitonic(u64* k, double* w, int64_t n2, int tid, int nthreads) {
  for (int64_t size = 2; size <= n2; size <<= 1)
    for (int64_t stride = size >> 1; stride > 0; stride >>= 1) {
      for (int64_t t = tid; t < n2 / 2; t += nthreads) {
        const int64_t lo = (t / stride) * 2 * stride + (t % stride), hi = lo + stride;
        const bool up = (lo & size) == 0;
        const u64 a = k[lo], b = k[hi];
        if ((a > b) == up) { k[lo] = b; k[hi] = a; const double x = w[lo]; w[lo] = w[hi]; w[hi] = x; }
      }
      __syncthreads();
    }
}

// One workgroup per listed row (more than ADJ_WAVE_ROW entries; at k = 50 a kNN graph of real data has thousands: in-degrees have a tail).
// Sources in ascending order (what the edge build writes unless the cells were renumbered): the transposed half arrives ordered by
// column already — the stable sort kept the emission order —, so only half W (at most k entries) is ordered, by a bitonic network in LDS,
// and the two halves are MERGED: every entry finds its place by one binary search in the other half.  Otherwise, or beyond what LDS
// holds that way: the whole row through the bitonic network (LDS up to ADJ_WG_ROW entries, global scratch gk / gw beyond — a row of that
// length is a hub of a degenerate graph: correct, not fast).
__global__ __launch_bounds__(256) void k_adj_rows_big(const AdjIn I, const int64_t* __restrict__ start, const int32_t* __restrict__ big,
                                                      const unsigned* __restrict__ n_big, int32_t* __restrict__ bcol, double* __restrict__ bw,
                                                      int64_t* __restrict__ len2, u64* __restrict__ gk, double* __restrict__ gw) {
  extern __shared__ unsigned char s_raw[];
  u64* sk = (u64*)s_raw;
  double* sw = (double*)(sk + ADJ_WG_ROW);
  __shared__ int s_total;
  __shared__ int s_cnt[256];
  const int tid = threadIdx.x;
  const bool merge_ok = I.se == nullptr && *I.unsorted == 0u;
  for (unsigned item = blockIdx.x; item < *n_big; item += gridDim.x) {
    const int64_t row = big[item], lo = start[row], n = start[row + 1] - lo;
    const int rb = I.rbeg[row], tb = I.tL[row];
    const int nw = (int)(n - (I.tL[row + 1] - tb));
    u64* k;
    double* w;
    int64_t nw2 = 1;
    while (nw2 < nw) nw2 <<= 1;
    if (merge_ok && nw2 + (n - nw) + n <= ADJ_WG_ROW) {
      const int nt = (int)(n - nw);
      u64* const tk = sk + nw2; double* const tw = sw + nw2;       // LDS: [half W, padded to nw2][half W^T][the merged row]
      for (int t = tid; t < (int)nw2; t += 256) {
        u64 kk = ~0ull; double ww = 0.0;
        if (t < nw) adj_load(I, rb, nw, tb, t, &kk, &ww);
        sk[t] = kk; sw[t] = ww;
      }
      for (int t = tid; t < nt; t += 256) adj_load(I, rb, nw, tb, nw + t, &tk[t], &tw[t]);
      __syncthreads();
      adj_bitonic(sk, sw, nw2, tid, 256);
      k = tk + nt; w = tw + nt;
      for (int t = tid; t < nt; t += 256) { const int at = t + adj_lower_bound(sk, nw, tk[t]); k[at] = tk[t]; w[at] = tw[t]; }
      for (int t = tid; t < nw; t += 256) { const int at = t + adj_lower_bound(tk, nt, sk[t]); k[at] = sk[t]; w[at] = sw[t]; }
      __syncthreads();
    } else {
      int64_t n2 = 1;
      while (n2 < n) n2 <<= 1;
      // a row too long for LDS is ordered in global scratch: n2 < 2 n entries at twice its room's start (the scratch arrays are twice the rooms)
      k = n2 <= ADJ_WG_ROW ? sk : gk + 2 * lo;
      w = n2 <= ADJ_WG_ROW ? sw : gw + 2 * lo;
      for (int64_t t = tid; t < n2; t += 256) {
        u64 kk = ~0ull; double ww = 0.0;
        if (t < n) adj_load(I, rb, nw, tb, t, &kk, &ww);
        k[t] = kk; w[t] = ww;
      }
      __syncthreads();
      adj_bitonic(k, w, n2, tid, 256);
    }
    if (tid == 0) s_total = 0;
    __syncthreads();
    // the heads of the runs of one column: every thread takes a contiguous slice, the slices' bases by a serial pass over 256 counts
    const int64_t per = (n + 255) / 256, t0 = (int64_t)tid * per, t1 = t0 + per < n ? t0 + per : n;
    int mine = 0;
    for (int64_t t = t0; t < t1; ++t) mine += (t == 0 || (k[t] >> 32) != (k[t - 1] >> 32)) ? 1 : 0;
    s_cnt[tid] = mine;
    __syncthreads();
    if (tid == 0) { int run = 0; for (int t = 0; t < 256; ++t) { const int c = s_cnt[t]; s_cnt[t] = run; run += c; } s_total = run; }
    __syncthreads();
    int at = s_cnt[tid];
    for (int64_t t = t0; t < t1; ++t) {
      if (!(t == 0 || (k[t] >> 32) != (k[t - 1] >> 32))) continue;
      const u64 c = k[t] >> 32;
      double sum = w[t];
      for (int64_t q = t + 1; q < n && (k[q] >> 32) == c; ++q) sum += w[q];
      bcol[lo + at] = (int32_t)c; bw[lo + at] = sum;
      ++at;
    }
    if (tid == 0) len2[row] = s_total;
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_adj_compact(int64_t N, const int64_t* __restrict__ start, const int64_t* __restrict__ indptr,
                                                     const int32_t* __restrict__ bcol, const double* __restrict__ bw,
                                                     int32_t* __restrict__ indices, double* __restrict__ x) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t row = (int64_t)blockIdx.x * 4 + wave; row < N; row += (int64_t)gridDim.x * 4) {
    const int64_t src = start[row], dst = indptr[row], n = indptr[row + 1] - dst;
    for (int64_t t = lane; t < n; t += 64) { indices[dst + t] = bcol[src + t]; x[dst + t] = bw[src + t]; }
  }
}

struct AdjWs {
  u64 *kv0, *kv1;                                       // cap each: the elements of the sort, ping and pong
  int64_t* hist;                                        // [digit][workgroup] counts of a pass
  uint32_t *tkey, *te, *skey, *se;                      // cap each
  AdjPk* pk;                                            // cap
  int32_t *rbeg, *rend, *nruns;                         // N
  int32_t *tL, *sL;                                     // N + 2
  uint32_t* flag;                                       // not_grouped, sources not ascending, rows listed as mid, as big
  int64_t* start;                                       // N + 1: start of every row's room
  int32_t* bcol; double* bw;                            // 2 cap each: the rooms
  int32_t *mid, *big;                                   // N each: the listed rows
  u64* gk; double* gw;                                  // 4 cap each: scratch of rows too long for LDS
};

size_t adj_carve(AdjWs* w, void* base, int64_t N, int64_t cap) {
  const size_t n = (size_t)(N > 0 ? N : 1), c = (size_t)(cap > 0 ? cap : 1), m = 2 * c;
  gficf_carver cv{(char*)base};
  AdjWs d;
  d.kv0 = cv.take<u64>(c); d.kv1 = cv.take<u64>(c);
  d.hist = cv.take<int64_t>(gficf_radix_sort_hist_len((int64_t)c, gficf_bit_width(N)));
  d.tkey = cv.take<uint32_t>(c); d.te = cv.take<uint32_t>(c);
  d.skey = cv.take<uint32_t>(c); d.se = cv.take<uint32_t>(c);
  d.pk = cv.take<AdjPk>(c);
  d.rbeg = cv.take<int32_t>(3 * n + 4); d.rend = d.rbeg + n; d.nruns = d.rend + n; d.flag = (uint32_t*)(d.nruns + n);   // one memset
  d.tL = cv.take<int32_t>(n + 2); d.sL = cv.take<int32_t>(n + 2);
  d.start = cv.take<int64_t>(n + 1);
  d.bcol = cv.take<int32_t>(m);
  d.bw = cv.take<double>(m);
  d.mid = cv.take<int32_t>(n);
  d.big = cv.take<int32_t>(n);
  d.gk = cv.take<u64>(2 * m);
  d.gw = cv.take<double>(2 * m);
  if (w) *w = d;
  return cv.total();
}

}  // namespace

extern "C" {

size_t gficf_adjacency_workspace_bytes(int64_t N, int64_t edge_capacity) {
  if (N <= 0 || edge_capacity <= 0) return 256;
  return adj_carve(nullptr, nullptr, N, edge_capacity);
}

int gficf_adjacency_device(gficf_ctx* ctx, int64_t N, int64_t edge_capacity, const int64_t* d_n_edges, const double* d_from,
                           const double* d_to, const double* d_weight, int grouped_by_source, void* d_ws, size_t ws_bytes,
                           int64_t* d_indptr, int32_t* d_indices, double* d_x) {
  GFICF_CTX_ENTER(ctx);
  if (N < 0 || edge_capacity < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (N > 0x7FFFFFFFll) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "N = %lld exceeds int32 ids", (long long)N);
  if (edge_capacity > 0x3FFFFFFFll) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^30 edges");
  if (!d_indptr) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (N == 0 || edge_capacity == 0) {
    GFICF_HIP_CHECK(hipMemsetAsync(d_indptr, 0, sizeof(int64_t) * (size_t)(N + 1), ctx->stream));
    return GFICF_OK;
  }
  if (!d_from || !d_to || !d_weight || !d_ws || !d_indices || !d_x) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  if (ws_bytes < gficf_adjacency_workspace_bytes(N, edge_capacity)) GFICF_FAIL(GFICF_ERR_CAPACITY, "adjacency workspace too small");
  static std::atomic<bool> attr_set[64];
  if (!attr_set[ctx->device & 63]) {
    GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_adj_rows_big, hipFuncAttributeMaxDynamicSharedMemorySize, ADJ_WG_ROW * 16));
    attr_set[ctx->device & 63] = true;
  }
  AdjWs w;
  adj_carve(&w, d_ws, N, edge_capacity);
  hipStream_t st = ctx->stream;
  const int b = gficf_bit_width(N);      // 2^b > N: an id in [0, N) never has all of its b bits set, so ADJ_NONE sorts behind every real key
  const unsigned ge = (unsigned)gficf_ceil_div(edge_capacity, 256), gn = (unsigned)gficf_ceil_div(N + 1, 256);
  const unsigned gr = (unsigned)(gficf_ceil_div(N, 4) < 4096 ? gficf_ceil_div(N, 4) : 4096);
  GFICF_HIP_CHECK(hipMemsetAsync(w.rbeg, 0, sizeof(int32_t) * (3 * (size_t)N + 4), st));     // runs of the sources + the three flags behind them
  hipLaunchKernelGGL(k_adj_edges, dim3(ge), dim3(256), 0, st, d_from, d_to, d_weight, edge_capacity, d_n_edges, N, w.kv0, w.pk, w.rbeg,
                     w.rend, w.nruns, w.flag, grouped_by_source != 0 ? 1 : 0, ctx->d_status);
  GFICF_HIP_CHECK(hipGetLastError());
  int rc = gficf_radix_sort_kv(ctx, w.kv0, w.kv1, w.hist, edge_capacity, b, w.tkey, w.te);
  if (rc) return rc;
  hipLaunchKernelGGL(k_adj_bounds, dim3(gn), dim3(256), 0, st, (const uint32_t*)w.tkey, edge_capacity, N, w.tL);
  AdjIn in;
  in.to = d_to; in.w = d_weight; in.pk = w.pk; in.rbeg = w.rbeg; in.rend = w.rend; in.se = nullptr; in.tL = w.tL; in.te = w.te; in.unsorted = w.flag + 1;
  bool grouped = grouped_by_source != 0;
  if (!grouped) {                                   // the caller does not know: ask the pass that just looked at every edge
    uint32_t ng = 0;
    GFICF_HIP_CHECK(hipMemcpyAsync(&ng, w.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    GFICF_HIP_CHECK(hipStreamSynchronize(st));
    grouped = ng == 0;
  }
  if (!grouped) {
    hipLaunchKernelGGL(k_adj_source_keys, dim3(ge), dim3(256), 0, st, d_from, d_to, edge_capacity, d_n_edges, N, w.kv0);
    GFICF_HIP_CHECK(hipGetLastError());
    rc = gficf_radix_sort_kv(ctx, w.kv0, w.kv1, w.hist, edge_capacity, b, w.skey, w.se);
    if (rc) return rc;
    hipLaunchKernelGGL(k_adj_bounds, dim3(gn), dim3(256), 0, st, (const uint32_t*)w.skey, edge_capacity, N, w.sL);
    in.rbeg = w.sL; in.rend = w.sL + 1; in.se = w.se;
  }
  hipLaunchKernelGGL(k_adj_caps, dim3(gn), dim3(256), 0, st, N, in.rbeg, in.rend, (const int32_t*)w.tL, in.se ? (const uint32_t*)nullptr : (const uint32_t*)w.flag,
                     w.start, d_indptr, w.mid, w.big, w.flag + 2);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = gficf_exclusive_scan_i64(ctx, w.start, N + 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k_adj_rows, dim3(gr), dim3(256), 0, st, in, N, (const int64_t*)w.start, w.bcol, w.bw, d_indptr);
  hipLaunchKernelGGL(k_adj_rows_mid, dim3(3328), dim3(64), 0, st, in, (const int64_t*)w.start, (const int32_t*)w.mid, (const unsigned*)(w.flag + 2),
                     w.bcol, w.bw, d_indptr);
  hipLaunchKernelGGL(k_adj_rows_big, dim3(1024), dim3(256), ADJ_WG_ROW * 16, st, in, (const int64_t*)w.start, (const int32_t*)w.big,
                     (const unsigned*)(w.flag + 3), w.bcol, w.bw, d_indptr, w.gk, w.gw);
  rc = gficf_exclusive_scan_i64(ctx, d_indptr, N + 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k_adj_compact, dim3(gr), dim3(256), 0, st, N, (const int64_t*)w.start, (const int64_t*)d_indptr, (const int32_t*)w.bcol,
                     (const double*)w.bw, d_indices, d_x);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

}  // extern "C"

// ------------------------------------------------------------------- host form (R glue)
struct gficf_adj_plan {
  int64_t N = 0, nnz = 0;
  int64_t* d_indptr = nullptr;
  int32_t* d_indices = nullptr;
  double* d_x = nullptr;
};

void gficf_adj_plan_free(gficf_ctx* ctx) {        // the buffers are pieces of GFICF_SLOT_ADJ_PLAN: nothing to release
  delete ctx->adj_plan;
  ctx->adj_plan = nullptr;
}

extern "C" {

int gficf_adjacency_host_plan(gficf_ctx* ctx, int64_t N, int64_t n_edges, const double* from, const double* to,
                              const double* weight, int64_t* nnz) {
  GFICF_CTX_ENTER(ctx);
  if (N < 0 || n_edges < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "negative size");
  if (!nnz) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "nnz is NULL");
  if (n_edges > 0 && (!from || !to || !weight)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL host pointer");
  gficf_adj_plan_free(ctx);
  gficf_adj_plan* p = new gficf_adj_plan();
  ctx->adj_plan = p;
  p->N = N;
  *nnz = 0;
  const size_t eb = sizeof(double) * (size_t)(n_edges > 0 ? n_edges : 1), cap = (size_t)(n_edges > 0 ? 2 * n_edges : 1);
  const size_t wsb = gficf_adjacency_workspace_bytes(N, n_edges);
  void *d_e = nullptr, *d_ws = nullptr;
  gficf_host_io io{ctx, "gficf_adjacency_host_plan"};
  io.get(GFICF_SLOT_STAGE0, 3 * eb, &d_e);
  io.get(GFICF_SLOT_STAGE1, wsb, &d_ws);
  gficf_carver cv;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    p->d_indptr = cv.take<int64_t>((size_t)(N + 1)); p->d_indices = cv.take<int32_t>(cap); p->d_x = cv.take<double>(cap);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_ADJ_PLAN);
  }
  double* d_from = (double*)d_e;
  double* d_to = d_from + (n_edges > 0 ? n_edges : 1);
  double* d_w = d_to + (n_edges > 0 ? n_edges : 1);
  io.up(d_from, from, sizeof(double) * (size_t)n_edges);
  io.up(d_to, to, sizeof(double) * (size_t)n_edges);
  io.up(d_w, weight, sizeof(double) * (size_t)n_edges);
  int rc = GFICF_OK;
  int64_t total = 0;
  if (io.ok()) {
    rc = gficf_adjacency_device(ctx, N, n_edges, nullptr, d_from, d_to, d_w, 0, d_ws, wsb, p->d_indptr, p->d_indices, p->d_x);
    if (!rc) io.down(&total, p->d_indptr + N, sizeof(int64_t));
  }
  rc = io.finish(rc);
  if (rc) { gficf_adj_plan_free(ctx); return rc; }
  p->nnz = total;
  *nnz = total;
  return GFICF_OK;
}

int gficf_adjacency_host_finish(gficf_ctx* ctx, void* indptr, int indptr_is_i64, int32_t* indices, double* x) {
  GFICF_CTX_ENTER(ctx);
  gficf_adj_plan* p = ctx->adj_plan;
  if (!p) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "gficf_adjacency_host_finish without a plan");
  if (!indptr || (p->nnz > 0 && (!indices || !x))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL output pointer");
  std::vector<int64_t> ip((size_t)p->N + 1);
  if (p->nnz > 0 && indices && x) {               // (fresh result vectors of the caller: huge pages + parallel first touch)
    gficf_prefault(indices, sizeof(int32_t) * (size_t)p->nnz);
    gficf_prefault(x, sizeof(double) * (size_t)p->nnz);
  }
  gficf_host_io io{ctx, "gficf_adjacency_host_finish"};
  io.down(ip.data(), p->d_indptr, sizeof(int64_t) * ip.size());
  io.down(indices, p->d_indices, sizeof(int32_t) * (size_t)p->nnz);
  io.down(x, p->d_x, sizeof(double) * (size_t)p->nnz);
  const int rc = io.drain(GFICF_OK);
  if (!rc) {
    if (indptr_is_i64) std::memcpy(indptr, ip.data(), sizeof(int64_t) * ip.size());
    else for (size_t c = 0; c < ip.size(); ++c) ((int32_t*)indptr)[c] = (int32_t)ip[c];
  }
  gficf_adj_plan_free(ctx);
  return rc;
}

}  // extern "C"
