// community_ops.h — what louvain.hip and leiden.hip share: the 2^-32 fixed-point scale, the hash of a label, the LDS table that
// sums a vertex's entries per neighbouring community, the numbering of clusters by decreasing size, a fill and an iota.
// Header-only, like block_ops.h and addon_sort.h: libgficf_leiden.so asks of libgficf_hip.so only what its C ABI and common.h
// give (the radix sort), so the kernels here are emitted into each of the two objects.
#pragma once

#include "block_ops.h"

namespace {

constexpr double GFICF_COMM_SCALE = 4294967296.0;      // 2^32: weights are integers in 2^-32 fixed point, so every sum commutes

__device__ __host__ inline uint32_t gficf_comm_hash(uint32_t v) {
  v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16;
  return v;
}

// Claims or finds community c's slot in a table of SLOTS (a power of two; empty keys are -1, empty sums 0) and adds w.
// *own: this thread claimed the slot — exactly one of the threads that bring c does.  Returns the slot, or -1 when the table is
// full (nothing is written then; the caller reports it).
template <int SLOTS>
__device__ inline int gficf_comm_insert(int32_t* key, gficf_u64* val, int32_t c, gficf_u64 w, bool* own) {
  uint32_t h = gficf_comm_hash((uint32_t)c) & (SLOTS - 1);
  *own = false;
  for (int probes = 0; probes < SLOTS; ++probes) {
    const int32_t old = atomicCAS(&key[h], -1, c);
    if (old == -1 || old == c) { *own = old == -1; atomicAdd(&val[h], w); return (int)h; }
    h = (h + 1) & (SLOTS - 1);
  }
  return -1;
}

template <typename T>
__global__ __launch_bounds__(256) void k_comm_fill(int64_t n, T v, T* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = v;
}

__global__ __launch_bounds__(256) void k_comm_iota(int64_t n, int32_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) out[v] = (int32_t)v;
}

// ---- final numbering: clusters by decreasing size, ties by id (Clustering::orderClustersByNNodes, reference :132-158)
// sort element of label c: (n - its size) << 32 | c; sorted stably by the key, the labels come out by decreasing size, ties by
// id, a label nobody carries last
__global__ __launch_bounds__(256) void k_comm_size_keys(int64_t C, int64_t n, const int32_t* __restrict__ cnt, gficf_u64* __restrict__ kv) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < C) kv[c] = ((gficf_u64)(n - cnt[c]) << 32) | (gficf_u64)c;
}

__global__ __launch_bounds__(256) void k_comm_rank(int64_t C, const uint32_t* __restrict__ sorted_ids, int32_t* __restrict__ rank) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p < C) rank[sorted_ids[p]] = (int32_t)p;
}

__global__ __launch_bounds__(256) void k_comm_final(int64_t n, const int32_t* __restrict__ lab, const int32_t* __restrict__ rank,
                                                    int32_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v < n) out[v] = rank[lab[v]];
}

// the buffers of the numbering, out of a caller's workspace: the sort's elements in and out and its output (n = max(N, 1) entries
// each), its histogram
struct gficf_comm_sort_bufs {
  gficf_u64* kv[2]; int64_t* hist; uint32_t *key, *id;
  void take(gficf_carver& cv, size_t n, int64_t N) {
    kv[0] = cv.take<gficf_u64>(n); kv[1] = cv.take<gficf_u64>(n); key = cv.take<uint32_t>(n); id = cv.take<uint32_t>(n);
    hist = cv.take<int64_t>((size_t)gficf_radix_sort_hist_len((int64_t)n, gficf_bit_width(N)));
  }
};

// out[v] = the rank of lab[v] among the labels [0, C) by decreasing cnt (members among the N vertices), ties by id; rank[c] = that
// rank.  Enqueued on the context's stream, nothing is waited for.
inline int gficf_comm_number_by_size(gficf_ctx* ctx, int64_t C, int64_t N, const int32_t* cnt, const int32_t* lab, const gficf_comm_sort_bufs& s,
                                     int32_t* rank, int32_t* out) {
  hipStream_t st = ctx->stream;
  const dim3 gC(gficf_grid_capped(C, 256, 1u << 30)), gN(gficf_grid_capped(N, 256, 1u << 30)), blk(256);
  hipLaunchKernelGGL(k_comm_size_keys, gC, blk, 0, st, C, N, cnt, s.kv[0]);
  GFICF_RC(gficf_radix_sort_kv(ctx, s.kv[0], s.kv[1], s.hist, C, gficf_bit_width(N), s.key, s.id));      // keys in [0, N]
  hipLaunchKernelGGL(k_comm_rank, gC, blk, 0, st, C, (const uint32_t*)s.id, rank);
  hipLaunchKernelGGL(k_comm_final, gN, blk, 0, st, N, lab, (const int32_t*)rank, out);
  return GFICF_OK;
}

}  // namespace
