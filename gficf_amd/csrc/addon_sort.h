// addon_sort.h — the stable sort of doubles, within groups, that markers.hip, gsea.hip, gsva.hip and hvg.hip share: three passes
// of the core's 32-bit gficf_radix_sort_kv over the 64-bit key of block_ops.h (its low half, its high half, then the group).
// Header-only; apart from block_ops.h because its two kernels are emitted into every object that includes it, so only the
// files that sort do.
#pragma once

#include <initializer_list>

#include "block_ops.h"

namespace {

// the buffers of one sort, out of a caller's workspace
struct gficf_sort_bufs {
  gficf_u64 *key, *kv0, *kv1;                              // the 64-bit keys as they lie; the elements of a pass, in and out
  int64_t* hist;
  uint32_t *okey, *oval;                                   // the last pass's keys and the order
  // n: the most elements any sort through these buffers has, n_key of them with a 64-bit key; group_bits: the widths of
  // every pass that is not 32 bits wide (the histogram is as long as the longest of them asks for)
  void take(gficf_carver& cv, size_t n_key, size_t n, std::initializer_list<int> group_bits) {
    key = cv.take<gficf_u64>(n_key);
    kv0 = cv.take<gficf_u64>(n + 1);
    kv1 = cv.take<gficf_u64>(n + 1);
    int64_t h = gficf_radix_sort_hist_len((int64_t)n, 32);
    for (const int b : group_bits) {
      const int64_t hb = gficf_radix_sort_hist_len((int64_t)n, b);
      h = hb > h ? hb : h;
    }
    hist = cv.take<int64_t>((size_t)h);
    okey = cv.take<uint32_t>(n);
    oval = cv.take<uint32_t>(n);
  }
};

// First pass: key[p] of every v[p], and the element key << 32 | p (the key's low 32 bits).  desc: the order descends.
// Each of the three may be NULL.  mask: an entry with mask[p] == 0 gets the key ~0, behind every double, and is looked at no
// further.  status: st_bit is raised by a value that is not finite.  count: the entries that are not masked out.
__global__ __launch_bounds__(256) void k_sort_keys(int64_t n, const double* __restrict__ v, int desc, const int32_t* __restrict__ mask,
                                                   uint32_t* __restrict__ status, uint32_t st_bit, int32_t* __restrict__ count,
                                                   gficf_u64* __restrict__ key, gficf_u64* __restrict__ kv) {
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < n; p += (int64_t)gridDim.x * 256) {
    gficf_u64 k = ~0ull;
    if (mask == nullptr || mask[p] != 0) {
      const double x = v[p];
      if (status != nullptr && !isfinite(x)) atomicOr(status, st_bit);
      k = desc ? ~gficf_f64_key(x) : gficf_f64_key(x);
      if (count != nullptr) atomicAdd(count, 1);
    }
    key[p] = k;
    kv[p] = (k << 32) | (gficf_u64)p;
  }
}

// Next pass: the element hi << 32 | p for every p = perm[i], in the order of the previous pass.  PART 0: hi is the high 32 bits
// of key[p].  PART 1: hi is the group of p, group[p], or p / G where group is NULL.
template <int PART>
__global__ __launch_bounds__(256) void k_sort_next(int64_t n, const uint32_t* __restrict__ perm, const gficf_u64* __restrict__ key,
                                                   const uint32_t* __restrict__ group, uint32_t G, gficf_u64* __restrict__ kv) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint32_t p = perm[i];
    const gficf_u64 hi = PART == 0 ? (key[p] >> 32) : (gficf_u64)(group != nullptr ? group[p] : p / G);
    kv[i] = (hi << 32) | (gficf_u64)p;
  }
}

// what is sorted and how: k_sort_keys' arguments, then the group of entry p (group[p], or p / G where group is NULL) and its
// width in bits; group_bits == 0: no groups, two passes
struct gficf_sort_args {
  const double* v;
  int desc;
  const int32_t* mask;
  uint32_t* status;
  uint32_t st_bit;
  int32_t* count;
  const uint32_t* group;
  uint32_t G;
  int group_bits;
};

// s.oval = the positions 0 .. n - 1 ordered by (group, key, position); s.okey = the groups in that order (without groups:
// the keys' high halves); s.key = the keys as they lie.  Everything is enqueued on the context's stream.
inline int gficf_sort_f64(gficf_ctx* ctx, const gficf_sort_bufs& s, int64_t n, const gficf_sort_args& a) {
  hipStream_t st = ctx->stream;
  const dim3 grid(gficf_grid_1d(n)), blk(256);
  hipLaunchKernelGGL(k_sort_keys, grid, blk, 0, st, n, a.v, a.desc, a.mask, a.status, a.st_bit, a.count, s.key, s.kv0);
  GFICF_HIP_CHECK(hipGetLastError());
  int rc = gficf_radix_sort_kv(ctx, s.kv0, s.kv1, s.hist, n, 32, s.okey, s.oval);                    // low 32 bits of the key
  if (rc) return rc;
  hipLaunchKernelGGL(k_sort_next<0>, grid, blk, 0, st, n, (const uint32_t*)s.oval, (const gficf_u64*)s.key, (const uint32_t*)nullptr, 0u, s.kv0);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = gficf_radix_sort_kv(ctx, s.kv0, s.kv1, s.hist, n, 32, s.okey, s.oval);                        // high 32 bits
  if (rc || a.group_bits == 0) return rc;
  hipLaunchKernelGGL(k_sort_next<1>, grid, blk, 0, st, n, (const uint32_t*)s.oval, (const gficf_u64*)nullptr, a.group, a.G, s.kv0);
  GFICF_HIP_CHECK(hipGetLastError());
  return gficf_radix_sort_kv(ctx, s.kv0, s.kv1, s.hist, n, a.group_bits, s.okey, s.oval);            // the group, stably
}

}  // namespace
