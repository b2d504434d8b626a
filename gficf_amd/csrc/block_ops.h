// block_ops.h — the device inlines the statistics add-ons (markers, gsea, gsva, tmm, hvg) and tsne, leiden share: wave and
// workgroup reductions, the LDS sort, the search and the sort key of a double; and the capped 1-D grid of their launches (and,
// through community_ops.h, of louvain.hip's).
// Inlines only, no kernel: including it emits nothing (the kernels of the 64-bit-key sort are in addon_sort.h).  Every
// workgroup function is for 256 threads and is reached by all of them.
#pragma once

#include "common.h"

typedef unsigned long long gficf_u64;

// the sum over the 64 lanes of a wave, in every lane
template <typename T>
__device__ inline T gficf_wave_sum(T v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// The folded sum: v is thread t's value, s 256 doubles of LDS; t is added to t + 128, + 64, ... + 1, the same tree whatever the
// values, and every thread gets the total.  The leading barrier makes a second call on the same s safe.
__device__ inline double gficf_block_sum_f64(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();                                         // the previous fold has been read
  s[t] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) s[t] += s[t + h];
    __syncthreads();
  }
  return s[0];
}

__device__ inline double gficf_block_max_f64(double v, double* s) {
  const int t = threadIdx.x;
  __syncthreads();
  s[t] = v;
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h) s[t] = fmax(s[t], s[t + h]);
    __syncthreads();
  }
  return s[0];
}

// ascending bitonic sort of the np2 (a power of two) keys of a[] by the whole workgroup
__device__ inline void gficf_lds_sort_u64(gficf_u64* a, int np2) {
  for (int k = 2; k <= np2; k <<= 1) {
    for (int h = k >> 1; h > 0; h >>= 1) {
      for (int i = threadIdx.x; i < np2; i += 256) {
        const int l = i ^ h;
        if (l > i) {
          const gficf_u64 a0 = a[i], a1 = a[l];
          if ((a0 > a1) == ((i & k) == 0)) { a[i] = a1; a[l] = a0; }
        }
      }
      __syncthreads();
    }
  }
}

// the first index of the ascending a[0 .. n) with a[i] >= v
template <typename T, typename I>
__device__ inline I gficf_lower_bound(const T* a, I n, T v) {
  I lo = 0, hi = n;
  while (lo < hi) {
    const I mid = (lo + hi) >> 1;
    if (a[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the order-preserving key of a double: a < b exactly where key(a) < key(b), -0.0 with +0.0; ~key orders descending
__device__ inline gficf_u64 gficf_f64_key(double v) {
  if (v == 0.0) v = 0.0;                                   // -0.0 ties with +0.0
  const gficf_u64 b = (gficf_u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | (1ull << 63));
}

// workgroups for n items at `per` a workgroup: at least one, at most cap (a kernel whose grid the cap can cut is grid-stride)
inline unsigned gficf_grid_capped(int64_t n, int64_t per, unsigned cap) {
  const int64_t b = gficf_ceil_div(n > 0 ? n : 1, per);
  return (unsigned)(b < (int64_t)cap ? b : (int64_t)cap);
}

// workgroups of 256 threads for n items, at most 16384: the kernels launched with it are grid-stride
inline unsigned gficf_grid_1d(int64_t n) { return gficf_grid_capped(n, 256, 16384); }
