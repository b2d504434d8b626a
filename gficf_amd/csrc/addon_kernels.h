// addon_kernels.h — the small boundary kernels of the embedding add-ons (umap.hip, tsne.hip, transform.hip).  Apart from
// addon_status.h because a kernel is emitted into every object that includes it, used or not (tsne.hip has no use for
// k_addon_finite: its k_ts_check looks at the coordinates).
#pragma once

#include "addon_status.h"

namespace {

// a buffer of n coordinates checked (grid-stride: at most 1024 workgroups are launched)
__global__ __launch_bounds__(256) void k_addon_finite(const float* __restrict__ Y, int64_t n, uint32_t* __restrict__ status) {
  bool bad = false;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) bad |= !isfinite(Y[t]);
  if (bad) atomicOr(status, GFICF_AST_VALUE);
}

// (N, 2) f32 row-major -> f64 column-major, the form the host entries return
__global__ __launch_bounds__(256) void k_addon_out(const float* __restrict__ Y, int64_t N, double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 2 * N) return;
  out[(t & 1) * N + (t >> 1)] = (double)Y[t];
}

// the entries of a caller's CSR graph, whatever its last row pointer claims
__device__ inline int64_t gficf_addon_nnz(const int64_t* rowptr, int64_t N, int64_t cap) {
  const int64_t n = rowptr[N];
  return n < 0 ? 0 : n > cap ? cap : n;
}

}  // namespace
