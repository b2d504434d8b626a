// knn_symmetrise.h — a kNN table's directed weights W turned into a symmetric CSR matrix: the graph stage of umap.hip and the
// affinity stage of tsne.hip end with it.  N points, `cols` columns of W (column-major, N each), M = 2 N cols items: every
// weight once as (i, j) and once as (j, i).  The two callers differ in the table column that belongs to column c of W
// (idx_col0 + c: UMAP's W keeps the self column, idx_col0 = 0; t-SNE's has none, idx_col0 = 1; sym_enqueue hands the kernels
// the table from that column on) and in how the two weights of a pair combine: a functor passed by value, whose body stays
// with the contract it implements (um_combine, ts_combine).
//
// Launches:
//   k_sym_key_col, (sort), k_sym_key_row, (sort)   the items sorted by (row, column) with the library's stable radix passes:
//                                   by column first, then by row; a dropped item carries the key N and sorts behind the rest
//   k_sym_heads      one lane per sorted item: the first of a (row, column) pair combines with its mirror, if that follows it
//   (scan), k_sym_emit   positions of the kept entries; columns, values, row pointers (a lane that sees a row change writes the
//                                   pointers of the rows in between), nnz
// No step looks at a row as a whole, so the in-degree of a point (up to N - 1) costs nothing special here.
#pragma once

#include "common.h"

namespace {

typedef unsigned long long u64;

// one lane per element: n stays below 2^32 + 2 here (N cols < 2^31), so the blocks fit a grid's x dimension
inline unsigned sym_grid(int64_t n) { return (unsigned)gficf_ceil_div(n > 0 ? n : 1, 256); }

// item t = 2 slot + dir, slot = c N + i: dir 0 is the entry (i, j) of W, dir 1 the entry (j, i) of its transpose;
// idx: the table from the column of W's column 0 on
struct SymItem { int32_t row, col; float w; };

__device__ inline SymItem sym_item(uint32_t t, const int32_t* __restrict__ idx, const float* __restrict__ W, int64_t N, int64_t ld) {
  const int64_t slot = t >> 1, c = slot / N, i = slot % N;
  const float w = W[slot];
  SymItem it;
  it.w = w;
  if (!(w > 0.f)) {                                             // dropped: the self entry, a bad id, an underflow
    it.row = (int32_t)N; it.col = 0;
    return it;
  }
  const int32_t j = idx[c * ld + i] - 1;                        // in [0, N): the kernel that wrote W zeroed the others
  it.row = (t & 1u) ? j : (int32_t)i;
  it.col = (t & 1u) ? (int32_t)i : j;
  return it;
}

__global__ __launch_bounds__(256) void k_sym_key_col(const int32_t* __restrict__ idx, const float* __restrict__ W, int64_t N,
                                                     int64_t ld, int64_t M, u64* __restrict__ kv) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= M) return;
  const SymItem it = sym_item((uint32_t)t, idx, W, N, ld);
  kv[t] = ((u64)(uint32_t)it.col << 32) | (u64)t;
}

__global__ __launch_bounds__(256) void k_sym_key_row(const int32_t* __restrict__ idx, const float* __restrict__ W, int64_t N,
                                                     int64_t ld, int64_t M, const uint32_t* __restrict__ order, u64* __restrict__ kv) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= M) return;
  const uint32_t t = order[p];
  const SymItem it = sym_item(t, idx, W, N, ld);
  kv[p] = ((u64)(uint32_t)it.row << 32) | (u64)t;
}

// combine(x, y): the value of a pair from its two weights (0 for a direction that is absent); it must not depend on their order
template <class Combine>
__global__ __launch_bounds__(256) void k_sym_heads(const int32_t* __restrict__ idx, const float* __restrict__ W, int64_t N,
                                                   int64_t ld, int64_t M, const uint32_t* __restrict__ item, Combine combine,
                                                   int64_t* __restrict__ flag, int32_t* __restrict__ tcol, float* __restrict__ tval) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > M) return;
  if (p == M) { flag[p] = 0; return; }
  const SymItem me = sym_item(item[p], idx, W, N, ld);
  int64_t keep = 0;
  if (me.row < N) {
    bool head = true;
    if (p > 0) {
      const SymItem pr = sym_item(item[p - 1], idx, W, N, ld);
      head = pr.row != me.row || pr.col != me.col;
    }
    if (head) {
      float other = 0.f;
      if (p + 1 < M) {
        const SymItem nx = sym_item(item[p + 1], idx, W, N, ld);
        if (nx.row == me.row && nx.col == me.col) other = nx.w;
      }
      const float v = combine(me.w, other);
      tcol[p] = me.col;
      tval[p] = v;
      keep = v > 0.f ? 1 : 0;
    }
  }
  flag[p] = keep;
}

__global__ __launch_bounds__(256) void k_sym_emit(int64_t N, int64_t M, const uint32_t* __restrict__ srow, const int64_t* __restrict__ pos,
                                                  const int32_t* __restrict__ tcol, const float* __restrict__ tval, int64_t* __restrict__ rowptr,
                                                  int32_t* __restrict__ col, float* __restrict__ val, int64_t* __restrict__ nnz) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p > M) return;
  const int64_t at = pos[p];
  if (p < M && pos[p + 1] != at) {
    col[at] = tcol[p];
    val[at] = tval[p];
  }
  int64_t row = p < M ? (int64_t)srow[p] : N, prev = p > 0 ? (int64_t)srow[p - 1] : -1;
  if (row > N) row = N;
  if (prev > N) prev = N;
  for (int64_t r = prev + 1; r <= row; ++r) rowptr[r] = at;     // the rows that begin here: this one and the empty ones before it
  if (p == M) *nnz = at;
}

// the scratch of the symmetrisation, carved out of the caller's workspace behind its W
struct SymWs {
  u64 *kv0, *kv1;
  int64_t* hist;
  uint32_t *okey, *oval;
  int64_t* flag;
  int32_t* tcol;
  float* tval;
};

inline void sym_carve(gficf_carver& cv, int64_t N, size_t M, SymWs& w) {
  w.kv0 = cv.take<u64>(M);
  w.kv1 = cv.take<u64>(M);
  w.hist = cv.take<int64_t>((size_t)gficf_radix_sort_hist_len((int64_t)M, gficf_bit_width(N)));
  w.okey = cv.take<uint32_t>(M);
  w.oval = cv.take<uint32_t>(M);
  w.flag = cv.take<int64_t>(M + 1);
  w.tcol = cv.take<int32_t>(M);
  w.tval = cv.take<float>(M);
}

// enqueues the whole sequence on the context's stream; the CSR outputs need room for M entries
template <class Combine>
int sym_enqueue(gficf_ctx* ctx, const SymWs& w, const int32_t* d_idx, int idx_col0, const float* d_W, int64_t N, int cols, int64_t ld,
                Combine combine, int64_t* d_rowptr, int32_t* d_col, float* d_val, int64_t* d_nnz) {
  hipStream_t st = ctx->stream;
  const int64_t M = 2 * N * cols;
  const int bits = gficf_bit_width(N);
  d_idx += (int64_t)idx_col0 * ld;
  hipLaunchKernelGGL(k_sym_key_col, dim3(sym_grid(M)), dim3(256), 0, st, d_idx, d_W, N, ld, M, w.kv0);
  GFICF_HIP_CHECK(hipGetLastError());
  int rc = gficf_radix_sort_kv(ctx, w.kv0, w.kv1, w.hist, M, bits, w.okey, w.oval);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sym_key_row, dim3(sym_grid(M)), dim3(256), 0, st, d_idx, d_W, N, ld, M, (const uint32_t*)w.oval, w.kv0);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = gficf_radix_sort_kv(ctx, w.kv0, w.kv1, w.hist, M, bits, w.okey, w.oval);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sym_heads<Combine>, dim3(sym_grid(M + 1)), dim3(256), 0, st, d_idx, d_W, N, ld, M, (const uint32_t*)w.oval,
                     combine, w.flag, w.tcol, w.tval);
  GFICF_HIP_CHECK(hipGetLastError());
  rc = gficf_exclusive_scan_i64(ctx, w.flag, M + 1);
  if (rc) return rc;
  hipLaunchKernelGGL(k_sym_emit, dim3(sym_grid(M + 1)), dim3(256), 0, st, N, M, (const uint32_t*)w.okey, (const int64_t*)w.flag,
                     (const int32_t*)w.tcol, (const float*)w.tval, d_rowptr, d_col, d_val, d_nnz);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

}  // namespace
