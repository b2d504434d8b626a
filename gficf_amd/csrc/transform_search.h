// transform_search.h — the rectangular search of transform.hip: M query rows against N training rows.
//
// The tile kernel is knn_tiles.h's, plain form: the very k_knn_tiles of knn.hip's square search, compiled from the same text, so
// a table over the same rows has the same bits.  What is the transform's own is where the parallelism comes from: with a few
// hundred queries there are only a handful of query tiles, so the candidate range is cut into S slices, S chosen from M so that
// (query tiles) x S fills the chip at two workgroups per CU — S is in the hundreds for a single query tile — and k_tr_merge, one
// wave per query, reduces the S partial lists.  No pruned form.
#pragma once

#include <cstdlib>

#include "common.h"
#include "knn_tiles.h"

namespace {

constexpr int TR_MAX_SPLIT = 512;    // slices of the candidate range, at most (k_tr_merge: 8 lists per lane)
constexpr int TR_MIN_SLICE = 2;      // candidate tiles per slice, at least (where there are that many)

// k best of the S <= TR_MAX_SPLIT partial lists of a query (each ascending) -> 1-based ids / distances, column-major.  One wave
// per query: lane l walks the lists l, l + 64, ...; per output the wave takes the smallest head (keys are distinct: they carry
// the id) and its owner steps on.
__global__ __launch_bounds__(256) void k_tr_merge(const u64* __restrict__ part, int64_t n_q, int S, int kk, int metric, int32_t* __restrict__ idx,
                                                  float* __restrict__ dist, int64_t ld_out) {
  constexpr int LPL = TR_MAX_SPLIT / 64;             // lists per lane
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n_q) return;                              // wave-uniform
  const u64* const base = part + q * S * kk;
  int pos[LPL];
  u64 head[LPL];
#pragma unroll
  for (int j = 0; j < LPL; ++j) {
    const int s = lane + 64 * j;
    pos[j] = 0;
    head[j] = s < S ? base[(int64_t)s * kk] : ~0ull;
  }
  for (int t = 0; t < kk; ++t) {
    u64 mine = head[0];
#pragma unroll
    for (int j = 1; j < LPL; ++j) mine = head[j] < mine ? head[j] : mine;
    u64 best = mine;
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
      const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best, w), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), w);
      const u64 o = ((u64)ohi << 32) | (u64)olo;
      best = o < best ? o : best;
    }
    if (best != ~0ull) {
#pragma unroll
      for (int j = 0; j < LPL; ++j) {
        if (head[j] == best) {
          const int s = lane + 64 * j;
          ++pos[j];
          head[j] = pos[j] < kk ? base[(int64_t)s * kk + pos[j]] : ~0ull;
        }
      }
    }
    if (lane == 0) {
      int32_t id = 0;
      float dv = INFINITY;
      if (best != ~0ull) {
        id = (int32_t)(uint32_t)best + 1;
        dv = sortable_f32((uint32_t)(best >> 32));
        if (metric == GFICF_KNN_EUCLIDEAN) dv = sqrtf(dv);
      }
      idx[(int64_t)t * ld_out + q] = id;
      if (dist) dist[(int64_t)t * ld_out + q] = dv;
    }
  }
}

// S: enough slices that (query tiles) x S workgroups cover the chip at two per CU, every slice TR_MIN_SLICE candidate tiles
// long where there are that many.  GFICF_TRANSFORM_SPLIT in the environment forces a value (tuning knob).
// num_cus counts up to TR_MAX_CUS: the workspace is sized without a context, for that many.
constexpr int TR_MAX_CUS = 256;
int tr_split(int num_cus, int64_t M, int64_t N) {
  const int64_t n_qt = gficf_ceil_div(M > 0 ? M : 1, KNN_TQ), n_ct = gficf_ceil_div(N > 0 ? N : 1, KNN_TC);
  int64_t S = gficf_ceil_div((int64_t)(num_cus < 1 ? 1 : num_cus > TR_MAX_CUS ? TR_MAX_CUS : num_cus) * 2, n_qt);
  if (S > n_ct / TR_MIN_SLICE) S = n_ct / TR_MIN_SLICE;
  if (S > TR_MAX_SPLIT) S = TR_MAX_SPLIT;
  if (S < 1) S = 1;
  if (const char* e = getenv("GFICF_TRANSFORM_SPLIT")) {
    const int v = atoi(e);
    if (v >= 1 && v <= TR_MAX_SPLIT) S = v;
  }
  return (int)S;
}

}  // namespace
