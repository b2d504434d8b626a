// transform_search.h — the rectangular search of transform.hip: M query rows against N training rows.
//
// The tile kernel has the register tiling of knn.hip's k_knn_tiles in its plain form and the same arithmetic, operation by
// operation (knn_dim there, tr_dim here), so a table over the same rows has the same bits: a tile of 64 queries in LDS
// ([dim][query]), candidate tiles of 128 rows streamed through a double-buffered LDS chunk of 16 dimensions, a 4 x 8 block of
// distances per thread, a sorted list of the k best keys sortable(distance) << 32 | id per query (registers up to k = 64, LDS
// beyond).  What differs is where the parallelism comes from: with a few hundred queries there are only a handful of query
// tiles, so the candidate range is cut into S slices, S chosen from M so that (query tiles) x S fills the chip at two
// workgroups per CU — S is in the hundreds for a single query tile — and k_tr_merge, one wave per query, reduces the S partial
// lists.  No pruned form.
#pragma once

#include <atomic>
#include <cfloat>
#include <cstdlib>
#include <type_traits>

#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int TR_TC = 128;           // candidates per tile
constexpr int TR_DK = 16;            // dims per LDS chunk of the candidate tile
constexpr int TR_THREADS = 256;
constexpr int TR_RQ = 4;             // query rows per thread
constexpr int TR_TQ = 16 * TR_RQ;    // queries per workgroup
constexpr int TR_MAX_SPLIT = 512;    // slices of the candidate range, at most (k_tr_merge: 8 lists per lane)
constexpr int TR_MIN_SLICE = 2;      // candidate tiles per slice, at least (where there are that many)

__device__ inline uint32_t tr_f32_sortable(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ inline float tr_sortable_f32(uint32_t s) { return __uint_as_float(s ^ (((s >> 31) - 1u) | 0x80000000u)); }

typedef __attribute__((address_space(3))) volatile u64 tr_lds_u64;
typedef float tr_f2 __attribute__((ext_vector_type(2)));

// Insertions of one tile row into its list in LDS (k > 64).  The 16 lanes of a group share the row; per round the lowest lane
// of each group that holds a candidate hands one key to its group, whose lanes rebuild the list together: lane t owns entries
// t, t + 16, ... and writes  cur <= key ? cur : (prev <= key ? key : prev).  One wave, program order: no lock.
template <int KL>
__device__ __noinline__ float tr_row_insert(uint32_t list_addr, int kk, float d0, float d1, float d2, float d3, float d4, float d5, float d6,
                                            float d7, float tau, bool live, uint32_t j0, int tid) {
  tr_lds_u64* const list = (tr_lds_u64*)(size_t)list_addr;
  const float dv[8] = {d0, d1, d2, d3, d4, d5, d6, d7};
  const int tx = tid & 15;
  uint32_t pass = 0;
  if (live) {
#pragma unroll
    for (int s = 0; s < 8; ++s) pass |= (dv[s] <= tau) ? 1u << s : 0u;
  }
  for (;;) {
    const u64 m = __ballot(pass != 0);
    if (m == 0) break;
    const uint32_t gm = (uint32_t)(m >> (tid & 48)) & 0xFFFFu;
    const int leader = __ffs(gm) - 1;                   // -1: this group has no candidate this round
    uint32_t khi = 0, klo = 0;
    if (pass != 0 && tx == leader) {
      const int s = __ffs(pass) - 1;
      pass &= pass - 1;
      float h = dv[0];
#pragma unroll
      for (int t = 1; t < 8; ++t) h = s == t ? dv[t] : h;
      khi = tr_f32_sortable(h);
      klo = j0 + (uint32_t)((s < 4 ? 0 : 64) + tx * 4 + (s & 3));
    }
    const int src = ((tid & 48) | (leader & 15)) << 2;
    khi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)khi);
    klo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)klo);
    if (leader >= 0) {
      const u64 key = ((u64)khi << 32) | (u64)klo;
      u64 nw[KL / 16];
#pragma unroll
      for (int e = 0; e < KL / 16; ++e) {
        const int pos = e * 16 + tx;
        const u64 cur = list[pos];
        const u64 prev = pos > 0 ? list[pos - 1] : 0ull;
        nw[e] = cur <= key ? cur : (prev <= key ? key : prev);
      }
#pragma unroll
      for (int e = 0; e < KL / 16; ++e) {
        const int pos = e * 16 + tx;
        if (pos < kk) list[pos] = nw[e];
      }
    }
  }
  const uint32_t tau_hi = (uint32_t)(list[kk - 1] >> 32);
  return tau_hi == 0xFFFFFFFFu ? INFINITY : tr_sortable_f32(tau_hi);     // list not full yet: everything enters
}

struct TrOperands {            // one dimension's slice of the tiles: 4 query values, 8 candidate values
  float4 a0, b0, b1;
};
__device__ inline void tr_read(TrOperands& o, const float* __restrict__ pa, const float* __restrict__ pb) {
  o.a0 = *reinterpret_cast<const float4*>(pa);
  o.b0 = *reinterpret_cast<const float4*>(pb);
  o.b1 = *reinterpret_cast<const float4*>(pb + 64);
}

// One dimension of the 4 x 8 register block: the accumulators are float pairs (two neighbouring candidates); a - b is one
// packed subtract, the euclidean / cosine updates are packed fmas, manhattan adds |d| with two plain adds per pair.
template <int METRIC>
__device__ inline void tr_dim(tr_f2 (&acc)[TR_RQ][4], const TrOperands& o) {
  const float a[4] = {o.a0.x, o.a0.y, o.a0.z, o.a0.w};
  const tr_f2 b[4] = {{o.b0.x, o.b0.y}, {o.b0.z, o.b0.w}, {o.b1.x, o.b1.y}, {o.b1.z, o.b1.w}};
#pragma unroll
  for (int r = 0; r < TR_RQ; ++r) {
    const tr_f2 ar = {a[r], a[r]};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (METRIC == GFICF_KNN_MANHATTAN) {
        const tr_f2 df = ar - b[s];
        acc[r][s].x = acc[r][s].x + __builtin_fabsf(df.x);
        acc[r][s].y = acc[r][s].y + __builtin_fabsf(df.y);
      } else if (METRIC == GFICF_KNN_EUCLIDEAN) {
        const tr_f2 df = ar - b[s];
        acc[r][s] = __builtin_elementwise_fma(df, df, acc[r][s]);
      } else {
        acc[r][s] = __builtin_elementwise_fma(ar, b[s], acc[r][s]);
      }
    }
  }
}

// Lists of up to 64 entries live in registers: lane t of the row's 16-lane group holds entries EPL t .. EPL t + EPL - 1; the
// entry in front of a lane's first one comes from the lane below through one DPP row shift (lane 0 reads 0: nothing in front).
template <int EPL>
__device__ __forceinline__ void tr_reg_insert(u64 (&lst)[EPL], u64 key) {
  const u64 last = lst[EPL - 1];
  const uint32_t plo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)last, 0x111, 0xf, 0xf, true);          // row_shr:1, zero fill
  const uint32_t phi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(last >> 32), 0x111, 0xf, 0xf, true);
  u64 prev = ((u64)phi << 32) | (u64)plo;
#pragma unroll
  for (int h = 0; h < EPL; ++h) {
    const u64 cur = lst[h];
    lst[h] = cur <= key ? cur : (prev <= key ? key : prev);
    prev = cur;
  }
}

struct TrTileArgs {
  const float* Q;          // n_q query rows
  int64_t n_q;
  const float* X;          // N candidate rows
  int64_t N;
  int d, dpad, kk, S;
  u64* part;               // [n_q][S][kk] partial lists
};

// One workgroup = one tile of 64 queries x the candidate tiles of slice sp of S, in order.
template <int METRIC, int KL>
__global__ __launch_bounds__(TR_THREADS, 2) void k_tr_tiles(const TrTileArgs A) {
  constexpr int TQ = TR_TQ, RQ = TR_RQ;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = A.d, dpad = A.dpad, kk = A.kk, S = A.S;
  const int64_t N = A.N;
  float* const sA = reinterpret_cast<float*>(smem);                          // [dpad][TQ]
  float* const sB = sA + (size_t)dpad * TQ;                                  // [2][DK][TC]
  constexpr bool REGL = KL <= 64;                                            // lists in registers (else in LDS)
  constexpr int EPL = KL / 16;                                               // list entries per lane of a row's 16-lane group
  u64* const sKey = reinterpret_cast<u64*>(sB + 2 * TR_DK * TR_TC);          // !REGL: [TQ][KL]
  const uint32_t key_addr = (uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)(unsigned char*)sKey;   // LDS byte address

  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  const int qt = blockIdx.x / S, sp = blockIdx.x % S;
  const int64_t q0 = (int64_t)qt * TQ;
  const int nq_live = A.n_q - q0 < TQ ? (int)(A.n_q - q0) : TQ;              // rows that are real queries
  if (nq_live <= 0) return;
  const int64_t n_ct = gficf_ceil_div(N, TR_TC);
  const int64_t ct0 = n_ct * sp / S, ct1 = n_ct * (sp + 1) / S;
  const int nq4 = dpad >> 2;                         // float4 per row
  const int nch = (d + TR_DK - 1) / TR_DK;           // chunks per candidate tile (padded dims are skipped)
  const float4* const X4 = reinterpret_cast<const float4*>(A.X);
  const float4* const Q4 = reinterpret_cast<const float4*>(A.Q);

  if (!REGL)
    for (int e = tid; e < TQ * KL; e += TR_THREADS) sKey[e] = ~0ull;
  u64 lst[RQ][REGL ? EPL : 1];                       // REGL: this lane's entries of its rows' lists
#pragma unroll
  for (int r = 0; r < RQ; ++r)
#pragma unroll
    for (int h = 0; h < (REGL ? EPL : 1); ++h) lst[r][h] = ~0ull;
  // query tile -> sA[dim][query]; consecutive lanes take consecutive queries (conflict-free LDS writes)
  for (int f = tid; f < TQ * nq4; f += TR_THREADS) {
    const int row = f & (TQ - 1), quad = f / TQ;
    const int64_t q = q0 + row;
    const float4 v = q < A.n_q ? Q4[q * nq4 + quad] : make_float4(0.f, 0.f, 0.f, 0.f);
    float* o = sA + (size_t)(quad * 4) * TQ + row;
    o[0] = v.x; o[TQ] = v.y; o[2 * TQ] = v.z; o[3 * TQ] = v.w;
  }

  // Staging of a candidate tile's dim chunk: 128 rows x 16 dims = 512 float4, two per thread (row row_l, float4 columns quad0
  // and quad0 + 2 of the chunk); consecutive lanes take consecutive rows, so the transposing LDS writes are conflict-free.
  const int row_l = tid & (TR_TC - 1), quad0 = tid >> 7;
  float* const st0 = sB + (size_t)(quad0 * 4) * TR_TC + row_l;
  auto load_chunk = [&](int64_t ct, int c, float4 (&v)[2]) {
    const int64_t j = ct * TR_TC + row_l;
    const int q4 = c * (TR_DK / 4) + quad0;
    const float4* src = X4 + j * nq4 + q4;
    v[0] = (j < N && q4 < nq4) ? src[0] : make_float4(0.f, 0.f, 0.f, 0.f);
    v[1] = (j < N && q4 + 2 < nq4) ? src[2] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store_chunk = [&](int buf, const float4 (&v)[2]) {
    float* o = st0 + (size_t)buf * TR_DK * TR_TC;
    o[0] = v[0].x; o[TR_TC] = v[0].y; o[2 * TR_TC] = v[0].z; o[3 * TR_TC] = v[0].w;
    o += 8 * TR_TC;
    o[0] = v[1].x; o[TR_TC] = v[1].y; o[2 * TR_TC] = v[1].z; o[3 * TR_TC] = v[1].w;
  };

  tr_f2 acc[RQ][4];
#pragma unroll
  for (int r = 0; r < RQ; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = tr_f2{0.0f, 0.0f};
  float tau[RQ];                // current k-th best distance of this thread's query rows
#pragma unroll
  for (int r = 0; r < RQ; ++r) tau[r] = INFINITY;

  __syncthreads();              // sA (and sKey) are in place
  int64_t cur = ct0 < ct1 ? ct0 : -1;
  float4 pre[2];
  if (cur >= 0) { load_chunk(cur, 0, pre); store_chunk(0, pre); }
  __syncthreads();

  int buf = 0;
  while (cur >= 0) {
    int64_t nxt = -1;
    for (int c = 0; c < nch; ++c) {
      bool have_next;
      if (c + 1 < nch) {
        load_chunk(cur, c + 1, pre);
        have_next = true;
      } else {
        nxt = cur + 1 < ct1 ? cur + 1 : -1;
        have_next = nxt >= 0;
        if (have_next) load_chunk(nxt, 0, pre);
      }
      const float* const pa = sA + (size_t)(c * TR_DK) * TQ + ty * 4;
      const float* const pb = sB + (size_t)buf * TR_DK * TR_TC + tx * 4;
      const int nd = d - c * TR_DK < TR_DK ? d - c * TR_DK : TR_DK;
      {
        // two dims per round (the rows are zero padded to a multiple of 4 dims, and a zero dim adds exactly 0 to every metric's
        // accumulator); the operands of the next dim are read from LDS while the current one is accumulated
        const int np = (nd + 1) >> 1;
        TrOperands oa, ob;
        tr_read(oa, pa, pb);
#pragma unroll 1
        for (int t = 0; t < np; ++t) {
          tr_read(ob, pa + (2 * t + 1) * TQ, pb + (2 * t + 1) * TR_TC);
          tr_dim<METRIC>(acc, oa);
          if (t + 1 < np) tr_read(oa, pa + (2 * t + 2) * TQ, pb + (2 * t + 2) * TR_TC);
          tr_dim<METRIC>(acc, ob);
        }
      }
      if (c == nch - 1) {
        const int64_t j0 = cur * TR_TC;
        const int nvalid = N - j0 < TR_TC ? (int)(N - j0) : TR_TC;      // only the last candidate tile can be short
        auto epilogue = [&](auto rag_tag) {
          constexpr bool RAG = decltype(rag_tag)::value;      // RAG: candidates at columns >= nvalid do not exist
#pragma unroll
          for (int r = 0; r < RQ; ++r) {
            const int row = ty * 4 + r;
            const bool live = row < nq_live;
            bool any = false;
#pragma unroll
            for (int s = 0; s < 8; ++s) {
              const float av = (s & 1) ? acc[r][s >> 1].y : acc[r][s >> 1].x;
              bool ok = (METRIC == GFICF_KNN_COSINE ? 1.0f - av : av) <= tau[r];
              if (RAG) ok = ok && (s < 4 ? 0 : 64) + tx * 4 + (s & 3) < nvalid;
              any |= ok;
            }
            if (__ballot(any && live) != 0) {
              float dv[8];
#pragma unroll
              for (int s = 0; s < 8; ++s) {
                const float av = (s & 1) ? acc[r][s >> 1].y : acc[r][s >> 1].x;
                dv[s] = METRIC == GFICF_KNN_COSINE ? 1.0f - av : av;
                if (RAG && (s < 4 ? 0 : 64) + tx * 4 + (s & 3) >= nvalid) dv[s] = NAN;       // never <= tau
              }
              if (REGL) {
                uint32_t pass = 0;
                if (live) {
#pragma unroll
                  for (int s = 0; s < 8; ++s) pass |= (dv[s] <= tau[r]) ? 1u << s : 0u;
                }
                for (;;) {
                  const u64 m = __ballot(pass != 0);
                  if (m == 0) break;
                  const uint32_t gm = (uint32_t)(m >> (tid & 48)) & 0xFFFFu;
                  const int leader = __ffs(gm) - 1;             // -1: this group has no candidate this round
                  uint32_t khi = 0, klo = 0;
                  if (pass != 0 && tx == leader) {
                    const int s = __ffs(pass) - 1;
                    pass &= pass - 1;
                    float h = dv[0];
#pragma unroll
                    for (int t = 1; t < 8; ++t) h = s == t ? dv[t] : h;
                    khi = tr_f32_sortable(h);
                    klo = (uint32_t)j0 + (uint32_t)((s < 4 ? 0 : 64) + tx * 4 + (s & 3));
                  }
                  const int src = ((tid & 48) | (leader & 15)) << 2;
                  khi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)khi);
                  klo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)klo);
                  if (leader >= 0) {
                    tr_reg_insert<REGL ? EPL : 1>(lst[r], ((u64)khi << 32) | (u64)klo);
                    // the list's k-th best may just have dropped: candidates it no longer admits need no round of their own
                    uint32_t tn = (uint32_t)(lst[r][0] >> 32);
#pragma unroll
                    for (int h = 1; h < (REGL ? EPL : 1); ++h) tn = ((kk - 1) % EPL) == h ? (uint32_t)(lst[r][h] >> 32) : tn;
                    tn = (uint32_t)__shfl((int)tn, (kk - 1) / EPL, 16);
                    if (tn != 0xFFFFFFFFu && pass != 0) {
                      const float tnew = tr_sortable_f32(tn);
                      uint32_t keep = 0;
#pragma unroll
                      for (int s = 0; s < 8; ++s) keep |= (dv[s] <= tnew) ? 1u << s : 0u;
                      pass &= keep;
                    }
                  }
                }
                // the row's k-th best: entry kk - 1 sits in lane (kk - 1) / EPL of the group
                uint32_t th = (uint32_t)(lst[r][0] >> 32);
#pragma unroll
                for (int h = 1; h < (REGL ? EPL : 1); ++h) th = ((kk - 1) % EPL) == h ? (uint32_t)(lst[r][h] >> 32) : th;
                th = (uint32_t)__shfl((int)th, (kk - 1) / EPL, 16);
                tau[r] = th == 0xFFFFFFFFu ? INFINITY : tr_sortable_f32(th);      // list not full yet: everything enters
              } else {
                tau[r] = tr_row_insert<KL>(key_addr + (uint32_t)(row * KL * 8), kk, dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], dv[6], dv[7], tau[r],
                                           live, (uint32_t)j0, tid);
              }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[r][s] = tr_f2{0.0f, 0.0f};
          }
        };
        if (nvalid < TR_TC) epilogue(std::true_type{});
        else epilogue(std::false_type{});
      }
      if (have_next) store_chunk(buf ^ 1, pre);
      __syncthreads();
      buf ^= 1;
    }
    cur = nxt;
  }

  // partial lists of this candidate slice (an empty slice writes its untouched lists: all ~0)
  if (REGL) {
#pragma unroll
    for (int r = 0; r < RQ; ++r) {
      const int64_t q = q0 + ty * 4 + r;
#pragma unroll
      for (int h = 0; h < (REGL ? EPL : 1); ++h) {
        const int e = EPL * tx + h;
        if (q < A.n_q && e < kk) A.part[(q * S + sp) * kk + e] = lst[r][h];
      }
    }
  } else {
    for (int e = tid; e < TQ * kk; e += TR_THREADS) {
      const int row = e / kk, t = e % kk;
      const int64_t q = q0 + row;
      if (q < A.n_q) A.part[(q * S + sp) * kk + t] = sKey[row * KL + t];
    }
  }
}

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
        dv = tr_sortable_f32((uint32_t)(best >> 32));
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
  const int64_t n_qt = gficf_ceil_div(M > 0 ? M : 1, TR_TQ), n_ct = gficf_ceil_div(N > 0 ? N : 1, TR_TC);
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

template <int METRIC, int KL>
int tr_launch(gficf_ctx* ctx, const TrTileArgs& a) {
  // LDS: the query tile, the two candidate chunks and, beyond k = 64, the lists: at d = 128, k = 128 that is 32 + 16 + 64 KiB =
  // 112 KiB, one workgroup per CU of 160 KiB; up to k = 64 it is at most 48 KiB and the two workgroups of the launch bound fit
  const size_t lds = (size_t)a.dpad * TR_TQ * 4 + 2 * TR_DK * TR_TC * 4 + (KL > 64 ? (size_t)TR_TQ * KL * 8 : 0);
  static std::atomic<bool> attr_set[64];
  if (!attr_set[ctx->device & 63]) {
    GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_tr_tiles<METRIC, KL>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64));
    attr_set[ctx->device & 63] = true;
  }
  const int64_t blocks = gficf_ceil_div(a.n_q, TR_TQ) * a.S;
  hipLaunchKernelGGL((k_tr_tiles<METRIC, KL>), dim3((unsigned)blocks), dim3(TR_THREADS), lds, ctx->stream, a);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

template <int METRIC>
int tr_launch_k(gficf_ctx* ctx, const TrTileArgs& a) {
  if (a.kk <= 32) return tr_launch<METRIC, 32>(ctx, a);
  if (a.kk <= 64) return tr_launch<METRIC, 64>(ctx, a);
  return tr_launch<METRIC, 128>(ctx, a);
}

int tr_launch_m(gficf_ctx* ctx, int metric, const TrTileArgs& a) {
  switch (metric) {
    case GFICF_KNN_MANHATTAN: return tr_launch_k<GFICF_KNN_MANHATTAN>(ctx, a);
    case GFICF_KNN_EUCLIDEAN: return tr_launch_k<GFICF_KNN_EUCLIDEAN>(ctx, a);
    default: return tr_launch_k<GFICF_KNN_COSINE>(ctx, a);
  }
}

}  // namespace
