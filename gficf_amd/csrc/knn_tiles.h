// knn_tiles.h — the tile kernel of the exact searches: ONE text for knn.hip (the square search, plain and pruned) and for
// transform.hip (the rectangular search of new cells against trained ones, plain form), so that a table over the same rows
// has the same bits in both libraries by construction, not by two texts edited in step.
//
// One workgroup = a tile of 64 queries x a sequence of candidate tiles: the query tile stays in LDS ([dim][query]), candidate
// tiles of 128 points stream through a double-buffered LDS chunk of 16 dims; every thread accumulates a 4 x 8 block of
// distances in registers.  Per query a sorted list of the k best 64-bit keys (sortable(distance) << 32 | index) lives in
// registers (k <= 64) or in LDS; a thread inserts a candidate only when it beats the list's last key (rare after the first
// tiles).  A query's row of the tile belongs to the 16 lanes of one wave, which take turns (wave-uniform loop, one elected lane
// per row and round): no locks.  What reduces the partial lists (the merge) and how the candidate range is split are the
// including file's own.
//
// The two including objects are built with different flags (knn.o: the compiler's default contraction; transform.o:
// -ffp-contract=off; both -fno-slp-vectorize).  NOTHING HERE MAY DEPEND ON FLOATING-POINT CONTRACTION, or on SLP vectorisation
// beyond what both objects are built with: every fused multiply-add in this file is a written-out builtin
// (__builtin_elementwise_fma) and no expression has the shape a * b + c for the compiler to fuse or not — that is why the two
// builds agree, instruction for instruction ("What an add-on shares").
#pragma once

#include <atomic>
#include <type_traits>

#include "common.h"

namespace {

constexpr int KNN_TC = 128;        // candidates per tile
constexpr int KNN_DK = 16;         // dims per LDS chunk of the candidate tile
constexpr int KNN_THREADS = 256;
// RQ = query rows per thread, a template parameter of the kernel that only ever is KNN_RQ = 4 (tile of 64 queries; measured faster
// than 8 = 128 queries, which the code still supports: 100 k x 50, 31 nearest, manhattan: 27.7 against 33.1 ms — fewer insertions
// per slice, lighter epilogue).  The parameter stays although nothing instantiates the 8-row form: writing the kernel without it
// (no a1 operand, rows ty * 4 + r) was tried and compiles to the same resources but not to the same instructions — the LDS reads
// of knn_dim's operands come out in another order — and a text that both searches share changes its code only for a reason.
constexpr int KNN_RQ = 4;
constexpr int KNN_TQ = 16 * KNN_RQ;    // queries per workgroup

typedef unsigned long long u64;

// order-preserving map float -> uint32 (and back)
__device__ inline uint32_t f32_sortable(float f) {
  const uint32_t u = __float_as_uint(f);
  return u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
}
__device__ inline float sortable_f32(uint32_t s) {
  return __uint_as_float(s ^ (((s >> 31) - 1u) | 0x80000000u));
}

// Insertions of one tile row.  The 16 lanes of a 16-lane group share the row (= the list).  The wave loops
// (uniformly) while any lane holds a candidate; per round the lowest such lane of each group hands one key
// to its group, and the group's lanes rebuild the list together: lane t owns entries t, t+16, ... and writes
//   cur <= key ? cur : (prev <= key ? key : prev)
// — an insertion shift with one LDS read and one LDS write per entry, no serial walk, no lock (one wave,
// program order).  Out of line: it runs rarely once the lists have warmed up and must not cost the
// distance loop its registers.
typedef __attribute__((address_space(3))) volatile u64 knn_lds_u64;

template <int KL>
__device__ __noinline__ float knn_row_insert(uint32_t list_addr, int kk, float d0, float d1, float d2, float d3, float d4, float d5,
                                             float d6, float d7, float tau, bool live, uint32_t j0, int tid,
                                             const int32_t* __restrict__ perm) {
  knn_lds_u64* const list = (knn_lds_u64*)(size_t)list_addr;      // LDS byte address of the row's list
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
      khi = f32_sortable(h);
      klo = j0 + (uint32_t)((s < 4 ? 0 : 64) + tx * 4 + (s & 3));
      if (perm) klo = (uint32_t)perm[klo];              // pruned search: the key carries the point's original id
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
  // this wave is the only writer of its rows' lists, so the caller's register copy of the k-th best stays exact
  const uint32_t tau_hi = (uint32_t)(list[kk - 1] >> 32);
  return tau_hi == 0xFFFFFFFFu ? INFINITY : sortable_f32(tau_hi);     // list not full yet: everything enters
}

// One dimension of the RQ x 8 register block.  Accumulators are float pairs (two neighbouring candidates), so
// that a - b is one packed subtract per pair (v_pk_add_f32 with the query value broadcast by op_sel), the
// euclidean / cosine updates are packed fmas, and manhattan adds |d| with the source modifier (two plain adds
// per pair: there is no packed abs).  Built with -fno-slp-vectorize: the SLP vectoriser would otherwise pack
// the two adds and pay for it with two v_and to clear the sign bits.
typedef float knn_f2 __attribute__((ext_vector_type(2)));

struct KnnOperands {            // one dimension's slice of the tiles: RQ query values, 8 candidate values
  float4 a0, a1, b0, b1;
};
template <int RQ>
__device__ inline void knn_read(KnnOperands& o, const float* __restrict__ pa, const float* __restrict__ pb) {
  o.a0 = *reinterpret_cast<const float4*>(pa);
  if (RQ == 8) o.a1 = *reinterpret_cast<const float4*>(pa + 64);
  o.b0 = *reinterpret_cast<const float4*>(pb);
  o.b1 = *reinterpret_cast<const float4*>(pb + 64);
}

template <int METRIC, int RQ>
__device__ inline void knn_dim(knn_f2 (&acc)[RQ][4], const KnnOperands& o) {
  const float a[8] = {o.a0.x, o.a0.y, o.a0.z, o.a0.w, o.a1.x, o.a1.y, o.a1.z, o.a1.w};
  const knn_f2 b[4] = {{o.b0.x, o.b0.y}, {o.b0.z, o.b0.w}, {o.b1.x, o.b1.y}, {o.b1.z, o.b1.w}};
#pragma unroll
  for (int r = 0; r < RQ; ++r) {
    const knn_f2 ar = {a[r], a[r]};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      if (METRIC == GFICF_KNN_MANHATTAN) {
        const knn_f2 df = ar - b[s];
        acc[r][s].x = acc[r][s].x + __builtin_fabsf(df.x);
        acc[r][s].y = acc[r][s].y + __builtin_fabsf(df.y);
      } else if (METRIC == GFICF_KNN_EUCLIDEAN) {
        const knn_f2 df = ar - b[s];
        acc[r][s] = __builtin_elementwise_fma(df, df, acc[r][s]);
      } else {
        acc[r][s] = __builtin_elementwise_fma(ar, b[s], acc[r][s]);
      }
    }
  }
}

// Lists of up to 64 entries live in registers: lane t of the row's 16-lane group holds entries EPL*t .. EPL*t+EPL-1
// (EPL = KL / 16).  An insertion is the same shift as in the LDS form, but the entry in front of a lane's first one
// comes from the lane below through one DPP row shift (the group's lane 0 reads 0, i.e. "nothing in front"), so a
// round is ~25 VALU instructions and no LDS round trip.  Every lane of the group calls it with the group's key.
template <int EPL>
__device__ __forceinline__ void knn_reg_insert(u64 (&lst)[EPL], u64 key) {
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

// Arguments of the tile kernel.  Queries and candidates are separate row-major arrays of dpad floats per row (dpad = d rounded
// up to 4, zero padded): the square search passes Q = X + q_begin rows in its plain form and its two reordered copies in its
// pruned form; the transform passes the new cells and the trained ones.  A value-initialised struct with the members up to
// `part` filled in is the plain form without a gate: knn_plain_args below.
struct KnnTileArgs {
  const float* Q;          // n_q query rows
  int64_t n_q;
  const float* X;          // N candidate rows
  int64_t N;
  int d, dpad, kk, S;
  u64* part;               // [n_q][S][kk] partial lists
  const int32_t* perm_x;   // PRUNE: original 0-based id of candidate row j (the keys carry original ids)
  const float* lb;         // PRUNE: [n_qt][n_ct] lower bound of the distance between query tile and candidate tile
  const int32_t* tile_n;   // PRUNE: points in candidate tile t (cells are padded to whole tiles: a prefix of the tile is real)
  const int32_t* qtile_n;  // PRUNE: queries in query tile qt
  const uint32_t* gate;    // optional: run only if *gate == gate_want (the pruned / plain choice is made on the device)
  uint32_t gate_want;
};

// The plain form's arguments: no gate, no permutation, no bounds.  Host only (no device code comes of it).
inline KnnTileArgs knn_plain_args(const float* Q, int64_t n_q, const float* X, int64_t N, int d, int dpad, int k, int S, u64* part) {
  KnnTileArgs a{};
  a.Q = Q; a.n_q = n_q; a.X = X; a.N = N;
  a.d = d; a.dpad = dpad; a.kk = k; a.S = S;
  a.part = part;
  return a;
}

// One workgroup = one tile of TQ = 16 * RQ queries x a sequence of candidate tiles.
//   PRUNE == false: the candidate tiles of slice sp of S, in order (an empty slice writes its untouched lists: all ~0).
//   PRUNE == true : S = 1; the candidate tiles in the order of their lower bound lb[qt][*], best first, and the
//     sequence ends at the first tile whose bound exceeds the largest k-th best distance of the tile's queries —
//     no point of that tile or of any later one can enter a list (the bound is a triangle-inequality bound
//     with slack for f32 rounding, built by knn_prune.h's k_knn_lb).  The next tile is chosen by every wave for itself from
//     the same LDS data (bounds, visited marks and the waves' k-th best maxima published one tile earlier,
//     double-buffered), so the waves agree without an extra barrier.
template <int METRIC, int KL, int RQ, bool PRUNE>
__global__ __launch_bounds__(KNN_THREADS, 2) void k_knn_tiles(const KnnTileArgs A) {
  constexpr int TQ = 16 * RQ;                                                // queries per workgroup
  if (A.gate != nullptr && *A.gate != A.gate_want) return;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int d = A.d, dpad = A.dpad, kk = A.kk, S = A.S;
  const int64_t N = A.N;
  float* const sA = reinterpret_cast<float*>(smem);                          // [dpad][TQ]
  float* const sB = sA + (size_t)dpad * TQ;                                  // [2][DK][TC]
  constexpr bool REGL = KL <= 64;                                            // lists in registers (else in LDS)
  constexpr int EPL = KL / 16;                                               // list entries per lane of a row's 16-lane group
  u64* const sKey = reinterpret_cast<u64*>(sB + 2 * KNN_DK * KNN_TC);        // !REGL: [TQ][KL]
  float* const sLb = reinterpret_cast<float*>(sKey + (REGL ? 0 : TQ * KL));  // PRUNE: [n_ct] bounds, +inf once visited
  const uint32_t key_addr = (uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)(unsigned char*)sKey;   // LDS byte address
  __shared__ float s_wtau[2][KNN_THREADS / 64];                              // PRUNE: per-wave max of the k-th best, by tile parity

  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4, lane = tid & 63, wave = tid >> 6;
  const int qt = blockIdx.x / S, sp = blockIdx.x % S;
  const int64_t q0 = (int64_t)qt * TQ;
  const int nq_live = (PRUNE && A.qtile_n) ? A.qtile_n[qt] : (A.n_q - q0 < TQ ? (int)(A.n_q - q0) : TQ);   // rows that are real queries
  if (nq_live <= 0) return;                          // padding tile (uniform over the workgroup, before any barrier)
  const int64_t n_ct = gficf_ceil_div(N, KNN_TC);
  const int64_t ct0 = PRUNE ? 0 : n_ct * sp / S, ct1 = PRUNE ? n_ct : n_ct * (sp + 1) / S;
  const int nq4 = dpad >> 2;                         // float4 per point row
  const int nch = (d + KNN_DK - 1) / KNN_DK;         // chunks per candidate tile (padded dims are skipped)
  const float4* const X4 = reinterpret_cast<const float4*>(A.X);
  const float4* const Q4 = reinterpret_cast<const float4*>(A.Q);

  if (!REGL)
    for (int e = tid; e < TQ * KL; e += KNN_THREADS) sKey[e] = ~0ull;
  u64 lst[RQ][REGL ? EPL : 1];                       // REGL: this lane's entries of its rows' lists
#pragma unroll
  for (int r = 0; r < RQ; ++r)
#pragma unroll
    for (int h = 0; h < (REGL ? EPL : 1); ++h) lst[r][h] = ~0ull;
  // query tile -> sA[dim][query]; consecutive lanes take consecutive queries (conflict-free LDS writes)
  for (int f = tid; f < TQ * nq4; f += KNN_THREADS) {
    const int row = f & (TQ - 1), quad = f / TQ;
    const int64_t q = q0 + row;
    const float4 v = q < A.n_q ? Q4[q * nq4 + quad] : make_float4(0.f, 0.f, 0.f, 0.f);
    float* o = sA + (size_t)(quad * 4) * TQ + row;
    o[0] = v.x; o[TQ] = v.y; o[2 * TQ] = v.z; o[3 * TQ] = v.w;
  }
  if (PRUNE) {
    for (int64_t e = tid; e < n_ct; e += KNN_THREADS) sLb[e] = A.lb[(int64_t)qt * n_ct + e];
    if (tid < 2 * (KNN_THREADS / 64)) s_wtau[tid / (KNN_THREADS / 64)][tid % (KNN_THREADS / 64)] = INFINITY;
  }

  // Staging of a candidate tile's dim chunk: 128 points x 16 dims = 512 float4, two per thread (point row_l,
  // float4 columns quad0 and quad0 + 2 of the chunk); consecutive lanes take consecutive points, so the
  // transposing LDS writes are conflict-free.
  const int row_l = tid & (KNN_TC - 1), quad0 = tid >> 7;
  float* const st0 = sB + (size_t)(quad0 * 4) * KNN_TC + row_l;             // LDS destination inside a buffer
  auto load_chunk = [&](int64_t ct, int c, float4 (&v)[2]) {
    const int64_t j = ct * KNN_TC + row_l;
    const int q4 = c * (KNN_DK / 4) + quad0;
    const float4* src = X4 + j * nq4 + q4;
    v[0] = (j < N && q4 < nq4) ? src[0] : make_float4(0.f, 0.f, 0.f, 0.f);
    v[1] = (j < N && q4 + 2 < nq4) ? src[2] : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store_chunk = [&](int buf, const float4 (&v)[2]) {
    float* o = st0 + (size_t)buf * KNN_DK * KNN_TC;
    o[0] = v[0].x; o[KNN_TC] = v[0].y; o[2 * KNN_TC] = v[0].z; o[3 * KNN_TC] = v[0].w;
    o += 8 * KNN_TC;
    o[0] = v[1].x; o[KNN_TC] = v[1].y; o[2 * KNN_TC] = v[1].z; o[3 * KNN_TC] = v[1].w;
  };
  // PRUNE: the unvisited tile with the smallest bound, or -1 when that bound is beyond every query's k-th best.
  // `skip` is the tile in work (its visited mark may not be visible to every wave yet); `par` selects the
  // published k-th best maxima of the tile before it.
  auto select_tile = [&](int64_t skip, int par) -> int64_t {
    float best = INFINITY;
    int bi = -1;
    for (int e = lane; e < (int)n_ct; e += 64) {
      const float v = sLb[e];
      if (e != (int)skip && v < best) { best = v; bi = e; }      // ascending e: the lowest index wins a tie
    }
#pragma unroll
    for (int w = 32; w >= 1; w >>= 1) {
      const float ov = __shfl_xor(best, w);
      const int oi = __shfl_xor(bi, w);
      if (ov < best || (ov == best && oi >= 0 && (bi < 0 || oi < bi))) { best = ov; bi = oi; }
    }
    float tmax = s_wtau[par][0];
#pragma unroll
    for (int w = 1; w < KNN_THREADS / 64; ++w) tmax = fmaxf(tmax, s_wtau[par][w]);
    return (bi >= 0 && best <= tmax) ? (int64_t)bi : -1;
  };

  knn_f2 acc[RQ][4];
#pragma unroll
  for (int r = 0; r < RQ; ++r)
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[r][s] = knn_f2{0.0f, 0.0f};

  float tau[RQ];                // current k-th best distance of this thread's query rows
#pragma unroll
  for (int r = 0; r < RQ; ++r) tau[r] = INFINITY;

  __syncthreads();              // sLb / s_wtau / sA are in place
  int64_t cur = PRUNE ? select_tile(-1, 0) : (ct0 < ct1 ? ct0 : -1);
  float4 pre[2];
  if (cur >= 0) { load_chunk(cur, 0, pre); store_chunk(0, pre); }
  __syncthreads();

  int buf = 0, tile_no = 0;
  while (cur >= 0) {
    if (PRUNE && tid == 0) sLb[cur] = INFINITY;              // visited; read by select_tile only after a later barrier
    int64_t nxt = -1;
    for (int c = 0; c < nch; ++c) {
      bool have_next;
      if (c + 1 < nch) {
        load_chunk(cur, c + 1, pre);
        have_next = true;
      } else {
        nxt = PRUNE ? select_tile(cur, (tile_no + 1) & 1) : (cur + 1 < ct1 ? cur + 1 : -1);
        have_next = nxt >= 0;
        if (have_next) load_chunk(nxt, 0, pre);
      }
      const float* const pa = sA + (size_t)(c * KNN_DK) * TQ + ty * 4;
      const float* const pb = sB + (size_t)buf * KNN_DK * KNN_TC + tx * 4;
      const int nd = d - c * KNN_DK < KNN_DK ? d - c * KNN_DK : KNN_DK;
      {
        // Two dims per round (the point rows are zero padded to a multiple of 4 dims, and a zero dim adds exactly 0
        // to every metric's accumulator, so an odd d costs one padded dim).  The operands of the next dim are read
        // from LDS while the current one is accumulated.  One rolled loop for full and short chunks alike: the
        // accumulators never change registers.
        const int np = (nd + 1) >> 1;
        KnnOperands oa, ob;
        knn_read<RQ>(oa, pa, pb);
#pragma unroll 1       // measured: unroll 2 duplicates the body with a remainder copy and runs 45 % slower
        for (int t = 0; t < np; ++t) {
          knn_read<RQ>(ob, pa + (2 * t + 1) * TQ, pb + (2 * t + 1) * KNN_TC);
          knn_dim<METRIC, RQ>(acc, oa);
          if (t + 1 < np) knn_read<RQ>(oa, pa + (2 * t + 2) * TQ, pb + (2 * t + 2) * KNN_TC);
          knn_dim<METRIC, RQ>(acc, ob);
        }
      }
      if (c == nch - 1) {
        // the tile's distances of this thread against the current k-th best of their queries
        const int64_t j0 = cur * KNN_TC;
        // Only the data set's last candidate tile can hold fewer than TC points; it gets its own copy of the
        // code below (RAG), so that all the other tiles do not pay for the masking.
        const int nvalid = (PRUNE && A.tile_n) ? A.tile_n[cur] : (N - j0 < KNN_TC ? (int)(N - j0) : KNN_TC);
        auto epilogue = [&](auto rag_tag) {
          constexpr bool RAG = decltype(rag_tag)::value;      // RAG: candidates at columns >= nvalid do not exist
#pragma unroll
          for (int r = 0; r < RQ; ++r) {
            const int row = (r < 4 ? 0 : 64) + ty * 4 + (r & 3);
            const bool live = row < nq_live;
            // common case after the first tiles: nothing in the whole wave beats its query's k-th best
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
                // Insertions (rare once the lists have warmed up).  The 16 lanes of a 16-lane group share this row
                // (= this list).  The wave loops (uniformly) while any lane holds a candidate; per round the lowest
                // such lane of each group hands one key to its group, whose lanes shift it into their registers.
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
                    khi = f32_sortable(h);
                    klo = (uint32_t)j0 + (uint32_t)((s < 4 ? 0 : 64) + tx * 4 + (s & 3));
                    if (PRUNE) klo = (uint32_t)A.perm_x[klo];   // the key carries the point's original id
                  }
                  const int src = ((tid & 48) | (leader & 15)) << 2;
                  khi = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)khi);
                  klo = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)klo);
                  if (leader >= 0) {
                    knn_reg_insert<REGL ? EPL : 1>(lst[r], ((u64)khi << 32) | (u64)klo);
                    {
                    // the list's k-th best may just have dropped: candidates it no longer admits need no round of their own
                    // (near tiles — the pruned form's, the pivot assignment's — pass most of their candidates by the stale bound)
                    uint32_t tn = (uint32_t)(lst[r][0] >> 32);
#pragma unroll
                    for (int h = 1; h < (REGL ? EPL : 1); ++h) tn = ((kk - 1) % EPL) == h ? (uint32_t)(lst[r][h] >> 32) : tn;
                    tn = (uint32_t)__shfl((int)tn, (kk - 1) / EPL, 16);
                    if (tn != 0xFFFFFFFFu && pass != 0) {
                      const float tnew = sortable_f32(tn);
                      uint32_t keep = 0;
#pragma unroll
                      for (int s = 0; s < 8; ++s) keep |= (dv[s] <= tnew) ? 1u << s : 0u;
                      pass &= keep;
                    }
                    }
                  }
                }
                // the row's k-th best: entry kk - 1 sits in lane (kk - 1) / EPL of the group
                uint32_t th = (uint32_t)(lst[r][0] >> 32);
#pragma unroll
                for (int h = 1; h < (REGL ? EPL : 1); ++h) th = ((kk - 1) % EPL) == h ? (uint32_t)(lst[r][h] >> 32) : th;
                th = (uint32_t)__shfl((int)th, (kk - 1) / EPL, 16);
                tau[r] = th == 0xFFFFFFFFu ? INFINITY : sortable_f32(th);      // list not full yet: everything enters
              } else {
                tau[r] = knn_row_insert<KL>(key_addr + (uint32_t)(row * KL * 8), kk, dv[0], dv[1], dv[2], dv[3], dv[4], dv[5], dv[6],
                                            dv[7], tau[r], live, (uint32_t)j0, tid, PRUNE ? A.perm_x : (const int32_t*)nullptr);
              }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[r][s] = knn_f2{0.0f, 0.0f};
          }
        };
        if (nvalid < KNN_TC) epilogue(std::true_type{});
        else epilogue(std::false_type{});
        if (PRUNE) {
          // this wave's largest k-th best (rows without a query do not count; an unfilled list is +inf).  From 0, never below: cosine
          // k-th bests can round below 0 while k_knn_lb clamps the bounds at 0 — tiles with bound 0 have to stay in reach
          float tm = 0.0f;
#pragma unroll
          for (int r = 0; r < RQ; ++r)
            if ((r < 4 ? 0 : 64) + ty * 4 + (r & 3) < nq_live) tm = fmaxf(tm, tau[r]);
          tm = fmaxf(tm, __shfl_xor(tm, 16));
          tm = fmaxf(tm, __shfl_xor(tm, 32));
          if (lane == 0) s_wtau[tile_no & 1][wave] = tm;
        }
      }
      if (have_next) store_chunk(buf ^ 1, pre);
      __syncthreads();
      buf ^= 1;
    }
    cur = nxt;
    ++tile_no;
  }

  // partial lists of this candidate slice
  if (REGL) {
#pragma unroll
    for (int r = 0; r < RQ; ++r) {
      const int64_t q = q0 + (r < 4 ? 0 : 64) + ty * 4 + (r & 3);
#pragma unroll
      for (int h = 0; h < (REGL ? EPL : 1); ++h) {
        const int e = EPL * tx + h;
        if (q < A.n_q && e < kk) A.part[(q * S + sp) * kk + e] = lst[r][h];
      }
    }
  } else {
    for (int e = tid; e < TQ * kk; e += KNN_THREADS) {
      const int row = e / kk, t = e % kk;
      const int64_t q = q0 + row;
      if (q < A.n_q) A.part[(q * S + sp) * kk + t] = sKey[row * KL + t];
    }
  }
}

// LDS: the query tile, the two candidate chunks, beyond k = 64 the lists and, pruned, the bounds of the query tile: at d = 128,
// k = 128 that is 32 + 16 + 64 KiB = 112 KiB, one workgroup per CU of 160 KiB; up to k = 64 the plain form takes at most 48 KiB
// and the two workgroups of the launch bound fit.
template <int METRIC, int KL, bool PRUNE>
int knn_launch(gficf_ctx* ctx, const KnnTileArgs& a) {
  const int64_t n_ct = gficf_ceil_div(a.N, KNN_TC);
  const size_t lds = (size_t)a.dpad * KNN_TQ * 4 + 2 * KNN_DK * KNN_TC * 4 + (KL > 64 ? (size_t)KNN_TQ * KL * 8 : 0) + (PRUNE ? (size_t)n_ct * 4 : 0);
  static std::atomic<bool> attr_set[64];
  if (!attr_set[ctx->device & 63]) {
    GFICF_HIP_CHECK(hipFuncSetAttribute((const void*)k_knn_tiles<METRIC, KL, KNN_RQ, PRUNE>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 64));
    attr_set[ctx->device & 63] = true;
  }
  const int64_t blocks = gficf_ceil_div(a.n_q, KNN_TQ) * a.S;
  hipLaunchKernelGGL((k_knn_tiles<METRIC, KL, KNN_RQ, PRUNE>), dim3((unsigned)blocks), dim3(KNN_THREADS), lds, ctx->stream, a);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

template <int METRIC, bool PRUNE>
int knn_launch_k(gficf_ctx* ctx, const KnnTileArgs& a) {
  if (a.kk <= 32) return knn_launch<METRIC, 32, PRUNE>(ctx, a);
  if (a.kk <= 64) return knn_launch<METRIC, 64, PRUNE>(ctx, a);
  return knn_launch<METRIC, 128, PRUNE>(ctx, a);
}

// metric: manhattan, euclidean or cosine (correlation is cosine over centred rows: gficf_knn_search_metric, common.h)
template <bool PRUNE>
int knn_launch_m(gficf_ctx* ctx, int metric, const KnnTileArgs& a) {
  switch (metric) {
    case GFICF_KNN_MANHATTAN: return knn_launch_k<GFICF_KNN_MANHATTAN, PRUNE>(ctx, a);
    case GFICF_KNN_EUCLIDEAN: return knn_launch_k<GFICF_KNN_EUCLIDEAN, PRUNE>(ctx, a);
    default: return knn_launch_k<GFICF_KNN_COSINE, PRUNE>(ctx, a);
  }
}

}  // namespace
