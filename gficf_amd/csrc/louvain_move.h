// louvain_move.h — local moving of louvain.hip: an iteration's snapshot and sum of squares (k_lv_pre), the move kernels of the three
// degree classes, the device's decision (k_lv_decide) and the sub-round's apply.
#pragma once

#include "louvain_shared.h"

namespace {

// Start of an iteration: the sum of the squared community totals of every running component, in a fixed order (LV_SQ_BLOCKS slices
// of its communities, a fixed tree inside each, the slices added up in slice order by k_lv_decide), and a copy of the totals and sizes
// as they are now (parity = iteration & 1): what an undo of the NEXT iteration's moves goes back to.
__global__ __launch_bounds__(256) void k_lv_pre(const LvCtl* __restrict__ ctl, int parity, const u64* __restrict__ K, const int32_t* __restrict__ size,
                                                u64* __restrict__ snapK, int32_t* __restrict__ snapS, double* __restrict__ part_sq) {
  __shared__ double s_p[256];
  const int b = blockIdx.y;
  const LvComp& C = ctl->c[b];
  if (C.level_done) return;
  (void)parity;
  const int64_t per = (C.n + LV_SQ_BLOCKS - 1) / LV_SQ_BLOCKS;
  const int64_t lo = C.v0 + (int64_t)blockIdx.x * per, hi = lo + per < C.v0 + C.n ? lo + per : C.v0 + C.n;
  double s = 0.0;
  for (int64_t c = lo + threadIdx.x; c < hi; c += 256) {
    const u64 kc = K[c];
    snapK[c] = kc; snapS[c] = size[c];
    const double k = (double)kc;
    s += k * k;
  }
  s_p[threadIdx.x] = s;
  __syncthreads();
  for (int d = 128; d > 0; d >>= 1) {
    if ((int)threadIdx.x < d) s_p[threadIdx.x] += s_p[threadIdx.x + d];
    __syncthreads();
  }
  if (threadIdx.x == 0) part_sq[b * LV_SQ_BLOCKS + blockIdx.x] = s_p[0];
}

// One wave per vertex (at most LV_SMALL_DEG entries, two per lane, loaded ONCE and evaluated for every copy of the graph).  The wave's
// table is cleared once: the lane that claims a slot ("owner") evaluates that community and hands the slot back empty.
// A vertex of at most 64 entries (one per lane) takes TWO copies per round: the entries go into the table once with copy b's communities and
// once with copy b + 1's — the community ids of two copies never meet — and the two evaluations overlap their latencies.
// The entries INSIDE the vertex's own community — in a settled partition most of the row — never go through the table: they are added up in
// an LDS cell of their own (one instruction; the kernel is bound by VALU issue, ~130 instructions per evaluation before this form, and the
// LDS pipe idles), which is the staying side of the decision and, FIRST (sub-round 0), the vertex's share of the internal weight of the
// labels this kernel reads, i.e. of the previous iteration's result (k_lv_decide turns it into Q).
// Lane l < 16 carries component l's state for the whole kernel (read with v_readlane: no control-block loads in the loop).
// Tried on one box, variants interleaved, and dropped (profiles/r06_louvain_ab.txt): the copies as the OUTER loop, two at a time over all
// vertices, so that what is gathered for them stays in L2 (the early iterations miss L2 35 % of the time, ~1 GB of fabric traffic a sub-round)
// — 11.1 ms against 10.4 at the config-3 shape with ten starts: re-reading the rows per pair costs more than the misses; the copies
// INTERLEAVED in the state arrays: more misses, not fewer; both entries probing in one wave-uniform loop instead of two per-lane loops: no change.
template <bool FIRST>
__global__ __launch_bounds__(256, 6) void k_lv_move_small(LvG g, const LvCtl* __restrict__ ctl, LvMove mv, const int32_t* __restrict__ comm,
                                                       const u64* __restrict__ K, const int32_t* __restrict__ size, int32_t* __restrict__ next,
                                                       const int32_t* __restrict__ mark_r, int32_t* __restrict__ mark_w, u64* __restrict__ iw,
                                                       u64* __restrict__ part_in, unsigned* __restrict__ part_mv) {
  __shared__ int32_t s_key[4][LV_SMALL_SLOTS];
  __shared__ u64 s_val[4][LV_SMALL_SLOTS];
  __shared__ u64 s_stay[4][2];
  __shared__ u64 s_acc[4][LV_MAX_B];
  __shared__ unsigned s_cnt[4][LV_MAX_B];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int32_t* key = s_key[wave];
  u64* val = s_val[wave];
  u64* cell = s_stay[wave];
  // the table belongs to this wave alone and LDS serves a wave's operations in issue order: a wave-level fence (no
  // workgroup barrier) is all that separates clearing, filling and reading it
  for (int t = lane; t < LV_SMALL_SLOTS; t += 64) { key[t] = -1; val[t] = 0ull; }
  if (lane < 2) cell[lane] = 0ull;
  int st_run = 0, st_S = 1;
  uint32_t st_off = 0;       // seed - v0: the class of union vertex gv is that of hash(gv + st_off)
  if (lane < LV_MAX_B) {
    const LvComp& C = ctl->c[lane];
    st_run = lv_runs(C, mv.s, FIRST) ? 1 : 0;
    st_S = C.S;
    st_off = C.seed - (uint32_t)C.v0;
  }
  GFICF_WAVE_SYNC();
  u64 acc = 0;               // lane b: internal weight summed for component b
  unsigned cnt = 0;          // lane b: vertices of component b that move
  // Look-ahead (round 6, late): the lanes first look at the wave's next 64 / P vertices at once — lane (j, b) at copy b of the j-th of them, P = the
  // copies rounded up to a power of two — and the wave then works through the vertices that have a copy to look at.  Before, a wave found out
  // vertex by vertex (row loaded, then one stamp per pair of copies, each load behind the last): 31 us a launch at 10 x 54 k vertices with NOTHING
  // to do, which is what the last ten iterations of a level are (a few hundred vertices still moving) — 3 - 5 us now.
  const int P = g.rep <= 1 ? 1 : g.rep <= 2 ? 2 : g.rep <= 4 ? 4 : g.rep <= 8 ? 8 : 16;
  const int la_j = lane / P, la_b = lane % P;
  const int64_t v_stride = (int64_t)gridDim.x * 4;
  for (int64_t vb = (int64_t)blockIdx.x * 4 + wave; vb < g.nb; vb += v_stride * (64 / P)) {
   u64 la_mask;
   {
    const int64_t vj = vb + (int64_t)la_j * v_stride;
    const bool there = la_b < g.rep && vj < g.nb;
    const int comp = there ? (g.vcomp ? (int)g.vcomp[vj] : la_b) : 0;
    const int run = __shfl(st_run, comp), S = __shfl(st_S, comp);           // (every lane takes part: the state sits in lanes 0 .. 15)
    const uint32_t off = (uint32_t)__shfl((int)st_off, comp);
    bool act = false;
    if (there && run) {
      const uint32_t gv = (uint32_t)((int64_t)la_b * g.nb + vj);
      const bool in_class = S == 1 || lv_class(gv + off, S) == mv.s;
      act = (in_class || FIRST) && mark_r[gv] >= mv.thr;
    }
    la_mask = __ballot(act);
   }
   while (la_mask) {                               // uniform over the wave
    const int jj = __builtin_ctzll(la_mask) / P;
    const unsigned look = (unsigned)((la_mask >> (jj * P)) & ((1ull << P) - 1ull));      // bit b: copy b of this vertex is looked at
    la_mask &= ~(((1ull << P) - 1ull) << (jj * P));
    const int64_t v = vb + (int64_t)jj * v_stride;
    const int64_t lo = g.beg[v], hi = g.end[v];
    if (hi - lo > LV_SMALL_DEG) continue;
    const int64_t e0 = lo + lane, e1 = e0 + 64;
    int32_t u0 = -1, u1 = -1;
    u64 w0 = 0, w1 = 0;
    if (e0 < hi) { u0 = g.nbr[e0]; w0 = g.wt[e0]; if (u0 == v) u0 = -1; }
    if (e1 < hi) { u1 = g.nbr[e1]; w1 = g.wt[e1]; if (u1 == v) u1 = -1; }
    const u64 kvv = g.kv[v];
    const double kvd = (double)kvv;
    const int comp0 = g.vcomp ? (int)g.vcomp[v] : 0;
    const bool pair = g.rep > 1 && hi - lo <= 64;
    for (int b = 0; b < g.rep; b += pair ? 2 : 1) {
      // side A: copy b (a coarse level: the vertex's component); side B: copy b + 1 in a pair round
      const int compA = g.vcomp ? comp0 : b, compB = b + 1;
      const uint32_t gvA = (uint32_t)(b * g.nb + v), gvB = gvA + (uint32_t)g.nb;
      int modeA = 0, modeB = 0;      // 0: not in this round, 1: only its share of the internal weight (sub-round 0, other class), 2: evaluate
      if (__builtin_amdgcn_readlane(st_run, compA)) {
        const int S = __builtin_amdgcn_readlane(st_S, compA);
        const bool in_class = S == 1 || lv_class(gvA + (uint32_t)__builtin_amdgcn_readlane((int)st_off, compA), S) == mv.s;
        modeA = in_class ? 2 : FIRST ? 1 : 0;
      }
      if (pair && compB < g.rep && __builtin_amdgcn_readlane(st_run, compB)) {
        const int S = __builtin_amdgcn_readlane(st_S, compB);
        const bool in_class = S == 1 || lv_class(gvB + (uint32_t)__builtin_amdgcn_readlane((int)st_off, compB), S) == mv.s;
        modeB = in_class ? 2 : FIRST ? 1 : 0;
      }
      // looked at only when it or a neighbour has moved since it was last looked at (the stamps this kernel reads were merged before it began;
      // read by the look-ahead above)
      if (modeA && !((look >> b) & 1u)) modeA = 0;
      if (modeB && !((look >> (b + 1)) & 1u)) modeB = 0;
      if (!modeA && !modeB) continue;
      const uint32_t baseA = gvA - (uint32_t)v, baseB = gvB - (uint32_t)v;
      // this lane's entries: (cx, wx) belongs to side A, (cy, wy) to side B in a pair round and to side A otherwise
      int32_t cvA = 0, cvB = 0, cx = -1, cy = -1;
      if (modeA) { cvA = comm[gvA]; if (u0 >= 0) cx = comm[baseA + (uint32_t)u0]; }
      if (pair) { if (modeB) { cvB = comm[gvB]; if (u0 >= 0) cy = comm[baseB + (uint32_t)u0]; } }
      else if (modeA && u1 >= 0) cy = comm[baseA + (uint32_t)u1];
      const u64 wx = w0, wy = pair ? w0 : w1;
      const int32_t cvy = pair ? cvB : cvA;
      const bool evA = modeA == 2, evB = modeB == 2, evY = pair ? evB : evA;
      const bool inx = cx >= 0 && cx == cvA, iny = cy >= 0 && cy == cvy;
      // totals and sizes the decisions need, on their way while the table is filled
      u64 Kx = 0, Ky = 0, KcvA = 0, KcvB = 0;
      int32_t szA = 0, szgA = 0, szB = 0, szgB = 0;
      if (evA) { KcvA = K[cvA]; szA = size[cvA]; szgA = size[gvA]; if (cx >= 0 && !inx) Kx = K[cx]; }
      if (evB) { KcvB = K[cvB]; szB = size[cvB]; szgB = size[gvB]; }
      if (evY && cy >= 0 && !iny) Ky = K[cy];
      if (inx) atomicAdd(&cell[0], wx);
      if (iny) atomicAdd(&cell[pair ? 1 : 0], wy);
      // Both entries go into the table together: the first probes back to back (one LDS round trip for the two), and a loop that the WAVE
      // leaves as soon as no lane is still probing (a scalar branch on a ballot; the per-lane probe loops this replaces were unrolled
      // into ~10 exec-mask instructions per probe and waited for every round trip twice).  At most 128 entries in 256 slots: it ends.
      int slotx = -1, sloty = -1;
      bool ownx = false, owny = false;
      if (evA && cx >= 0 && !inx) slotx = gficf_comm_insert<LV_SMALL_SLOTS>(key, val, cx, wx, &ownx);
      if (evY && cy >= 0 && !iny) sloty = gficf_comm_insert<LV_SMALL_SLOTS>(key, val, cy, wy, &owny);
      GFICF_WAVE_SYNC();
      const u64 stayA = cell[0], stayB = cell[1];
      LvBest ba{-INFINITY, INT32_MAX}, bb{-INFINITY, INT32_MAX};
      if (ownx) {
        ba.g = (double)val[slotx] - kvd * (double)Kx * mv.r; ba.c = cx;
        key[slotx] = -1; val[slotx] = 0ull;
      }
      if (owny) {
        LvBest& t = pair ? bb : ba;
        const double gain = (double)val[sloty] - kvd * (double)Ky * mv.r;
        if (lv_better(gain, cy, t.g, t.c)) { t.g = gain; t.c = cy; }
        key[sloty] = -1; val[sloty] = 0ull;
      }
      if (evA) ba = lv_wave_best(ba);
      if (evB) bb = lv_wave_best(bb);
      GFICF_WAVE_SYNC();                            // every lane has read the cells and the slots: they are emptied before the next round fills them
      if (lane < 2) cell[lane] = 0ull;
      if (modeA) {
        if (FIRST) {                             // the change of its share of the internal weight since it was last looked at
          const u64 was = iw[gvA];
          if (lane == 0) iw[gvA] = stayA;
          if (lane == compA) acc += stayA - was;
        }
        if (evA) {
          bool moved;
          const int32_t to = lv_decide_vertex((int64_t)gvA, cvA, ba.g, ba.c, stayA, kvv, mv.r, KcvA, szA, szgA, size, &moved);
          if (lane == 0) next[gvA] = to;
          if (lane == compA) cnt += moved ? 1u : 0u;
          if (moved) {                           // it and its neighbours are looked at again
            if (lane == 0) mark_w[gvA] = mv.epoch;
            if (u0 >= 0) mark_w[baseA + (uint32_t)u0] = mv.epoch;
            if (!pair && u1 >= 0) mark_w[baseA + (uint32_t)u1] = mv.epoch;
          }
        }
      }
      if (modeB) {
        if (FIRST) {
          const u64 was = iw[gvB];
          if (lane == 0) iw[gvB] = stayB;
          if (lane == compB) acc += stayB - was;
        }
        if (evB) {
          bool moved;
          const int32_t to = lv_decide_vertex((int64_t)gvB, cvB, bb.g, bb.c, stayB, kvv, mv.r, KcvB, szB, szgB, size, &moved);
          if (lane == 0) next[gvB] = to;
          if (lane == compB) cnt += moved ? 1u : 0u;
          if (moved) {
            if (lane == 0) mark_w[gvB] = mv.epoch;
            if (u0 >= 0) mark_w[baseB + (uint32_t)u0] = mv.epoch;
          }
        }
      }
    }
   }
  }
  if (lane < LV_MAX_B) { s_acc[wave][lane] = acc; s_cnt[wave][lane] = cnt; }
  __syncthreads();
  if (threadIdx.x < LV_MAX_B) {
    const int t = threadIdx.x;
    const unsigned c = s_cnt[0][t] + s_cnt[1][t] + s_cnt[2][t] + s_cnt[3][t];
    const size_t at = (size_t)blockIdx.x * LV_MAX_B + t;
    if (FIRST) { part_in[at] = s_acc[0][t] + s_acc[1][t] + s_acc[2][t] + s_acc[3][t]; part_mv[at] = c; }
    else part_mv[at] += c;                      // the same grid in every sub-round of the iteration: the slot is this block's
  }
}

// One wave per listed vertex and copy (LV_SMALL_DEG < entries <= LV_MID_DEG; workgroups of two waves, a 1024-slot table and a list of the
// claimed slots each).  The entries stream through in chunks of 64; up to 512 of them in one pass, beyond that in P passes, pass p taking the
// communities of hash class p.  Nothing is cleared or scanned: the claimed slots are listed, evaluated from the list and handed back empty.
template <bool FIRST>
__global__ __launch_bounds__(128) void k_lv_move_mid(LvG g, const LvCtl* __restrict__ ctl, LvMove mv, int64_t n_list, const int32_t* __restrict__ list,
                                                     const int32_t* __restrict__ comm, const u64* __restrict__ K, const int32_t* __restrict__ size,
                                                     int32_t* __restrict__ next, const int32_t* __restrict__ mark_r, int32_t* __restrict__ mark_w,
                                                     u64* __restrict__ iw, u64* __restrict__ part_in, unsigned* __restrict__ part_mv,
                                                     uint32_t* __restrict__ status) {
  __shared__ int32_t s_key[2][LV_MID_SLOTS];
  __shared__ u64 s_val[2][LV_MID_SLOTS];
  __shared__ uint16_t s_list[2][LV_MID_SLOTS];
  __shared__ u64 s_acc[2][LV_MAX_B];
  __shared__ unsigned s_cnt[2][LV_MAX_B];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int32_t* key = s_key[wave];
  u64* val = s_val[wave];
  uint16_t* claimed = s_list[wave];
  for (int t = lane; t < LV_MID_SLOTS; t += 64) { key[t] = -1; val[t] = 0ull; }
  GFICF_WAVE_SYNC();
  const u64 lt = (1ull << lane) - 1ull;
  u64 acc = 0;
  unsigned cnt = 0;
  for (int64_t item = (int64_t)blockIdx.x * 2 + wave; item < n_list * g.rep; item += (int64_t)gridDim.x * 2) {
    const int b = (int)(item / n_list);
    const int64_t v = list[item - (int64_t)b * n_list];
    const LvSide A = lv_side<FIRST>(g, ctl, mv.s, b, v, comm, K, size);
    if (!A.mode || mark_r[A.gv] < mv.thr) continue;          // (pruning: see LvMove)
    const int64_t lo = g.beg[v], hi = g.end[v];
    if (FIRST && A.mode == 1) {
      u64 t = 0;
      for (int64_t e = lo + lane; e < hi; e += 64) {
        const int32_t u = g.nbr[e];
        if (u != v && comm[A.base + u] == A.cv) t += g.wt[e];
      }
      t = lv_wave_sum(t);
      const u64 was = iw[A.gv];
      if (lane == 0) iw[A.gv] = t;
      if (lane == A.comp) acc += t - was;
      continue;
    }
    const u64 kvv = g.kv[v];
    const double kvd = (double)kvv;
    LvBest best{-INFINITY, INT32_MAX};
    u64 stay = 0;                                  // this lane's entries inside the vertex's own community (never through the table: see k_lv_move_small)
    const uint32_t P = (uint32_t)((hi - lo + LV_MID_SLOTS / 2 - 1) / (LV_MID_SLOTS / 2));
    for (uint32_t p = 0; p < (P ? P : 1u); ++p) {
      int n_claimed = 0;
      // four chunks of 64 entries a step: their neighbour ids, then their communities, are loaded together (a chunk at a time every step waited
      // for two dependent round trips, three to eight times a row); every lane stays in the loop: the ballots below are the whole wave's
      for (int64_t e = lo + lane; e - lane < hi; e += 256) {
        int32_t uu[4] = {-1, -1, -1, -1}, cc[4] = {-1, -1, -1, -1};
        u64 ww[4] = {0ull, 0ull, 0ull, 0ull};
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if (e + 64 * h < hi) { uu[h] = g.nbr[e + 64 * h]; ww[h] = g.wt[e + 64 * h]; }
#pragma unroll
        for (int h = 0; h < 4; ++h)
          if (uu[h] >= 0 && uu[h] != v) cc[h] = comm[A.base + uu[h]];
#pragma unroll
        for (int h = 0; h < 4; ++h) {
          if (e - lane + 64 * h >= hi) break;                          // uniform: the row ended with an earlier chunk
          bool own = false;
          int slot = -1;
          const int32_t c = cc[h];
          if (c >= 0) {
            if (c == A.cv) { if (p == 0) stay += ww[h]; }
            else if (P <= 1 || (gficf_comm_hash((uint32_t)c) >> 13) % P == p) {
              slot = gficf_comm_insert<LV_MID_SLOTS>(key, val, c, ww[h], &own);
              if (slot < 0) atomicOr(status, GFICF_ST_TOO_DENSE);     // a hash class that overflows the table
            }
          }
          const u64 m = __ballot(own);
          if (own) claimed[n_claimed + __popcll(m & lt)] = (uint16_t)slot;
          n_claimed += __popcll(m);
        }
      }
      GFICF_WAVE_SYNC();
      for (int i = lane; i < n_claimed; i += 64) {
        const int slot = claimed[i];
        const int32_t c = key[slot];
        const double gain = (double)val[slot] - kvd * (double)K[c] * mv.r;
        key[slot] = -1; val[slot] = 0ull;
        if (lv_better(gain, c, best.g, best.c)) { best.g = gain; best.c = c; }
      }
      GFICF_WAVE_SYNC();
    }
    best = lv_wave_best(best);
    stay = lv_wave_sum(stay);
    bool moved;
    const int32_t to = lv_decide_vertex(A.gv, A.cv, best.g, best.c, stay, kvv, mv.r, A.Kcv, A.szcv, A.szgv, size, &moved);
    if (lane == 0) next[A.gv] = to;
    if (FIRST) {
      const u64 was = iw[A.gv];
      if (lane == 0) iw[A.gv] = stay;
      if (lane == A.comp) acc += stay - was;
    }
    if (lane == A.comp) cnt += moved ? 1u : 0u;
    if (moved) {
      if (lane == 0) mark_w[A.gv] = mv.epoch;
      for (int64_t e = lo + lane; e < hi; e += 64) mark_w[A.base + g.nbr[e]] = mv.epoch;
    }
  }
  if (lane < LV_MAX_B) { s_acc[wave][lane] = acc; s_cnt[wave][lane] = cnt; }
  __syncthreads();
  if (threadIdx.x < LV_MAX_B) {
    const int t = threadIdx.x;
    const size_t at = (size_t)blockIdx.x * LV_MAX_B + t;
    if (FIRST) { part_in[at] = s_acc[0][t] + s_acc[1][t]; part_mv[at] = s_cnt[0][t] + s_cnt[1][t]; }
    else part_mv[at] += s_cnt[0][t] + s_cnt[1][t];
  }
}

// One workgroup per listed vertex and copy (more than LV_MID_DEG entries): an 8192-slot table, P passes over the entries.
template <int SLOTS, bool FIRST>
__global__ __launch_bounds__(256) void k_lv_move_big(LvG g, const LvCtl* __restrict__ ctl, LvMove mv, int large, int64_t n_list, const int32_t* __restrict__ big,
                                                     const int32_t* __restrict__ comm, const u64* __restrict__ K, const int32_t* __restrict__ size,
                                                     int32_t* __restrict__ next, const int32_t* __restrict__ mark_r, int32_t* __restrict__ mark_w,
                                                     u64* __restrict__ iw, u64* __restrict__ part_in, unsigned* __restrict__ part_mv,
                                                     uint32_t* __restrict__ status) {
  extern __shared__ unsigned char s_raw[];
  u64* val = (u64*)s_raw;
  int32_t* key = (int32_t*)(val + SLOTS);
  __shared__ int s_moved;
  __shared__ double s_g[256];
  __shared__ u64 s_w[4], s_in[4];
  __shared__ int32_t s_c[256];
  __shared__ u64 s_acc[LV_MAX_B];
  __shared__ unsigned s_cnt[LV_MAX_B];
  const int tid = threadIdx.x;
  if (tid < LV_MAX_B) { s_acc[tid] = 0ull; s_cnt[tid] = 0u; }
  __syncthreads();
  const int32_t* list = large ? big + (g.nb - n_list) : big;
  for (int64_t item = blockIdx.x; item < n_list * g.rep; item += gridDim.x) {
    const int b = (int)(item / n_list);
    const int64_t v = list[item - (int64_t)b * n_list];
    const int comp = g.vcomp ? (int)g.vcomp[v] : b;
    const LvComp& C = ctl->c[comp];
    if (!lv_runs(C, mv.s, FIRST)) continue;                                       // uniform per workgroup
    const int64_t base = (int64_t)b * g.nb, gv = base + v;
    const bool in_class = C.S == 1 || (int)(gficf_comm_hash((uint32_t)(gv - C.v0) + C.seed) % (uint32_t)C.S) == mv.s;
    if (!FIRST && !in_class) continue;
    if (mark_r[gv] < mv.thr) continue;                                            // (pruning: see LvMove)
    const int64_t lo = g.beg[v], hi = g.end[v];
    const int32_t cv = comm[gv];
    const u64 kvv = g.kv[v];
    if (FIRST && !in_class) {
      u64 t = 0;
      for (int64_t e = lo + tid; e < hi; e += 256) {
        const int32_t u = g.nbr[e];
        if (u != v && comm[base + u] == cv) t += g.wt[e];
      }
      t = lv_wave_sum(t);
      if ((tid & 63) == 0) s_in[tid >> 6] = t;
      __syncthreads();
      if (tid == 0) {
        const u64 now = s_in[0] + s_in[1] + s_in[2] + s_in[3];
        s_acc[comp] += now - iw[gv];
        iw[gv] = now;
      }
      __syncthreads();
      continue;
    }
    const double kvd = (double)kvv;
    double bg = -INFINITY;
    u64 stay_w = 0;
    int32_t bc = INT32_MAX;
    // A vertex with more entries than the table comfortably holds (every entry can be its own community) is done in
    // P passes over its entries, pass p taking the communities of hash class p: about deg / P <= SLOTS / 2 of them at a time.
    const uint32_t P = (uint32_t)((hi - lo + SLOTS / 2 - 1) / (SLOTS / 2));
    for (uint32_t p = 0; p < (P ? P : 1u); ++p) {
      for (int t = tid; t < SLOTS; t += 256) { key[t] = -1; val[t] = 0ull; }
      __syncthreads();
      for (int64_t e = lo + tid; e < hi; e += 256) {
        const int32_t u = g.nbr[e];
        if (u == v) continue;
        const int32_t c = comm[base + u];
        const uint32_t hc = gficf_comm_hash((uint32_t)c);
        if (P > 1 && (hc >> 13) % P != p) continue;
        uint32_t h = hc & (SLOTS - 1);
        int probes = 0;
        for (;;) {
          const int32_t old = atomicCAS(&key[h], -1, c);
          if (old == -1 || old == c) { atomicAdd(&val[h], g.wt[e]); break; }
          h = (h + 1) & (SLOTS - 1);
          if (++probes >= SLOTS) { atomicOr(status, GFICF_ST_TOO_DENSE); break; }   // a hash class that overflows the table
        }
      }
      __syncthreads();
      for (int t = tid; t < SLOTS; t += 256) {
        const int32_t c = key[t];
        if (c < 0) continue;
        const u64 w = val[t];
        if (c == cv) { stay_w = w; continue; }
        const double gain = (double)w - kvd * (double)K[c] * mv.r;
        if (lv_better(gain, c, bg, bc)) { bg = gain; bc = c; }
      }
      __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) { const u64 o = __shfl_xor(stay_w, d); stay_w = o > stay_w ? o : stay_w; }
    if ((tid & 63) == 0) s_w[tid >> 6] = stay_w;
    s_g[tid] = bg; s_c[tid] = bc;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
      if (tid < d && lv_better(s_g[tid + d], s_c[tid + d], s_g[tid], s_c[tid])) { s_g[tid] = s_g[tid + d]; s_c[tid] = s_c[tid + d]; }
      __syncthreads();
    }
    if (tid == 0) {
      bg = s_g[0]; bc = s_c[0];
      stay_w = s_w[0];
      for (int t = 1; t < 4; ++t) stay_w = s_w[t] > stay_w ? s_w[t] : stay_w;
      bool moved;
      next[gv] = lv_decide_vertex(gv, cv, bg, bc, stay_w, kvv, mv.r, K[cv], size[cv], size[gv], size, &moved);
      s_cnt[comp] += moved ? 1u : 0u;
      if (FIRST) { s_acc[comp] += stay_w - iw[gv]; iw[gv] = stay_w; }
      s_moved = moved ? 1 : 0;
      if (moved) mark_w[gv] = mv.epoch;
    }
    __syncthreads();
    if (s_moved)
      for (int64_t e = lo + tid; e < hi; e += 256) mark_w[base + g.nbr[e]] = mv.epoch;
    __syncthreads();
  }
  __syncthreads();
  if (tid < LV_MAX_B) {
    const size_t at = (size_t)blockIdx.x * LV_MAX_B + tid;
    if (FIRST) { part_in[at] = s_acc[tid]; part_mv[at] = s_cnt[tid]; }
    else part_mv[at] += s_cnt[tid];
  }
}

// The decision of iteration `it` for every component (one block).  The partial sums of the sub-round-0 kernels give the internal weight
// of the labels as the iteration found them, i.e. the result of iteration it - 1, and the number of vertices that moved in it:
//   it == 0: Q of the level's starting labels; go on.           moved == 0: the level has converged.
//   Q < Q before: simultaneous moves made it worse -> undo iteration it - 1, the level ends.
//   else accept; a gain below 1e-7 ends the level.              LV_MAX_ITERS iterations: the level ends.
__global__ __launch_bounds__(1024) void k_lv_decide(LvCtl* ctl, LvParts pt, int nb_small, int nb_mid, int nb_large, int it, double two_w, double q_coef,
                                                   LvHost* __restrict__ host) {
  __shared__ u64 s_in[16][LV_MAX_B];
  __shared__ unsigned s_mv[16][LV_MAX_B];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int B = ctl->B;
  const int pv = (it & 1) ^ 1;                   // the moved counts of the iteration before this one
  {
    // element e of a slab = (row e / 16, component e % 16): thread t takes elements t, t + 1024, ... — always component t % 16, coalesced
    u64 a = 0;
    unsigned m = 0;
    // (eight loads in flight per slab and thread: one load behind the other, the 0.5 MB of partial sums took 21 us of a 29-launch critical path)
    auto slab = [&](const u64* __restrict__ in, const unsigned* __restrict__ mvp, int n) {
      for (int e0 = tid; e0 < n; e0 += 8 * 1024) {
        u64 av[8];
        unsigned mv8[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int e = e0 + j * 1024;
          av[j] = e < n ? in[e] : 0ull;
          mv8[j] = (it && e < n) ? mvp[e] : 0u;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) { a += av[j]; m += mv8[j]; }
      }
    };
    slab(pt.in_small, pt.mv_small[pv], nb_small * LV_MAX_B);
    slab(pt.in_mid, pt.mv_mid[pv], nb_mid * LV_MAX_B);
    slab(pt.in_large, pt.mv_large[pv], nb_large * LV_MAX_B);
    for (int d = 32; d >= LV_MAX_B; d >>= 1) { a += __shfl_xor(a, d); m += __shfl_xor(m, d); }      // lanes l, l + 16, l + 32, l + 48 hold component l % 16
    if (lane < LV_MAX_B) { s_in[wave][lane] = a; s_mv[wave][lane] = m; }
  }
  __syncthreads();
  __shared__ int s_cont[LV_MAX_B];
  if (tid < LV_MAX_B) {
    int cont = 0;
    if (tid < B) {
      LvComp& C = ctl->c[tid];
      if (C.level_done) {
        C.action = LV_IDLE;
      } else {
        u64 in_now = C.in_run;                       // + what the sub-round-0 kernels found changed (differences: the sums wrap as they should)
        unsigned moved = 0;
        for (int w = 0; w < 16; ++w) { in_now += s_in[w][tid]; moved += s_mv[w][tid]; }
        C.in_run = in_now;
        double sq = 0.0;
        for (int j = 0; j < LV_SQ_BLOCKS; ++j) sq += pt.sq[tid * LV_SQ_BLOCKS + j];
        const double q = ((double)(in_now + C.self_w)) / two_w - q_coef * sq;          // sq = sum of squared community totals (fixed point)
        int action;
        if (C.iter == 0) { C.q_prev = q; C.in_w = in_now; action = LV_CONTINUE; }
        else if (moved == 0) action = LV_STOP_KEEP;
        else if (q < C.q_prev) action = LV_STOP_UNDO;
        else {
          C.level_moved = 1;
          C.in_w = in_now;
          const bool small_gain = q - C.q_prev < 1e-7;
          C.q_prev = q;
          action = small_gain ? LV_STOP_KEEP : LV_CONTINUE;
        }
        if (action == LV_CONTINUE && C.iter >= LV_MAX_ITERS) action = LV_STOP_KEEP;
        if (action != LV_CONTINUE) C.level_done = 1;
        C.action = action;
        C.iter += 1;
        cont = action == LV_CONTINUE;
        host->q_iter[tid] = q;
        host->mv_iter[tid] = moved;
      }
    }
    s_cont[tid] = cont;
  }
  __syncthreads();
  if (tid == 0) {
    int n = 0;
    for (int b = 0; b < LV_MAX_B; ++b) n += s_cont[b];
    host->n_cont[it] = n;
    __threadfence_system();
  }
}

// Applies the sub-round's moves to the labels, totals and sizes.  Sub-round 0 also carries out the iteration's decision: go on -> keep a
// copy of the labels as they are (what an undo of this iteration's moves goes back to); undo -> the labels, totals and sizes of one
// iteration ago come back.
__global__ __launch_bounds__(256) void k_lv_apply(LvG g, const LvCtl* __restrict__ ctl, int s, int parity, int32_t* __restrict__ comm,
                                                  const int32_t* __restrict__ next, u64* __restrict__ K, int32_t* __restrict__ size,
                                                  int32_t* __restrict__ snapc0, int32_t* __restrict__ snapc1, const u64* __restrict__ snapK_prev,
                                                  const int32_t* __restrict__ snapS_prev, int32_t* __restrict__ mark_r, const int32_t* __restrict__ mark_w) {
  int32_t* const snap_now = parity ? snapc1 : snapc0;
  const int32_t* const snap_prev = parity ? snapc0 : snapc1;
  for (int64_t gv = (int64_t)blockIdx.x * 256 + threadIdx.x; gv < g.n; gv += (int64_t)gridDim.x * 256) {
    const int64_t b = g.rep > 1 ? gv / g.nb : 0;
    const int comp = g.vcomp ? (int)g.vcomp[gv] : (int)b;
    const LvComp& C = ctl->c[comp];
    const int action = C.action;
    if (C.level_done && action == LV_IDLE) continue;
    // the stamps the sub-round's move kernels wrote become readable: those kernels read mark_r and write mark_w only, so what a vertex
    // sees never depends on when a neighbour's store lands
    { const int32_t mw = mark_w[gv]; if (mw > mark_r[gv]) mark_r[gv] = mw; }
    if (s == 0) {
      if (action == LV_CONTINUE) snap_now[gv] = comm[gv];
      else if (action == LV_STOP_UNDO) { comm[gv] = snap_prev[gv]; K[gv] = snapK_prev[gv]; size[gv] = snapS_prev[gv]; }
    }
    if (action != LV_CONTINUE || s >= C.S) continue;
    if (C.S != 1 && (int)(gficf_comm_hash((uint32_t)(gv - C.v0) + C.seed) % (uint32_t)C.S) != s) continue;
    const int32_t a = comm[gv], to = next[gv];
    if (a == to) continue;
    const u64 k = g.kv[gv - b * g.nb];
    atomicAdd(&K[a], 0ull - k);
    atomicAdd(&K[to], k);
    atomicSub(&size[a], 1);
    atomicAdd(&size[to], 1);
    comm[gv] = to;
  }
}

}  // namespace
