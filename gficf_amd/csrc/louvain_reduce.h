// louvain_reduce.h — the end of a level of louvain.hip: the communities in use renumbered by a scan, the labels of the finest
// vertices, and the level's graph reduced by the new ids into the next level's multigraph.
#pragma once

#include "louvain_shared.h"

namespace {

// ---- renumbering
__global__ __launch_bounds__(256) void k_lv_used(int64_t n, const int32_t* __restrict__ size, int64_t* __restrict__ flag) {
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c <= n; c += (int64_t)gridDim.x * 256) flag[c] = c < n && size[c] > 0 ? 1 : 0;
}

// After the scan: every component's first new id and number of communities; does its descent go on?
//   (reference loop: runLouvainAlgorithm recurses while the reduced network is smaller, src/ModularityOptimizer.cpp:594-612)
// refine: a refinement level of algorithm 2 (no descent, the labels are renumbered only).
__global__ void k_lv_ctl_renumbered(LvCtl* ctl, const int64_t* __restrict__ newid, int64_t n_union, int seeded, int refine, int algorithm, int level,
                                    LvHost* __restrict__ host) {
  const int b = threadIdx.x;
  if (b == 0) { ctl->n_union2 = newid[n_union]; host->n_union2 = newid[n_union]; }
  if (b >= LV_MAX_B) return;
  LvComp& C = ctl->c[b];
  C.newbase = newid[C.v0];
  C.n2 = C.live ? newid[C.v0 + C.n] - newid[C.v0] : 0;
  if (C.live) {
    C.q_final = C.q_prev;
    C.n_labels = C.n2;
    if (!refine) {
      C.any_move |= C.level_moved;
      const bool done = C.n2 == C.n || C.n2 <= 1 || (!C.level_moved && !(seeded && C.n2 < C.n));      // nothing merged: the descent is done
      C.cont = done ? 0 : 1;
      if (C.cont) {
        C.self_w += C.in_w;
        if (algorithm == 2 && C.n_saved == level && level < LV_MAX_SAVED) C.saved_n[++C.n_saved] = C.n2;
      }
    }
  } else {
    C.cont = 0;
  }
  host->c[b].n2 = C.n2; host->c[b].q_prev = C.q_prev; host->c[b].cont = C.cont; host->c[b].any_move = C.any_move;
  host->c[b].level_moved = C.level_moved; host->c[b].live = C.live;
}

// lab[b][v] = new LOCAL id (new id - the component's first) of the community of the level's vertex that original vertex v of start b
// maps to: src == NULL -> v itself (level 0), else src[b][v] (a local vertex id of the level; may be lab itself: one read, one write per thread)
__global__ __launch_bounds__(256) void k_lv_relabel(int64_t N, const LvCtl* __restrict__ ctl, const int32_t* src, const int32_t* __restrict__ comm,
                                                    const int64_t* __restrict__ newid, int32_t* lab) {
  const int b = blockIdx.y;
  const LvComp& C = ctl->c[b];
  if (!C.live) return;
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < N; v += (int64_t)gridDim.x * 256) {
    const size_t at = (size_t)b * (size_t)N + (size_t)v;
    const int64_t x = C.v0 + (src ? (int64_t)src[at] : v);
    lab[at] = (int32_t)(newid[comm[x]] - C.newbase);
  }
}

// ---- reduction: the level's graph by the labels newid[comm[.]] -> the next level's (a multigraph in pointerB / pointerE form)
// Row capacities (the entries of a community's members: no row can need more), vertex weights and components of the new vertices.
// cap must be zero.  Few communities: the capacities are summed in LDS first (see k_lv_accum).
__global__ __launch_bounds__(256) void k_lv_rowcap(LvG g, const LvCtl* __restrict__ ctl, const int32_t* __restrict__ comm, const int64_t* __restrict__ newid,
                                                   const u64* __restrict__ K, const int32_t* __restrict__ size, int64_t* __restrict__ cap,
                                                   u64* __restrict__ kv2, uint8_t* __restrict__ vcomp2) {
  __shared__ u64 s_cap[LV_ACC_BINS];
  const bool binned = ctl->n_union2 <= LV_ACC_BINS;
  if (binned) {
    for (int t = threadIdx.x; t < LV_ACC_BINS; t += 256) s_cap[t] = 0ull;
    __syncthreads();
  }
  for (int64_t gv = (int64_t)blockIdx.x * 256 + threadIdx.x; gv < g.n; gv += (int64_t)gridDim.x * 256) {
    const int64_t b = g.rep > 1 ? gv / g.nb : 0;
    const int64_t v = gv - b * g.nb;
    const int comp = g.vcomp ? (int)g.vcomp[gv] : (int)b;
    const LvComp& C = ctl->c[comp];
    if (!C.live) continue;                                // (not numbered; and its own label may coincide with a live community's id when the labels are a rebuilt level's ids)
    const int32_t c = comm[gv];
    if (size[c] <= 0) continue;
    // the new vertex its community becomes: weight and component written by every member alike (the members of a community belong to
    // one component; a community id need not lie in its component's vertex range: the rebuilt levels of algorithm 2)
    const int64_t c2 = newid[c];
    kv2[c2] = C.cont ? K[c] : 0ull;
    vcomp2[c2] = (uint8_t)comp;
    if (!C.cont) continue;
    const u64 deg = (u64)(g.end[v] - g.beg[v]);
    if (deg == 0) continue;
    if (binned) atomicAdd(&s_cap[c2], deg);
    else atomicAdd((u64*)&cap[c2], deg);
  }
  if (binned) {
    __syncthreads();
    for (int t = threadIdx.x; t < LV_ACC_BINS; t += 256)
      if (s_cap[t]) atomicAdd((u64*)&cap[t], s_cap[t]);
  }
}

// One wave per vertex and copy (at most LV_SMALL_DEG entries): the entries summed per neighbouring NEW community; one entry per
// community is appended to the row of the vertex's own new community (cur: the rows' fill counts).  Entries inside the community
// are dropped (their weight is carried as the level's internal weight).
__global__ __launch_bounds__(256) void k_lv_emit_small(LvG g, const LvCtl* __restrict__ ctl, const int32_t* __restrict__ comm, const int64_t* __restrict__ newid,
                                                       const int64_t* __restrict__ beg2, int32_t* __restrict__ cur, int32_t* __restrict__ nbr2,
                                                       u64* __restrict__ wt2) {
  __shared__ int32_t s_key[4][LV_SMALL_SLOTS];
  __shared__ u64 s_val[4][LV_SMALL_SLOTS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int32_t* key = s_key[wave];
  u64* val = s_val[wave];
  for (int t = lane; t < LV_SMALL_SLOTS; t += 64) { key[t] = -1; val[t] = 0ull; }
  GFICF_WAVE_SYNC();
  const u64 lt = (1ull << lane) - 1ull;
  for (int64_t v = (int64_t)blockIdx.x * 4 + wave; v < g.nb; v += (int64_t)gridDim.x * 4) {
    const int64_t lo = g.beg[v], hi = g.end[v];
    if (hi - lo > LV_SMALL_DEG || hi == lo) continue;
    const int64_t e0 = lo + lane, e1 = e0 + 64;
    int32_t u0 = -1, u1 = -1;
    u64 w0 = 0, w1 = 0;
    if (e0 < hi) { u0 = g.nbr[e0]; w0 = g.wt[e0]; if (u0 == v) u0 = -1; }
    if (e1 < hi) { u1 = g.nbr[e1]; w1 = g.wt[e1]; if (u1 == v) u1 = -1; }
    for (int b = 0; b < g.rep; ++b) {
      const int comp = g.vcomp ? (int)g.vcomp[v] : b;
      if (!ctl->c[comp].cont) continue;
      const int64_t base = (int64_t)b * g.nb;
      const int32_t cv = (int32_t)newid[comm[base + v]];
      int32_t c0 = u0 >= 0 ? (int32_t)newid[comm[base + u0]] : -1, c1 = u1 >= 0 ? (int32_t)newid[comm[base + u1]] : -1;
      if (c0 == cv) c0 = -1;
      if (c1 == cv) c1 = -1;
      int slot0 = -1, slot1 = -1;
      bool own0 = false, own1 = false;
      if (c0 >= 0) {
        uint32_t h = gficf_comm_hash((uint32_t)c0) & (LV_SMALL_SLOTS - 1);
        for (;;) {
          const int32_t old = atomicCAS(&key[h], -1, c0);
          if (old == -1) { own0 = true; break; }
          if (old == c0) break;
          h = (h + 1) & (LV_SMALL_SLOTS - 1);
        }
        slot0 = (int)h;
        atomicAdd(&val[h], w0);
      }
      if (c1 >= 0) {
        uint32_t h = gficf_comm_hash((uint32_t)c1) & (LV_SMALL_SLOTS - 1);
        for (;;) {
          const int32_t old = atomicCAS(&key[h], -1, c1);
          if (old == -1) { own1 = true; break; }
          if (old == c1) break;
          h = (h + 1) & (LV_SMALL_SLOTS - 1);
        }
        slot1 = (int)h;
        atomicAdd(&val[h], w1);
      }
      GFICF_WAVE_SYNC();
      const u64 m0 = __ballot(own0), m1 = __ballot(own1);
      const int n0 = __popcll(m0), total = n0 + __popcll(m1);
      int32_t p = 0;
      if (lane == 0 && total) p = atomicAdd(&cur[cv], total);
      p = __shfl(p, 0);
      const int64_t row = beg2[cv];
      if (own0) {
        const int64_t at = row + p + __popcll(m0 & lt);
        nbr2[at] = c0; wt2[at] = val[slot0];
        key[slot0] = -1; val[slot0] = 0ull;
      }
      if (own1) {
        const int64_t at = row + p + n0 + __popcll(m1 & lt);
        nbr2[at] = c1; wt2[at] = val[slot1];
        key[slot1] = -1; val[slot1] = 0ull;
      }
      GFICF_WAVE_SYNC();
    }
  }
}

template <int SLOTS>
__global__ __launch_bounds__(256) void k_lv_emit_big(LvG g, const LvCtl* __restrict__ ctl, int large, int64_t n_list, const int32_t* __restrict__ big,
                                                     const int32_t* __restrict__ comm, const int64_t* __restrict__ newid, const int64_t* __restrict__ beg2,
                                                     int32_t* __restrict__ cur, int32_t* __restrict__ nbr2, u64* __restrict__ wt2,
                                                     uint32_t* __restrict__ status) {
  extern __shared__ unsigned char s_raw[];
  u64* val = (u64*)s_raw;
  int32_t* key = (int32_t*)(val + SLOTS);
  __shared__ int s_n;
  __shared__ int32_t s_base;
  const int tid = threadIdx.x;
  const int32_t* list = large ? big + (g.nb - n_list) : big;
  for (int64_t item = blockIdx.x; item < n_list * g.rep; item += gridDim.x) {
    const int b = (int)(item / n_list);
    const int64_t v = list[item - (int64_t)b * n_list];
    const int comp = g.vcomp ? (int)g.vcomp[v] : b;
    if (!ctl->c[comp].cont) continue;
    const int64_t base = (int64_t)b * g.nb;
    const int64_t lo = g.beg[v], hi = g.end[v];
    const int32_t cv = (int32_t)newid[comm[base + v]];
    const int64_t row = beg2[cv];
    const uint32_t P = (uint32_t)((hi - lo + SLOTS / 2 - 1) / (SLOTS / 2));
    for (uint32_t p = 0; p < (P ? P : 1u); ++p) {
      for (int t = tid; t < SLOTS; t += 256) { key[t] = -1; val[t] = 0ull; }
      if (tid == 0) s_n = 0;
      __syncthreads();
      for (int64_t e = lo + tid; e < hi; e += 256) {
        const int32_t u = g.nbr[e];
        if (u == v) continue;
        const int32_t c = (int32_t)newid[comm[base + u]];
        if (c == cv) continue;
        const uint32_t hc = gficf_comm_hash((uint32_t)c);
        if (P > 1 && (hc >> 13) % P != p) continue;
        uint32_t h = hc & (SLOTS - 1);
        int probes = 0;
        for (;;) {
          const int32_t old = atomicCAS(&key[h], -1, c);
          if (old == -1 || old == c) { atomicAdd(&val[h], g.wt[e]); break; }
          h = (h + 1) & (SLOTS - 1);
          if (++probes >= SLOTS) { atomicOr(status, GFICF_ST_TOO_DENSE); break; }
        }
      }
      __syncthreads();
      int mine = 0;
      for (int t = tid; t < SLOTS; t += 256) mine += key[t] >= 0 ? 1 : 0;
      const int rank0 = mine ? atomicAdd(&s_n, mine) : 0;
      __syncthreads();
      if (tid == 0) s_base = s_n ? atomicAdd(&cur[cv], s_n) : 0;
      __syncthreads();
      int64_t at = row + s_base + rank0;
      for (int t = tid; t < SLOTS; t += 256)
        if (key[t] >= 0) { nbr2[at] = key[t]; wt2[at] = val[t]; ++at; }
      __syncthreads();
    }
  }
}

// end2 = beg2 + fill count
__global__ __launch_bounds__(256) void k_lv_finish_rows(const int64_t* __restrict__ n_dev, const int64_t* __restrict__ beg2, const int32_t* __restrict__ cur,
                                                        int64_t* __restrict__ end2) {
  const int64_t n = *n_dev;
  for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < n; c += (int64_t)gridDim.x * 256) end2[c] = beg2[c] + cur[c];
}

}  // namespace
