// louvain_shared.h — what the kernel headers of louvain.hip and its driver share: the table and grid constants, the level's graph,
// the control block and its pinned mirror, the per-block partial sums, and the device inlines of the move kernels (the DPP wave
// reductions, the decision for one vertex).  louvain.hip's head comment describes the algorithm.
#pragma once

#include <cmath>

#include "common.h"
#include "community_ops.h"

namespace {

typedef unsigned long long u64;

constexpr int LV_SMALL_DEG = 128;              // up to here: one wave per vertex, 256-slot table
constexpr int LV_SMALL_SLOTS = 256;
constexpr int LV_MID_DEG = 4096, LV_MID_SLOTS = 1024;   // up to here: still one wave per vertex, a 1024-slot table of its own, passes by hash class beyond 512 entries
constexpr int LV_EMIT_SLOTS = 2048;            // the reduction's workgroup-per-vertex table for the same vertices
constexpr int LV_BIG_SLOTS = 8192;             // beyond: one workgroup per vertex, 32 KB keys + 64 KB sums
constexpr int LV_MAX_ITERS = 64;
constexpr int LV_MAX_SAVED = 12;              // levels whose vertex map is kept for the refinement of algorithm 2
constexpr int LV_MAX_B = 16;                  // starts run together
constexpr int LV_GRID = 1536;                 // persistent grid of the wave-per-vertex kernels (workgroups of 4 waves): what is RESIDENT at once on 256 CUs
                                              // (k_lv_move_small is held to 80 VGPRs: six workgroups a CU) — 2048 ran as 1.6 rounds of five a CU (8.1 -> 7.7 ms at
                                              // config 3, 10 starts; six a CU: 7.35; eight spill: 8.5)
constexpr int LV_GRID_BIG = 1280;             // ... of the middle-degree (two waves, 28 KB of LDS: five a CU) and workgroup-per-vertex kernels
constexpr int LV_SQ_BLOCKS = 64;              // slices of a component's communities in the fixed-order sum of squares
constexpr int LV_ACC_BINS = 4096;

enum { LV_IDLE = 0, LV_CONTINUE = 1, LV_STOP_KEEP = 2, LV_STOP_UNDO = 3 };

// One level's union graph.  Level 0: `rep` copies of the caller's matrix, never materialised (union vertex b * nb + v has
// the row of v with every neighbour shifted by b * nb); coarse levels: rep == 1.  Rows are [beg[v], end[v]).
struct LvG {
  int64_t n;                 // union vertices = rep * nb
  int64_t nb;                // vertices of the stored graph
  int32_t rep;
  const int64_t* beg;
  const int64_t* end;
  const int32_t* nbr;
  const u64* wt;
  const u64* kv;             // [nb] vertex weights
  const uint8_t* vcomp;      // [n] component of a union vertex; NULL at level 0: the copy number (also when there is one copy only)
};

struct LvComp {              // one start ("component" of the union)
  int64_t v0, n;             // its vertices at the current level: union ids [v0, v0 + n)
  int64_t seed_base;         // seeded start: community of a vertex = seed_base + its seed label
  int64_t lab_base;          // first LDS bin of its seed labels (binned accumulation)
  int64_t n_labels;          // the labels of the last renumbering lie in [0, n_labels)
  int64_t newbase, n2;       // after the level's renumbering: first new id, communities in use
  u64 self_w, in_w;          // weight folded into the level's vertices; internal weight of the accepted labels on the level's graph
  u64 in_run;                // internal weight of the labels as they are (kept up to date by the changes the sub-round-0 kernels report)
  double q_prev, q_final;
  uint32_t seed;             // of the sub-round class hash: what a "random start" varies
  int32_t S;                 // sub-rounds of the level
  int32_t live;              // takes part in this level
  int32_t cont;              // goes on to the next level (set when the level is renumbered)
  int32_t level_done, action, iter, level_moved, any_move, finished;
  int32_t n_saved, pad;
  int64_t saved_n[LV_MAX_SAVED + 1];
};

struct LvCtl {               // device control block
  LvComp c[LV_MAX_B];
  int32_t B, pad;
  unsigned n_mid, n_large;   // vertices of the workgroup path (list counts) of the graph the lists were built for
  int64_t n_union2;          // union vertices after the renumbering
};

struct LvHostComp { int64_t n2; double q_prev; int32_t cont, any_move, level_moved, live; };
struct LvHost {              // pinned host memory the control kernels write (read after an event)
  int32_t n_cont[LV_MAX_ITERS + 2];
  int64_t n_union2;
  unsigned n_mid, n_large;
  LvHostComp c[LV_MAX_B];
  double q_iter[LV_MAX_B];   // (debug trace)
  unsigned mv_iter[LV_MAX_B];
};

struct LvParts {             // per-block partial sums of the move kernels, fixed slots (no atomics, no clearing)
  // internal weight: written by an iteration's sub-round-0 kernels, read by the same iteration's k_lv_decide.  Moved vertices: summed over
  // ALL sub-rounds of an iteration and read by the NEXT iteration's k_lv_decide, after that iteration's sub-round 0 has started a new
  // count — hence two sets, by iteration parity.
  u64* in_small;  unsigned* mv_small[2];     // [LV_GRID][LV_MAX_B]
  u64* in_mid;    unsigned* mv_mid[2];       // [LV_GRID_BIG][LV_MAX_B]
  u64* in_large;  unsigned* mv_large[2];
  double* sq;                              // [LV_MAX_B][LV_SQ_BLOCKS]
};

__device__ __host__ static inline int lv_sub_rounds_of(int64_t n, int s_env) {
  if (s_env >= 1 && s_env <= 64) return s_env;
  // sub-rounds an iteration is cut into (vertices of one hash class move together).  One is too few (modularity 0.03 - 0.06 below the reference's
  // on weakly structured graphs: neighbours move at once), two to sixteen give the same quality within run-to-run differences of 0.003 on graphs of 300
  // to 60 000 vertices (tools/louvain_subrounds_probe.py, profiles/r06_louvain_subrounds.txt).  Through round 6's first form small levels took 8 / 16:
  // the coarse levels of a big problem are a few hundred vertices, and 16 sub-rounds x 3 launches an iteration were 1 ms of the 10.8 at config 3.
  return n > 50000 ? 2 : 4;
}

// ---- local moving
struct LvMove {
  double r;            // resolution / 2W (in fixed-point units of 2W)
  int s;               // this sub-round's hash class
  // Pruning ("fast local moving"): a vertex is looked at again only when it or one of its neighbours has moved since it was last looked at.
  // Every sub-round kernel of a level has an epoch (iteration * sub-rounds + sub-round + 1); a vertex that decides to move stamps itself and
  // its neighbours with it (plain stores of one value: no clearing, no race); a vertex of this kernel's class was last looked at one
  // iteration ago, so it is looked at now iff its stamp >= thr = epoch - sub-rounds (stamps start at 0: everybody in iteration 0).
  int epoch, thr;
};

__device__ static inline bool lv_better(double g, int32_t c, double bg, int32_t bc) { return g > bg || (g == bg && c < bc); }

// Wave reductions on DPP row operations (no LDS traffic; the ds_bpermute butterflies they replace were ~1.2 us of the ~4.5 us a vertex took).
// Every lane must be active.  quad_perm [1,0,3,2] / [2,3,0,1], row_half_mirror, row_mirror leave each row of 16 uniform; row_bcast15 (rows
// 1, 3) and row_bcast31 (rows 2, 3) carry the rows' results down: lane 63 holds the wave's, read back with v_readlane.
template <int CTRL, int RM>
__device__ static inline int lv_dpp(int old, int x) { return __builtin_amdgcn_update_dpp(old, x, CTRL, RM, 0xF, false); }

template <int CTRL, int RM>
__device__ static inline void lv_sum_step(u64& x) {
  const uint32_t lo = (uint32_t)lv_dpp<CTRL, RM>(0, (int)(uint32_t)x), hi = (uint32_t)lv_dpp<CTRL, RM>(0, (int)(uint32_t)(x >> 32));
  x += ((u64)hi << 32) | lo;
}
__device__ static inline u64 lv_wave_sum(u64 x) {
  lv_sum_step<0xB1, 0xF>(x); lv_sum_step<0x4E, 0xF>(x); lv_sum_step<0x141, 0xF>(x); lv_sum_step<0x140, 0xF>(x);
  lv_sum_step<0x142, 0xA>(x); lv_sum_step<0x143, 0xC>(x);
  return ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), 63) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 63);
}

struct LvBest { double g; int32_t c; };      // best gain and its community (ties: the smaller id)

template <int CTRL, int RM>
__device__ static inline double lv_dpp_f64(double x) {
  return __hiloint2double(lv_dpp<CTRL, RM>(__double2hiint(x), __double2hiint(x)), lv_dpp<CTRL, RM>(__double2loint(x), __double2loint(x)));
}
// The wave's best, in every lane: the largest gain (v_max_f64 over the DPP steps), then the smallest community among the lanes that hold it —
// the same order as lv_better, in about half the instructions of reducing the pair at once.
__device__ static inline LvBest lv_wave_best(LvBest x) {
  double m = x.g;
  m = fmax(m, lv_dpp_f64<0xB1, 0xF>(m)); m = fmax(m, lv_dpp_f64<0x4E, 0xF>(m)); m = fmax(m, lv_dpp_f64<0x141, 0xF>(m));
  m = fmax(m, lv_dpp_f64<0x140, 0xF>(m)); m = fmax(m, lv_dpp_f64<0x142, 0xA>(m)); m = fmax(m, lv_dpp_f64<0x143, 0xC>(m));
  m = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(m), 63), __builtin_amdgcn_readlane(__double2loint(m), 63));
  int k = x.g == m ? x.c : INT32_MAX;
  k = min(k, lv_dpp<0xB1, 0xF>(k, k)); k = min(k, lv_dpp<0x4E, 0xF>(k, k)); k = min(k, lv_dpp<0x141, 0xF>(k, k));
  k = min(k, lv_dpp<0x140, 0xF>(k, k)); k = min(k, lv_dpp<0x142, 0xA>(k, k)); k = min(k, lv_dpp<0x143, 0xC>(k, k));
  return LvBest{m, __builtin_amdgcn_readlane(k, 63)};
}

// does component C take part in the sub-round kernel (s, first)?  first = the kernel of sub-round 0, which runs BEFORE the iteration's
// decision: every component whose level has not ended
__device__ static inline bool lv_runs(const LvComp& C, int s, bool first) {
  return first ? !C.level_done : (C.action == LV_CONTINUE && s < C.S);
}

// the decision for vertex gv, identical in every lane (all inputs are wave-uniform).  Kcv, szcv, szgv: total and size of its community, size of
// the community that carries its own id — loaded by the caller before the table work, off the critical path
__device__ static inline int32_t lv_decide_vertex(int64_t gv, int32_t cv, double bg, int32_t bc, u64 stay_w, u64 kvv, double r, u64 Kcv, int32_t szcv,
                                                  int32_t szgv, const int32_t* __restrict__ size, bool* moved) {
  const double kvd = (double)kvv;
  const double g_stay = (double)stay_w - kvd * (double)(Kcv - kvv) * r;
  bool move = bc != INT32_MAX && bg > g_stay;
  if (move && szcv == 1 && size[bc] == 1 && bc > cv) move = false;      // two singletons never swap
  int32_t to = move ? bc : cv;
  // every option loses: alone is better (the reference's move into an unused cluster, :546-550).  The unused cluster
  // is the vertex's own id when nobody holds it — unique per vertex, so simultaneous escapes never meet.
  if ((move ? bg : g_stay) < 0.0 && szcv > 1 && szgv == 0) { to = (int32_t)gv; move = true; }
  *moved = move;
  return to;
}

// one copy's view of a vertex in a round of k_lv_move_small
struct LvSide {
  int mode;                  // 0: not in this round, 1: only its share of the internal weight (sub-round 0, other class), 2: evaluate
  int comp;
  int64_t base, gv;
  int32_t cv;
  u64 Kcv; int32_t szcv, szgv;
};

template <bool FIRST>
__device__ static inline LvSide lv_side(const LvG& g, const LvCtl* __restrict__ ctl, int s, int b, int64_t v, const int32_t* __restrict__ comm,
                                        const u64* __restrict__ K, const int32_t* __restrict__ size) {
  LvSide x;
  x.mode = 0; x.comp = 0; x.base = 0; x.gv = 0; x.cv = 0; x.Kcv = 0; x.szcv = 0; x.szgv = 0;
  if (b >= g.rep) return x;
  x.comp = g.vcomp ? (int)g.vcomp[v] : b;
  const LvComp& C = ctl->c[x.comp];
  if (!lv_runs(C, s, FIRST)) return x;
  x.base = (int64_t)b * g.nb; x.gv = x.base + v;
  const bool in_class = C.S == 1 || (int)(gficf_comm_hash((uint32_t)(x.gv - C.v0) + C.seed) % (uint32_t)C.S) == s;
  if (!FIRST && !in_class) return x;
  x.mode = in_class ? 2 : 1;
  x.cv = comm[x.gv];
  if (in_class) { x.Kcv = K[x.cv]; x.szcv = size[x.cv]; x.szgv = size[x.gv]; }
  return x;
}

// hash class of a vertex for S sub-rounds (S is a power of two unless GFICF_LOUVAIN_SUBROUNDS says otherwise)
__device__ static inline int lv_class(uint32_t x, int S) {
  const uint32_t h = gficf_comm_hash(x);
  return (S & (S - 1)) == 0 ? (int)(h & (uint32_t)(S - 1)) : (int)(h % (uint32_t)S);
}

}  // namespace
