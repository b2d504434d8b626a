/* gficf_slm.h — C ABI of libgficf_slm.so: the smart local moving algorithm (Waltman, van Eck 2013), algorithm 3 of the
 * reference's RunModularityClustering (src/ModularityOptimizer.cpp:651-690, runSmartLocalMovingAlgorithm), on the symmetric
 * weighted adjacency matrix of the kNN -> Jaccard graph, on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links, in the manner of include/gficf_leiden.h: it takes that
 * library's gficf_ctx and uses its stream, device pool, scan, radix sort, status codes and gficf_last_error().  The core ABI, the
 * gficf_louvain_* entries (which go on refusing algorithm 3) and libgficf_leiden.so are not changed.  The matrix is the one
 * gficf_adjacency_* produce: indptr int64 (N + 1), indices int32 0-based, x f64 (CSC == CSR: it must be symmetric).
 *
 * RELAXED CONTRACT.  The algorithm and its objective are SLM's; the visiting order and the java.util.Random bits are not the
 * reference's.  The OBJECTIVE, the 2^-32 fixed-point weights (a weight is llrint(x * 2^32), 0 on the diagonal), the validation
 * and the numbers k_v, K_c, 2W are those of include/gficf_leiden.h, word for word.
 *
 * ONE ITERATION starts from a partition made canonical (a community's label is its smallest member) and repeats over levels,
 * at most 64:
 *   1. LOCAL MOVING on the level: exactly step 1 of include/gficf_leiden.h in its parallel form — S = 4 hash classes, the stamp,
 *      the decision, "a pass that lowers Q is undone and ends the level", at most 64 passes, hseed(seed, level).
 *   2. STOP if every community of the level is a single level-vertex.
 *   3. SUB-MOVING.  Inside every community, from singletons (every level-vertex alone, its sub-community's total = k_v), the
 *      local moving of step 1 with three differences:
 *        (a) THE FENCE: an entry (u, w) of v exists only if comm[u] == comm[v].  Entries across the fence give no candidate, add
 *            nothing to e(v, .) or to the staying side, and carry no stamp;
 *        (b) the totals K and the sizes are those of the sub-communities;
 *        (c) the class hash is taken with (seed ^ 0x27D4EB2F) (uint32_t) in place of seed.
 *      k_v and resolution / 2W are the full graph's, as in the reference's sub-networks (:406-447, :542).  The Q of the undo rule
 *      is the Q of the sub-partition on the level's graph (its internal weight needs no fence: a sub-community lies inside one
 *      community).  The result is made canonical: a sub-community's label is its smallest member.
 *   4. STOP if the sub-moving merged nothing.
 *   5. AGGREGATE by the sub-communities in ascending order of their labels, every new vertex seeded in the community its
 *      members were in: step 4 of include/gficf_leiden.h.
 * DIFFERENCES FROM THE REFERENCE, stated: no move to an empty cluster when every gain is negative (reference :550-554; Leiden's
 * moving form has none either); the reference recurses until one node is left, here the stops are 2 and 4.
 *
 * ITERATIONS.  n_iter iterations, each from the previous one's result; the run ends early when an iteration returns its own
 * start (an iteration is a function of its start alone, so every further one would repeat it; the reference never clears its
 * `update` flag for algorithm 3, :964-965, and always runs all of them).
 * STARTS.  Start s of n_start is the whole run with seed (seed + s) mod 2^32; the result is the one of largest Q, ties to the
 * smaller s.  Starts run one after another.
 * RESULT.  labels int32, 0-based, clusters numbered by decreasing size, ties by smallest member (as gficf_leiden_device).  A
 * matrix without edges: every vertex alone, Q = 0.  The same bits on every call; no floating-point atomics.
 *
 * SUBMOVE ENTRIES: step 3 alone on the finest graph under the caller's partition d_labels_in (labels in [0, N), used as they
 * are, as the fence), with the class hash of (seed ^ 0x27D4EB2F, level).  d_sub_out[v] = the smallest member of v's
 * sub-community.
 *
 * Arguments and errors are those of include/gficf_leiden.h (n_start < 1 or n_iter < 1: GFICF_ERR_INVALID_ARG); a failed call
 * leaves the context usable.  With GFICF_SLM_DEBUG set in the environment every level writes a line to stderr. */
#ifndef GFICF_SLM_H
#define GFICF_SLM_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_SLM_ABI_VERSION 1

typedef struct gficf_slm_info {
  int64_t n_clusters;   /* clusters of the result */
  int32_t start;        /* the start (0-based) the result came from */
  int32_t iterations;   /* iterations that start ran (fewer than n_iter: the last one returned its own start) */
  int32_t levels;       /* levels of its last iteration */
  int32_t reserved;
  double modularity;    /* Q of the returned labels */
} gficf_slm_info;

typedef struct gficf_slm_submove_info {
  int64_t n_sub;        /* sub-communities */
  int32_t passes;       /* passes of the sub-moving */
  int32_t reserved;
} gficf_slm_submove_info;

int gficf_slm_abi_version(void);

size_t gficf_slm_workspace_bytes(int64_t N, int64_t nnz);
int gficf_slm_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz,
                     double resolution, int n_start, int n_iter, uint32_t seed, const int32_t* d_init_or_null, void* d_ws, size_t ws_bytes,
                     int32_t* d_labels, gficf_slm_info* info);
int gficf_slm_submove_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz,
                             double resolution, const int32_t* d_labels_in, uint32_t seed, int level, void* d_ws, size_t ws_bytes,
                             int32_t* d_sub_out, gficf_slm_submove_info* info);
/* host arrays; nnz = indptr[N] */
int gficf_slm_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz, double resolution,
                   int n_start, int n_iter, uint32_t seed, const int32_t* init_or_null, int32_t* labels, gficf_slm_info* info);
int gficf_slm_submove_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz,
                           double resolution, const int32_t* labels_in, uint32_t seed, int level, int32_t* sub_out,
                           gficf_slm_submove_info* info);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_SLM_H */
