/* gficf_leiden.h — C ABI of libgficf_leiden.so: Leiden community detection (Traag, Waltman, van Eck 2019) on the symmetric
 * weighted adjacency matrix of the kNN -> Jaccard graph, what clustcells(community.algo = "leiden") of the reference runs
 * (R/clustCells.R:100-107: leiden::leiden(object = g, resolution_parameter = resolution)), on the MI355X (gfx950).
 *
 * An add-on to libgficf_hip.so (include/gficf_hip.h), which it links: it takes that library's gficf_ctx and uses its stream,
 * device pool, scan, radix sort, status codes and gficf_last_error().  The core ABI is not changed.  The matrix is the one
 * gficf_adjacency_* produce: indptr int64 (N + 1), indices int32 0-based, x f64 (CSC == CSR: it must be symmetric).
 *
 * RELAXED CONTRACT.  The algorithm and its objective are Leiden's; the visiting order and the random bits are not leidenalg's.
 *
 * OBJECTIVE (leidenalg's default, RBConfigurationVertexPartition; the Q of include/gficf_hip.h, Louvain section):
 *     Q = (1/2W) [ sum_ij A_ij delta(c_i, c_j)  -  resolution * sum_c K_c^2 / 2W ],     K_c = the summed degrees of c.
 *   The diagonal is ignored.  Weights must be finite and in [0, 2^20] (GFICF_ERR_BAD_VALUE), a stored zero is no edge.  The
 *   leiden R package takes the edge weights from the igraph object's "weight" attribute and its default is n_iterations = 2;
 *   neither can be checked where that package is not installed, and both are taken as stated in its manual.  clustcells passes
 *   its `resolution` (default 0.8) and n_iterations = 2.
 *
 * ONE ITERATION starts from a partition (singletons, the caller's init, or the previous iteration's result; in every case
 * relabelled so that a community's label is its smallest member — the answer does not depend on how the start was spelled)
 * and repeats over levels:
 *   1. LOCAL MOVING.  Every vertex moves to the neighbouring community of largest gain, or stays:
 *        gain(v -> c) = e(v, c) - resolution * k_v * K_c / 2W        (k_v taken out of v's old community; ties: smaller label)
 *      until nothing moves.  Only a vertex with a neighbour that moved since its last turn is looked at again.
 *   2. STOP if every community of the level is a single level-vertex.
 *   3. REFINEMENT.  Inside every community C, from singletons: a vertex v moves only while it is alone in its refined
 *      community, only if it is well connected, e(v, C - v) >= resolution * k_v (K_C - k_v) / 2W, only into a refined
 *      community r of C that it has an edge to and that is well connected, E(r, C - r) >= resolution * K_r (K_C - K_r) / 2W,
 *      and only at gain e(v, r) - resolution * k_v K_r / 2W >= 0.
 *      THE ONE ALGORITHMIC DIFFERENCE: leidenalg draws r at random with weight exp(gain / theta); here v takes the largest
 *      gain, ties to the smaller label (theta -> 0).
 *   4. AGGREGATE.  The refined communities become the vertices of the next level (entries summed, self-loops kept, k summed);
 *      each starts in the community its members were in.  STOP if the refinement merged nothing.
 *
 * PARALLEL FORM, deterministic bit for bit on every call:
 *   * weights in 2^-32 fixed point (u64): every sum that decides something is an integer sum and does not depend on order;
 *   * local moving in synchronous sub-rounds: the vertices of a level fall into S = 4 classes by a hash of
 *     (vertex, seed, level); sub-round s of an iteration moves class s on one snapshot of the labels and totals, and the totals
 *     are applied between sub-rounds.  Two singletons never swap (the one with the smaller label stays).  The hash does not
 *     depend on the iteration number: leiden(n_iterations = 2) == leiden(1) resumed from leiden(1)'s labels, bit for bit.
 *     A pass over the four classes that lowers Q is undone and ends the level; at most 64 passes a level.
 *     THE CLASS of vertex v of a level is h(v ^ hseed) % 4, with
 *         h(v):  v ^= v >> 16;  v *= 0x7feb352d;  v ^= v >> 15;  v *= 0x846ca68b;  v ^= v >> 16        (uint32_t)
 *         hseed = h(seed * 0x9E3779B1 + level * 0x85EBCA77 + 0x165667B1)                               (uint32_t, level from 0)
 *     THE STAMP.  Sub-rounds are counted t = 1, 2, ... from the start of the level (sub-round s of pass p: t = 4 p + s + 1).
 *     Every vertex that moves in sub-round t stamps t on the target of each of its entries of NON-ZERO weight — a stored zero
 *     and the level-0 diagonal are no edges and carry no stamp; the self-loop of a coarser level has weight and stamps the
 *     mover itself.  A vertex of class s is looked at in sub-round t iff t <= 4 (the first pass: everybody) or its stamp is
 *     >= t - 4 (something next to it moved since its last turn, that turn's own sub-round included).
 *     THE DECISION of v, on the labels, totals and sizes as they stood before the sub-round: its candidates are the communities
 *     other than its own that an entry (u != v, weight != 0) leads to; none: it stays.  The best is the one of largest gain,
 *     ties to the smaller label; v moves iff best > stay or (best == stay and the best label is smaller than its own), where
 *     stay = e(v, own) - resolution * k_v (K_own - k_v) / 2W; a singleton does not move to a singleton of larger label.  All
 *     moves of a sub-round are applied together.  After the pass: nothing moved ends the level; Q lower than before the pass
 *     restores the snapshot and ends the level (Q in f64: where the exact values are equal the rounding of sum K^2 decides —
 *     DESIGN.md section 15, "exact ties");
 *   * the numbers: a weight is llrint(x * 2^32), and 0 on the diagonal of the matrix; k_v is the sum of row v and 2W the sum
 *     of all k_v; a vertex of a coarser level has the summed k of its members (which includes its self-loop).  Gains and the
 *     tests of the refinement are evaluated in f64 from these integers (r = resolution / 2W rounded once): a comparison whose
 *     sides differ by less than the f64 rounding of their terms may fall either way between builds of this library, never
 *     between calls;
 *   * refinement in rounds.  Every eligible singleton v proposes its best target among the refined communities that had more
 *     than one member at the start of the round and the singletons of smaller id than v.  A proposal commits iff the target
 *     had more than one member at the start of the round or its single member proposed nothing this round.  Rounds repeat
 *     until nobody proposes.  PROGRESS: the proposing vertex of smallest id always commits (its target is a community of more
 *     than one member, or a singleton of still smaller id — which then did not propose, or it would be the smallest), so a
 *     round with a proposal shrinks the set of singletons: at most n rounds.  Members of a community of more than one never
 *     move, a singleton that is joined proposed nothing and stays: every commit joins v to a community that still holds the
 *     neighbour it saw, so every refined community is connected.  Several vertices may join one r in a round on start-of-round
 *     figures (K_r, E(r, C - r), recomputed before the next round): only the refined partition's structure is contracted,
 *     not each gain.
 *     In other words a proposal of v to p commits iff p itself proposed nothing.  e(v, C - v) is computed once; K_r and
 *     E(r, C - r) are recomputed after every round that commits; a refined community's label is the id of the singleton it
 *     grew from;
 *   * aggregation: every vertex sums its entries per neighbouring refined community and appends one entry per community to
 *     the row of its own (rows in begin / end form; a row may name a neighbour once per member vertex — every consumer sums
 *     per community anyway).  The new vertices are the refined communities in ascending order of their labels; entries of
 *     weight 0 are dropped, self-loops kept; a new vertex starts in the smallest new id among its old community's members.
 *     At most 64 levels.  Between iterations a community is relabelled by its smallest member.
 *   Rows up to 128 entries are handled by one wave with a 256-slot LDS table, longer ones by a workgroup with a 4096-slot
 *   table, in ceil(min(entries, vertices of the level) / 1024) passes over the row by hash class of the community.
 *   GFICF_ERR_UNSUPPORTED only if one such class overflows the table (not observed).  No floating-point atomics.
 *
 * RESULT.  labels int32, 0-based, clusters numbered by decreasing size, ties by first vertex, as gficf_louvain_device does;
 * *n_clusters; *modularity = Q of the returned labels.  A matrix without edges: every vertex alone, Q = 0.
 *
 * REFINE ENTRIES: the refinement stage alone on the caller's partition (labels in [0, N)).  d_refined_out[v] = the SMALLEST
 * member id of v's refined community, which gives the answer one spelling; *n_refined = their number.
 *
 * Arguments: NULL pointers, negative sizes, n_iterations < 1, a resolution that is negative or not finite:
 * GFICF_ERR_INVALID_ARG; an init or input label outside [0, N): GFICF_ERR_BAD_ID; a malformed matrix: GFICF_ERR_BAD_CSC /
 * GFICF_ERR_BAD_VALUE; a workspace that is too small: GFICF_ERR_CAPACITY.  All of them before any entry is followed.  The
 * entries synchronise the stream (once per pass of local moving and per refinement round). */
#ifndef GFICF_LEIDEN_H
#define GFICF_LEIDEN_H

#include <stddef.h>
#include <stdint.h>

#include "gficf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GFICF_LEIDEN_ABI_VERSION 1

int gficf_leiden_abi_version(void);

size_t gficf_leiden_workspace_bytes(int64_t N, int64_t nnz);
int gficf_leiden_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz,
                        double resolution, int n_iterations, int seed, const int32_t* d_init_or_null, int32_t* d_labels, int64_t* n_clusters,
                        double* modularity, void* d_ws, size_t ws_bytes);
/* host arrays; nnz = indptr[N] */
int gficf_leiden_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz, double resolution,
                      int n_iterations, int seed, const int32_t* init_or_null, int32_t* labels, int64_t* n_clusters, double* modularity);

size_t gficf_leiden_refine_workspace_bytes(int64_t N, int64_t nnz);
int gficf_leiden_refine_device(gficf_ctx* ctx, int64_t N, const int64_t* d_indptr, const int32_t* d_indices, const double* d_x, int64_t nnz,
                               double resolution, const int32_t* d_labels_in, int32_t* d_refined_out, int64_t* n_refined, void* d_ws,
                               size_t ws_bytes);
int gficf_leiden_refine_host(gficf_ctx* ctx, int64_t N, const int64_t* indptr, const int32_t* indices, const double* x, int64_t nnz,
                             double resolution, const int32_t* labels_in, int32_t* refined_out, int64_t* n_refined);

#ifdef __cplusplus
}
#endif

#endif /* GFICF_LEIDEN_H */
