// addon_status.h — what the add-on libraries share of their workspace and their deferred checks: how a caller's block is
// carved, the status word at its head and how a *_sync entry reads it.  Header-only: an add-on asks of libgficf_hip.so only what every build of ABI 7 exports.
#pragma once

#include "common.h"

// bits of the status word of the graph add-ons (umap, tsne, spectral, transform); each *_sync entry words its own messages.
// markers.hip, pca.hip, gsea.hip and leiden.hip give the bits of their words other meanings.
constexpr uint32_t GFICF_AST_ID = 1u;        // a neighbour id, a label or a column of the graph out of range
constexpr uint32_t GFICF_AST_VALUE = 2u;     // a non-finite distance or coordinate, a bad value of the graph
constexpr uint32_t GFICF_AST_CSC = 4u;       // a row pointer of the graph that decreases or leaves [0, capacity]

// a caller's workspace carved: carve(base) takes the pieces from base on and returns their total; base == nullptr only counts
template <typename F>
inline int gficf_addon_carve(void* ws, size_t ws_bytes, F&& carve) {
  const size_t need = carve((char*)nullptr);
  if (ws_bytes < need) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "workspace too small: %zu < %zu bytes", ws_bytes, need);
  carve((char*)ws);
  return GFICF_OK;
}

// the head of a *_sync entry: the status word at the head of the workspace read behind everything enqueued; the stream's own
// verdict (gficf_ctx_sync) is returned, and *st is the add-on's to decode when that is GFICF_OK
inline int gficf_addon_read_status(gficf_ctx* ctx, const void* ws, uint32_t* st) {
  GFICF_CTX_ENTER(ctx);
  if (!ws) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL workspace");
  *st = 0;
  GFICF_HIP_CHECK(hipMemcpyAsync(st, ws, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
  return gficf_ctx_sync(ctx);
}
