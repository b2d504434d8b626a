// prim_probe.hip — test infrastructure: C entries onto the internal primitives of libgficf_hip.so (common.h), which its C ABI
// does not export.  Built and loaded by tests/helpers/prim_probe.py; never part of the product.
#include "common.h"

extern "C" {

int probe_radix_sort_kv(void* ctx, void* kv0, void* kv1, void* hist, int64_t M, int b, void* okey, void* oval) {
  return gficf_radix_sort_kv((gficf_ctx*)ctx, (unsigned long long*)kv0, (unsigned long long*)kv1, (int64_t*)hist, M, b, (uint32_t*)okey,
                             (uint32_t*)oval);
}

int64_t probe_radix_sort_hist_len(int64_t M, int b) { return gficf_radix_sort_hist_len(M, b); }

int probe_exclusive_scan_i64(void* ctx, void* d, int64_t n) { return gficf_exclusive_scan_i64((gficf_ctx*)ctx, (int64_t*)d, n); }

uint32_t probe_get_scan_epoch(void* ctx) { return ((gficf_ctx*)ctx)->scan_epoch; }

void probe_set_scan_epoch(void* ctx, uint32_t epoch) { ((gficf_ctx*)ctx)->scan_epoch = epoch; }

int probe_ctx_sync(void* ctx) { return gficf_ctx_sync((gficf_ctx*)ctx); }

}  // extern "C"
