// prim_probe.hip — test infrastructure: C entries onto the internal primitives of libgficf_hip.so (common.h), which its C ABI
// does not export, and onto the header-only code the add-ons share (block_ops.h, addon_sort.h) and louvain.hip shares with
// leiden.hip (community_ops.h).  Built and loaded by tests/helpers/prim_probe.py; never part of the product.
#include "addon_sort.h"
#include "block_ops.h"
#include "common.h"
#include "community_ops.h"

namespace {

// block b: the 256 partials a[256 b + t] and b2[256 b + t]; out[4 b ..] = sum(a), sum(b2), max(a), max(b2), one after the other
// through ONE LDS buffer
__global__ __launch_bounds__(256) void k_probe_block(const double* __restrict__ a, const double* __restrict__ b2, double* __restrict__ out) {
  __shared__ double s[256];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const double x = a[i], y = b2[i];
  const double sx = gficf_block_sum_f64(x, s), sy = gficf_block_sum_f64(y, s);
  const double mx = gficf_block_max_f64(x, s), my = gficf_block_max_f64(y, s);
  if (threadIdx.x == 0) {
    double* o = out + 4 * (int64_t)blockIdx.x;
    o[0] = sx; o[1] = sy; o[2] = mx; o[3] = my;
  }
}

// block b sorts data[np2 b .. np2 (b + 1)) in LDS
__global__ __launch_bounds__(256) void k_probe_lds_sort(gficf_u64* __restrict__ data, int np2) {
  extern __shared__ __align__(16) unsigned char probe_lds[];
  gficf_u64* a = (gficf_u64*)probe_lds;
  gficf_u64* mine = data + (int64_t)blockIdx.x * np2;
  for (int i = threadIdx.x; i < np2; i += 256) a[i] = mine[i];
  __syncthreads();
  gficf_lds_sort_u64(a, np2);
  for (int i = threadIdx.x; i < np2; i += 256) mine[i] = a[i];
}

template <typename T, typename I>
__global__ __launch_bounds__(256) void k_probe_lower(const T* __restrict__ a, I n, const T* __restrict__ q, int64_t m, I* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) out[i] = gficf_lower_bound(a, n, q[i]);
}

// One wave and a table of 256 slots with 64 guard entries behind it.  Round r: lane l brings community c[64 r + l] (negative:
// the lane sits the round out) with weight w[64 r + l]; slot / own = what gficf_comm_insert reported.  The table and its guard
// are copied out at the end (320 entries each).
constexpr int PROBE_SLOTS = 256, PROBE_GUARD = 64;
__global__ __launch_bounds__(64) void k_probe_insert(int rounds, const int32_t* __restrict__ c, const gficf_u64* __restrict__ w, int32_t* __restrict__ slot,
                                                     int32_t* __restrict__ own, int32_t* __restrict__ key_out, gficf_u64* __restrict__ val_out) {
  __shared__ int32_t key[PROBE_SLOTS + PROBE_GUARD];
  __shared__ gficf_u64 val[PROBE_SLOTS + PROBE_GUARD];
  const int lane = threadIdx.x;
  for (int t = lane; t < PROBE_SLOTS + PROBE_GUARD; t += 64) { key[t] = t < PROBE_SLOTS ? -1 : 0x5A5A5A5A; val[t] = t < PROBE_SLOTS ? 0ull : 0x5A5A5A5A5A5A5A5Aull; }
  GFICF_WAVE_SYNC();
  for (int r = 0; r < rounds; ++r) {
    const int i = r * 64 + lane;
    if (c[i] >= 0) {
      bool o = false;
      slot[i] = gficf_comm_insert<PROBE_SLOTS>(key, val, c[i], w[i], &o);
      own[i] = o ? 1 : 0;
    }
    GFICF_WAVE_SYNC();
  }
  for (int t = lane; t < PROBE_SLOTS + PROBE_GUARD; t += 64) { key_out[t] = key[t]; val_out[t] = val[t]; }
}

}  // namespace

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

// The grouped f64 sort of addon_sort.h through buffers carved as the add-ons carve them: gficf_sort_bufs::take for n elements
// (all with 64-bit keys) and the one group width.  ws == NULL: only *total (the block to allocate) is written.  Otherwise
// offs[0 .. 6) = the byte offsets of key, kv0, kv1, hist, okey, oval in ws, and the sort of v[0 .. n) is enqueued.
int probe_sort_f64(void* ctx, void* ws, int64_t n, const double* v, int desc, const int32_t* mask, uint32_t* status, uint32_t st_bit, int32_t* count,
                   const uint32_t* group, uint32_t G, int group_bits, int64_t* offs, int64_t* total) {
  gficf_carver cv;
  cv.base = (char*)ws;
  gficf_sort_bufs s;
  if (group_bits) s.take(cv, (size_t)n, (size_t)n, {group_bits});
  else s.take(cv, (size_t)n, (size_t)n, {});
  *total = (int64_t)cv.total();
  if (!ws) return GFICF_OK;
  const void* p[6] = {s.key, s.kv0, s.kv1, s.hist, s.okey, s.oval};
  for (int i = 0; i < 6; ++i) offs[i] = (int64_t)((const char*)p[i] - (const char*)ws);
  return gficf_sort_f64((gficf_ctx*)ctx, s, n, {v, desc, mask, status, st_bit, count, group, G, group_bits});
}

// nblocks x 256 partials each of a and b -> out[4 * nblocks]
int probe_block_ops(void* ctx, const double* a, const double* b, int64_t nblocks, double* out) {
  hipLaunchKernelGGL(k_probe_block, dim3((unsigned)nblocks), dim3(256), 0, ((gficf_ctx*)ctx)->stream, a, b, out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// nblocks lists of np2 (a power of two, at most 8192) keys each, sorted in place
int probe_lds_sort_u64(void* ctx, void* data, int np2, int64_t nblocks) {
  if (np2 < 1 || np2 > 8192 || (np2 & (np2 - 1))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "np2 = %d", np2);
  const size_t lds = sizeof(gficf_u64) * (size_t)np2;
  GFICF_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_probe_lds_sort), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_probe_lds_sort, dim3((unsigned)nblocks), dim3(256), lds, ((gficf_ctx*)ctx)->stream, (gficf_u64*)data, np2);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int probe_lower_bound_f64(void* ctx, const double* a, int64_t n, const double* q, int64_t m, int64_t* out) {
  hipLaunchKernelGGL((k_probe_lower<double, int64_t>), dim3(gficf_grid_1d(m)), dim3(256), 0, ((gficf_ctx*)ctx)->stream, a, n, q, m, out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int probe_lower_bound_u32(void* ctx, const uint32_t* a, int n, const uint32_t* q, int64_t m, int* out) {
  hipLaunchKernelGGL((k_probe_lower<uint32_t, int>), dim3(gficf_grid_1d(m)), dim3(256), 0, ((gficf_ctx*)ctx)->stream, a, n, q, m, out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// The numbering by decreasing size of community_ops.h through buffers carved as louvain.hip and leiden.hip carve them.
// ws == NULL: only *total (the block to allocate) is written.  Otherwise offs[0 .. 5) = the byte offsets of kv[0], kv[1], key,
// id, hist in ws, and the numbering of the labels [0, C) of N vertices is enqueued.
int probe_comm_number(void* ctx, void* ws, int64_t C, int64_t N, const int32_t* cnt, const int32_t* lab, int32_t* rank, int32_t* out, int64_t* offs,
                      int64_t* total) {
  gficf_carver cv;
  cv.base = (char*)ws;
  gficf_comm_sort_bufs s;
  s.take(cv, (size_t)(N > 0 ? N : 1), N);
  *total = (int64_t)cv.total();
  if (!ws) return GFICF_OK;
  const void* p[5] = {s.kv[0], s.kv[1], s.key, s.id, s.hist};
  for (int i = 0; i < 5; ++i) offs[i] = (int64_t)((const char*)p[i] - (const char*)ws);
  const int rc = gficf_comm_number_by_size((gficf_ctx*)ctx, C, N, cnt, lab, s, rank, out);
  if (rc) return rc;
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

// `rounds` rounds of 64 inserts by one wave into one 256-slot table (k_probe_insert)
int probe_comm_insert(void* ctx, int rounds, const int32_t* c, const unsigned long long* w, int32_t* slot, int32_t* own, int32_t* key_out,
                      unsigned long long* val_out) {
  hipLaunchKernelGGL(k_probe_insert, dim3(1), dim3(64), 0, ((gficf_ctx*)ctx)->stream, rounds, c, w, slot, own, key_out, val_out);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

unsigned probe_grid_capped(int64_t n, int64_t per, unsigned cap) { return gficf_grid_capped(n, per, cap); }

unsigned probe_grid_1d(int64_t n) { return gficf_grid_1d(n); }

}  // extern "C"
