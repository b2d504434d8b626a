// radix_sort.hip — the library's one sort: stable LSD passes over 8-byte elements key << 32 | value, by the key's low b bits.
//
// Users: the adjacency build (destination << 32 | edge number, b = bits of N), the pruned kNN search's cell layout and
// gficf_knn_pivot_order_device ((coarse, fine) pivot key << 32 | point index, b = 20), and the final numbering of Louvain's clusters
// ((N - size) << 32 | cluster, b = bits of N: stable on clusters laid out in id order, so ties keep the smaller id first).
#include "common.h"

namespace {

typedef unsigned long long u64;

// Stable partition passes, least significant digit first (round 6, for the adjacency build: a library onesweep sort took three 8-bit passes
// for the 17 bits of 100 k cells; digits of up to 10 bits make it two).  A pass = per-workgroup digit counts
// (k_rs_hist) -> one scan of the [digit][workgroup] matrix -> k_rs_scatter.  Stable by construction: a workgroup owns RS_TILE consecutive
// elements, its wave w the w-th quarter, a wave walks its quarter 64 consecutive elements at a time; an element's place = the scanned
// count of its (digit, workgroup) + the earlier waves' elements of that digit + the wave's own earlier ones + the lower lanes' in its round.
constexpr int RS_TILE = 4096;
constexpr int RS_MAX_BITS = 10;
constexpr int RS_MAX_WGS = 768;           // workgroups of a pass (each walks ceil(tiles / RS_MAX_WGS) tiles): bounds the count matrix, and is what is resident at
                                          // once (52 KB of LDS a workgroup: three a CU) — a grid beyond that runs as one and a fraction rounds

__device__ inline unsigned rs_digit(u64 el, int shift, unsigned mask) { return (unsigned)(el >> (32 + shift)) & mask; }

__global__ __launch_bounds__(256) void k_rs_hist(const u64* __restrict__ in, int64_t M, int shift, int bits, int64_t tiles_per_wg,
                                                 int64_t* __restrict__ hist) {
  __shared__ unsigned cnt[1 << RS_MAX_BITS];
  const unsigned nb = 1u << bits, mask = nb - 1u;
  for (unsigned d = threadIdx.x; d < nb; d += 256) cnt[d] = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * tiles_per_wg * RS_TILE;
  int64_t end = base + tiles_per_wg * RS_TILE;
  if (end > M) end = M;
  for (int64_t i0 = base + threadIdx.x; i0 < end; i0 += 256 * 8) {      // eight loads in flight
    u64 v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { const int64_t i = i0 + 256 * j; v[j] = in[i < end ? i : end - 1]; }
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (i0 + 256 * j < end) atomicAdd(&cnt[rs_digit(v[j], shift, mask)], 1u);
  }
  __syncthreads();
  for (unsigned d = threadIdx.x; d < nb; d += 256) hist[(int64_t)d * gridDim.x + blockIdx.x] = (int64_t)cnt[d];
}

// LAST: the pass writes the key and the value apart (what the callers read); otherwise the element as it is.
// A workgroup walks its tiles in order and carries every digit's next place in the output along (in the registers of the digit's
// thread).  A tile is put in order in LDS first and written out from there: consecutive threads then write consecutive places of one
// digit's run (a wave's store touches ~8 runs instead of ~50 scattered places).
template <bool LAST>
__global__ __launch_bounds__(256) void k_rs_scatter(const u64* __restrict__ in, int64_t M, int shift, int bits, int64_t tiles_per_wg,
                                                    const int64_t* __restrict__ hist, u64* __restrict__ out, uint32_t* __restrict__ okey,
                                                    uint32_t* __restrict__ oval) {
  __shared__ unsigned cnt[4][1 << RS_MAX_BITS];                // counts of (wave, digit), then the wave's next place inside the tile
  __shared__ unsigned delta[1 << RS_MAX_BITS];                 // a digit's first place inside the tile, then (its place in the output) - that
  __shared__ u64 stage[RS_TILE];
  const unsigned nb = 1u << bits, mask = nb - 1u;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned gpos[(1 << RS_MAX_BITS) / 256];                     // next output place of digit threadIdx.x + 256 j
#pragma unroll
  for (unsigned j = 0; j < (1u << RS_MAX_BITS) / 256u; ++j) {
    const unsigned d = threadIdx.x + 256u * j;
    gpos[j] = d < nb ? (unsigned)hist[(int64_t)d * gridDim.x + blockIdx.x] : 0u;
  }
  const int64_t first_tile = (int64_t)blockIdx.x * tiles_per_wg;
  for (int64_t tile = first_tile; tile < first_tile + tiles_per_wg && tile * RS_TILE < M; ++tile) {
    for (unsigned d = threadIdx.x; d < 4u * (1u << RS_MAX_BITS); d += 256) (&cnt[0][0])[d] = 0u;
    __syncthreads();
    const int64_t tbase = tile * RS_TILE, wbase = tbase + (int64_t)wave * (RS_TILE / 4);
    u64 el[RS_TILE / 256];
#pragma unroll
    for (int r = 0; r < RS_TILE / 256; ++r) {                  // (all the loads first, no branch around them: sixteen in flight)
      const int64_t idx = wbase + r * 64 + lane;
      el[r] = in[idx < M ? idx : M - 1];
    }
#pragma unroll
    for (int r = 0; r < RS_TILE / 256; ++r)
      if (wbase + r * 64 + lane < M) atomicAdd(&cnt[wave][rs_digit(el[r], shift, mask)], 1u);
    __syncthreads();
    if (wave == 0) {                                           // exclusive scan of the tile's digit counts: (nb + 63) / 64 digits a lane
      const unsigned per = (nb + 63u) / 64u;
      unsigned loc[(1 << RS_MAX_BITS) / 64];
      unsigned sum = 0;
#pragma unroll
      for (unsigned j = 0; j < (1u << RS_MAX_BITS) / 64u; ++j) {
        const unsigned d = lane * per + j;
        loc[j] = sum;
        if (j < per && d < nb) sum += cnt[0][d] + cnt[1][d] + cnt[2][d] + cnt[3][d];
      }
      unsigned inc = sum;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) { const unsigned v = __shfl_up(inc, off); if (lane >= off) inc += v; }
      const unsigned base = inc - sum;
#pragma unroll
      for (unsigned j = 0; j < (1u << RS_MAX_BITS) / 64u; ++j) {
        const unsigned d = lane * per + j;
        if (j < per && d < nb) delta[d] = base + loc[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (unsigned j = 0; j < (1u << RS_MAX_BITS) / 256u; ++j) {     // counts -> first places inside the tile, wave by wave
      const unsigned d = threadIdx.x + 256u * j;
      if (d < nb) {
        const unsigned first = delta[d];
        unsigned run = first;
#pragma unroll
        for (int w = 0; w < 4; ++w) { const unsigned c = cnt[w][d]; cnt[w][d] = run; run += c; }
        delta[d] = gpos[j] - first;
        gpos[j] += run - first;
      }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RS_TILE / 256; ++r) {
      const int64_t idx = wbase + r * 64 + lane;
      const bool valid = idx < M;
      const unsigned d = rs_digit(el[r], shift, mask);
      u64 peers = __ballot(valid);                             // the lanes of this round holding the same digit
      for (int b = 0; b < bits; ++b) {
        const bool bit = (d >> b) & 1u;
        const u64 m = __ballot(bit);
        peers &= bit ? m : ~m;
      }
      const unsigned below = (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
      const unsigned at = valid ? cnt[wave][d] + below : 0u;
      GFICF_WAVE_SYNC();
      if (valid && below == 0u) cnt[wave][d] += (unsigned)__popcll(peers);    // the lowest lane of the group moves the wave's place on
      if (valid) stage[at] = el[r];
      GFICF_WAVE_SYNC();
    }
    __syncthreads();
    const int tile_n = (int)(M - tbase < RS_TILE ? M - tbase : RS_TILE);
    for (int i = threadIdx.x; i < tile_n; i += 256) {
      const u64 e = stage[i];
      const unsigned to = (unsigned)i + delta[rs_digit(e, shift, mask)];
      if (LAST) { okey[to] = (uint32_t)(e >> 32); oval[to] = (uint32_t)e; }
      else out[to] = e;
    }
    __syncthreads();
  }
}

inline int rs_passes(int b) { return (b + RS_MAX_BITS - 1) / RS_MAX_BITS; }
inline int rs_bits(int b) { const int p = rs_passes(b); return (b + p - 1) / p; }             // digit width: the passes share the bits evenly

}  // namespace

// [digit][workgroup] counts of the first (widest) pass
int64_t gficf_radix_sort_hist_len(int64_t M, int b) {
  if (b < 1) b = 1;
  if (b > 32) b = 32;
  const int64_t tiles = M > 0 ? gficf_ceil_div(M, RS_TILE) : 1;
  return ((int64_t)1 << rs_bits(b)) * (tiles < RS_MAX_WGS ? tiles : RS_MAX_WGS);
}

int gficf_radix_sort_kv(gficf_ctx* ctx, u64* kv0, u64* kv1, int64_t* hist, int64_t M, int b, uint32_t* okey, uint32_t* oval) {
  if (b < 1 || b > 32) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "radix sort over %d key bits", b);
  if (M < 0 || M > (int64_t)UINT32_MAX) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "radix sort of %lld elements", (long long)M);
  if (M == 0) return GFICF_OK;
  const int P = rs_passes(b), bp = rs_bits(b);
  const int64_t ntiles = gficf_ceil_div(M, RS_TILE);
  const int64_t tpw = gficf_ceil_div(ntiles, RS_MAX_WGS);                  // tiles a workgroup walks
  const unsigned G = (unsigned)gficf_ceil_div(ntiles, tpw);
  u64 *in = kv0, *out = kv1;
  for (int p = 0; p < P; ++p) {
    const int shift = p * bp, bits = b - shift < bp ? b - shift : bp;
    hipLaunchKernelGGL(k_rs_hist, dim3(G), dim3(256), 0, ctx->stream, (const u64*)in, M, shift, bits, tpw, hist);
    GFICF_HIP_CHECK(hipGetLastError());
    const int rc = gficf_exclusive_scan_i64(ctx, hist, ((int64_t)1 << bits) * (int64_t)G);
    if (rc) return rc;
    if (p == P - 1)
      hipLaunchKernelGGL(k_rs_scatter<true>, dim3(G), dim3(256), 0, ctx->stream, (const u64*)in, M, shift, bits, tpw, (const int64_t*)hist,
                         (u64*)nullptr, okey, oval);
    else
      hipLaunchKernelGGL(k_rs_scatter<false>, dim3(G), dim3(256), 0, ctx->stream, (const u64*)in, M, shift, bits, tpw, (const int64_t*)hist,
                         out, (uint32_t*)nullptr, (uint32_t*)nullptr);
    GFICF_HIP_CHECK(hipGetLastError());
    u64* t = in; in = out; out = t;
  }
  return GFICF_OK;
}
