// gsea_exact.hip — the exact one-sided tail of the enrichment score at gseaParam = 0: P(maxP >= x) or P(minP <= x) over the
// m-subsets of G positions, a lattice-path count run as a first-passage recurrence in f64.  Built into libgficf_gsea_exact.so,
// which links libgficf_hip.so and uses its context, pool and error plumbing (include/gficf_gsea_exact.h states the contract,
// the arithmetic and the order of the additions).
//
// Launches, all on the context's stream:
//   k_gx_prepare     inv_t = 1 / (G - t) for t in [0, G); per pair the deferred checks and the tails that need no sweep
//                    (x == 0 -> 1; a rejected pair or a size above GFICF_GSEA_EXACT_MAX_SIZE -> NaN)
//   k_gx_tail<R>     R = 64, 32, ..., 1 (the long sweeps first): one wave per pair, the waves whose pair is not of class R
//                    leave at once.  Lane l keeps A(i, t - i) for the hit indices i in [l R, (l + 1) R) in R registers; a step
//                    is a multiply by the miss factor, a shift by one index of the hit mass (one DPP wave shift per lane) and
//                    an add.  No LDS, no barrier, no atomics on the results.
#include <cmath>

#include "addon_status.h"
#include "common.h"
#include "gficf_gsea_exact.h"

namespace {

constexpr uint32_t GX_ST_SIZE = 1u;    // a size outside [1, G - 1]
constexpr uint32_t GX_ST_VALUE = 2u;   // an enrichment score that is not finite or lies outside [-1, 1]
constexpr int GX_MAX_R = (GFICF_GSEA_EXACT_MAX_SIZE + 1) / 64;

static_assert(GX_MAX_R == 64, "the classes launched below end at R = 64");

// R of a size: the smallest power of two with 64 R >= m + 1 (m >= 1)
__device__ inline int gx_class(int32_t m) {
  int R = 1;
  while (64 * R < m + 1) R <<= 1;
  return R;
}

// is hit ip (1-based) after jp misses of the walk blocked?  x > 0: top(ip, jp) >= x.  x < 0: the walk runs over the mirrored
// set, the comparison is the set's own bottom(m - ip + 1, G - m - jp) <= x.  The expressions of k_gs_es (gsea.hip).
__device__ inline bool gx_blocked(bool pos, int32_t ip, int32_t jp, int32_t m, int32_t gm, double dm, double dgm, double inv_m, double x) {
#pragma clang fp contract(off)
  if (pos) return (double)ip / dm - (double)jp / dgm >= x;
  const double top = (double)(m - ip + 1) / dm - (double)(gm - jp) / dgm;
  return top - inv_m <= x;
}

// lane l reads lane l - 1; lane 0 reads 0.0
__device__ inline double gx_shift_up(double v) {
  const unsigned long long u = (unsigned long long)__double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)u, 0x138, 0xf, 0xf, false);           // wave_shr:1
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(u >> 32), 0x138, 0xf, 0xf, false);
  return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (unsigned long long)(uint32_t)lo));
}

__global__ __launch_bounds__(256) void k_gx_prepare(int32_t G, int64_t n, const int32_t* __restrict__ size, const double* __restrict__ es,
                                                    double* __restrict__ tail, double* __restrict__ inv, uint32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < G) inv[i] = 1.0 / (double)(G - (int32_t)i);
  if (i < n) {
    const int32_t m = size[i];
    const double x = es[i];
    const bool bad_m = m < 1 || m >= G, bad_x = !(fabs(x) <= 1.0);
    if (bad_m) atomicOr(status, GX_ST_SIZE);
    if (bad_x) atomicOr(status, GX_ST_VALUE);
    if (bad_m || bad_x || m > GFICF_GSEA_EXACT_MAX_SIZE) tail[i] = NAN;
    else if (x == 0.0) tail[i] = 1.0;
  }
}

template <int R>
__global__ __launch_bounds__(256) void k_gx_tail(int32_t G, int64_t n, const int32_t* __restrict__ size, const double* __restrict__ es,
                                                 const double* __restrict__ inv, double* __restrict__ tail) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= n) return;
  const int32_t m = size[q];
  const double x = es[q];
  if (m < 1 || m >= G || m > GFICF_GSEA_EXACT_MAX_SIZE || !(fabs(x) <= 1.0) || x == 0.0 || gx_class(m) != R) return;   // wave-uniform
  const int32_t gm = G - m;
  const double dm = (double)m, dgm = (double)gm, inv_m = 1.0 / dm;
  const bool pos = x > 0.0;
  // until[r]: the hit out of index i = lane R + r (into i + 1) is blocked in the steps t <= until[r] = J(i + 1) + i
  int32_t until[R];
  int32_t t_end = -1;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int32_t i = lane * R + r;
    int32_t u = -1;
    if (i < m && gx_blocked(pos, i + 1, 0, m, gm, dm, dgm, inv_m, x)) {
      int32_t lo = 0, hi = gm + 1;                             // blocked at lo, not at hi (gm + 1: past the last j)
      while (hi - lo > 1) {
        const int32_t mid = lo + ((hi - lo) >> 1);
        if (gx_blocked(pos, i + 1, mid, m, gm, dm, dgm, inv_m, x)) lo = mid; else hi = mid;
      }
      u = lo + i;
    }
    until[r] = u;
    t_end = u > t_end ? u : t_end;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    const int32_t o = __shfl_xor(t_end, d);
    t_end = o > t_end ? o : t_end;
  }
  t_end = __builtin_amdgcn_readfirstlane(t_end);               // <= G - 1: J <= G - m and i <= m - 1
  double a[R];
#pragma unroll
  for (int r = 0; r < R; ++r) a[r] = 0.0;
  if (lane == 0) a[0] = 1.0;
  const double hcb = (double)(m - lane * R);                   // m - i of the lane's first index
  double mcb = (double)(gm + lane * R);                        // G - m - j = G - m - t + i of the lane's first index, at t = 0
  double part = 0.0;
  for (int32_t t = 0; t <= t_end; ++t) {
    const double w = inv[t];
    const double hl = a[R - 1] * ((hcb - (double)(R - 1)) * w);
    const double cl = t > until[R - 1] ? hl : 0.0;
    part += hl - cl;
    const double cin = gx_shift_up(cl);
#pragma unroll
    for (int r = R - 1; r >= 1; --r) {
      const double h = a[r - 1] * ((hcb - (double)(r - 1)) * w);
      const double c = t > until[r - 1] ? h : 0.0;
      part += h - c;
      a[r] = a[r] * ((mcb + (double)r) * w) + c;
    }
    a[0] = a[0] * (mcb * w) + cin;
    mcb -= 1.0;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) part += __shfl_xor(part, d);
  if (lane == 0) tail[q] = part;
}

struct GxWs {
  uint32_t* status;
  double* inv;
};

static size_t gx_carve(char* base, int64_t G, GxWs& w) {
  gficf_carver cv;
  cv.base = base;
  w.status = cv.take<uint32_t>(1);
  w.inv = cv.take<double>((size_t)G);
  return cv.total();
}

static int gx_check_sizes(int64_t G, int64_t n) {
  if (G < 2 || n < 0) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "G = %lld, n = %lld: a size is out of range", (long long)G, (long long)n);
  if (G > GFICF_GSEA_EXACT_MAX_G) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "G = %lld genes: at most %d", (long long)G, GFICF_GSEA_EXACT_MAX_G);
  if (n > INT32_MAX) GFICF_FAIL(GFICF_ERR_UNSUPPORTED, "more than 2^31 - 1 pairs");
  return GFICF_OK;
}

template <int R>
static void gx_launch(hipStream_t st, int64_t G, int64_t n, const int32_t* d_size, const double* d_es, const double* inv, double* d_tail) {
  hipLaunchKernelGGL(k_gx_tail<R>, dim3((unsigned)gficf_ceil_div(n, 4)), dim3(256), 0, st, (int32_t)G, n, d_size, d_es, inv, d_tail);
}

}  // namespace

extern "C" {

int gficf_gsea_exact_abi_version(void) { return GFICF_GSEA_EXACT_ABI_VERSION; }

size_t gficf_gsea_tail_workspace_bytes(int64_t G, int64_t n) {
  if (G < 2 || n < 0 || G > GFICF_GSEA_EXACT_MAX_G || n > INT32_MAX) return 0;
  GxWs w;
  return gx_carve(nullptr, G, w);
}

int gficf_gsea_tail_device(gficf_ctx* ctx, int64_t G, int64_t n, const int32_t* d_size, const double* d_es, double* d_tail, void* ws,
                           size_t ws_bytes) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(gx_check_sizes(G, n));
  if (!ws || (n > 0 && (!d_size || !d_es || !d_tail))) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL device pointer");
  GxWs w;
  GFICF_RC(gficf_addon_carve(ws, ws_bytes, [&](char* base) { return gx_carve(base, G, w); }));
  hipStream_t st = ctx->stream;
  GFICF_HIP_CHECK(hipMemsetAsync(w.status, 0, sizeof(uint32_t), st));
  if (n == 0) return GFICF_OK;
  hipLaunchKernelGGL(k_gx_prepare, dim3((unsigned)gficf_ceil_div(G > n ? G : n, 256)), dim3(256), 0, st, (int32_t)G, n, d_size, d_es, d_tail, w.inv,
                     w.status);
  GFICF_HIP_CHECK(hipGetLastError());
  gx_launch<64>(st, G, n, d_size, d_es, w.inv, d_tail);
  gx_launch<32>(st, G, n, d_size, d_es, w.inv, d_tail);
  gx_launch<16>(st, G, n, d_size, d_es, w.inv, d_tail);
  gx_launch<8>(st, G, n, d_size, d_es, w.inv, d_tail);
  gx_launch<4>(st, G, n, d_size, d_es, w.inv, d_tail);
  gx_launch<2>(st, G, n, d_size, d_es, w.inv, d_tail);
  gx_launch<1>(st, G, n, d_size, d_es, w.inv, d_tail);
  GFICF_HIP_CHECK(hipGetLastError());
  return GFICF_OK;
}

int gficf_gsea_tail_sync(gficf_ctx* ctx, const void* ws) {
  uint32_t st;
  GFICF_RC(gficf_addon_read_status(ctx, ws, &st));
  if (st & GX_ST_SIZE) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "a set size outside [1, G - 1]");
  if (st & GX_ST_VALUE) GFICF_FAIL(GFICF_ERR_BAD_VALUE, "an enrichment score that is not finite or lies outside [-1, 1]");
  return GFICF_OK;
}

int gficf_gsea_tail_host(gficf_ctx* ctx, int64_t G, int64_t n, const int32_t* size, const double* es, double* tail) {
  GFICF_CTX_ENTER(ctx);
  GFICF_RC(gx_check_sizes(G, n));
  if (n > 0 && (!size || !es || !tail)) GFICF_FAIL(GFICF_ERR_INVALID_ARG, "NULL pointer");
  const size_t wsb = gficf_gsea_tail_workspace_bytes(G, n), cnt = (size_t)(n > 0 ? n : 1);
  gficf_host_io io{ctx, "gficf_gsea_tail_host"};
  gficf_carver cv;
  int32_t* d_size; double *d_es, *d_tail; char* d_ws;
  for (int pass = 0; pass < 2 && io.ok(); ++pass) {
    d_size = cv.take<int32_t>(cnt); d_es = cv.take<double>(cnt); d_tail = cv.take<double>(cnt);
    d_ws = cv.take<char>(wsb);
    if (pass == 0) io.e = cv.bind(ctx, GFICF_SLOT_STAGE0);
  }
  io.up(d_size, size, sizeof(int32_t) * (size_t)n);
  io.up(d_es, es, sizeof(double) * (size_t)n);
  int rc = GFICF_OK;
  if (io.ok()) {
    rc = gficf_gsea_tail_device(ctx, G, n, d_size, d_es, d_tail, d_ws, wsb);
    if (!rc) io.down(tail, d_tail, sizeof(double) * (size_t)n);
  }
  if (!io.ok() || rc) return io.drain(rc);
  return gficf_gsea_tail_sync(ctx, d_ws);
}

}  // extern "C"
