// spectral_ritz.h — the host mathematics of the spectral solve (spectral.hip, SpRun): what happens between a cycle's read-back and
// the next upload.  sp_ritz (Rayleigh-Ritz on the live columns, the residual estimate), sp_final_rotation (Z[:, :b]) and
// sp_restart_choice (which Ritz vectors a thick restart keeps), on top of sp_jacobi.  Plain C++17 and the standard library: no
// GPU header, so tests/helpers/spectral_ritz_probe.cpp compiles it with the host compiler (tests/test_spectral_ritz_cpu.py).
// Every sum runs in the order written here: the bits of the solve depend on it.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

// eigen-decomposition of the symmetric n x n matrix A (row-major, destroyed): cyclic Jacobi, rows and columns swept in a fixed
// order.  ev: the eigenvalues in DESCENDING order, Z (n x n row-major): column l the vector of ev[l].
static inline void sp_jacobi(std::vector<double>& A, int n, std::vector<double>& ev, std::vector<double>& Z) {
  std::vector<double> Q((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) Q[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i)
      for (int j = 0; j < n; ++j) (i == j ? diag : off) += A[(size_t)i * n + j] * A[(size_t)i * n + j];
    if (off <= 1e-32 * diag || off == 0.0) break;
    for (int p = 0; p < n - 1; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = A[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double tau = (A[(size_t)q * n + q] - A[(size_t)p * n + p]) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
        const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = A[(size_t)k * n + p], akq = A[(size_t)k * n + q];
          A[(size_t)k * n + p] = c * akp - s * akq;
          A[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = A[(size_t)p * n + k], aqk = A[(size_t)q * n + k];
          A[(size_t)p * n + k] = c * apk - s * aqk;
          A[(size_t)q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double qkp = Q[(size_t)k * n + p], qkq = Q[(size_t)k * n + q];
          Q[(size_t)k * n + p] = c * qkp - s * qkq;
          Q[(size_t)k * n + q] = s * qkp + c * qkq;
        }
      }
  }
  std::vector<int> order((size_t)n);
  for (int i = 0; i < n; ++i) order[(size_t)i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return A[(size_t)x * n + x] > A[(size_t)y * n + y]; });
  ev.assign((size_t)n, 0.0);
  Z.assign((size_t)n * n, 0.0);
  for (int l = 0; l < n; ++l) {
    ev[(size_t)l] = A[(size_t)order[(size_t)l] * n + order[(size_t)l]];
    for (int k = 0; k < n; ++k) Z[(size_t)k * n + l] = Q[(size_t)k * n + order[(size_t)l]];
  }
}

// a residual norm against its bound: tol x max(|theta|, eps^(2/3))
static inline bool sp_within_tol(double resid, double theta, double tol) {
  const double eps23 = std::pow(2.0, -52.0 * 2.0 / 3.0);
  return resid <= tol * std::max(std::fabs(theta), eps23);
}

// how many Ritz vectors a thick restart keeps out of n
static inline int sp_keep_count(int b, int n) { return std::min(b + 2, n); }

struct SpRitz {
  int n = 0;                    // live columns
  bool pass = false;            // every estimate of the leading b within tol
  std::vector<int> live;
  std::vector<double> ev;       // n, descending
  std::vector<double> Zfull;    // me x n row-major: the row of a column that is not live is zero
  std::vector<double> theta;    // b: what finish() uploads, untouched until its synchronisation
  std::vector<double> A, Z;     // scratch
};

// Rayleigh-Ritz on the live columns of a cycle of me columns (a column < keep, or one whose flag is set).  The projected matrix:
// diag(kept) on the keep kept columns, zero off it there; elsewhere hH (element (i, j) at i + ldh j, read for i <= j only).  The
// estimate of pair l: sqrt(z' G z), z the last bw rows of column l, hG (b x b, (x, y) at x b + y) the Gram matrix of the last
// remainder.  Returns n; n < b (too few directions for the caller) leaves everything but live and n as it was.
static inline int sp_ritz(int me, int keep, int bw, int b, int ldh, const double* kept, const double* hH, const int32_t* hflags, const double* hG, double tol,
                          SpRitz& r) {
  r.live.clear();
  for (int j = 0; j < me; ++j)
    if (j < keep || hflags[j]) r.live.push_back(j);
  const int n = r.n = (int)r.live.size();
  if (n < b) return n;
  const std::vector<int>& live = r.live;
  r.A.assign((size_t)n * n, 0.0);
  for (int x = 0; x < n; ++x)
    for (int y = x; y < n; ++y) {
      const int i = live[(size_t)x], j = live[(size_t)y];
      const double h = j < keep ? (i == j ? kept[i] : 0.0) : hH[(size_t)i + (size_t)ldh * (size_t)j];
      r.A[(size_t)x * n + y] = r.A[(size_t)y * n + x] = h;
    }
  sp_jacobi(r.A, n, r.ev, r.Z);
  std::vector<double>& Zfull = r.Zfull;
  Zfull.assign((size_t)me * n, 0.0);
  for (int x = 0; x < n; ++x)
    for (int l = 0; l < n; ++l) Zfull[(size_t)live[(size_t)x] * n + l] = r.Z[(size_t)x * n + l];
  r.theta.assign((size_t)b, 0.0);
  r.pass = true;
  for (int l = 0; l < b; ++l) {
    double s = 0.0;
    for (int x = 0; x < bw; ++x)
      for (int y = 0; y < bw; ++y) s += Zfull[(size_t)(me - bw + x) * n + l] * hG[(size_t)x * b + y] * Zfull[(size_t)(me - bw + y) * n + l];
    r.theta[(size_t)l] = r.ev[(size_t)l];
    r.pass = r.pass && sp_within_tol(std::sqrt(s > 0.0 ? s : 0.0), r.ev[(size_t)l], tol);
  }
  return n;
}

// up = Zfull[:, :b], me x b row-major: X = V up
static inline void sp_final_rotation(const SpRitz& r, int me, int b, std::vector<double>& up) {
  up.assign((size_t)me * b, 0.0);
  for (int j = 0; j < me; ++j)
    for (int l = 0; l < b; ++l) up[(size_t)j * b + l] = r.Zfull[(size_t)j * r.n + l];
}

struct SpRestart {
  int kp = 0;                   // kept Ritz vectors
  std::vector<int> sel;         // which: kp columns of Zfull
  std::vector<double> up, zl;   // Zfull[:, sel] (me x kp) and the last bw rows of Zfull[:, :b] (b x b, rows >= bw zero): uploaded
  std::vector<double> kept;     // ev[sel]: the leading diagonal of the next cycle's projected matrix
};

// thick restart: the leading kp Ritz vectors; the residuals of the leading b (W_last zl) become the next block
static inline void sp_restart_choice(const SpRitz& r, int me, int keep, int bw, int b, int mc, SpRestart& o) {
  const int n = r.n, kp = o.kp = sp_keep_count(b, n);
  const std::vector<double>& Zfull = r.Zfull;
  std::vector<int>& sel = o.sel;
  sel.assign((size_t)kp, 0);
  for (int l = 0; l < kp; ++l) sel[(size_t)l] = l;
  if (keep > 0 && n > kp && mc - kp < 2 * b) {
    // one block per restarted cycle: the extra kept vectors are the Ritz vectors that carry most of the last leading b (rows < b of Z)
    std::vector<double> carried((size_t)n, -1.0);
    for (int l = b; l < n; ++l) {
      double s = 0.0;
      for (int i = 0; i < b; ++i) s += Zfull[(size_t)i * n + l] * Zfull[(size_t)i * n + l];
      carried[(size_t)l] = s;
    }
    for (int x = b; x < kp; ++x) {
      int at = -1;
      for (int l = b; l < n; ++l)
        if (carried[(size_t)l] >= 0.0 && (at < 0 || carried[(size_t)l] > carried[(size_t)at])) at = l;   // strict: the lowest index on ties
      sel[(size_t)x] = at;
      carried[(size_t)at] = -1.0;
    }
    std::sort(sel.begin() + b, sel.end());
  }
  o.up.assign((size_t)me * kp, 0.0);
  for (int j = 0; j < me; ++j)
    for (int l = 0; l < kp; ++l) o.up[(size_t)j * kp + l] = Zfull[(size_t)j * n + sel[(size_t)l]];
  o.zl.assign((size_t)b * b, 0.0);
  for (int x = 0; x < bw; ++x)
    for (int l = 0; l < b; ++l) o.zl[(size_t)x * b + l] = Zfull[(size_t)(me - bw + x) * n + l];
  o.kept.assign((size_t)kp, 0.0);
  for (int l = 0; l < kp; ++l) o.kept[(size_t)l] = r.ev[(size_t)sel[(size_t)l]];
}
