// spectral_ritz_probe.cpp — extern "C" wrappers over the three functions of gficf_amd/csrc/spectral_ritz.h, for ctypes
// (tests/test_spectral_ritz_cpu.py builds it with the host compiler; no GPU, no HIP).  With -DSPECTRAL_RITZ_PROBE_MAIN it is a
// stand-alone program that runs every branch once, the form in which the header can be put under the host sanitizers.
#include "spectral_ritz.h"

extern "C" {

// returns n and live[:n]; with n >= b also ev[:n], Zfull (me x n), theta[:b] and *pass
int probe_sp_ritz(int me, int keep, int bw, int b, int ldh, const double* kept, const double* hH, const int32_t* hflags, const double* hG, double tol,
                  int* live, double* ev, double* Zfull, double* theta, int* pass) {
  SpRitz r;
  const int n = sp_ritz(me, keep, bw, b, ldh, kept, hH, hflags, hG, tol, r);
  std::copy(r.live.begin(), r.live.end(), live);
  if (n < b) return n;
  std::copy(r.ev.begin(), r.ev.end(), ev);
  std::copy(r.Zfull.begin(), r.Zfull.end(), Zfull);
  std::copy(r.theta.begin(), r.theta.end(), theta);
  *pass = r.pass ? 1 : 0;
  return n;
}

void probe_sp_final_rotation(int me, int n, int b, const double* Zfull, double* up) {
  SpRitz r;
  r.n = n;
  r.Zfull.assign(Zfull, Zfull + (size_t)me * n);
  std::vector<double> u;
  sp_final_rotation(r, me, b, u);
  std::copy(u.begin(), u.end(), up);
}

// returns kp; sel[:kp], up (me x kp), zl (b x b), kept[:kp]
int probe_sp_restart_choice(int n, int me, int keep, int bw, int b, int mc, const double* Zfull, const double* ev, int* sel, double* up, double* zl,
                            double* kept) {
  SpRitz r;
  r.n = n;
  r.Zfull.assign(Zfull, Zfull + (size_t)me * n);
  r.ev.assign(ev, ev + n);
  SpRestart o;
  sp_restart_choice(r, me, keep, bw, b, mc, o);
  std::copy(o.sel.begin(), o.sel.end(), sel);
  std::copy(o.up.begin(), o.up.end(), up);
  std::copy(o.zl.begin(), o.zl.end(), zl);
  std::copy(o.kept.begin(), o.kept.end(), kept);
  return o.kp;
}

}  // extern "C"

#ifdef SPECTRAL_RITZ_PROBE_MAIN
#include <cstdio>
#include <limits>

// every block width at me = b .. 64: a first cycle (NaN below the diagonal), dropped columns down to fewer than b, a restarted
// cycle (NaN in the kept columns of H), the estimate at both verdicts, both restart choices, and kp == n
int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  uint64_t seed = 1;
  auto rnd = [&] { seed = seed * 6364136223846793005ull + 1442695040888963407ull; return (double)(seed >> 11) / 9007199254740992.0 - 0.5; };
  int runs = 0, bad = 0;
  for (int b : {1, 2, 3, 8})
    for (int me = b; me <= 64; me += (me < 3 * b + 3 ? 1 : 13))
      for (int variant = 0; variant < 4; ++variant) {                                 // 0: first cycle, 1: dropped, 2: restarted, 3: too few live
        const int keep = variant == 2 && me > b + 2 ? b + 2 : 0, bw = std::min(b, me - keep), ldh = me + 3;
        std::vector<double> hH((size_t)ldh * me, nan), hG((size_t)b * b), kept((size_t)keep);
        std::vector<int32_t> flags((size_t)me, 1);
        for (int j = keep; j < me; ++j)
          for (int i = 0; i <= j; ++i) hH[(size_t)i + (size_t)ldh * j] = rnd();
        for (int x = 0; x < b; ++x)
          for (int y = 0; y <= x; ++y) hG[(size_t)x * b + y] = hG[(size_t)y * b + x] = x == y ? 1.0 : 0.1 * rnd();
        for (int l = 0; l < keep; ++l) kept[(size_t)l] = 1.0 - 0.1 * l;
        if (variant == 1 && me > b) flags[(size_t)(me - 1 - (me - b) / 2)] = 0;
        if (variant == 3)
          for (int j = b - 1; j < me; ++j) flags[(size_t)j] = 0;
        std::vector<int> live((size_t)me), sel((size_t)b + 2);
        std::vector<double> ev((size_t)me), Z((size_t)me * me), theta((size_t)b), up((size_t)me * (b + 2)), zl((size_t)b * b), kp_ev((size_t)b + 2);
        int pass = -1;
        const int n = probe_sp_ritz(me, keep, bw, b, ldh, kept.data(), hH.data(), flags.data(), hG.data(), variant == 0 ? 1e-4 : 1e4, live.data(),
                                    ev.data(), Z.data(), theta.data(), &pass);
        ++runs;
        if (n < b) { bad += variant != 3; continue; }
        for (int l = 0; l < n; ++l) bad += !std::isfinite(ev[(size_t)l]) || (l > 0 && ev[(size_t)l] > ev[(size_t)l - 1]);
        for (size_t t = 0; t < (size_t)me * n; ++t) bad += !std::isfinite(Z[t]);
        bad += pass != 0 && pass != 1;
        probe_sp_final_rotation(me, n, b, Z.data(), up.data());
        for (int mc : {me, 3 * b + 2 + me}) {                                         // the carried-weight rule where it applies, and the identity
          const int kp = probe_sp_restart_choice(n, me, keep, bw, b, mc, Z.data(), ev.data(), sel.data(), up.data(), zl.data(), kp_ev.data());
          bad += kp != std::min(b + 2, n);
          for (int l = 0; l < kp; ++l) bad += sel[(size_t)l] < 0 || sel[(size_t)l] >= n || kp_ev[(size_t)l] != ev[(size_t)sel[(size_t)l]];
        }
      }
  std::printf("%d runs, %d failed checks\n", runs, bad);
  return bad ? 1 : 0;
}
#endif
