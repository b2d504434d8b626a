// umap_force.h — the arithmetic a UMAP sweep applies to one running position, shared by umap.hip (k_um_epoch) and transform.hip
// (k_tr_layout): include/gficf_umap.h states it operation by operation and include/gficf_transform.h promises the same, so both
// are built from this one text (each with -ffp-contract=off).
// The force functions read a, b, m2ab (-2ab) and g2b (2 gamma b) from the caller's own parameter struct (UmLay, TrLay).
#pragma once

#include "common.h"

namespace {

typedef unsigned long long u64;

// a distance as the graph takes it: the cosine and correlation metrics of the search (1 - cos in f32) can round a hair below 0
__device__ inline float uf_dist(float d) { return fmaxf(d, 0.f); }

__device__ inline u64 uf_mix(u64 z) {         // the splitmix64 finaliser
  z ^= z >> 30; z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27; z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

__device__ inline float uf_clip(float x) { return fminf(fmaxf(x, -4.f), 4.f); }

template <bool T1, class Lay>
__device__ inline void uf_attract(float& yx, float& yy, float jx, float jy, float alpha, const Lay& L) {
  const float dx = yx - jx, dy = yy - jy, d2 = dx * dx + dy * dy;
  float coef = 0.f;
  if (d2 > 0.f) {
    if (T1) {
      coef = -2.f / (d2 + 1.f);
    } else {
      const float pd = powf(d2, L.b);
      coef = (L.m2ab * pd) / (d2 * (L.a * pd + 1.f));
    }
  }
  yx += alpha * uf_clip(coef * dx);
  yy += alpha * uf_clip(coef * dy);
}

template <bool T1, class Lay>
__device__ inline void uf_repulse(float& yx, float& yy, float jx, float jy, float alpha, const Lay& L) {
  const float dx = yx - jx, dy = yy - jy, d2 = dx * dx + dy * dy;
  float sx = 4.f, sy = 4.f;
  if (d2 > 0.f) {
    float coef;
    if (T1) {
      coef = L.g2b / ((0.001f + d2) * (d2 + 1.f));
    } else {
      const float pd = powf(d2, L.b);
      coef = L.g2b / ((0.001f + d2) * (L.a * pd + 1.f));
    }
    sx = uf_clip(coef * dx);
    sy = uf_clip(coef * dy);
  }
  yx += alpha * sx;
  yy += alpha * sy;
}

}  // namespace
