// Per-row device helpers of the wide (CSR) model shared by the evaluation /
// logits kernels (wide_kernels.hip) and the scoring kernel (score_kernels.hip):
// the KP weights of one feature, one row's margins with a wave per row, and the
// evaluation's argmax rule.
#pragma once
#include "common.h"

namespace psx {

template <int KP>
__device__ __forceinline__ void ldk(const float* __restrict__ p, float (&o)[KP]) {
  if constexpr (KP % 4 == 0) {
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) {
      const f32x4 t = *(const f32x4*)(p + 4 * q);
      o[4 * q] = t[0];
      o[4 * q + 1] = t[1];
      o[4 * q + 2] = t[2];
      o[4 * q + 3] = t[3];
    }
  } else if constexpr (KP == 2) {
    const float2 t = *(const float2*)p;
    o[0] = t.x;
    o[1] = t.y;
  } else {
    o[0] = p[0];
  }
}

template <int KP>
__device__ __forceinline__ void wide_row_margins(int64_t F, const int64_t* __restrict__ indptr,
                                                 const int32_t* __restrict__ idx, const uint16_t* __restrict__ val,
                                                 int64_t row, const float* __restrict__ w, float (&z)[KP]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < KP; ++k) z[k] = 0.f;
  const int64_t a = indptr[row], b = indptr[row + 1];
  for (int64_t e = a + lane; e < b; e += 64) {
    const int f = idx[e];
    const float v = bf2f(val[e]);
    float wv[KP];
    ldk<KP>(w + (int64_t)f * KP, wv);
#pragma unroll
    for (int k = 0; k < KP; ++k) z[k] += v * wv[k];
  }
#pragma unroll
  for (int k = 0; k < KP; ++k) z[k] = wave_sum(z[k]);
  float bv[KP];
  ldk<KP>(w + F * KP, bv);
#pragma unroll
  for (int k = 0; k < KP; ++k) z[k] += bv[k];
}

template <int KP>
__device__ __forceinline__ int wide_argmax(int K, const float (&z)[KP]) {
  if (K == 1) return z[0] > 0.f ? 1 : 0;
  int best = 0;
  float bz = -INFINITY;
#pragma unroll
  for (int k = 0; k < KP; ++k)
    if (k < K && z[k] > bz) {
      bz = z[k];
      best = k;
    }
  return best;
}

}  // namespace psx
