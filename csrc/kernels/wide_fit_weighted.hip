// Weighted full-batch fit kernels of the wide (CSR) model (gfx950 / CDNA4): the
// evaluation of wide_fit_kernels.hip with a weight per row and a held-out fold (the
// objective is stated in wide_fit_weighted.h).
//
//   wide_fit_weights_kernel  per row v = sample_weight * class_weight[y] and ONE fp32
//                            ueff[r] = +v (training row) or -v (held-out row); the
//                            workgroup's fp64 sums of u, of h and of the rows with u > 0
//                            -> wpart; a one-workgroup finish adds them in workgroup
//                            order into wsum = (W, W_ho, L)
//   wide_fit_stats_w_kernel  a wavefront per column over the inverted index, cells summed
//                            first: per lane sum u x, sum u, the live cells' count, min
//                            and max, combined by butterflies; a second pass for the
//                            centred squares.  A feature that takes one value on the
//                            rows of positive training weight (absent = 0) gets sigma 0
//                            EXACTLY, decided on the count against L and on min / max
//   wide_fit_rows_w_kernel   wide_fit_rows_kernel's row walk; ueff[r] is one wave-uniform
//                            load.  v == 0: no margins, a zero residual row.  Training
//                            row: R[r] = u res, the wave's sums take u res and u nll.
//                            Held-out row: R[r] = 0, the held-out sum takes v nll.  R
//                            carries the weight, so the column pass and the intercept
//                            sums are the plain kernels, launched unchanged
//   wide_fit_reduce_w_kernel, wide_fit_dots_w_kernel
//                            the plain reduction with 1/W (the device double) for 1/N,
//                            the loss over W and the held-out mean into a double of its own
// Every sum runs in an order fixed by the data and the options; no atomics, no
// cross-workgroup waits, no scratch.  With unit weights and no held-out fold every
// kernel here computes what its plain counterpart computes, bit for bit (u = 1 is
// exact in every product it enters, W = N).
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "wide_fit_weighted.h"
#include "wide_row.h"

namespace psx {

namespace {

template <int KP>
__device__ __forceinline__ void stk(float* __restrict__ p, const float (&v)[KP]) {
  if constexpr (KP % 4 == 0) {
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) *(f32x4*)(p + 4 * q) = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
  } else if constexpr (KP == 2) {
    *(float2*)p = float2{v[0], v[1]};
  } else {
    p[0] = v[0];
  }
}

// (wide_fit_kernels.hip's rule) the value of the (column, row) cell whose first entry is e
__device__ __forceinline__ double cell_value(const WideFitDev& dv, int64_t e, int64_t b) {
  const int r = dv.crow[e];
  double x = (double)bf2f(dv.cval[e]);
  for (int64_t j = e + 1; j < b && dv.crow[j] == r; ++j) x += (double)bf2f(dv.cval[j]);
  return x;
}

__device__ __forceinline__ bool held_bit(float ue) { return (__float_as_uint(ue) >> 31) != 0; }
// training weight of a row from its ueff: 0 for a held-out row (ueff <= -0.f)
__device__ __forceinline__ double train_weight(float ue) { return held_bit(ue) ? 0.0 : (double)ue; }

template <class T>
__device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T t = __shfl_xor(v, o, 64);
    v = t < v ? t : v;
  }
  return v;
}
template <class T>
__device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const T t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

}  // namespace

// ---------------------------------------------------------------------------
// Thread t of workgroup g takes rows g*256 + t, + gridDim*256, ...; lanes by
// butterfly, the 4 waves in order.
__global__ __launch_bounds__(256) void wide_fit_weights_kernel(WideFitDev dv, WideFitWeightsDev wd) {
  __shared__ double red[4][3];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  double su = 0.0, sh = 0.0, sl = 0.0;
  for (int64_t r = (int64_t)blockIdx.x * 256 + t; r < dv.N; r += (int64_t)gridDim.x * 256) {
    const int y = dv.y[r];
    float c = 0.f;  // a select chain: a table indexed by a lane's label would live in scratch
#pragma unroll
    for (int k = 0; k < 16; ++k) c = y == k ? wd.cw[k] : c;
    const float v = (wd.sw ? wd.sw[r] : 1.f) * c;
    const bool held = wd.holdout >= 0 && wd.fold && (int)wd.fold[r] == wd.holdout;
    wd.ueff[r] = held ? -v : v;  // v == 0: -0.f on a held-out row
    su += held ? 0.0 : (double)v;
    sh += held ? (double)v : 0.0;
    sl += (!held && v > 0.f) ? 1.0 : 0.0;
  }
  su = wave_sum(su);
  sh = wave_sum(sh);
  sl = wave_sum(sl);
  if (lane == 0) {
    red[wv][0] = su;
    red[wv][1] = sh;
    red[wv][2] = sl;
  }
  __syncthreads();
  if (t < 3) wd.wpart[(size_t)blockIdx.x * 3 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

__global__ __launch_bounds__(64) void wide_fit_weights_fin_kernel(WideFitWeightsDev wd, int G) {
  const int t = threadIdx.x;
  if (t >= 3) return;
  double a = 0.0;
  for (int g = 0; g < G; ++g) a += wd.wpart[(size_t)g * 3 + t];
  wd.wsum[t] = a;
}

// ---------------------------------------------------------------------------
// wide_fit_stats_kernel with a weight per cell (the row's training weight), operation
// for operation: n -> W, the cell count -> the present cells' weight.
__global__ __launch_bounds__(256) void wide_fit_stats_w_kernel(WideFitDev dv, WideFitWeightsDev wd) {
  const int lane = threadIdx.x & 63;
  const double n = wd.wsum[0], L = wd.wsum[2];
  const float* __restrict__ ueff = wd.ueff;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < dv.U; u += (int64_t)gridDim.x * 4) {
    const int64_t a = dv.colptr[u], b = dv.colptr[u + 1];
    double s = 0.0, cnt = 0.0, live = 0.0, mn = INFINITY, mx = -INFINITY;
    for (int64_t e = a + lane; e < b; e += 64) {
      if (e > a && dv.crow[e - 1] == dv.crow[e]) continue;  // not the first entry of its cell
      const double wt = train_weight(ueff[dv.crow[e]]);
      const double x = cell_value(dv, e, b);
      s += wt * x;
      cnt += wt;
      if (wt > 0.0) {
        live += 1.0;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
      }
    }
    s = wave_sum(s);
    cnt = wave_sum(cnt);
    live = wave_sum(live);
    mn = wave_min(mn);
    mx = wave_max(mx);
    const double m = s / n;
    double q = 0.0;
    for (int64_t e = a + lane; e < b; e += 64) {
      if (e > a && dv.crow[e - 1] == dv.crow[e]) continue;
      const double wt = train_weight(ueff[dv.crow[e]]);
      const double c = cell_value(dv, e, b) - m;
      const double wc = wt * c;  // (= c at weight 1: the plain kernel's c * c below)
      q += wc * c;
    }
    q = wave_sum(q);
    // one value on the live rows?  A live row without a cell holds 0.
    if (live < L) {
      mn = mn < 0.0 ? mn : 0.0;
      mx = mx > 0.0 ? mx : 0.0;
    }
    double sd = 0.0;
    if (n > 1.0 && live > 0.0 && mx > mn) {
      const double var = (q + (n - cnt) * m * m) / (n - 1.0);
      sd = var > 0.0 ? sqrt(var) : 0.0;
    }
    if (lane == 0) {
      dv.std_[u] = (float)sd;
      dv.inv_std[u] = sd > 0.0 ? (float)(1.0 / sd) : 0.f;
    }
  }
}

// ---------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void wide_fit_rows_w_kernel(WideFitDev dv, const float* __restrict__ ueff) {
  const int lane = threadIdx.x & 63, K = dv.K;
  // (the wave's index through readfirstlane: the row and everything loaded by it is wave-uniform)
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t W = (int64_t)gridDim.x * 4;
  float racc[KP], lacc = 0.f, hacc = 0.f;
#pragma unroll
  for (int k = 0; k < KP; ++k) racc[k] = 0.f;
  for (int64_t r = w; r < dv.N; r += W) {
    const float ue = ueff[r];
    const bool held = held_bit(ue);
    const float v = fabsf(ue);
    float z[KP], res[KP];
    if (v == 0.f) {  // the row counts nowhere: no margins
#pragma unroll
      for (int k = 0; k < KP; ++k) res[k] = 0.f;
      if (lane == 0) stk<KP>(dv.R + r * KP, res);
      continue;
    }
    wide_row_margins<KP>((int64_t)dv.U, dv.indptr, dv.col, dv.val, r, dv.weff, z);
    const int y = dv.y[r];
    float nll;
    if (K == 1) {  // sigmoid, from exp(-|z|) so that neither side overflows
      const float z0 = z[0], e = expf(-fabsf(z0));
      const float p = z0 >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
#pragma unroll
      for (int k = 0; k < KP; ++k) res[k] = 0.f;
      res[0] = p - (y > 0 ? 1.f : 0.f);
      nll = fmaxf(z0, 0.f) + log1pf(e) - (y > 0 ? z0 : 0.f);
    } else {
      float m = -INFINITY, s = 0.f, zy = 0.f;
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) m = fmaxf(m, z[k]);
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        res[k] = k < K ? expf(z[k] - m) : 0.f;
        s += res[k];
        if (k == y) zy = z[k];
      }
      const float inv = 1.f / s;
#pragma unroll
      for (int k = 0; k < KP; ++k) res[k] = k < K ? res[k] * inv - (k == y ? 1.f : 0.f) : 0.f;
      nll = logf(s) - (zy - m);
    }
    if (held) {
      hacc += v * nll;
#pragma unroll
      for (int k = 0; k < KP; ++k) res[k] = 0.f;
    } else {
#pragma unroll
      for (int k = 0; k < KP; ++k) {
        res[k] = v * res[k];
        racc[k] += res[k];
      }
      lacc += v * nll;
    }
    if (lane == 0) stk<KP>(dv.R + r * KP, res);
  }
  if (lane == 0) {
    float* p = dv.part + w * 32;
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) p[k] = racc[k];
    p[16] = lacc;
    p[17] = hacc;
  }
}

// ---------------------------------------------------------------------------
// wide_fit_reduce_kernel with 1/W for 1/N.  A copy (wide_fit_kernels.hip stays as it
// is) to be kept in step with it by hand; the line that differs forms invN.
__global__ __launch_bounds__(256) void wide_fit_reduce_w_kernel(WideFitDev dv, const double* __restrict__ wsum,
                                                                double reg, int raw) {
  __shared__ double red[4][kFitDotStride];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int KP = dv.KP, UKP = dv.U * KP, H = dv.H;
  const float invN = (float)(1.0 / wsum[0]);  // = 1.f / (float)N for W = N < 2^24
  double a_gg = 0.0, a_gd = 0.0, a_gc = 0.0, a_bb = 0.0, a_s[kMaxHist], a_y[kMaxHist];
#pragma unroll
  for (int i = 0; i < kMaxHist; ++i) a_s[i] = a_y[i] = 0.0;
  for (int64_t e64 = (int64_t)blockIdx.x * 256 + t; e64 < dv.n; e64 += (int64_t)gridDim.x * 256) {
    const int e = (int)e64;
    float g, bt = 0.f;
    if (e < UKP) {
      const int u = e / KP, k = e - u * KP;
      const int i0 = dv.col_item0[u], i1 = dv.col_item0[u + 1];
      float s = 0.f;
      for (int i = i0; i < i1; ++i) s += dv.gitem[(int64_t)i * KP + k];
      if (!raw) {
        bt = dv.beta_t[e];
        // both products rounded, then added: what the plain kernel's build computes (one packed
        // multiply and an add); left to the compiler this file's build fuses the second product
        {
#pragma clang fp contract(off)
          const float gl = s * invN * dv.inv_std[u], gr = (float)reg * bt;
          g = gl + gr;
        }
      } else {
        g = s * invN;
      }
    } else {
      g = dv.bsum[e - UKP] * invN;
    }
    dv.g_t[e] = g;
    if (raw) continue;
    const double gd = (double)g;
    a_gg += gd * gd;
    a_gd += gd * (double)dv.d[e];
    a_gc += gd * (double)dv.g_c[e];
    a_bb += (double)bt * (double)bt;
#pragma unroll
    for (int i = 0; i < kMaxHist; ++i)
      if (i < H) {
        a_s[i] += (double)dv.S[(size_t)i * dv.nv + e] * gd;
        a_y[i] += (double)dv.Y[(size_t)i * dv.nv + e] * gd;
      }
  }
  if (raw) return;
  double v = wave_sum(a_gg);
  if (lane == 0) red[wv][0] = v;
  v = wave_sum(a_gd);
  if (lane == 0) red[wv][1] = v;
  v = wave_sum(a_gc);
  if (lane == 0) red[wv][2] = v;
#pragma unroll
  for (int i = 0; i < kMaxHist; ++i)
    if (i < H) {
      const double s0 = wave_sum(a_s[i]), s1 = wave_sum(a_y[i]);
      if (lane == 0) {
        red[wv][3 + i] = s0;
        red[wv][3 + H + i] = s1;
      }
    }
  v = wave_sum(a_bb);
  if (lane == 0) red[wv][3 + 2 * H] = v;
  __syncthreads();
  if (t < 3 + 2 * H + 1)
    dv.dpart[(size_t)blockIdx.x * kFitDotStride + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
}

// One workgroup (fit_dots_body of fit_body.h with W for N): the NB partial dots, the
// waves' training-loss partials (part[g * 32 + 16]) / W -> the result block, and the
// held-out partials (part[g * 32 + 17]) / W_ho -> wd.ho (0 without held-out weight).
__global__ __launch_bounds__(256) void wide_fit_dots_w_kernel(WideFitDev dv, WideFitWeightsDev wd, int NB, double reg,
                                                              int raw) {
  __shared__ double red[4][64];
  __shared__ double lred[2][256];
  const int t = threadIdx.x, k = t & 63, q = t >> 6;
  const int nd = raw ? 0 : 3 + 2 * dv.H + 1;
  double a = 0.0;
  if (k < nd)
    for (int b = q; b < NB; b += 4) a += dv.dpart[(size_t)b * kFitDotStride + k];
  red[q][k] = a;
  double ls = 0.0, hs = 0.0;
  for (int g = t; g < dv.W; g += 256) {
    ls += (double)dv.part[(size_t)g * 32 + 16];
    hs += (double)dv.part[(size_t)g * 32 + 17];
  }
  lred[0][t] = ls;
  lred[1][t] = hs;
  __syncthreads();
  if (t < nd - 1) dv.out[kFitOutDots + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (t == 0) {
    double loss = 0.0;
    for (int i = 0; i < 256; ++i) loss += lred[0][i];
    loss /= wd.wsum[0];
    double bb = 0.0;
    if (nd > 0) bb = ((red[0][nd - 1] + red[1][nd - 1]) + red[2][nd - 1]) + red[3][nd - 1];
    dv.out[kFitOutF] = loss + 0.5 * reg * bb;
    dv.out[kFitOutLoss] = loss;
  }
  if (t == 64) {
    double h = 0.0;
    for (int i = 0; i < 256; ++i) h += lred[1][i];
    const double who = wd.wsum[1];
    *wd.ho = who > 0.0 ? h / who : 0.0;
  }
}

// ---------------------------------------------------------------------------
void launch_wide_fit_weights(const WideFitDev& dv, const WideFitWeightsDev& wd, hipStream_t s) {
  const int G = wide_fit_weights_grid(dv.N);
  wide_fit_weights_kernel<<<G, 256, 0, s>>>(dv, wd);
  wide_fit_weights_fin_kernel<<<1, 64, 0, s>>>(wd, G);
}

void launch_wide_fit_stats_w(const WideFitDev& dv, const WideFitWeightsDev& wd, hipStream_t s) {
  if (dv.U <= 0) return;
  int64_t b = (dv.U + 3) / 4;
  if (b > (1 << 16)) b = 1 << 16;
  wide_fit_stats_w_kernel<<<(unsigned)b, 256, 0, s>>>(dv, wd);
}

void launch_wide_fit_rows_w(const WideFitDev& dv, const WideFitWeightsDev& wd, int G, hipStream_t s) {
  dispatch_wide_kp("wide fit: padded classes", dv.KP,
                   [&](auto kp) { wide_fit_rows_w_kernel<kp()><<<G, 256, 0, s>>>(dv, wd.ueff); });
}

void launch_wide_fit_reduce_w(const WideFitDev& dv, const WideFitWeightsDev& wd, double reg, int raw, hipStream_t s) {
  const int NB = wide_fit_reduce_grid(dv.n);
  launch_wide_fit_bsum(dv, s);
  wide_fit_reduce_w_kernel<<<NB, 256, 0, s>>>(dv, wd.wsum, reg, raw);
  wide_fit_dots_w_kernel<<<1, 256, 0, s>>>(dv, wd, NB, reg, raw);
}

}  // namespace psx
