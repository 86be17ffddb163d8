// Full-batch fit kernels of the wide (CSR) model (gfx950 / CDNA4): the objective of
// fit_kernels.hip,
//
//   f(beta, b) = mean loss + 0.5 * reg * sum(beta^2),  beta = coef * sigma
//
// (multinomial cross entropy, or softplus(z) - y z for the one-logit model), in the
// subspace of the U features the dataset touches.  The gradient is a scatter over up
// to 10^8 destinations; it is computed without atomics as "store every contribution
// row once, then gather per destination":
//
//   wide_fit_rows_kernel  a wavefront per row (wave w of W owns rows w, w + W, ...):
//                         margins (wide_row_margins of wide_row.h), softmax / sigmoid
//                         with the row maximum subtracted, the residual row
//                         R[r][0..KP) stored once with plain contiguous stores; the
//                         wave's loss and residual sums stay in registers -> one
//                         partial per wave
//   wide_fit_cols_*       a pass over the inverted index (CSC ordered by (column, row)):
//                         per work item (column, begin, end) the sum of
//                         cval[e] * R[crow[e]][k] -> gitem[item][k].  Items of up to
//                         kWideFitShort entries take a KP-lane group each (64/KP items
//                         per wave, the group reads one residual row coalesced); longer
//                         ones a whole wave (lanes stride the entries with 16-B residual
//                         loads, then a butterfly)
//   wide_fit_bsum_kernel  the W residual-sum partials -> the intercept gradient
//   wide_fit_reduce       a column's items summed in chunk order,
//                         g_t = sum / N / sigma + reg * beta_t, partial fp64 dots
//   fit_dots_body (fit_body.h) / fit_update_body (fit_step.h): f_t and the dots, one controller
//                         action -- the dense fit's arithmetic.
// Every sum runs in an order fixed by the data and the options (col_chunk, max_wg):
// a fit is bit-reproducible.  No atomics, no cross-workgroup waits.
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "fit_body.h"
#include "wide_fit_kernels.h"
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

// the value of the (column, row) cell whose first entry is e: entries of one column
// with the same row are adjacent and are summed before anything else is done with them
__device__ __forceinline__ double cell_value(const WideFitDev& dv, int64_t e, int64_t b) {
  const int r = dv.crow[e];
  double x = (double)bf2f(dv.cval[e]);
  for (int64_t j = e + 1; j < b && dv.crow[j] == r; ++j) x += (double)bf2f(dv.cval[j]);
  return x;
}

}  // namespace

// ---------------------------------------------------------------------------
// sigma of every touched feature over all N rows (absent rows count as zeros), fp64
// and two-pass: the mean first, then the centred squares of the present cells plus
// (N - present) * mean^2.  A wavefront per column.
__global__ __launch_bounds__(256) void wide_fit_stats_kernel(WideFitDev dv) {
  const int lane = threadIdx.x & 63;
  const double n = (double)dv.N;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < dv.U; u += (int64_t)gridDim.x * 4) {
    const int64_t a = dv.colptr[u], b = dv.colptr[u + 1];
    double s = 0.0, cnt = 0.0;
    for (int64_t e = a + lane; e < b; e += 64) {
      if (e > a && dv.crow[e - 1] == dv.crow[e]) continue;  // not the first entry of its cell
      s += cell_value(dv, e, b);
      cnt += 1.0;
    }
    s = wave_sum(s);
    cnt = wave_sum(cnt);
    const double m = s / n;
    double q = 0.0;
    for (int64_t e = a + lane; e < b; e += 64) {
      if (e > a && dv.crow[e - 1] == dv.crow[e]) continue;
      const double c = cell_value(dv, e, b) - m;
      q += c * c;
    }
    q = wave_sum(q);
    double sd = 0.0;
    if (n > 1.0) {
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
__device__ __forceinline__ void wide_fit_write_trial(const WideFitDev& dv, int e, float bt) {
  dv.beta_t[e] = bt;
  if (e < dv.U * dv.KP) {
    const float iv = dv.inv_std[e / dv.KP];
    dv.weff[e] = iv > 0.f ? bt * iv : dv.wfix[e];
  } else {
    dv.weff[e] = bt;
  }
}

__global__ __launch_bounds__(256) void wide_fit_begin_kernel(WideFitDev dv, const float* __restrict__ w0,
                                                             int zero_const, int raw) {
  const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= dv.n) return;
  const int e = (int)e64, KP = dv.KP, UKP = dv.U * KP;
  const int u = e < UKP ? e / KP : dv.U, k = e - u * KP;
  float w = 0.f;
  if (w0 && k < dv.K) w = w0[(e < UKP ? (int64_t)dv.uniq[u] : dv.F) * KP + k];
  if (raw) {  // one evaluation at the weights themselves
    dv.weff[e] = w;
    return;
  }
  float xv = w;
  if (e < UKP) {
    const float sd = dv.std_[u];
    xv = w * sd;
    dv.wfix[e] = (sd > 0.f || zero_const) ? 0.f : w;
  } else {
    dv.wfix[e] = 0.f;
  }
  dv.x[e] = xv;
  dv.d[e] = 0.f;
  dv.g_c[e] = 0.f;
  for (int i = 0; i < dv.H; ++i) {
    dv.S[(size_t)i * dv.nv + e] = 0.f;
    dv.Y[(size_t)i * dv.nv + e] = 0.f;
  }
  wide_fit_write_trial(dv, e, xv);
}

// ---------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void wide_fit_rows_kernel(WideFitDev dv) {
  const int lane = threadIdx.x & 63, K = dv.K;
  const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), W = (int64_t)gridDim.x * 4;
  float racc[KP], lacc = 0.f;
#pragma unroll
  for (int k = 0; k < KP; ++k) racc[k] = 0.f;
  for (int64_t r = w; r < dv.N; r += W) {
    float z[KP], res[KP];
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
#pragma unroll
    for (int k = 0; k < KP; ++k) racc[k] += res[k];
    lacc += nll;
    if (lane == 0) stk<KP>(dv.R + r * KP, res);
  }
  if (lane == 0) {
    float* p = dv.part + w * 32;
#pragma unroll
    for (int k = 0; k < 16; ++k) p[k] = 0.f;
#pragma unroll
    for (int k = 0; k < KP; ++k) p[k] = racc[k];
    p[16] = lacc;
  }
}

// ---------------------------------------------------------------------------
// Short items: a group of KP lanes per item, lane k of the group sums class k over
// the item's entries in order (the group reads one residual row of 4*KP bytes).
template <int KP>
__global__ __launch_bounds__(256) void wide_fit_cols_short_kernel(WideFitDev dv) {
  constexpr int GPB = 256 / KP;
  const int k = threadIdx.x % KP;
  const float* __restrict__ R = dv.R;
  for (int64_t i = (int64_t)blockIdx.x * GPB + threadIdx.x / KP; i < dv.n_short; i += (int64_t)gridDim.x * GPB) {
    const int it = dv.short_items[i];
    const int64_t a = dv.item_begin[it], b = dv.item_end[it];
    float acc = 0.f;
    for (int64_t e = a; e < b; ++e) acc += bf2f(dv.cval[e]) * R[(int64_t)dv.crow[e] * KP + k];
    dv.gitem[(int64_t)it * KP + k] = acc;
  }
}

// Long items: a wavefront per item.  A residual row is read by KP/4 lanes with 16-B
// loads (KP < 4: one lane), so 64 / (KP/4) entries are in flight per step; the lanes
// of one class quad are then combined by a butterfly.
template <int KP>
__global__ __launch_bounds__(256) void wide_fit_cols_long_kernel(WideFitDev dv) {
  constexpr int VW = KP < 4 ? KP : 4, LPE = KP / VW, EPS = 64 / LPE;
  const int lane = threadIdx.x & 63, sub = lane % LPE, slot = lane / LPE;
  const float* __restrict__ R = dv.R;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < dv.n_long; i += (int64_t)gridDim.x * 4) {
    const int it = dv.long_items[i];
    const int64_t a = dv.item_begin[it], b = dv.item_end[it];
    float acc[VW];
#pragma unroll
    for (int j = 0; j < VW; ++j) acc[j] = 0.f;
#pragma unroll 4
    for (int64_t e = a + slot; e < b; e += EPS) {
      const float v = bf2f(dv.cval[e]);
      float rv[VW];
      ldk<VW>(R + (int64_t)dv.crow[e] * KP + sub * VW, rv);
#pragma unroll
      for (int j = 0; j < VW; ++j) acc[j] += v * rv[j];
    }
#pragma unroll
    for (int o = 32; o >= LPE; o >>= 1) {
#pragma unroll
      for (int j = 0; j < VW; ++j) acc[j] += __shfl_xor(acc[j], o, 64);
    }
    if (slot == 0) stk<VW>(dv.gitem + (int64_t)it * KP + sub * VW, acc);
  }
}

// ---------------------------------------------------------------------------
// The W per-wave residual sums -> bsum[16]: 16 strided lanes per class, combined in order.
__global__ __launch_bounds__(256) void wide_fit_bsum_kernel(WideFitDev dv) {
  __shared__ float red[16][16];
  const int t = threadIdx.x, k = t & 15, q = t >> 4;
  float a = 0.f;
  for (int g = q; g < dv.W; g += 16) a += dv.part[(size_t)g * 32 + k];
  red[q][k] = a;
  __syncthreads();
  if (t < 16) {
    float s = 0.f;
    for (int i = 0; i < 16; ++i) s += red[i][t];
    dv.bsum[t] = s;
  }
}

// Element e of g_t (a column's items summed in chunk order) and this workgroup's
// partial dots: a thread takes elements e, e + stride, ... and keeps its products in
// fp64 registers; waves by butterfly, the 4 waves combined in order.  The item sum is
// serial per (column, class): its length for the longest column is N / col_chunk, which
// is why the reduction's time falls with col_chunk (440 adds at the default 2048 and
// 10^6 rows, 16 k at col_chunk 64: keep col_chunk >= N / 1000 or so at large N).
__global__ __launch_bounds__(256) void wide_fit_reduce_kernel(WideFitDev dv, double reg, int raw) {
  __shared__ double red[4][kFitDotStride];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int KP = dv.KP, UKP = dv.U * KP, H = dv.H;
  const float invN = 1.f / (float)dv.N;
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
        g = s * invN * dv.inv_std[u] + (float)reg * bt;
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

__global__ __launch_bounds__(256) void wide_fit_dots_kernel(WideFitDev dv, int NB, double reg, int raw) {
  fit_dots_body(dv.dpart, dv.part, dv.out, dv.H, dv.N, NB, dv.W, reg, raw);
}

__global__ __launch_bounds__(256) void wide_fit_update_kernel(WideFitDev dv, FitStep st) {
  const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= dv.n) return;
  fit_update_body(dv, st, (int)e64, [&](int i, float bt) { wide_fit_write_trial(dv, i, bt); });
}

// Back to the original feature space and the full vector: coef = beta / sigma through
// uniq, coefficients centred over the classes when `center`, intercepts whenever
// K >= 2; padding classes zero.  Thread u < U: feature uniq[u]; thread U: the intercepts.
__global__ __launch_bounds__(256) void wide_fit_finalize_kernel(WideFitDev dv, int center, float* __restrict__ w_out) {
  const int64_t u64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u64 > dv.U) return;
  const int u = (int)u64, KP = dv.KP, K = dv.K;
  const bool icpt = u == dv.U;
  const float iv = icpt ? 0.f : dv.inv_std[u];
  const float* x = dv.x + (int64_t)u * KP;
  const float* wf = dv.wfix + (int64_t)u * KP;
  float* o = w_out + (icpt ? dv.F : (int64_t)dv.uniq[u]) * KP;
  float mean = 0.f;
  for (int k = 0; k < K; ++k) mean += icpt ? x[k] : (iv > 0.f ? x[k] * iv : wf[k]);
  mean = (K >= 2 && (icpt || center)) ? mean / (float)K : 0.f;
  for (int k = 0; k < KP; ++k) {
    const float v = icpt ? x[k] : (iv > 0.f ? x[k] * iv : wf[k]);
    o[k] = k < K ? v - mean : 0.f;
  }
}

__global__ __launch_bounds__(256) void wide_fit_scatter_kernel(WideFitDev dv, const float* __restrict__ src,
                                                               float* __restrict__ dst) {
  const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= dv.n) return;
  const int e = (int)e64, KP = dv.KP, UKP = dv.U * KP;
  const int u = e < UKP ? e / KP : dv.U, k = e - u * KP;
  dst[(e < UKP ? (int64_t)dv.uniq[u] : dv.F) * KP + k] = src[e];
}

// ---------------------------------------------------------------------------
static unsigned blocks_of(int64_t n, int per, int64_t cap) {
  int64_t b = (n + per - 1) / per;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

void launch_wide_fit_stats(const WideFitDev& dv, hipStream_t s) {
  if (dv.U <= 0) return;
  wide_fit_stats_kernel<<<blocks_of(dv.U, 4, 1 << 16), 256, 0, s>>>(dv);
}

void launch_wide_fit_begin(const WideFitDev& dv, const float* w0, int zero_const, int raw, hipStream_t s) {
  wide_fit_begin_kernel<<<blocks_of(dv.n, 256, INT64_MAX), 256, 0, s>>>(dv, w0, zero_const, raw);
}

static const char kWideFitKP[] = "wide fit: padded classes";

void launch_wide_fit_rows(const WideFitDev& dv, int G, hipStream_t s) {
  dispatch_wide_kp(kWideFitKP, dv.KP, [&](auto kp) { wide_fit_rows_kernel<kp()><<<G, 256, 0, s>>>(dv); });
}

void launch_wide_fit_cols(const WideFitDev& dv, hipStream_t s) {
  if (dv.n_short > 0)
    dispatch_wide_kp(kWideFitKP, dv.KP, [&](auto kp) {
      wide_fit_cols_short_kernel<kp()><<<blocks_of(dv.n_short, 256 / kp(), 1 << 16), 256, 0, s>>>(dv);
    });
  if (dv.n_long > 0)
    dispatch_wide_kp(kWideFitKP, dv.KP, [&](auto kp) {
      wide_fit_cols_long_kernel<kp()><<<blocks_of(dv.n_long, 4, 1 << 16), 256, 0, s>>>(dv);
    });
}

int wide_fit_reduce_grid(int n) { return (int)blocks_of(n, 256, kWideReduceMaxWG); }

void launch_wide_fit_reduce(const WideFitDev& dv, double reg, int raw, hipStream_t s) {
  const int NB = wide_fit_reduce_grid(dv.n);
  wide_fit_bsum_kernel<<<1, 256, 0, s>>>(dv);
  wide_fit_reduce_kernel<<<NB, 256, 0, s>>>(dv, reg, raw);
  wide_fit_dots_kernel<<<1, 256, 0, s>>>(dv, NB, reg, raw);
}

void launch_wide_fit_update(const WideFitDev& dv, const FitStep& st, hipStream_t s) {
  wide_fit_update_kernel<<<blocks_of(dv.n, 256, INT64_MAX), 256, 0, s>>>(dv, st);
}

void launch_wide_fit_finalize(const WideFitDev& dv, int center, float* w_out, hipStream_t s) {
  wide_fit_finalize_kernel<<<blocks_of((int64_t)dv.U + 1, 256, INT64_MAX), 256, 0, s>>>(dv, center, w_out);
}

void launch_wide_fit_scatter(const WideFitDev& dv, const float* src, float* dst, hipStream_t s) {
  wide_fit_scatter_kernel<<<blocks_of(dv.n, 256, INT64_MAX), 256, 0, s>>>(dv, src, dst);
}

}  // namespace psx
