// Full-batch fit kernels (gfx950 / CDNA4): Spark's LogisticRegression.fit with
// standardization=true, elasticNetParam=0 on a dataset resident in HBM.
//
//   f(beta, b) = mean cross entropy + 0.5 * reg * sum(beta^2),  beta = coef * sigma
//
// One evaluation is three ordinary launches:
//   fit_lossgrad_kernel  G workgroups take the 32-row tiles wg, wg+G, ...; each tile
//                        is staged once and, while it sits in LDS, runs the MFMA
//                        forward against the trial weights' hi/lo fragments, the
//                        softmax and the backward R^T X (fwd_body<FP, true> of
//                        solve_body.h, the streaming solver's tile body, unchanged)
//                        -> one partial gradient, loss and residual sums per workgroup
//   fit_reduce_kernel    g_t = (1/N) 1/sigma sum of the partials + reg * beta_t and
//                        per-workgroup fp64 partials of the controller's dots
//   fit_dots_kernel      f_t and the dots (num_dots(hist) layout)
// The host runs solver_ctrl.h's ctrl_step on them and fit_update_kernel applies the
// resulting action.  Every sum runs in a fixed order (strided lanes combined in
// order, butterflies): a fit is bit-reproducible.  No atomics at all.
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "fit_body.h"
#include "fit_kernels.h"
#include "solve_body.h"

namespace psx {

static_assert(kPartStride == 32, "fit_reduce / fit_dots index fwd_body's partials with stride 32");
static_assert(3 + 2 * kMaxHist + 1 <= kFitDotStride && kFitDotStride <= 64, "partial dots of one reduce workgroup");

// ---------------------------------------------------------------------------
// Column sums and sums of squares: per tile in fp32 (32 rows of bf16 values),
// across tiles in fp64; one partial per workgroup.
template <int FP>
__global__ __launch_bounds__(256) void fit_stats_kernel(FitDev dv) {
  constexpr int C = FP / 8;   // 16-B chunks per row
  constexpr int L = 256 / C;  // row lanes
  static_assert(C * L == 256, "FP in {128..2048}");
  constexpr int RPL = 32 / L;  // rows of a tile per lane
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = (double*)smem;  // [L][C][16]
  const int t = threadIdx.x, ch = t % C, rl = t / C;
  const int ntiles = dv.Npad >> 5;
  double s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * 32;
    float fs[8], fq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) fs[e] = fq[e] = 0.f;
    u16x8 v[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) v[j] = *(const u16x8*)(dv.X + (row0 + rl + L * j) * FP + ch * 8);
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
      const bool in = row0 + rl + L * j < dv.N;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = in ? bf2f(v[j][e]) : 0.f;
        fs[e] += x;
        fq[e] += x * x;
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      s[e] += fs[e];
      q[e] += fq[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    red[(rl * C + ch) * 16 + e] = s[e];
    red[(rl * C + ch) * 16 + 8 + e] = q[e];
  }
  __syncthreads();
  for (int k = t; k < C * 16; k += 256) {  // k = chunk * 16 + {sum e | square e}
    double a = 0.0;
    for (int r = 0; r < L; ++r) a += red[r * C * 16 + k];
    const int c = k >> 4, e = k & 15, f = c * 8 + (e & 7);
    dv.spart[((size_t)blockIdx.x * 2 + (e >> 3)) * FP + f] = a;
  }
}

// sigma_f = sample std (n - 1) from the G partials, summed in workgroup order.
__global__ __launch_bounds__(256) void fit_stats_fin_kernel(FitDev dv, int G) {
  const int f = blockIdx.x * 256 + threadIdx.x, FP = dv.FP;
  if (f >= FP) return;
  double a = 0.0, b = 0.0;
  for (int g = 0; g < G; ++g) {
    a += dv.spart[((size_t)g * 2) * FP + f];
    b += dv.spart[((size_t)g * 2 + 1) * FP + f];
  }
  const double n = (double)dv.N;
  double sd = 0.0;
  if (f < dv.F && n > 1.0) {
    const double mean = a / n;
    const double var = (b - n * mean * mean) / (n - 1.0);
    sd = var > 0.0 ? sqrt(var) : 0.0;
  }
  dv.std_[f] = (float)sd;
  dv.inv_std[f] = sd > 0.0 ? (float)(1.0 / sd) : 0.f;
}

// ---------------------------------------------------------------------------
// The effective weight of standardised coefficient v of feature f, and the trial
// point's fragments / intercepts.
__device__ __forceinline__ void fit_write_trial(const FitDev& dv, int e, float bt) {
  const int KF = dv.K * dv.FP;
  dv.beta_t[e] = bt;
  if (e < KF) {
    const int c = e / dv.FP, f = e - c * dv.FP;
    const float iv = dv.inv_std[f];
    write_frag(dv.whi, dv.wlo, c, f, iv > 0.f ? bt * iv : dv.wfix[e]);
  } else {
    dv.b_eff[e - KF] = bt;
  }
}

__global__ __launch_bounds__(256) void fit_begin_kernel(FitDev dv, const float* w0, int zero_const, int raw) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= dv.n) return;
  const int KF = dv.K * dv.FP;
  const float w = w0 ? w0[e] : 0.f;
  if (raw) {  // one evaluation at the weights themselves
    if (e < KF) {
      const int c = e / dv.FP, f = e - c * dv.FP;
      write_frag(dv.whi, dv.wlo, c, f, f < dv.F ? w : 0.f);
    } else {
      dv.b_eff[e - KF] = w;
    }
    return;
  }
  float xv = w;
  if (e < KF) {
    const int c = e / dv.FP, f = e - c * dv.FP;
    const float sd = dv.std_[f];
    xv = w * sd;
    dv.wfix[e] = (sd > 0.f || zero_const || f >= dv.F) ? 0.f : w;
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
  fit_write_trial(dv, e, xv);
}

// ---------------------------------------------------------------------------
template <int FP>
__global__ __launch_bounds__(256) void fit_lossgrad_kernel(SolverCfg cfg, SolveParams pr, SolveDev sdv,
                                                           float* __restrict__ gpart) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NT = FP / 64;
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0, 0, 0, 0};
  const int wg = blockIdx.x;
  if (wg >= ((pr.B + 31) >> 5)) return;  // no tile: no partial (the reduction sums min(G, tiles) of them)
  fwd_body<FP, true>(cfg, pr, 0, sdv, lds, wg, gridDim.x, acc);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, K = cfg.K;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int f = (w * NT + n) * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (lane >> 4) * 4 + i;
      if (c < K) gpart[((size_t)wg * K + c) * FP + f] = acc[n][i];
    }
  }
}

// ---------------------------------------------------------------------------
// 64 elements per workgroup; element e's nfw partials are summed by 4 strided lanes
// (8 loads in flight each), the 4 sums combined in order.  Wave 0 then forms g_t and
// this workgroup's partial dots.
__global__ __launch_bounds__(256) void fit_reduce_kernel(FitDev dv, int nfw, double reg, int raw) {
  __shared__ float red[4][64];
  const int t = threadIdx.x, l = t & 63, sub = t >> 6;
  const int e = blockIdx.x * 64 + l, KF = dv.K * dv.FP;
  float a = 0.f;
  if (e < dv.n) {
    const float* src = e < KF ? dv.gpart + e : dv.part + (e - KF);
    const size_t stride = e < KF ? (size_t)KF : (size_t)kPartStride;
    constexpr int U = 8;
    for (int g0 = sub; g0 < nfw; g0 += 4 * U) {
      float v[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int g = g0 + 4 * u;
        v[u] = g < nfw ? src[(size_t)g * stride] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) a += v[u];
    }
  }
  red[sub][l] = a;
  __syncthreads();
  if (t >= 64) return;
  float g = 0.f, bt = 0.f;
  if (e < dv.n) {
    const float s = ((red[0][l] + red[1][l]) + red[2][l]) + red[3][l];
    const float invN = 1.f / (float)dv.N;
    if (e < KF && !raw) {
      const int f = e & (dv.FP - 1);
      bt = dv.beta_t[e];
      g = s * invN * dv.inv_std[f] + (float)reg * bt;
    } else {
      g = s * invN;
    }
    dv.g_t[e] = g;
  }
  if (raw) return;
  double* dp = dv.dpart + (size_t)blockIdx.x * kFitDotStride;
  const bool in = e < dv.n;
  const double gd = (double)g;
  double v = wave_sum(gd * gd);
  if (l == 0) dp[0] = v;
  v = wave_sum(in ? gd * (double)dv.d[e] : 0.0);
  if (l == 0) dp[1] = v;
  v = wave_sum(in ? gd * (double)dv.g_c[e] : 0.0);
  if (l == 0) dp[2] = v;
  const int H = dv.H;
  for (int i = 0; i < H; ++i) {
    const double sv = in ? (double)dv.S[(size_t)i * dv.nv + e] : 0.0;
    const double yv = in ? (double)dv.Y[(size_t)i * dv.nv + e] : 0.0;
    const double a0 = wave_sum(sv * gd), a1 = wave_sum(yv * gd);
    if (l == 0) {
      dp[3 + i] = a0;
      dp[3 + H + i] = a1;
    }
  }
  v = wave_sum(e < KF ? (double)bt * (double)bt : 0.0);
  if (l == 0) dp[3 + 2 * H] = v;
}

// One workgroup: f_t, the mean loss and the dots (fit_dots_body of fit_body.h).
__global__ __launch_bounds__(256) void fit_dots_kernel(FitDev dv, int NB, int nfw, double reg, int raw) {
  fit_dots_body(dv.dpart, dv.part, dv.out, dv.H, dv.N, NB, nfw, reg, raw);
}

// ---------------------------------------------------------------------------
// One controller action on the vectors (fit_update_body of fit_step.h).
__global__ __launch_bounds__(256) void fit_update_kernel(FitDev dv, FitStep st) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= dv.n) return;
  fit_update_body(dv, st, e, [&](int i, float bt) { fit_write_trial(dv, i, bt); });
}

// Back to the original feature space: coef = beta / sigma, coefficients centred over
// the classes when `center`, intercepts always; packed [K][FP] + K.
__global__ __launch_bounds__(256) void fit_finalize_kernel(FitDev dv, int center, float* __restrict__ w_out) {
  const int f = blockIdx.x * 256 + threadIdx.x, FP = dv.FP, K = dv.K;
  if (f >= FP) return;
  const float iv = dv.inv_std[f];
  float mean = 0.f;
  for (int c = 0; c < K; ++c) {
    const int e = c * FP + f;
    mean += f < dv.F ? (iv > 0.f ? dv.x[e] * iv : dv.wfix[e]) : 0.f;
  }
  mean = (center && f < dv.F) ? mean / (float)K : 0.f;
  for (int c = 0; c < K; ++c) {
    const int e = c * FP + f;
    const float v = f < dv.F ? (iv > 0.f ? dv.x[e] * iv : dv.wfix[e]) : 0.f;
    w_out[e] = v - mean;
  }
  if (f == 0) {
    float bm = 0.f;
    for (int c = 0; c < K; ++c) bm += dv.x[K * FP + c];
    bm /= (float)K;
    for (int c = 0; c < K; ++c) w_out[K * FP + c] = dv.x[K * FP + c] - bm;
  }
}

// ---------------------------------------------------------------------------
void prepare_fit_kernels() {
  static bool done = false;
  if (done) return;
  for_each_fp([](auto fp) {
    (void)hipFuncSetAttribute((const void*)fit_lossgrad_kernel<fp()>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)eval_lds_bytes(fp()));
  });
  done = true;
}

int fit_reduce_grid(int n) { return (n + 63) / 64; }

void launch_fit_stats(const FitDev& dv, int G, hipStream_t s) {
  const size_t lb = (size_t)256 * 16 * sizeof(double);
  dispatch_fp("fit: padded width", dv.FP, [&](auto fp) { fit_stats_kernel<fp()><<<G, 256, lb, s>>>(dv); });
  fit_stats_fin_kernel<<<(dv.FP + 255) / 256, 256, 0, s>>>(dv, G);
}

void launch_fit_begin(const FitDev& dv, const float* w0, int zero_const, int raw, hipStream_t s) {
  fit_begin_kernel<<<(dv.n + 255) / 256, 256, 0, s>>>(dv, w0, zero_const, raw);
}

void launch_fit_lossgrad(const FitDev& dv, int G, hipStream_t s) {
  SolverCfg cfg{};
  cfg.K = dv.K;
  cfg.F = dv.F;
  cfg.Fp = dv.FP;
  cfg.cap = dv.Npad;
  const SolveParams pr{dv.N, 0, 0, 0};
  SolveDev sdv{};
  sdv.X = dv.X;
  sdv.y = dv.y;
  sdv.b_eff = dv.b_eff;
  sdv.whi = dv.whi;
  sdv.wlo = dv.wlo;
  sdv.part = dv.part;
  const size_t lb = eval_lds_bytes(dv.FP);
  dispatch_fp("fit: padded width", dv.FP, [&](auto fp) {
    fit_lossgrad_kernel<fp()><<<G, 256, lb, s>>>(cfg, pr, sdv, dv.gpart);
  });
}

void launch_fit_reduce(const FitDev& dv, int G, double reg, int raw, hipStream_t s) {
  const int ntiles = dv.Npad >> 5, nfw = ntiles < G ? ntiles : G, NB = fit_reduce_grid(dv.n);
  fit_reduce_kernel<<<NB, 256, 0, s>>>(dv, nfw, reg, raw);
  fit_dots_kernel<<<1, 256, 0, s>>>(dv, NB, nfw, reg, raw);
}

void launch_fit_update(const FitDev& dv, const FitStep& st, hipStream_t s) {
  fit_update_kernel<<<(dv.n + 255) / 256, 256, 0, s>>>(dv, st);
}

void launch_fit_finalize(const FitDev& dv, int center, float* w_out, hipStream_t s) {
  fit_finalize_kernel<<<(dv.FP + 255) / 256, 256, 0, s>>>(dv, center, w_out);
}

}  // namespace psx
