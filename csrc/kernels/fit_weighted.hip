// Weighted full-batch fit kernels (gfx950 / CDNA4): fit_kernels.hip's evaluation with
// a weight per row and a held-out fold (the objective is stated in fit_weighted.h).
//
// A row's weights are formed per tile from three streams -- sample_weight (fp32),
// fold (uint8) and the label, with the 16-entry class-weight table and the held-out
// fold as kernel arguments:
//     u = training weight (0 for held-out rows and rows >= N),  h = held-out weight.
//   fit_stats_w_kernel     sum u x and sum u x^2 per tile in fp32, across tiles in
//                          fp64, plus the workgroup's sum u and sum h; its finish
//                          writes sigma, 1/sigma, W and W_ho
//   fit_lossgrad_w_kernel  the plain kernel's tile walk with a body of its own: the
//                          row epilogue scales the residual by u BEFORE the bf16
//                          hi/lo split, so the MFMA backward R^T X is the unweighted
//                          one, and sums u CE and h CE separately -- the held-out loss
//                          comes out of the same read of the rows
//   fit_reduce_w_kernel,   the plain reduction and dots with 1/W (the device double)
//   fit_dots_w_kernel      for 1/N, and the held-out mean into a double of its own
// Every sum runs in a fixed order; no atomics, no scratch.  With unit weights and no
// held-out fold every kernel here computes what its plain counterpart computes, bit
// for bit (u = 1 is exact in every product it enters, W = N).
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "fit_weighted.h"
#include "solve_body.h"

namespace psx {

// The raw streams of row `row` (label y), then the pair (u, h).  Split in two so the
// loads are issued with the tile's row loads and consumed after them.
struct RowWeightIn {
  float s;
  int fold;
};
__device__ __forceinline__ RowWeightIn load_row_weight(const FitWeightsDev& wd, int64_t row) {
  return {wd.sw ? wd.sw[row] : 1.f, wd.fold ? (int)wd.fold[row] : -1};
}
__device__ __forceinline__ void row_weight(const FitWeightsDev& wd, const RowWeightIn in, int y, bool valid, float& u,
                                           float& h) {
  float c = 0.f;  // a select chain: a table indexed by a lane's label would live in scratch
#pragma unroll
  for (int k = 0; k < 16; ++k) c = y == k ? wd.cw[k] : c;
  const float v = valid ? in.s * c : 0.f;
  const bool held = wd.holdout >= 0 && in.fold == wd.holdout;
  u = held ? 0.f : v;
  h = held ? v : 0.f;
}

// ---------------------------------------------------------------------------
// fit_stats_kernel's split (thread = 16-B chunk ch of the rows rl, rl + L, ...), plus
// every feature's min and max over the rows of positive training weight.
// Threads 0..31 form the tile's weights into LDS (two buffers: one barrier per tile)
// and keep the sums of u and h of their row position in fp64.
template <int FP>
__global__ __launch_bounds__(256) void fit_stats_w_kernel(FitDev dv, FitWeightsDev wd) {
  constexpr int C = FP / 8;
  constexpr int L = 256 / C;
  static_assert(C * L == 256, "FP in {128..2048}");
  constexpr int RPL = 32 / L;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = (double*)smem;          // [L][C][16]
  double* wred = red + 256 * 16;        // [32][2]
  float* wl = (float*)(wred + 32 * 2);  // [2 buffers][32] u
  float* mm = wl + 64;                  // [L][C][16] min | max over the rows of positive u
  const int t = threadIdx.x, ch = t % C, rl = t / C;
  const int ntiles = dv.Npad >> 5;
  double s[8], q[8], su = 0.0, sh = 0.0;
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.0;
  float mn[8], mx[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) mn[e] = INFINITY, mx[e] = -INFINITY;
  int buf = 0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x, buf ^= 32) {
    const int64_t row0 = (int64_t)tile * 32;
    RowWeightIn wi{};
    int yv = 0;
    if (t < 32) {
      wi = load_row_weight(wd, row0 + t);
      yv = dv.y[row0 + t];
    }
    u16x8 v[RPL];
#pragma unroll
    for (int j = 0; j < RPL; ++j) v[j] = *(const u16x8*)(dv.X + (row0 + rl + L * j) * FP + ch * 8);
    if (t < 32) {
      float u, h;
      row_weight(wd, wi, yv, row0 + t < dv.N, u, h);
      wl[buf + t] = u;
      su += u;
      sh += h;
    }
    __syncthreads();
    float fs[8], fq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) fs[e] = fq[e] = 0.f;
#pragma unroll
    for (int j = 0; j < RPL; ++j) {
      const float u = wl[buf + rl + L * j];  // 0 for rows >= N
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float x = bf2f(v[j][e]), ux = u > 0.f ? u * x : 0.f;  // (a select: 0 * Inf of a row left out is NaN)
        fs[e] += ux;
        fq[e] += ux * x;
        mn[e] = u > 0.f ? fminf(mn[e], x) : mn[e];
        mx[e] = u > 0.f ? fmaxf(mx[e], x) : mx[e];
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
    mm[(rl * C + ch) * 16 + e] = mn[e];
    mm[(rl * C + ch) * 16 + 8 + e] = mx[e];
  }
  if (t < 32) {
    wred[t * 2] = su;
    wred[t * 2 + 1] = sh;
  }
  __syncthreads();
  for (int k = t; k < C * 16; k += 256) {  // k = chunk * 16 + {sum e | square e}
    double a = 0.0;
    for (int r = 0; r < L; ++r) a += red[r * C * 16 + k];
    const int c = k >> 4, e = k & 15, f = c * 8 + (e & 7);
    dv.spart[((size_t)blockIdx.x * 2 + (e >> 3)) * FP + f] = a;
    float m = mm[k];
    for (int r = 1; r < L; ++r) m = e < 8 ? fminf(m, mm[r * C * 16 + k]) : fmaxf(m, mm[r * C * 16 + k]);
    wd.mmpart[((size_t)blockIdx.x * 2 + (e >> 3)) * FP + f] = m;
  }
  if (t < 2) {  // row positions in order
    double a = 0.0;
    for (int r = 0; r < 32; ++r) a += wred[r * 2 + t];
    wd.wpart[(size_t)blockIdx.x * 2 + t] = a;
  }
}
constexpr size_t kStatsWLds =
    (size_t)256 * 16 * sizeof(double) + 32 * 2 * sizeof(double) + 2 * 32 * sizeof(float) + 256 * 16 * sizeof(float);
static_assert(kStatsWLds <= 64 * 1024, "fit_stats_w_kernel's LDS needs no raised limit");

// sigma_f = weighted sample std over the training rows (fit_stats_fin_kernel with
// n -> W), from the G partials summed in workgroup order; W and W_ho -> wd.wsum.
// A feature with one value on the rows of positive weight has sigma 0 EXACTLY: its
// sums of rounded products u x do not cancel as the plain sums of x do, so the
// decision is taken on the rows' min and max.
__global__ __launch_bounds__(256) void fit_stats_w_fin_kernel(FitDev dv, FitWeightsDev wd, int G) {
  const int f = blockIdx.x * 256 + threadIdx.x, FP = dv.FP;
  if (f >= FP) return;
  double a = 0.0, b = 0.0, n = 0.0, nh = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int g = 0; g < G; ++g) {
    mn = fminf(mn, wd.mmpart[((size_t)g * 2) * FP + f]);
    mx = fmaxf(mx, wd.mmpart[((size_t)g * 2 + 1) * FP + f]);
    a += dv.spart[((size_t)g * 2) * FP + f];
    b += dv.spart[((size_t)g * 2 + 1) * FP + f];
    n += wd.wpart[(size_t)g * 2];
    nh += wd.wpart[(size_t)g * 2 + 1];
  }
  double sd = 0.0;
  if (f < dv.F && n > 1.0 && mx > mn) {
    const double mean = a / n;
    const double var = (b - n * mean * mean) / (n - 1.0);
    sd = var > 0.0 ? sqrt(var) : 0.0;
  }
  dv.std_[f] = (float)sd;
  dv.inv_std[f] = sd > 0.0 ? (float)(1.0 / sd) : 0.f;
  if (f == 0) {
    wd.wsum[0] = n;
    wd.wsum[1] = nh;
  }
}

// ---------------------------------------------------------------------------
// LDS behind the tile image: logits 8 KB, rt 2 KB, then the words below -- inside
// the 1.5 KB eval_lds_bytes leaves there (the plain body uses the first 400 B).
constexpr int kWTailBytes = 32 * 4 /*labels*/ + 64 * 4 /*rsum*/ + 8 * 4 /*loss, held-out loss per wave*/ +
                            2 * 32 * 4 /*u, h*/;
static_assert(eval_lds_bytes(2048) == (size_t)32 * 2048 * 2 + 8192 + 2048 + 1536 && kWTailBytes <= 1536,
              "the weighted tile body's LDS layout");

// G workgroups take the 32-row tiles wg, wg+G, ... (fwd_body<FP, true> of solve_body.h
// on the window [0, N), its pieces unchanged); per workgroup one partial gradient,
// 16 class residual sums, the training loss and the held-out loss.
template <int FP>
__global__ __launch_bounds__(256) void fit_lossgrad_w_kernel(FitDev dv, FitWeightsDev wd) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NT = FP / 64;
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0, 0, 0, 0};
  const int wg = blockIdx.x, G = gridDim.x, K = dv.K, N = dv.N;
  const int ntiles = (N + 31) >> 5;
  if (wg >= ntiles) return;  // no tile: no partial (the reduction sums min(G, tiles) of them)
  char* red_base = lds + 32 * FP * 2;
  unsigned short* rt = (unsigned short*)(red_base + 8192);  // [2][16][32]
  int* ylds = (int*)(red_base + 8192 + 2048);
  float* rsum = (float*)(ylds + 32);  // [4 waves][16]
  float* lred = rsum + 64;            // [4 waves] training loss, [4 waves] held-out loss
  float* uw = lred + 8;               // [32] training weight of the tile's rows
  float* hw = uw + 32;                // [32] held-out weight
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;

  float loss = 0.f, hloss = 0.f;
  const int sr = tid >> 3, sc0 = (tid & 7) * 2;
  float rs0 = 0.f, rs1 = 0.f;
  const float bz0 = dv.b_eff[sc0], bz1 = dv.b_eff[sc0 + 1];
  // the trial weights do not depend on the tile: fetched before staging up to FP 1024
  constexpr bool kPre = FP <= 1024;
  WFrag<kPre ? FP : 128> wf;
  if constexpr (kPre) load_wfrag<FP>(wf, dv.whi, dv.wlo, K);
  for (int tile = wg; tile < ntiles; tile += G) {
    const int64_t row0 = (int64_t)tile * 32;
    // labels and weight streams issued with the tile's loads (one round trip)
    RowWeightIn wi{};
    int yv = 0;
    if (tid < 32) {
      yv = dv.y[row0 + tid];
      wi = load_row_weight(wd, row0 + tid);
    }
    stage_tile<FP>(lds, dv.X, row0, 32, dv.Npad, false);
    if (tid < 32) {
      float u, h;
      row_weight(wd, wi, yv, row0 + tid < N, u, h);
      ylds[tid] = yv;
      uw[tid] = u;
      hw[tid] = h;
    }
    __syncthreads();
    f32x4 a0, a1;
    if constexpr (kPre)
      forward_tile_pre<FP>(lds, wf, a0, a1);
    else
      forward_tile<FP>(lds, dv.whi, dv.wlo, a0, a1);
    store_partial_logits(red_base, a0, a1);
    __syncthreads();
    {  // softmax + cross entropy: 8 threads per row, 2 classes each
      const bool v0 = sc0 < K, v1 = sc0 + 1 < K;
      const float z0 = v0 ? load_logit(red_base, sr, sc0) + bz0 : -INFINITY;
      const float z1 = v1 ? load_logit(red_base, sr, sc0 + 1) + bz1 : -INFINITY;
      float mx = fmaxf(z0, z1);
      mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
      const float e0 = v0 ? __expf(z0 - mx) : 0.f, e1 = v1 ? __expf(z1 - mx) : 0.f;
      float se = e0 + e1;
      se += __shfl_xor(se, 1, 64);
      se += __shfl_xor(se, 2, 64);
      se += __shfl_xor(se, 4, 64);
      const bool valid = tile * 32 + sr < N;
      const int yl = ylds[sr];
      const float u = uw[sr], h = hw[sr];
      const float inv = 1.f / se;
      const float p0 = valid && v0 ? e0 * inv - (yl == sc0 ? 1.f : 0.f) : 0.f;
      const float p1 = valid && v1 ? e1 * inv - (yl == sc0 + 1 ? 1.f : 0.f) : 0.f;
      const float r0 = u * p0, r1 = u * p1;  // weighted residual: the backward below is the plain R^T X
      if (valid) {
        const float lse = mx + __logf(se);
        if (yl == sc0) {
          const float ce = lse - z0;
          loss += u * ce;
          hloss += h * ce;
        }
        if (yl == sc0 + 1) {
          const float ce = lse - z1;
          loss += u * ce;
          hloss += h * ce;
        }
      }
      rs0 += r0;
      rs1 += r1;
      unsigned short hi, lo;
      split_bf16(r0, hi, lo);
      rt[sc0 * 32 + sr] = hi;
      rt[512 + sc0 * 32 + sr] = lo;
      split_bf16(r1, hi, lo);
      rt[(sc0 + 1) * 32 + sr] = hi;
      rt[512 + (sc0 + 1) * 32 + sr] = lo;
    }
    __syncthreads();
    bwd_tile_acc<FP>(lds, rt, acc);
    __syncthreads();  // the next tile's staging overwrites the image, rt and the weights
  }
  // fixed order: a butterfly over the lanes of one class pair, then the waves in order
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    rs0 += __shfl_xor(rs0, o, 64);
    rs1 += __shfl_xor(rs1, o, 64);
  }
  if (lane < 8) {
    rsum[w * 16 + sc0] = rs0;
    rsum[w * 16 + sc0 + 1] = rs1;
  }
  loss = wave_sum(loss);
  hloss = wave_sum(hloss);
  if (lane == 0) {
    lred[w] = loss;
    lred[4 + w] = hloss;
  }
  __syncthreads();
  float* part = dv.part + (size_t)wg * kPartStride;
  float pv = 0.f;
  if (tid < 16) pv = ((rsum[tid] + rsum[16 + tid]) + rsum[32 + tid]) + rsum[48 + tid];
  if (tid == 16) pv = lred[0] + lred[1] + lred[2] + lred[3];
  if (tid == 17) pv = lred[4] + lred[5] + lred[6] + lred[7];
  if (tid < 18) part[tid] = pv;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int f = (w * NT + n) * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (lane >> 4) * 4 + i;
      if (c < K) dv.gpart[((size_t)wg * K + c) * FP + f] = acc[n][i];
    }
  }
}

// ---------------------------------------------------------------------------
// fit_reduce_kernel with 1/W for 1/N: 64 elements per workgroup, element e's nfw
// partials summed by 4 strided lanes, the 4 sums combined in order; wave 0 then forms
// g_t and this workgroup's partial dots.  A copy of fit_reduce_kernel (fit_kernels.hip,
// whose code stays as it is) to be kept in step with it by hand; the lines that differ
// are the one that forms invW (there: invN = 1.f / (float)dv.N) and the unfused sum
// that forms g_t below it.
__global__ __launch_bounds__(256) void fit_reduce_w_kernel(FitDev dv, const double* __restrict__ wsum, int nfw,
                                                           double reg, int raw) {
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
    const float invW = (float)(1.0 / wsum[0]);  // = 1.f / (float)N for W = N < 2^24
    if (e < KF && !raw) {
      const int f = e & (dv.FP - 1);
      bt = dv.beta_t[e];
      // both products rounded, then added: what the plain kernel's build computes (one packed
      // multiply and an add); left to the compiler this file's build fuses the second product
      {
#pragma clang fp contract(off)
        const float gl = s * invW * dv.inv_std[f], gr = (float)reg * bt;
        g = gl + gr;
      }
    } else {
      g = s * invW;
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

// One workgroup (fit_dots_body of fit_body.h with W for N): the NB partial dots, the
// nfw training-loss partials (part[g * 32 + 16]) / W -> the result block, and the
// held-out partials (part[g * 32 + 17]) / W_ho -> wd.ho (0 without held-out weight).
__global__ __launch_bounds__(256) void fit_dots_w_kernel(FitDev dv, FitWeightsDev wd, int NB, int nfw, double reg,
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
  for (int g = t; g < nfw; g += 256) {
    ls += (double)dv.part[(size_t)g * kPartStride + 16];
    hs += (double)dv.part[(size_t)g * kPartStride + 17];
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
void prepare_fit_weighted_kernels() {
  static bool done = false;
  if (done) return;
  for_each_fp([](auto fp) {
    (void)hipFuncSetAttribute((const void*)fit_lossgrad_w_kernel<fp()>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)eval_lds_bytes(fp()));
  });
  done = true;
}

void launch_fit_stats_w(const FitDev& dv, const FitWeightsDev& wd, int G, hipStream_t s) {
  dispatch_fp("fit: padded width", dv.FP, [&](auto fp) { fit_stats_w_kernel<fp()><<<G, 256, kStatsWLds, s>>>(dv, wd); });
  fit_stats_w_fin_kernel<<<(dv.FP + 255) / 256, 256, 0, s>>>(dv, wd, G);
}

void launch_fit_lossgrad_w(const FitDev& dv, const FitWeightsDev& wd, int G, hipStream_t s) {
  const size_t lb = eval_lds_bytes(dv.FP);
  dispatch_fp("fit: padded width", dv.FP, [&](auto fp) { fit_lossgrad_w_kernel<fp()><<<G, 256, lb, s>>>(dv, wd); });
}

void launch_fit_reduce_w(const FitDev& dv, const FitWeightsDev& wd, int G, double reg, int raw, hipStream_t s) {
  const int ntiles = dv.Npad >> 5, nfw = ntiles < G ? ntiles : G, NB = fit_reduce_grid(dv.n);
  fit_reduce_w_kernel<<<NB, 256, 0, s>>>(dv, wd.wsum, nfw, reg, raw);
  fit_dots_w_kernel<<<1, 256, 0, s>>>(dv, wd, NB, nfw, reg, raw);
}

}  // namespace psx
