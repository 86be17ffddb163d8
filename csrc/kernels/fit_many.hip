// Many dense fits per read of the rows (gfx950 / CDNA4; the names are in fit_many.h).
//
// fit_lossgrad_w_kernel is bandwidth-bound and fills K of the 16 columns of its MFMA
// products; the other columns multiply zero fragments.  Here a tile is staged once and
// serves GP groups of 16 columns, every group packed with 16 / KP models:
//
//   fit_lossgrad_many_kernel<FP, KP, GP>
//       workgroup wg takes the 32-row tiles wg, wg + G, ... as the plain kernel does.
//       Per tile: stage_tile once; the row's base weight v = sample_weight *
//       class_weight[y] once; then three phases over the groups, one barrier each --
//         forward   X_tile . W_g^T against group g's hi/lo fragments into the group's
//                   own logits buffer (GP buffers of 8 KB: no barrier between groups)
//         rows      a SEGMENTED softmax and cross entropy: 8 threads per row, 2 columns
//                   each; max and sum are butterflies over the KP / 2 threads of a slot.
//                   u = v [fold != holdout_slot], h = v [fold == holdout_slot]; the
//                   residual is scaled by u before the bf16 hi/lo split -> the group's
//                   own rt image (2 KB)
//         backward  bwd_tile_acc into acc[g][FP / 64], the transposed reads of the one
//                   staged image shared by all groups
//       LDS: the image, GP x 10 KB, 0.4 KB of row words and GP x 0.5 KB of end-of-kernel
//       sums: 138.9 KB at FP 2048 (GP 1), 95.9 KB at FP 1024 (GP 3).
//   fit_many_{begin, reduce, dots, update, finalize}_kernel
//       the vector kernels of a fit with the model on blockIdx.y, reading a device
//       array of FitManyModel; update reads the models' FitSteps from pinned memory.
//
// Every sum runs in a fixed order that does not depend on the slot a model occupies:
// butterflies over aligned lane groups, waves in order, workgroups in order.  A column
// of an MFMA product depends on that column's operands alone.  The row phase is built
// with floating-point contraction off, so the unrolled copies of the groups cannot
// differ in where a product is fused.  No atomics, no scratch.
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "fit_many.h"
#include "solve_body.h"

namespace psx {

constexpr int kGroupLds = 8192 + 2048;  // one group's logits buffer and rt image
constexpr size_t many_lds_bytes(int FP, int GP) {
  return (size_t)32 * FP * 2 + (size_t)GP * kGroupLds + 3 * 32 * 4 + (size_t)GP * (64 + 64) * 4;
}
static_assert(many_lds_bytes(2048, many_groups(2048, 2)) <= 160 * 1024, "gfx950 has 160 KB of LDS");

// The rows phase of one group for the thread's (row sr, columns sc0, sc0 + 1).
template <int KP>
__device__ __forceinline__ void many_rows(const char* red, unsigned short* rt, int K, int sr, int sc0, float bz0,
                                          float bz1, int hold, int yl, float v, int fold, bool valid, float& loss,
                                          float& hloss, float& rs0, float& rs1) {
#pragma clang fp contract(off)
  const int k0 = sc0 & (KP - 1);  // the columns' classes within their slot
  const bool v0 = k0 < K, v1 = k0 + 1 < K;
  const float z0 = v0 ? load_logit(red, sr, sc0) + bz0 : -INFINITY;
  const float z1 = v1 ? load_logit(red, sr, sc0 + 1) + bz1 : -INFINITY;
  float mx = fmaxf(z0, z1);
#pragma unroll
  for (int o = 1; o < KP / 2; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  const float e0 = v0 ? __expf(z0 - mx) : 0.f, e1 = v1 ? __expf(z1 - mx) : 0.f;
  float se = e0 + e1;
#pragma unroll
  for (int o = 1; o < KP / 2; o <<= 1) se += __shfl_xor(se, o, 64);
  const bool held = hold >= 0 && fold == hold;
  const float u = held ? 0.f : v, h = held ? v : 0.f;
  const float inv = 1.f / se;
  const float p0 = valid && v0 ? e0 * inv - (yl == k0 ? 1.f : 0.f) : 0.f;
  const float p1 = valid && v1 ? e1 * inv - (yl == k0 + 1 ? 1.f : 0.f) : 0.f;
  const float r0 = u * p0, r1 = u * p1;  // weighted residual: the backward is the plain R^T X
  if (valid) {
    const float lse = mx + __logf(se);
    if (yl == k0) {
      const float ce = lse - z0;
      loss += u * ce;
      hloss += h * ce;
    }
    if (yl == k0 + 1) {
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

template <int FP, int KP, int GP>
__global__ __launch_bounds__(256) void fit_lossgrad_many_kernel(FitManyPass ps) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  constexpr int NT = FP / 64, SPG = 16 / KP, SP = GP * SPG;
  f32x4 acc[GP][NT];
#pragma unroll
  for (int g = 0; g < GP; ++g)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[g][n] = f32x4{0, 0, 0, 0};
  const int wg = blockIdx.x, G = gridDim.x, K = ps.K, N = ps.N;
  const int ntiles = (N + 31) >> 5;
  if (wg >= ntiles) return;  // no tile: no partial (the reduction sums min(G, tiles) of them)
  char* red0 = lds + 32 * FP * 2;  // group g: logits at red0 + g * kGroupLds, rt 8 KB behind them
  int* ylds = (int*)(red0 + GP * kGroupLds);
  float* vw = (float*)(ylds + 32);  // [32] base weight of the tile's rows (0 for rows >= N)
  int* fl = (int*)(vw + 32);        // [32] fold of the tile's rows
  float* rsum = (float*)(fl + 32);  // [GP][4 waves][16]
  float* lred = rsum + GP * 64;     // [GP][training | held-out][4 waves][8 slots]
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sr = tid >> 3, sc0 = (tid & 7) * 2;

  float loss[GP], hloss[GP], rs0[GP], rs1[GP], bz0[GP], bz1[GP];
  int hold[GP];
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    loss[g] = hloss[g] = rs0[g] = rs1[g] = 0.f;
    bz0[g] = ps.b_eff[g * 16 + sc0];
    bz1[g] = ps.b_eff[g * 16 + sc0 + 1];
    hold[g] = ps.hold[g * SPG + sc0 / KP];
  }
  for (int tile = wg; tile < ntiles; tile += G) {
    const int64_t row0 = (int64_t)tile * 32;
    // labels and weight streams issued with the tile's loads (one round trip)
    int yv = 0, fv = -1;
    float sv = 1.f;
    if (tid < 32) {
      yv = ps.y[row0 + tid];
      if (ps.sw) sv = ps.sw[row0 + tid];
      if (ps.fold) fv = (int)ps.fold[row0 + tid];
    }
    stage_tile<FP>(lds, ps.X, row0, 32, ps.Npad, false);
    if (tid < 32) {
      float c = 0.f;  // a select chain: a table indexed by a lane's label would live in scratch
#pragma unroll
      for (int k = 0; k < 16; ++k) c = yv == k ? ps.cw[k] : c;
      ylds[tid] = yv;
      vw[tid] = row0 + tid < N ? sv * c : 0.f;
      fl[tid] = fv;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      if (!((ps.gmask >> g) & 1u)) continue;
      f32x4 a0, a1;
      forward_tile<FP>(lds, ps.whi + (size_t)g * 16 * FP, ps.wlo + (size_t)g * 16 * FP, a0, a1);
      store_partial_logits(red0 + g * kGroupLds, a0, a1);
    }
    __syncthreads();
    {
      const int yl = ylds[sr], fr = fl[sr];
      const float v = vw[sr];
      const bool valid = tile * 32 + sr < N;
#pragma unroll
      for (int g = 0; g < GP; ++g) {
        if (!((ps.gmask >> g) & 1u)) continue;
        char* red = red0 + g * kGroupLds;
        many_rows<KP>(red, (unsigned short*)(red + 8192), K, sr, sc0, bz0[g], bz1[g], hold[g], yl, v, fr, valid,
                      loss[g], hloss[g], rs0[g], rs1[g]);
      }
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < GP; ++g) {
      if (!((ps.gmask >> g) & 1u)) continue;
      bwd_tile_acc<FP>(lds, (const unsigned short*)(red0 + g * kGroupLds + 8192), acc[g]);
    }
    __syncthreads();  // the next tile's staging overwrites the image and the row words
  }
  // fixed order: butterflies over the lanes of one column pair / one slot, then the waves in order
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    float a = rs0[g], b = rs1[g], l = loss[g], h = hloss[g];
#pragma unroll
    for (int o = 1; o < KP / 2; o <<= 1) {
      l += __shfl_xor(l, o, 64);
      h += __shfl_xor(h, o, 64);
    }
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
      l += __shfl_xor(l, o, 64);
      h += __shfl_xor(h, o, 64);
    }
    if (lane < 8) {
      rsum[(g * 4 + w) * 16 + sc0] = a;
      rsum[(g * 4 + w) * 16 + sc0 + 1] = b;
      if ((sc0 & (KP - 1)) == 0) {
        lred[((g * 2 + 0) * 4 + w) * 8 + sc0 / KP] = l;
        lred[((g * 2 + 1) * 4 + w) * 8 + sc0 / KP] = h;
      }
    }
  }
  __syncthreads();
  float* part = ps.part + (size_t)wg * SP * kPartStride;
  if (tid < GP * 16) {
    const int g = tid >> 4, c = tid & 15, k = c & (KP - 1);
    const float* r = rsum + g * 64 + c;
    if (k < K && ((ps.gmask >> g) & 1u)) part[(g * SPG + c / KP) * kPartStride + k] = ((r[0] + r[16]) + r[32]) + r[48];
  } else if (tid >= 64 && tid < 64 + 2 * SP) {
    const int q = tid - 64, slot = q >> 1, ho = q & 1, g = slot / SPG;
    const float* r = lred + ((g * 2 + ho) * 4) * 8 + slot % SPG;
    if ((ps.gmask >> g) & 1u) part[slot * kPartStride + 16 + ho] = ((r[0] + r[8]) + r[16]) + r[24];
  }
#pragma unroll
  for (int g = 0; g < GP; ++g) {
    if (!((ps.gmask >> g) & 1u)) continue;
#pragma unroll
    for (int n = 0; n < NT; ++n) {
      const int f = (w * NT + n) * 16 + (lane & 15);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = (lane >> 4) * 4 + i, k = c & (KP - 1);
        if (k < K) ps.gpart[(((size_t)wg * SP + g * SPG + c / KP) * K + k) * FP + f] = acc[g][n][i];
      }
    }
  }
}

// ---------------------------------------------------------------------------
// The trial point of model `md`: fit_write_trial of fit_kernels.hip with the class's
// column shifted to the model's slot.
__device__ __forceinline__ void many_write_trial(const FitManyModel& md, int e, float bt) {
  const FitDev& dv = md.dv;
  const int KF = dv.K * dv.FP;
  dv.beta_t[e] = bt;
  if (e < KF) {
    const int c = e / dv.FP, f = e - c * dv.FP;
    const float iv = dv.inv_std[f];
    write_frag(dv.whi, dv.wlo, md.col0 + c, f, iv > 0.f ? bt * iv : dv.wfix[e]);
  } else {
    dv.b_eff[md.col0 + e - KF] = bt;
  }
}

// fit_begin_kernel per model.
__global__ __launch_bounds__(256) void fit_many_begin_kernel(const FitManyModel* __restrict__ mm, int zero_const,
                                                             int raw) {
  const FitManyModel& md = mm[blockIdx.y];
  const FitDev& dv = md.dv;
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= dv.n) return;
  const int KF = dv.K * dv.FP;
  const float w = md.w0 ? md.w0[e] : 0.f;
  if (raw) {  // one evaluation at the weights themselves
    if (e < KF) {
      const int c = e / dv.FP, f = e - c * dv.FP;
      write_frag(dv.whi, dv.wlo, md.col0 + c, f, f < dv.F ? w : 0.f);
    } else {
      dv.b_eff[md.col0 + e - KF] = w;
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
  many_write_trial(md, e, xv);
}

// fit_reduce_w_kernel per model: the slot's partials lie gstride / pstride floats apart.
__global__ __launch_bounds__(256) void fit_many_reduce_kernel(const FitManyModel* __restrict__ mm,
                                                              const int* __restrict__ live, int m0, int nfw, int raw) {
  const int m = m0 + blockIdx.y;
  if (!live[m]) return;
  const FitManyModel& md = mm[m];
  const FitDev& dv = md.dv;
  __shared__ float red[4][64];
  const int t = threadIdx.x, l = t & 63, sub = t >> 6;
  const int e = blockIdx.x * 64 + l, KF = dv.K * dv.FP;
  float a = 0.f;
  if (e < dv.n) {
    const float* src = e < KF ? dv.gpart + e : dv.part + (e - KF);
    const size_t stride = e < KF ? (size_t)md.gstride : (size_t)md.pstride;
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
    const float invW = (float)(1.0 / md.wsum[0]);
    if (e < KF && !raw) {
      const int f = e & (dv.FP - 1);
      bt = dv.beta_t[e];
      {  // both products rounded, then added (as fit_reduce_w_kernel)
#pragma clang fp contract(off)
        const float gl = s * invW * dv.inv_std[f], gr = (float)md.reg * bt;
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

// fit_dots_w_kernel per model; the held-out mean goes behind the result block.
__global__ __launch_bounds__(256) void fit_many_dots_kernel(const FitManyModel* __restrict__ mm,
                                                            const int* __restrict__ live, int m0, int NB, int nfw,
                                                            int raw) {
  const int m = m0 + blockIdx.y;
  if (!live[m]) return;
  const FitManyModel& md = mm[m];
  const FitDev& dv = md.dv;
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
    ls += (double)dv.part[(size_t)g * md.pstride + 16];
    hs += (double)dv.part[(size_t)g * md.pstride + 17];
  }
  lred[0][t] = ls;
  lred[1][t] = hs;
  __syncthreads();
  if (t < nd - 1) dv.out[kFitOutDots + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (t == 0) {
    double loss = 0.0;
    for (int i = 0; i < 256; ++i) loss += lred[0][i];
    loss /= md.wsum[0];
    double bb = 0.0;
    if (nd > 0) bb = ((red[0][nd - 1] + red[1][nd - 1]) + red[2][nd - 1]) + red[3][nd - 1];
    dv.out[kFitOutF] = loss + 0.5 * md.reg * bb;
    dv.out[kFitOutLoss] = loss;
  }
  if (t == 64) {
    double h = 0.0;
    for (int i = 0; i < 256; ++i) h += lred[1][i];
    const double who = md.wsum[1];
    dv.out[kFitOutWords] = who > 0.0 ? h / who : 0.0;
  }
}

// One controller action per model (fit_update_body of fit_step.h); the action is read
// from pinned memory once per workgroup.  kActNone: a finished model, nothing moves.
__global__ __launch_bounds__(256) void fit_many_update_kernel(const FitManyModel* __restrict__ mm,
                                                              const FitStep* __restrict__ steps) {
  static_assert(sizeof(FitStep) % 8 == 0 && sizeof(FitStep) / 8 <= 256, "FitStep is copied in 8-byte words");
  __shared__ FitStep st;
  if (threadIdx.x < sizeof(FitStep) / 8)
    ((unsigned long long*)&st)[threadIdx.x] = ((const unsigned long long*)(steps + blockIdx.y))[threadIdx.x];
  __syncthreads();
  if (st.action == kActNone) return;
  const FitManyModel& md = mm[blockIdx.y];
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= md.dv.n) return;
  fit_update_body(md.dv, st, e, [&](int i, float bt) { many_write_trial(md, i, bt); });
}

// fit_finalize_kernel per model.
__global__ __launch_bounds__(256) void fit_many_finalize_kernel(const FitManyModel* __restrict__ mm,
                                                                float* __restrict__ w_all) {
  const FitManyModel& md = mm[blockIdx.y];
  const FitDev& dv = md.dv;
  const int f = blockIdx.x * 256 + threadIdx.x, FP = dv.FP, K = dv.K;
  if (f >= FP) return;
  float* w_out = w_all + (size_t)blockIdx.y * dv.n;
  const bool center = md.reg == 0.0;
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
template <class F>
static void for_each_many(F&& f) {
  for_each_fp([&](auto fp) { for_each_int<2, 4, 8, 16>([&](auto kp) { f(fp, kp); }); });
}

void prepare_fit_many_kernels() {
  static bool done = false;
  if (done) return;
  for_each_many([](auto fp, auto kp) {
    constexpr int GP = many_groups(fp(), kp());
    (void)hipFuncSetAttribute((const void*)fit_lossgrad_many_kernel<fp(), kp(), GP>,
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)many_lds_bytes(fp(), GP));
  });
  done = true;
}

void launch_fit_many_lossgrad(const FitManyPass& ps, int FP, int G, hipStream_t s) {
  dispatch_fp("fit_many: padded width", FP, [&](auto fp) {
    dispatch_int<2, 4, 8, 16>("fit_many: padded classes", many_kp(ps.K), [&](auto kp) {
      constexpr int GP = many_groups(fp(), kp());
      fit_lossgrad_many_kernel<fp(), kp(), GP><<<G, 256, many_lds_bytes(fp(), GP), s>>>(ps);
    });
  });
}

void launch_fit_many_begin(const FitManyModel* mm, int M, int n, int zero_const, int raw, hipStream_t s) {
  fit_many_begin_kernel<<<dim3((n + 255) / 256, M), 256, 0, s>>>(mm, zero_const, raw);
}

void launch_fit_many_reduce(const FitManyModel* mm, const int* live, int m0, int cnt, int n, int nfw, int raw,
                            hipStream_t s) {
  fit_many_reduce_kernel<<<dim3(fit_reduce_grid(n), cnt), 256, 0, s>>>(mm, live, m0, nfw, raw);
  fit_many_dots_kernel<<<dim3(1, cnt), 256, 0, s>>>(mm, live, m0, fit_reduce_grid(n), nfw, raw);
}


void launch_fit_many_update(const FitManyModel* mm, const FitStep* steps, int M, int n, hipStream_t s) {
  fit_many_update_kernel<<<dim3((n + 255) / 256, M), 256, 0, s>>>(mm, steps);
}

void launch_fit_many_finalize(const FitManyModel* mm, int M, int FP, float* w_out, hipStream_t s) {
  fit_many_finalize_kernel<<<dim3((FP + 255) / 256, M), 256, 0, s>>>(mm, w_out);
}

}  // namespace psx
