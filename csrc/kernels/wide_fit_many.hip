// Many wide (CSR) fits per read of the rows (gfx950 / CDNA4; the names are in
// wide_fit_many.h).  M models lie side by side in the 32 fp32 of one 128-byte line, so
// one gather of a feature's line, one read of col / val / crow / cval, of the inverted
// index and of the work items serves all of them:
//
//   wide_many_weights_kernel     v[r] = sample_weight * class_weight[y], one fp32 per row for
//                                every model; the held-out fold is decided per (row, slot)
//                                in the row pass from fold[r] == hold[slot]
//   wide_fit_rows_many_kernel<KP>
//       a wavefront per row (wave w of W owns rows w, w + W, ...).  Inside a row the wave
//       is 8 entry groups of 8 lanes: lane (g, q) takes the entries a + g, a + g + 8, ...
//       and of each the 16-byte quarter q of the feature's line, so the 8 lanes of a
//       group read the line as one coalesced 128-byte run and 8 lines are in flight per
//       step.  A lane keeps 4 column accumulators; the 8 groups are combined by a 3-step
//       butterfly (12 shuffles per row, not 32 x 6), after which every lane holds the
//       margins of its 4 columns.
//       Margins -> slots BY SHUFFLES, not through LDS: at KP <= 4 a lane's 4 columns
//       already are 4 / KP whole slots and nothing moves; at KP 8 / 16 the 2 / 4 lanes of
//       a slot fetch each other's quarters (4 / 12 shuffles) and each runs the slot's
//       softmax on the full z[KP] -- the same instructions in every lane of the slot, so
//       its own quarter of the residual is there without a second exchange.  A 128-byte
//       LDS scratch per wave would need a write, a wait and a read per row for the same
//       movement, and make the kernel's occupancy depend on LDS; this way the kernel has
//       no LDS and no barrier at all.
//       The slot's arithmetic is the plain kernel's (row maximum subtracted, exp(-|z|)
//       for one logit, the same nll).  Training row: R[r][slot] = v * residual; held-out
//       row: 0, and v * nll goes to the slot's held-out sum.  Lanes 0..7 store R[r] as
//       one contiguous 128-byte run.  Per wave: 32 residual sums and per slot the
//       training and the held-out loss (kWideManyPart floats).
//   wide_many_cols_short_kernel  items of <= kWideFitShort entries: 32 lanes per item, lane
//                                c sums column c over the item's entries in order
//   wide_many_cols_long_kernel   a wavefront per item, 8 lanes per entry with 16-byte
//                                loads of the residual line, 8 entries per step, the
//                                same butterfly
//   wide_many_bsum_kernel        the W residual-sum partials -> bsum[32], in a fixed order
//   wide_many_{begin, reduce, dots, update, finalize, scatter}_kernel
//       the vector kernels of a wide fit with the model on blockIdx.y, reading a device
//       array of WideManyModel; the solver vectors stay per model in the compact layout
//       and only the trial point is written into the model's slot of the lines.
//
// Every sum runs in an order fixed by the data and the options (col_chunk, max_wg) and
// is the same for every column of a line; products that feed a sum are explicit fmaf or
// built with contraction off, so two slots cannot differ in where a product is fused.
// No atomics, no cross-workgroup waits, no LDS in the passes over the data, plain
// vector stores; N * 32 and I * 32 are indexed in int64_t.
#include <hip/hip_runtime.h>

#include "common.h"
#include "dispatch.h"
#include "fit_body.h"
#include "wide_fit_many.h"

namespace psx {

namespace {

// the 8 entry groups of a wave combined: afterwards every lane holds its quarter's sums
__device__ __forceinline__ void groups_sum(float (&a)[4]) {
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a[j] += __shfl_xor(a[j], o, 64);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
struct WideManyCw {
  float c[16];
};

__global__ __launch_bounds__(256) void wide_many_weights_kernel(const int32_t* __restrict__ y,
                                                                const float* __restrict__ sw, int64_t N,
                                                                float* __restrict__ v, WideManyCw cw) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < N; r += (int64_t)gridDim.x * 256) {
    const int yr = y[r];
    float c = 0.f;  // a select chain: a table indexed by a lane's label would live in scratch
#pragma unroll
    for (int k = 0; k < 16; ++k) c = yr == k ? cw.c[k] : c;
    v[r] = (sw ? sw[r] : 1.f) * c;
  }
}

// ---------------------------------------------------------------------------
template <int KP>
__global__ __launch_bounds__(256) void wide_fit_rows_many_kernel(WideManyPass ps) {
#pragma clang fp contract(off)
  constexpr int SPL = KP < 4 ? 4 / KP : 1;  // whole slots in a lane's 4 columns
  constexpr int LPS = KP > 4 ? KP / 4 : 1;  // lanes (quarters) of one slot
  constexpr int CPS = KP < 4 ? KP : 4;      // columns of one slot that this lane stores
  const WideFitDev& dv = ps.dv;
  const int lane = threadIdx.x & 63, q = lane & 7, eg = lane >> 3, K = dv.K;
  // (the wave's index through readfirstlane: the row and everything loaded by it is wave-uniform)
  const int64_t w = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t W = (int64_t)gridDim.x * 4;
  const float* __restrict__ wm = ps.wm;
  const int slot0 = 4 * q / KP, sub = q & (LPS - 1);  // first slot of the lane; its quarter within the slot
  int hold[SPL];
  bool alive[SPL];
#pragma unroll
  for (int si = 0; si < SPL; ++si) {
    int h = -1;  // (a select chain over the kernel arguments, once per kernel)
#pragma unroll
    for (int i = 0; i < kWideLine; ++i) h = slot0 + si == i ? ps.hold[i] : h;
    hold[si] = h;
    alive[si] = ((ps.live >> (slot0 + si)) & 1u) != 0;
  }
  const f32x4 bv = *(const f32x4*)(wm + dv.U * kWideLine + 4 * q);
  float racc[4] = {0.f, 0.f, 0.f, 0.f}, lacc[SPL], hacc[SPL];
#pragma unroll
  for (int si = 0; si < SPL; ++si) lacc[si] = hacc[si] = 0.f;

  for (int64_t r = w; r < dv.N; r += W) {
    const float v = ps.v[r];
    float out[4] = {0.f, 0.f, 0.f, 0.f};
    float* Rr = dv.R + r * kWideLine + 4 * q;
    if (v == 0.f) {  // the row counts nowhere: no margins
      if (eg == 0) *(f32x4*)Rr = f32x4{0.f, 0.f, 0.f, 0.f};
      continue;
    }
    const int64_t a = dv.indptr[r], b = dv.indptr[r + 1];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int64_t e = a + eg; e < b; e += 8) {
      const int f = dv.col[e];
      const float x = bf2f(dv.val[e]);
      const f32x4 wv = *(const f32x4*)(wm + (int64_t)f * kWideLine + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(x, wv[j], acc[j]);
    }
    groups_sum(acc);
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += bv[j];
    const int y = dv.y[r];
    const int fr = ps.fold ? (int)ps.fold[r] : -1;
#pragma unroll
    for (int si = 0; si < SPL; ++si) {
      float z[KP], res[KP];
      if constexpr (KP <= 4) {
#pragma unroll
        for (int k = 0; k < KP; ++k) z[k] = acc[si * KP + k];
      } else {  // the quarters of the slot's other lanes
#pragma unroll
        for (int i = 0; i < LPS; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j) z[i * 4 + j] = __shfl(acc[j], (lane & ~(LPS - 1)) + i, 64);
      }
      if (!alive[si]) continue;  // a finished job: its residual columns stay 0
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
      if (hold[si] >= 0 && fr == hold[si]) {
        hacc[si] += v * nll;
      } else {
        lacc[si] += v * nll;
#pragma unroll
        for (int j = 0; j < CPS; ++j) {
          float rj = res[j];  // this lane's quarter of the slot (a select chain, no indexed registers)
#pragma unroll
          for (int i = 1; i < LPS; ++i) rj = sub == i ? res[i * 4 + j] : rj;
          out[si * CPS + j] = v * rj;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) racc[j] += out[j];
    if (eg == 0) *(f32x4*)Rr = f32x4{out[0], out[1], out[2], out[3]};
  }
  if (eg == 0) {  // every group holds the same sums: group 0 writes the wave's partial
    float* p = dv.part + w * kWideManyPart;
    *(f32x4*)(p + 4 * q) = f32x4{racc[0], racc[1], racc[2], racc[3]};
    if (sub == 0) {
#pragma unroll
      for (int si = 0; si < SPL; ++si) {
        p[kWideLine + slot0 + si] = lacc[si];
        p[2 * kWideLine + slot0 + si] = hacc[si];
      }
    }
  }
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wide_many_cols_short_kernel(WideFitDev dv) {
  const int c = threadIdx.x & 31;
  const float* __restrict__ R = dv.R;
  for (int64_t i = (int64_t)blockIdx.x * 8 + (threadIdx.x >> 5); i < dv.n_short; i += (int64_t)gridDim.x * 8) {
    const int it = dv.short_items[i];
    const int64_t a = dv.item_begin[it], b = dv.item_end[it];
    float acc = 0.f;
    for (int64_t e = a; e < b; ++e)
      acc = __builtin_fmaf(bf2f(dv.cval[e]), R[(int64_t)dv.crow[e] * kWideLine + c], acc);
    dv.gitem[(int64_t)it * kWideLine + c] = acc;
  }
}

__global__ __launch_bounds__(256) void wide_many_cols_long_kernel(WideFitDev dv) {
  const int lane = threadIdx.x & 63, q = lane & 7, eg = lane >> 3;
  const float* __restrict__ R = dv.R;
  for (int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); i < dv.n_long; i += (int64_t)gridDim.x * 4) {
    const int it = dv.long_items[i];
    const int64_t a = dv.item_begin[it], b = dv.item_end[it];
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int64_t e = a + eg; e < b; e += 8) {
      const float x = bf2f(dv.cval[e]);
      const f32x4 rv = *(const f32x4*)(R + (int64_t)dv.crow[e] * kWideLine + 4 * q);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_fmaf(x, rv[j], acc[j]);
    }
    groups_sum(acc);
    if (eg == 0) *(f32x4*)(dv.gitem + (int64_t)it * kWideLine + 4 * q) = f32x4{acc[0], acc[1], acc[2], acc[3]};
  }
}

// The W per-wave residual sums -> bsum[32]: 8 strided lanes per column, combined in order.
__global__ __launch_bounds__(256) void wide_many_bsum_kernel(WideFitDev dv) {
  __shared__ float red[8][kWideLine];
  const int t = threadIdx.x, c = t & 31, q = t >> 5;
  float a = 0.f;
  for (int g = q; g < dv.W; g += 8) a += dv.part[(size_t)g * kWideManyPart + c];
  red[q][c] = a;
  __syncthreads();
  if (t < kWideLine) {
    float s = 0.f;
    for (int i = 0; i < 8; ++i) s += red[i][t];
    dv.bsum[t] = s;
  }
}

// ---------------------------------------------------------------------------
// The rule of wide_fit_write_trial, into the model's slot of its feature's line.
__device__ __forceinline__ void wide_many_write_trial(const WideManyModel& md, int e, float bt) {
  const WideFitDev& dv = md.dv;
  const int KP = dv.KP, u = e / KP, k = e - u * KP;
  dv.beta_t[e] = bt;
  float val = bt;  // the intercept row (u == U)
  if (u < dv.U) {
    const float iv = dv.inv_std[u];
    val = iv > 0.f ? bt * iv : dv.wfix[e];
  }
  md.wm[(int64_t)u * kWideLine + md.col0 + k] = val;
}

// wide_fit_begin_kernel per model.
__global__ __launch_bounds__(256) void wide_many_begin_kernel(const WideManyModel* __restrict__ mm, int zero_const,
                                                              int raw) {
  const WideManyModel& md = mm[blockIdx.y];
  const WideFitDev& dv = md.dv;
  const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= dv.n) return;
  const int e = (int)e64, KP = dv.KP, u = e / KP, k = e - u * KP;
  float w = 0.f;
  if (md.w0 && k < dv.K) w = md.w0[(u < dv.U ? (int64_t)dv.uniq[u] : dv.F) * KP + k];
  if (raw) {  // one evaluation at the weights themselves
    md.wm[(int64_t)u * kWideLine + md.col0 + k] = w;
    return;
  }
  float xv = w;
  if (u < dv.U) {
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
  wide_many_write_trial(md, e, xv);
}

// wide_fit_reduce_w_kernel per model: a column's items summed in chunk order out of the
// model's slot, g_t = sum / W_d * inv_std_d[u] + reg_m * beta_t, the partial fp64 dots.
__global__ __launch_bounds__(256) void wide_many_reduce_kernel(const WideManyModel* __restrict__ mm,
                                                               const int* __restrict__ live, int m0, int raw) {
  const int m = m0 + blockIdx.y;
  if (!live[m]) return;
  const WideManyModel& md = mm[m];
  const WideFitDev& dv = md.dv;
  __shared__ double red[4][kFitDotStride];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int KP = dv.KP, UKP = (int)dv.U * KP, H = dv.H, col0 = md.col0;
  const float invW = (float)(1.0 / md.wsum[0]);
  const float reg = (float)md.reg;
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
      for (int i = i0; i < i1; ++i) s += dv.gitem[(int64_t)i * kWideLine + col0 + k];
      if (!raw) {
        bt = dv.beta_t[e];
        {  // both products rounded, then added (as wide_fit_reduce_w_kernel)
#pragma clang fp contract(off)
          const float gl = s * invW * dv.inv_std[u], gr = reg * bt;
          g = gl + gr;
        }
      } else {
        g = s * invW;
      }
    } else {
      g = dv.bsum[col0 + e - UKP] * invW;
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

// wide_fit_dots_w_kernel per model: the slot's loss partials of the W waves, in order;
// the held-out mean goes behind the result block.
__global__ __launch_bounds__(256) void wide_many_dots_kernel(const WideManyModel* __restrict__ mm,
                                                             const int* __restrict__ live, int m0, int NB, int raw) {
  const int m = m0 + blockIdx.y;
  if (!live[m]) return;
  const WideManyModel& md = mm[m];
  const WideFitDev& dv = md.dv;
  __shared__ double red[4][64];
  __shared__ double lred[2][256];
  const int t = threadIdx.x, k = t & 63, q = t >> 6, slot = md.col0 / dv.KP;
  const int nd = raw ? 0 : 3 + 2 * dv.H + 1;
  double a = 0.0;
  if (k < nd)
    for (int b = q; b < NB; b += 4) a += dv.dpart[(size_t)b * kFitDotStride + k];
  red[q][k] = a;
  double ls = 0.0, hs = 0.0;
  for (int g = t; g < dv.W; g += 256) {
    ls += (double)dv.part[(size_t)g * kWideManyPart + kWideLine + slot];
    hs += (double)dv.part[(size_t)g * kWideManyPart + 2 * kWideLine + slot];
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
__global__ __launch_bounds__(256) void wide_many_update_kernel(const WideManyModel* __restrict__ mm,
                                                               const FitStep* __restrict__ steps) {
  static_assert(sizeof(FitStep) % 8 == 0 && sizeof(FitStep) / 8 <= 256, "FitStep is copied in 8-byte words");
  __shared__ FitStep st;
  if (threadIdx.x < sizeof(FitStep) / 8)
    ((unsigned long long*)&st)[threadIdx.x] = ((const unsigned long long*)(steps + blockIdx.y))[threadIdx.x];
  __syncthreads();
  if (st.action == kActNone) return;
  const WideManyModel& md = mm[blockIdx.y];
  const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= md.dv.n) return;
  fit_update_body(md.dv, st, (int)e64, [&](int i, float bt) { wide_many_write_trial(md, i, bt); });
}

// wide_fit_finalize_kernel per model, into the model's full vector.
__global__ __launch_bounds__(256) void wide_many_finalize_kernel(const WideManyModel* __restrict__ mm,
                                                                 float* __restrict__ w_all) {
  const WideManyModel& md = mm[blockIdx.y];
  const WideFitDev& dv = md.dv;
  const int64_t u64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u64 > dv.U) return;
  const int u = (int)u64, KP = dv.KP, K = dv.K;
  const bool icpt = u == dv.U, center = md.reg == 0.0;
  const float iv = icpt ? 0.f : dv.inv_std[u];
  const float* x = dv.x + (int64_t)u * KP;
  const float* wf = dv.wfix + (int64_t)u * KP;
  float* o = w_all + (int64_t)blockIdx.y * (dv.F + 1) * KP + (icpt ? dv.F : (int64_t)dv.uniq[u]) * KP;
  float mean = 0.f;
  for (int k = 0; k < K; ++k) mean += icpt ? x[k] : (iv > 0.f ? x[k] * iv : wf[k]);
  mean = (K >= 2 && (icpt || center)) ? mean / (float)K : 0.f;
  for (int k = 0; k < KP; ++k) {
    const float v = icpt ? x[k] : (iv > 0.f ? x[k] * iv : wf[k]);
    o[k] = k < K ? v - mean : 0.f;
  }
}

__global__ __launch_bounds__(256) void wide_many_scatter_kernel(const WideManyModel* __restrict__ mm,
                                                                float* __restrict__ grads) {
  const WideManyModel& md = mm[blockIdx.y];
  const WideFitDev& dv = md.dv;
  const int64_t e64 = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e64 >= dv.n) return;
  const int e = (int)e64, KP = dv.KP, u = e / KP, k = e - u * KP;
  grads[(int64_t)blockIdx.y * (dv.F + 1) * KP + (u < dv.U ? (int64_t)dv.uniq[u] : dv.F) * KP + k] = dv.g_t[e];
}

// ---------------------------------------------------------------------------
static unsigned blocks_of(int64_t n, int per, int64_t cap) {
  int64_t b = (n + per - 1) / per;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

void launch_wide_many_weights(const WideFitDev& dv, const float* sw, const float (&cw)[16], float* v, hipStream_t s) {
  WideManyCw t;
  for (int k = 0; k < 16; ++k) t.c[k] = cw[k];
  wide_many_weights_kernel<<<blocks_of(dv.N, 256, 1024), 256, 0, s>>>(dv.y, sw, dv.N, v, t);
}

void launch_wide_many_begin(const WideManyModel* mm, int M, int n, int zero_const, int raw, hipStream_t s) {
  wide_many_begin_kernel<<<dim3(blocks_of(n, 256, INT64_MAX), M), 256, 0, s>>>(mm, zero_const, raw);
}

void launch_wide_many_eval(const WideManyPass& ps, int G, hipStream_t s) {
  const WideFitDev& dv = ps.dv;
  dispatch_wide_kp("wide fit_many: padded classes", dv.KP,
                   [&](auto kp) { wide_fit_rows_many_kernel<kp()><<<G, 256, 0, s>>>(ps); });
  if (dv.n_short > 0) wide_many_cols_short_kernel<<<blocks_of(dv.n_short, 8, 1 << 16), 256, 0, s>>>(dv);
  if (dv.n_long > 0) wide_many_cols_long_kernel<<<blocks_of(dv.n_long, 4, 1 << 16), 256, 0, s>>>(dv);
  wide_many_bsum_kernel<<<1, 256, 0, s>>>(dv);
}

void launch_wide_many_reduce(const WideManyModel* mm, const int* live, int m0, int cnt, int n, int raw,
                             hipStream_t s) {
  const int NB = wide_fit_reduce_grid(n);
  wide_many_reduce_kernel<<<dim3(NB, cnt), 256, 0, s>>>(mm, live, m0, raw);
  wide_many_dots_kernel<<<dim3(1, cnt), 256, 0, s>>>(mm, live, m0, NB, raw);
}

void launch_wide_many_update(const WideManyModel* mm, const FitStep* steps, int M, int n, hipStream_t s) {
  wide_many_update_kernel<<<dim3(blocks_of(n, 256, INT64_MAX), M), 256, 0, s>>>(mm, steps);
}

void launch_wide_many_finalize(const WideManyModel* mm, int M, int64_t U, float* w_all, hipStream_t s) {
  wide_many_finalize_kernel<<<dim3(blocks_of(U + 1, 256, INT64_MAX), M), 256, 0, s>>>(mm, w_all);
}

void launch_wide_many_scatter(const WideManyModel* mm, int M, int n, float* grads, hipStream_t s) {
  wide_many_scatter_kernel<<<dim3(blocks_of(n, 256, INT64_MAX), M), 256, 0, s>>>(mm, grads);
}

}  // namespace psx
