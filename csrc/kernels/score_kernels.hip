// Scoring kernels (gfx950 / CDNA4): see score_kernels.h for the outputs.
//
// Replaces the reference's predict() (LogisticRegressionTaskSpark.java:236-251,
// SURVEY C11), which only ever fed the metrics of the training loop: here every
// row's prediction, probabilities and loss reach the caller, in one pass.
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "lr_kernels.h"
#include "score_kernels.h"
#include "tile.h"
#include "wide_row.h"

namespace psx {

namespace {

// (1 - sigmoid(z), sigmoid(z))[c], from exp(-|z|) so that neither side overflows
__device__ __forceinline__ float sigmoid_side(float z, int c) {
  const float e = expf(-fabsf(z));
  const float big = 1.f / (1.f + e), small = e / (1.f + e);
  return ((z >= 0.f) == (c == 1)) ? big : small;
}

// softplus(z) - y z, stable for both signs (wide_kernels.hip: row_residual)
__device__ __forceinline__ float binary_nll(float z, int y) {
  return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))) - (y ? z : 0.f);
}

__device__ __forceinline__ int clamp_label(int y, bool binary) {
  if (binary) return y > 0 ? 1 : 0;
  return y < 0 ? 0 : (y > 15 ? 15 : y);
}

// workgroup counts -> one global integer atomic per non-zero cell
__device__ __forceinline__ void flush_counts(const int* cl, const int* noor, const ScoreOut& o) {
  const int v = cl[threadIdx.x];
  if (v) atomicAdd(o.conf + threadIdx.x, v);
  if (threadIdx.x == 0 && *noor) atomicAdd(o.oor, *noor);
}

// Score-histogram bin of a one-vs-rest log-odds l (score_kernels.h): clamped in
// float before the conversion, so +inf lands in bin 511, -inf and NaN in bin 0
// (fmaxf returns its other operand for a NaN).
__device__ __forceinline__ int hist_bin(float l) {
  return 256 + (int)fminf(fmaxf(rintf(16.f * l), -256.f), 255.f);
}

// workgroup table [Ch][2][512] -> one global integer atomic per non-zero cell
__device__ __forceinline__ void flush_hist(const int* ht, int Ch, int* hist) {
  for (int i = threadIdx.x; i < Ch * kHistCells; i += 256) {
    const int v = ht[i];
    if (v) atomicAdd(hist + i, v);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// Dense (multinomial, 2 <= K <= 16: the dense model has no one-logit form):
// 32-row tiles as logits_kernel; the margins stay in the LDS reduction buffer.
// The row epilogue (max, argmax, sum of exponentials, label margin) runs once
// per row on 32 threads and leaves the row's max and sum in LDS; the
// probabilities -- the only sizeable output stream -- are then written by all
// 256 threads as one contiguous run of nrows * K floats per tile.
//
// HM (the score histogram, score_kernels.h): kHistOff is the kernel as it was.
// Otherwise the epilogue also leaves the row's margins (intercepts included) and
// its label in LDS, and all 256 threads walk the tile's nrows * K entries as the
// probability writer does: the log-odds from a direct sum over the other classes,
// the bin, one integer atomic.  kHistLds counts in a workgroup-private table of
// K * 4 KB behind eval_lds_bytes(FP), flushed once after the tile loop.  At
// FP 2048 only 20,992 B are left beside the tile, a table of 5 classes; kHistGlobal
// is the form for K > 5 there: the same entries, added straight to the global
// table.  Half-width counters would still need 32 KB at K = 16 and a table
// resident for part of the classes would walk the entries several times, while
// global integer atomics need no LDS at all and give the identical table.  They
// are slow where many rows share a bin (every workgroup adds to the same words:
// profiles/r14, tools/bench_score.py --curves), so launch_score takes this form
// only where the LDS table does not fit.
template <int FP, int HM = kHistOff>
__global__ __launch_bounds__(256) void score_kernel(int K, const uint16_t* __restrict__ X,
                                                    const int32_t* __restrict__ y, int T,
                                                    const uint16_t* __restrict__ wf_hi,
                                                    const uint16_t* __restrict__ wf_lo, const float* __restrict__ b,
                                                    ScoreOut o) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* red_base = lds + 32 * FP * 2;
  int* cl = (int*)(red_base + 8192);  // [16][16]
  float* rmax = (float*)(cl + 256);   // [32] row maximum
  float* rsum = rmax + 32;            // [32] sum of exp(z - max)
  int* noor = (int*)(rsum + 32);
  int* rlab = noor + 1;                  // [32] the rows' labels            (HM only)
  float* zt = (float*)(rlab + 32);       // [32][16] margins with intercepts (HM only)
  int* ht = (int*)(lds + eval_lds_bytes(FP));  // [K][2][512]                (kHistLds only)
  const int tid = threadIdx.x;
  const bool need_sum = o.proba != nullptr || (y != nullptr && o.nll != nullptr);
  cl[tid] = 0;
  if (tid == 0) *noor = 0;
  if constexpr (HM == kHistLds)
    for (int i = tid; i < K * kHistCells; i += 256) ht[i] = 0;
  constexpr bool kPre = FP <= 1024;
  WFrag<kPre ? FP : 128> wf;
  if constexpr (kPre) load_wfrag<FP>(wf, wf_hi, wf_lo, K);
  const int ntiles = (T + 31) / 32;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int nrows = min(32, T - tile * 32);
    const int64_t row0 = (int64_t)tile * 32;
    const int ylab = (y != nullptr && tid < nrows) ? y[row0 + tid] : 0;  // travels with the tile's loads
    stage_tile<FP>(lds, X, row0, nrows, 0, false);
    __syncthreads();
    f32x4 a0, a1;
    if constexpr (kPre)
      forward_tile_pre<FP>(lds, wf, a0, a1);
    else
      forward_tile<FP>(lds, wf_hi, wf_lo, a0, a1);
    store_partial_logits(red_base, a0, a1);
    __syncthreads();
    if (tid < nrows) {
      int best = 0;
      float bz = -INFINITY;
      for (int c = 0; c < K; ++c) {
        const float z = load_logit(red_base, tid, c) + b[c];
        if constexpr (HM != kHistOff) zt[tid * 16 + c] = z;
        if (z > bz) {
          bz = z;
          best = c;
        }
      }
      if constexpr (HM != kHistOff) rlab[tid] = ylab;
      float s = 0.f;
      if (need_sum)
        for (int c = 0; c < K; ++c) s += expf(load_logit(red_base, tid, c) + b[c] - bz);
      rmax[tid] = bz;
      rsum[tid] = s;
      o.pred[row0 + tid] = best;
      if (y != nullptr) {
        const bool in_range = ylab >= 0 && ylab < K;
        if (!in_range) atomicAdd(noor, 1);
        if (o.nll != nullptr)
          o.nll[row0 + tid] =
              in_range ? logf(s) - (load_logit(red_base, tid, ylab) + b[ylab] - bz) : __builtin_nanf("");
        atomicAdd(&cl[clamp_label(ylab, false) * 16 + best], 1);
      }
    }
    if (o.proba != nullptr) {
      __syncthreads();
      float* dst = o.proba + row0 * K;
      for (int e = tid; e < nrows * K; e += 256) {
        const int r = e / K, c = e - r * K;
        dst[e] = expf(load_logit(red_base, r, c) + b[c] - rmax[r]) / rsum[r];
      }
    }
    if constexpr (HM != kHistOff) {
      if (o.proba == nullptr) __syncthreads();  // zt, rlab, rmax (the probability writer has synchronised)
      for (int e = tid; e < nrows * K; e += 256) {
        const int r = e / K, c = e - r * K;
        const int yl = rlab[r];
        if (yl < 0 || yl >= K) continue;  // counted in oor, enters no cell
        const float* zr = zt + r * 16;
        const float m = rmax[r];
        float so = 0.f;  // over the other classes, never s - e_c
        for (int j = 0; j < K; ++j)
          if (j != c) so += expf(zr[j] - m);
        const int cell = (c * 2 + (yl == c ? 1 : 0)) * kHistBins + hist_bin((zr[c] - m) - logf(so));
        if constexpr (HM == kHistLds)
          atomicAdd(ht + cell, 1);
        else
          atomicAdd(o.hist + cell, 1);
      }
    }
    __syncthreads();
  }
  if (y != nullptr) flush_counts(cl, noor, o);
  if constexpr (HM == kHistLds) flush_hist(ht, K, o.hist);
}

// ---------------------------------------------------------------------------
// Wide: one wavefront per CSR row (any length), 4 rows per workgroup pass.  After
// the wave reduction every lane holds the row's margins, so the epilogue needs no
// further exchange: lane 0 writes the row's scalars, lanes [0, C) its probabilities
// (the 4 rows of a workgroup pass are adjacent, their C floats contiguous).
//
// HIST (the score histogram): lane c < Ch also computes the log-odds of class c
// with a predicated sum over the other classes (binary: the margin itself) and
// counts it in a workgroup-private LDS table [Ch][2][512], flushed at the end.
template <int KP, bool HIST = false>
__global__ __launch_bounds__(256) void wide_score_kernel(int K, int64_t F, const int64_t* __restrict__ indptr,
                                                         const int32_t* __restrict__ idx,
                                                         const uint16_t* __restrict__ val,
                                                         const int32_t* __restrict__ y, int T,
                                                         const float* __restrict__ w, ScoreOut o) {
  __shared__ int cl[256];
  __shared__ int noor;
  extern __shared__ __attribute__((aligned(16))) int wide_ht[];  // [K][2][512] (HIST only)
  const int tid = threadIdx.x, lane = tid & 63;
  const bool binary = K == 1;
  const int C = binary ? 2 : K;
  cl[tid] = 0;
  if (tid == 0) noor = 0;
  if constexpr (HIST)
    for (int i = tid; i < K * kHistCells; i += 256) wide_ht[i] = 0;
  __syncthreads();
  for (int64_t r = (int64_t)blockIdx.x * 4 + (tid >> 6); r < T; r += (int64_t)gridDim.x * 4) {
    float z[KP];
    wide_row_margins<KP>(F, indptr, idx, val, r, w, z);
    const int best = wide_argmax<KP>(K, z);
    float m = -INFINITY, s = 0.f;
    if (!binary) {
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) m = fmaxf(m, z[k]);
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k < K) s += expf(z[k] - m);
    }
    if (o.proba != nullptr && lane < C) {
      float zl = 0.f;
#pragma unroll
      for (int k = 0; k < KP; ++k)
        if (k == lane) zl = z[k];
      o.proba[r * C + lane] = binary ? sigmoid_side(z[0], lane) : expf(zl - m) / s;
    }
    if constexpr (HIST) {
      if (lane < K) {
        const int yl = y[r];
        float zl = 0.f, so = 0.f;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
          if (k == lane) zl = z[k];
          if (k < K && k != lane) so += expf(z[k] - m);
        }
        const float l = binary ? z[0] : (zl - m) - logf(so);
        const int side = binary ? (yl > 0 ? 1 : 0) : (yl == lane ? 1 : 0);
        if (binary || (yl >= 0 && yl < K)) atomicAdd(&wide_ht[(lane * 2 + side) * kHistBins + hist_bin(l)], 1);
      }
    }
    if (lane == 0) {
      o.pred[r] = best;
      if (y != nullptr) {
        const int ylab = y[r];
        const bool in_range = binary || (ylab >= 0 && ylab < K);
        if (!in_range) atomicAdd(&noor, 1);
        if (o.nll != nullptr) {
          float v = __builtin_nanf("");
          if (binary) {
            v = binary_nll(z[0], ylab > 0);
          } else if (in_range) {
            float zy = 0.f;
#pragma unroll
            for (int k = 0; k < KP; ++k)
              if (k == ylab) zy = z[k];
            v = logf(s) - (zy - m);
          }
          o.nll[r] = v;
        }
        atomicAdd(&cl[clamp_label(ylab, binary) * 16 + best], 1);
      }
    }
  }
  __syncthreads();
  if (y != nullptr) flush_counts(cl, &noor, o);
  if constexpr (HIST) flush_hist(wide_ht, K, o.hist);
}

// ---------------------------------------------------------------------------
void prepare_score_kernels() {
  static bool done = false;
  if (done) return;
  constexpr hipFuncAttribute kDyn = hipFuncAttributeMaxDynamicSharedMemorySize;
  for_each_fp([&](auto fp) {
    const size_t tile = eval_lds_bytes(fp()), room = kLdsPerWorkgroup - tile;
    const size_t table = room < 16 * kHistCells * 4 ? room / (kHistCells * 4) * (kHistCells * 4) : 16 * kHistCells * 4;
    (void)hipFuncSetAttribute((const void*)score_kernel<fp()>, kDyn, (int)tile);
    (void)hipFuncSetAttribute((const void*)score_kernel<fp(), kHistGlobal>, kDyn, (int)tile);
    (void)hipFuncSetAttribute((const void*)score_kernel<fp(), kHistLds>, kDyn, (int)(tile + table));
  });
  for_each_wide_kp([&](auto kp) {  // 64 KB of table at K = 16, beside 1 KB of static LDS
    (void)hipFuncSetAttribute((const void*)wide_score_kernel<kp(), true>, kDyn, kp() * kHistCells * 4);
  });
  done = true;
}

int score_hist_form(int FP, int K) {
  return eval_lds_bytes(FP) + (size_t)K * kHistCells * 4 <= kLdsPerWorkgroup ? kHistLds : kHistGlobal;
}

bool launch_score(int FP, int K, const uint16_t* X, const int32_t* y, int T, const uint16_t* wf_hi,
                  const uint16_t* wf_lo, const float* b, const ScoreOut& o, hipStream_t s, int hist_form) {
  int hm = kHistOff;
  if (o.hist != nullptr && y != nullptr) {
    hm = hist_form ? hist_form : score_hist_form(FP, K);
    if (hm == kHistLds && score_hist_form(FP, K) != kHistLds) return false;
  }
  const size_t lds = eval_lds_bytes(FP) + (hm == kHistLds ? (size_t)K * kHistCells * 4 : 0);
  const int ntiles = (T + 31) / 32;
  const int grid = ntiles < 1024 ? ntiles : 1024;
  if (grid <= 0) return true;
  dispatch_fp("score: padded width", FP, [&](auto fp) {
    if (hm == kHistLds)
      score_kernel<fp(), kHistLds><<<grid, 256, lds, s>>>(K, X, y, T, wf_hi, wf_lo, b, o);
    else if (hm == kHistGlobal)
      score_kernel<fp(), kHistGlobal><<<grid, 256, lds, s>>>(K, X, y, T, wf_hi, wf_lo, b, o);
    else
      score_kernel<fp()><<<grid, 256, lds, s>>>(K, X, y, T, wf_hi, wf_lo, b, o);
  });
  return true;
}

void launch_wide_score(int K, int KP, int64_t F, const int64_t* indptr, const int32_t* idx, const uint16_t* val,
                       const int32_t* y, int T, const float* w, const ScoreOut& o, hipStream_t s) {
  if (T <= 0) return;
  const int nwg = (T + 3) / 4;  // 4 rows per workgroup pass
  const int grid = nwg < 1024 ? nwg : 1024;
  const bool hist = o.hist != nullptr && y != nullptr;
  dispatch_wide_kp("wide_score: padded classes", KP, [&](auto kp) {
    if (hist)
      wide_score_kernel<kp(), true><<<grid, 256, K * kHistCells * 4, s>>>(K, F, indptr, idx, val, y, T, w, o);
    else
      wide_score_kernel<kp()><<<grid, 256, 0, s>>>(K, F, indptr, idx, val, y, T, w, o);
  });
}

}  // namespace psx
