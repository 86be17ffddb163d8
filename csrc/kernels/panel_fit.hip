// Panel kernels (gfx950 / CDNA4): the full-batch fit and the scorer for dense bf16 rows
// wider than one LDS tile, 2,048 < F <= 16,384, padded to FP in {4096, 8192, 16384}.
//
// fit_lossgrad_kernel<FP> keeps a whole 32-row tile in LDS (128 KB at 2,048) and a
// workgroup's R^T X accumulators in registers (FP / 16 per thread): neither scales.
// Here the work is split over features as well as rows.  The rows are cut into panels
// of 1,024 columns; the grid of the heavy kernels is (G row blocks, live panels), row
// block g walking the 32-row tiles g, g + G, ... as the dense kernels do.  One
// evaluation is three streaming launches and READS THE ROWS TWICE (fusing the two
// passes needs hand-offs between the workgroups of one tile and is left out on purpose):
//
//   panel_fwd_kernel    workgroup (g, p) stages the 32 x 1,024 sub-tile of panel p (row
//                       stride FP, column offset p * 1,024; 16-B loads, the swizzled
//                       dual-use image of tile.h), holds the panel's trial-weight
//                       fragments (bf16 hi/lo, 16 classes x 1,024) in registers across
//                       its tiles, runs the v_mfma_f32_16x16x32_bf16 forward and stores
//                       the panel's partial logits in fp32: zpart[p][Npad][16], 64 B per
//                       row and panel, 3 % of the row bytes
//   panel_resid_kernel  8 threads per row: the partials summed in panel order, the
//                       intercept, softmax and cross entropy, the residual p - onehot
//                       (zero for rows >= N) split into bf16 hi/lo and written in the
//                       transposed per-tile image bwd_tile_acc reads, rt[tile][2][16][32];
//                       per workgroup the class residual sums and the loss -> part[g][32]
//   panel_bwd_kernel    workgroup (g, p) stages the same sub-tiles again beside the tile's
//                       rt image and accumulates R^T X of its 1,024 columns in registers
//                       (bwd_tile_acc<1024> of solve_body.h, unchanged); at the end it
//                       writes its slice gpart[g][K][p * 1,024 ...] of the [G][K][FP]
//                       partials
//
// fit_reduce / fit_dots / fit_begin / fit_update / fit_finalize of fit_kernels.hip then
// run UNCHANGED: they take FP at run time, fit_reduce masks with FP - 1 (FP stays a power
// of two), and write_frag's fragment order ((f >> 3) * 16 + c) * 8 + (f & 7) is
// chunk-major, so panel p's fragments are the contiguous words [p * 16 * 1,024,
// (p + 1) * 16 * 1,024) of whi / wlo: no panel-ordered copy of any of them is needed.
//
// A panel with no real feature (F = 2,049 in FP 4,096 has two) is never launched: its
// partial logits are not summed, its statistics are zero by rule and its slice of gpart
// keeps the zeros it was allocated with.
//
// Every sum runs in a fixed order (waves in order, panels in order, butterflies,
// workgroups in order in fit_reduce): a fit is bit-reproducible.  No float atomics;
// panel_score_kernel counts with integer atomics as score_kernel does.
// LDS per workgroup: eval_lds_bytes(1024), two workgroups per CU.
#include <hip/hip_runtime.h>

#include "lr_kernels.h"
#include "panel_fit.h"
#include "solve_body.h"
#include "tile.h"

namespace psx {

namespace {

constexpr int kImageBytes = 32 * kPanelCols * 2;  // the staged sub-tile; logits 8 KB and rt 2 KB follow it
static_assert(eval_lds_bytes(kPanelCols) >= (size_t)kImageBytes + 8192 + 2048, "panel tile body's LDS layout");
static_assert(kPartStride == 32, "fit_reduce / fit_dots index the residual partials with stride 32");

// Rows [row0, row0 + 32) x columns [col0, col0 + 1,024) of X (row stride FP) into the LDS
// image of tile.h: thread t takes 16-B chunk t & 127 of the rows t >> 7, + 2, ... (a wave
// reads 1 KB of one row), all 16 loads issued before the first LDS write.
__device__ __forceinline__ void stage_panel(char* lds, const uint16_t* __restrict__ X, int64_t row0, int FP,
                                            int col0) {
  const int cg = threadIdx.x & 127, rl = threadIdx.x >> 7;
  const uint16_t* src = X + (row0 + rl) * FP + col0 + cg * 8;
  u16x8 v[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = *(const u16x8*)(src + (int64_t)(2 * j) * FP);
  char* dst = lds + (cg >> 4) * 8192;
#pragma unroll
  for (int j = 0; j < 16; ++j) *(u16x8*)(dst + lds_off(rl + 2 * j, cg & 15)) = v[j];
}

// The margins of classes sc0, sc0 + 1 of `row`: the live panels' partials in panel order.
__device__ __forceinline__ void sum_panels(const FitDev& dv, const PanelDev& pd, int64_t row, int sc0, float& z0,
                                           float& z1) {
  const float* src = pd.zpart + row * 16 + sc0;
  const size_t stride = (size_t)dv.Npad * 16;
  z0 = z1 = 0.f;
#pragma unroll 4
  for (int p = 0; p < pd.PL; ++p) {
    const float2 v = *(const float2*)(src + p * stride);
    z0 += v.x;
    z1 += v.y;
  }
}

}  // namespace

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void panel_fwd_kernel(FitDev dv, PanelDev pd) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  char* red_base = lds + kImageBytes;
  const int g = blockIdx.x, G = gridDim.x, p = blockIdx.y;
  const int ntiles = dv.Npad >> 5, tid = threadIdx.x;
  const int sr = tid >> 3, sc0 = (tid & 7) * 2;
  WFrag<kPanelCols> wf;  // the panel's trial weights do not depend on the tile
  load_wfrag<kPanelCols>(wf, dv.whi + (size_t)p * kPanelFragWords, dv.wlo + (size_t)p * kPanelFragWords, dv.K);
  float* zp = pd.zpart + (size_t)p * dv.Npad * 16;
  for (int tile = g; tile < ntiles; tile += G) {
    const int64_t row0 = (int64_t)tile * 32;
    stage_panel(lds, dv.X, row0, dv.FP, p * kPanelCols);
    __syncthreads();
    f32x4 a0, a1;
    forward_tile_pre<kPanelCols>(lds, wf, a0, a1);
    store_partial_logits(red_base, a0, a1);
    __syncthreads();  // (also: every wave is done with the image before the next tile's staging)
    // the four waves' K-slices in wave order; the tile's [32][16] block is one 2 KB run
    const float2 z{load_logit(red_base, sr, sc0), load_logit(red_base, sr, sc0 + 1)};
    *(float2*)(zp + (row0 + sr) * 16 + sc0) = z;
  }
}

// ---------------------------------------------------------------------------
// The softmax epilogue of fit_lossgrad_w_kernel on the summed partials, G workgroups.
__global__ __launch_bounds__(256) void panel_resid_kernel(FitDev dv, PanelDev pd) {
  __shared__ __attribute__((aligned(16))) unsigned short rt[1024];  // [2][16][32]
  __shared__ float rsum[64];                                        // [4 waves][16]
  __shared__ float lred[4];
  const int g = blockIdx.x, G = gridDim.x, K = dv.K, N = dv.N;
  const int ntiles = dv.Npad >> 5;
  if (g >= ntiles) return;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sr = tid >> 3, sc0 = (tid & 7) * 2;
  const bool v0 = sc0 < K, v1 = sc0 + 1 < K;
  const float bz0 = dv.b_eff[sc0], bz1 = dv.b_eff[sc0 + 1];
  float loss = 0.f, rs0 = 0.f, rs1 = 0.f;
  for (int tile = g; tile < ntiles; tile += G) {
    const int64_t row = (int64_t)tile * 32 + sr;
    const int yl = dv.y[row];
    float z0, z1;
    sum_panels(dv, pd, row, sc0, z0, z1);
    z0 = v0 ? z0 + bz0 : -INFINITY;
    z1 = v1 ? z1 + bz1 : -INFINITY;
    float mx = fmaxf(z0, z1);
    mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
    const float e0 = v0 ? __expf(z0 - mx) : 0.f, e1 = v1 ? __expf(z1 - mx) : 0.f;
    float se = e0 + e1;
    se += __shfl_xor(se, 1, 64);
    se += __shfl_xor(se, 2, 64);
    se += __shfl_xor(se, 4, 64);
    const bool valid = row < N;
    const float inv = 1.f / se;
    const float r0 = valid && v0 ? e0 * inv - (yl == sc0 ? 1.f : 0.f) : 0.f;
    const float r1 = valid && v1 ? e1 * inv - (yl == sc0 + 1 ? 1.f : 0.f) : 0.f;
    if (valid) {
      const float lse = mx + __logf(se);
      if (yl == sc0) loss += lse - z0;
      if (yl == sc0 + 1) loss += lse - z1;
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
    __syncthreads();
    if (tid < 128) *(u16x8*)(pd.rt + (size_t)tile * 1024 + tid * 8) = *(const u16x8*)(rt + tid * 8);
    __syncthreads();  // the next tile overwrites rt
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
  if (lane == 0) lred[w] = loss;
  __syncthreads();
  float pv = 0.f;
  if (tid < 16) pv = ((rsum[tid] + rsum[16 + tid]) + rsum[32 + tid]) + rsum[48 + tid];
  if (tid == 16) pv = lred[0] + lred[1] + lred[2] + lred[3];
  if (tid < 17) dv.part[(size_t)g * kPartStride + tid] = pv;
}

// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void panel_bwd_kernel(FitDev dv, PanelDev pd) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  unsigned short* rt = (unsigned short*)(lds + kImageBytes + 8192);  // [2][16][32]
  constexpr int NT = kPanelCols / 64;
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0, 0, 0, 0};
  const int g = blockIdx.x, G = gridDim.x, p = blockIdx.y, K = dv.K, FP = dv.FP;
  const int ntiles = dv.Npad >> 5, tid = threadIdx.x;
  if (g >= ntiles) return;  // no tile: no partial (the reduction sums min(G, tiles) of them)
  for (int tile = g; tile < ntiles; tile += G) {
    u16x8 rv = u16x8{0, 0, 0, 0, 0, 0, 0, 0};  // the tile's residual image travels with its row loads
    if (tid < 128) rv = *(const u16x8*)(pd.rt + (size_t)tile * 1024 + tid * 8);
    stage_panel(lds, dv.X, (int64_t)tile * 32, FP, p * kPanelCols);
    if (tid < 128) *(u16x8*)(rt + tid * 8) = rv;
    __syncthreads();
    bwd_tile_acc<kPanelCols>(lds, rt, acc);
    __syncthreads();  // the next tile's staging overwrites the image and rt
  }
  const int lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int f = p * kPanelCols + (w * NT + n) * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (lane >> 4) * 4 + i;
      if (c < K) dv.gpart[((size_t)g * K + c) * FP + f] = acc[n][i];
    }
  }
}

// ---------------------------------------------------------------------------
// Column sums and sums of squares as fit_stats_kernel forms them: per tile in fp32 (16
// rows of bf16 values per thread), across tiles in fp64; one partial per row block.
// Thread t: 16-B chunk t & 127 of panel p, rows t >> 7, + 2, ... of every tile.
__global__ __launch_bounds__(256) void panel_stats_kernel(FitDev dv) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* red = (double*)smem;  // [2 row lanes][128 chunks][16]
  const int t = threadIdx.x, ch = t & 127, rl = t >> 7, p = blockIdx.y, FP = dv.FP;
  const int ntiles = dv.Npad >> 5;
  const uint16_t* src = dv.X + p * kPanelCols + ch * 8;
  double s[8], q[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.0;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * 32 + rl;
    float fs[8], fq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) fs[e] = fq[e] = 0.f;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // two batches of 8 loads in flight
      u16x8 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = *(const u16x8*)(src + (row0 + 2 * (8 * h + j)) * FP);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = row0 + 2 * (8 * h + j) < dv.N;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float x = in ? bf2f(v[j][e]) : 0.f;
          fs[e] += x;
          fq[e] += x * x;
        }
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
    red[(rl * 128 + ch) * 16 + e] = s[e];
    red[(rl * 128 + ch) * 16 + 8 + e] = q[e];
  }
  __syncthreads();
  for (int k = t; k < 128 * 16; k += 256) {  // k = chunk * 16 + {sum e | square e}
    const double a = red[k] + red[128 * 16 + k];
    const int c = k >> 4, e = k & 15, f = p * kPanelCols + c * 8 + (e & 7);
    dv.spart[((size_t)blockIdx.x * 2 + (e >> 3)) * FP + f] = a;
  }
}
constexpr size_t kPanelStatsLds = (size_t)2 * 128 * 16 * sizeof(double);

// fit_stats_fin_kernel's sigma rules (sample std, n - 1, from the G partials in row-block
// order; 0 for a constant feature); the padding features, whose panels may never have
// been visited, read no partial.
__global__ __launch_bounds__(256) void panel_stats_fin_kernel(FitDev dv, int G) {
  const int f = blockIdx.x * 256 + threadIdx.x, FP = dv.FP;
  if (f >= FP) return;
  const double n = (double)dv.N;
  double sd = 0.0;
  if (f < dv.F && n > 1.0) {
    double a = 0.0, b = 0.0;
    for (int g = 0; g < G; ++g) {
      a += dv.spart[((size_t)g * 2) * FP + f];
      b += dv.spart[((size_t)g * 2 + 1) * FP + f];
    }
    const double mean = a / n;
    const double var = (b - n * mean * mean) / (n - 1.0);
    sd = var > 0.0 ? sqrt(var) : 0.0;
  }
  dv.std_[f] = (float)sd;
  dv.inv_std[f] = sd > 0.0 ? (float)(1.0 / sd) : 0.f;
}

// ---------------------------------------------------------------------------
// After panel_fwd_kernel on the final weights: score_kernel's row outputs from the summed
// partials, 8 threads per row.  Argmax with strict >, the lowest class winning a tie and a
// NaN margin never winning; labels clamped to [0, 15] for the confusion cell; a label
// outside [0, K) gives a NaN loss and is counted in *oor.  Integer atomics only.
__global__ __launch_bounds__(256) void panel_score_kernel(FitDev dv, PanelDev pd, ScoreOut o) {
  __shared__ int cl[256];  // [16][16]
  __shared__ int noor;
  const int tid = threadIdx.x, K = dv.K, N = dv.N;
  const int sr = tid >> 3, sc0 = (tid & 7) * 2;
  const bool v0 = sc0 < K, v1 = sc0 + 1 < K;
  const float bz0 = dv.b_eff[sc0], bz1 = dv.b_eff[sc0 + 1];
  cl[tid] = 0;
  if (tid == 0) noor = 0;
  __syncthreads();
  const int ntiles = (N + 31) >> 5;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row = (int64_t)tile * 32 + sr;  // < Npad: readable; only rows < N are written
    const bool valid = row < N;
    const int yl = dv.y[row];
    float z0, z1;
    sum_panels(dv, pd, row, sc0, z0, z1);
    z0 += bz0;
    z1 += bz1;
    float bv = v0 && z0 == z0 ? z0 : -INFINITY;
    int bi = sc0;
    if (v1 && z1 > bv) {
      bv = z1;
      bi = sc0 + 1;
    }
#pragma unroll
    for (int x = 1; x < 8; x <<= 1) {
      const float ov = __shfl_xor(bv, x, 64);
      const int oi = __shfl_xor(bi, x, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    const float e0 = v0 ? expf(z0 - bv) : 0.f, e1 = v1 ? expf(z1 - bv) : 0.f;
    float se = e0 + e1;
    se += __shfl_xor(se, 1, 64);
    se += __shfl_xor(se, 2, 64);
    se += __shfl_xor(se, 4, 64);
    float zy = yl == sc0 ? z0 : (yl == sc0 + 1 ? z1 : 0.f);  // one lane of the row holds the label's margin
    zy += __shfl_xor(zy, 1, 64);
    zy += __shfl_xor(zy, 2, 64);
    zy += __shfl_xor(zy, 4, 64);
    if (!valid) continue;
    if (o.proba != nullptr) {
      if (v0) o.proba[row * K + sc0] = e0 / se;
      if (v1) o.proba[row * K + sc0 + 1] = e1 / se;
    }
    if ((tid & 7) == 0) {
      o.pred[row] = bi;
      const bool in_range = yl >= 0 && yl < K;
      if (!in_range) atomicAdd(&noor, 1);
      if (o.nll != nullptr) o.nll[row] = in_range ? logf(se) - (zy - bv) : __builtin_nanf("");
      const int yc = yl < 0 ? 0 : (yl > 15 ? 15 : yl);
      atomicAdd(&cl[yc * 16 + bi], 1);
    }
  }
  __syncthreads();
  const int v = cl[tid];
  if (v) atomicAdd(o.conf + tid, v);
  if (tid == 0 && noor) atomicAdd(o.oor, noor);
}

// ---------------------------------------------------------------------------
void prepare_panel_kernels() {
  static bool done = false;
  if (done) return;
  constexpr hipFuncAttribute kDyn = hipFuncAttributeMaxDynamicSharedMemorySize;
  (void)hipFuncSetAttribute((const void*)panel_fwd_kernel, kDyn, (int)eval_lds_bytes(kPanelCols));
  (void)hipFuncSetAttribute((const void*)panel_bwd_kernel, kDyn, (int)eval_lds_bytes(kPanelCols));
  done = true;
}

void launch_panel_stats(const FitDev& dv, const PanelDev& pd, int G, hipStream_t s) {
  panel_stats_kernel<<<dim3(G, pd.PL), 256, kPanelStatsLds, s>>>(dv);
  panel_stats_fin_kernel<<<(dv.FP + 255) / 256, 256, 0, s>>>(dv, G);
}

void launch_panel_step(const FitDev& dv, const PanelDev& pd, int G, int step, hipStream_t s) {
  const size_t lb = eval_lds_bytes(kPanelCols);
  if (step == 0) panel_fwd_kernel<<<dim3(G, pd.PL), 256, lb, s>>>(dv, pd);
  if (step == 1) panel_resid_kernel<<<G, 256, 0, s>>>(dv, pd);
  if (step == 2) panel_bwd_kernel<<<dim3(G, pd.PL), 256, lb, s>>>(dv, pd);
}

void launch_panel_lossgrad(const FitDev& dv, const PanelDev& pd, int G, hipStream_t s) {
  for (int step = 0; step < 3; ++step) launch_panel_step(dv, pd, G, step, s);
}

void launch_panel_score(const FitDev& dv, const PanelDev& pd, int G, const ScoreOut& o, hipStream_t s) {
  launch_panel_step(dv, pd, G, 0, s);
  const int ntiles = (dv.N + 31) >> 5;
  panel_score_kernel<<<ntiles < 1024 ? ntiles : 1024, 256, 0, s>>>(dv, pd, o);
}

}  // namespace psx
