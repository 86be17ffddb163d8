// fp32-row kernels (gfx950 / CDNA4): the full-batch fit and the scorer for dense rows kept
// in fp32, float [Npad][FP], FP in {128, 256, 512, 1024}.
//
// The bf16 family rounds a row value to 8 significant bits when it is loaded.  The fit
// standardises by sigma without centring, so a column whose variation is small next to its
// magnitude (100 +- 1) loses its information there.  Here a 32-row tile is read ONCE as fp32
// and staged as TWO bf16 images in LDS, hi = bf16(x) and lo = bf16(x - hi) (stage_tile_f32 of
// tile.h; x = hi + lo to 2^-18 relative), both in the swizzled dual-use layout, and every
// product runs on v_mfma_f32_16x16x32_bf16 against operands that are split the same way:
//
//   forward   Z = x_hi (W_hi + W_lo) + x_lo W_hi           3 MFMAs per k-step and row half
//   backward  G += (R_hi + R_lo)^T x_hi + R_hi^T x_lo      3 MFMAs per 16-feature N-tile
//
// (the dropped lo x lo products are below the split's own 2^-18).  7/4 of the bf16 body's
// MFMAs for twice its row bytes.
//
//   fit_lossgrad_f32_kernel<FP>  G workgroups walk the 32-row tiles g, g + G, ...  The trial
//                       weights' fragments are fetched into registers once per workgroup,
//                       before the first staging.  Per tile: one read of the rows into the
//                       two images (the labels travel with the loads), the forward on both,
//                       the 8-threads-per-row softmax / cross entropy, the residual split
//                       into rt[2][16][32], the backward on both images into FP / 64
//                       accumulators per thread.  At the end part[g][0..16] and the
//                       gpart[g][K][FP] slice, the layout launch_fit_reduce reads.
//   fit_stats_f32_kernel<FP> + fit_stats_f32_fin_kernel   column sums, sums of squares,
//                       minimum and maximum in one pass, every element widened to double
//                       BEFORE it enters a sum (an fp32 sum of 16 values at 1000 rounds by
//                       as much as a variance of 1), and "constant" decided on max > min,
//                       not on the sign of a cancelled difference.
//   score_f32_kernel<FP>  the same staging and forward, then the row outputs of
//                       score_kernels.h (argmax with strict >, lowest class on a tie, NaN
//                       never winning; labels clamped for the confusion cell; NaN loss and
//                       *oor for a label outside [0, K)); integer atomics only.
//
//   <FP, true>          the centred instantiations of the two kernels above: the same bodies
//                       over stage_tile_f32c, which subtracts the column's centre c_f in fp32
//                       before the split.  A column at 100 +- 1 then spends the 16 bits of
//                       hi + lo on its variation, and the optimiser sees a problem whose
//                       conditioning does not grow with (mean / sigma)^2.  The statistics
//                       pass writes c; three one-line fp64 vector kernels map the intercepts
//                       (b' = b + sum_f c_f w_f) and the gradient between the coordinates.
//
// LDS per workgroup: fit_f32_lds_bytes(FP) = two images + the 11.75 KB tail: 142,848 B at
// 1,024 (one workgroup per CU), 77,312 at 512 (two), 44,544 at 256, 28,160 at 128.
// Every sum runs in a fixed order (waves in order, butterflies, workgroups in order in
// fit_reduce): a fit is bit-reproducible.
#include <hip/hip_runtime.h>

#include "dispatch.h"
#include "fit_f32.h"
#include "solve_body.h"
#include "tile.h"

namespace psx {

namespace {

static_assert(kPartStride == 32, "fit_reduce / fit_dots index the residual partials with stride 32");

template <class F>
void dispatch_f32_fp(int fp, F&& f) {
  dispatch_int<128, 256, 512, 1024>("fp32 rows: padded width", fp, std::forward<F>(f));
}

// The workgroup's LDS: [hi image][lo image][logits 8 KB][rt 2 KB][labels][rsum][lred]
template <int FP>
struct F32Lds {
  static constexpr int kImage = 32 * FP * 2;
  char *hi, *lo, *red;
  unsigned short* rt;  // [2][16][32]
  int* ylab;           // [32]
  float* rsum;         // [4 waves][16]
  float* lred;         // [4]
  __device__ __forceinline__ explicit F32Lds(char* lds)
      : hi(lds), lo(lds + kImage), red(lds + 2 * kImage), rt((unsigned short*)(red + 8192)),
        ylab((int*)(red + 8192 + 2048)), rsum((float*)(ylab + 32)), lred(rsum + 64) {}
};
static_assert(8192 + 2048 + (32 + 64 + 4) * 4 <= 8192 + 2048 + 1024 + 512, "the tail of eval_lds_bytes");

// Centred mode.  stage_tile_f32 (tile.h) with x - c_f formed in fp32 before the split, so the
// 16 bits of hi + lo are spent on the column's variation and not on its magnitude.  Thread t
// stages the chunks q = t + 256 j and 256 is a multiple of CPR = FP / 8, so its column group
// q % CPR = t % CPR is the same for every chunk of every tile: it needs 8 centre values, ever.
// A padding row (zeros) stages as -c; its residual is 0 and its outputs are never written.
template <int FP>
__device__ __forceinline__ void stage_tile_f32c(char* lds_hi, char* lds_lo, const float* __restrict__ X, int64_t row0,
                                                const f32x4 c0, const f32x4 c1) {
  constexpr int CPR = FP / 8;            // 8-feature chunks per row
  constexpr int PER_T = 32 * CPR / 256;  // chunks per thread
  constexpr int BATCH = PER_T < 8 ? PER_T : 8;
  static_assert(256 % CPR == 0, "a thread's column group does not depend on the chunk");
  const int cg = threadIdx.x % CPR, rbase = threadIdx.x / CPR;
#pragma unroll
  for (int b0 = 0; b0 < PER_T; b0 += BATCH) {
    f32x4 v[BATCH][2];
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int row = rbase + (256 / CPR) * (b0 + j);
      const float* src = X + (row0 + row) * FP + cg * 8;
      v[j][0] = *(const f32x4*)src;
      v[j][1] = *(const f32x4*)(src + 4);
    }
#pragma unroll
    for (int j = 0; j < BATCH; ++j) {
      const int row = rbase + (256 / CPR) * (b0 + j);
      u16x8 h, l;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        unsigned short hh, ll;
        split_bf16(v[j][e >> 2][e & 3] - (e < 4 ? c0[e & 3] : c1[e & 3]), hh, ll);
        h[e] = hh;
        l[e] = ll;
      }
      const int o = (cg >> 4) * 8192 + lds_off(row, cg & 15);
      *(u16x8*)(lds_hi + o) = h;
      *(u16x8*)(lds_lo + o) = l;
    }
  }
}

// The staging thread's 8 centre values: fetched once per workgroup, beside the weight
// fragments, and held in registers at every width (0 B of scratch, profiles/r24/README.md).
template <int FP, bool kCenter>
struct Center {
  __device__ __forceinline__ explicit Center(const float*) {}
};
template <int FP>
struct Center<FP, true> {
  f32x4 c0, c1;
  __device__ __forceinline__ explicit Center(const float* __restrict__ c) {
    const float* src = c + (threadIdx.x % (FP / 8)) * 8;
    c0 = *(const f32x4*)src;
    c1 = *(const f32x4*)(src + 4);
  }
};

// One read of the tile's fp32 rows into the two images and both forwards; the partial
// logits of the four waves are in L.red after the barrier.
template <int FP, bool kCenter>
__device__ __forceinline__ void stage_and_forward(const F32Lds<FP>& L, const float* __restrict__ X,
                                                  const int32_t* __restrict__ y, int64_t row0, const WFrag<FP>& wf,
                                                  const Center<FP, kCenter>& cen) {
  const int tid = threadIdx.x;
  const int yv = tid < 32 ? y[row0 + tid] : 0;  // issued with the tile's loads (one round trip)
  if constexpr (kCenter) {
    stage_tile_f32c<FP>(L.hi, L.lo, X, row0, cen.c0, cen.c1);
  } else {
    stage_tile_f32<FP>(L.hi, L.lo, X, row0);
  }
  if (tid < 32) L.ylab[tid] = yv;
  __syncthreads();
  f32x4 a0, a1;
  forward_tile_pre<FP>(L.hi, wf, a0, a1);     // x_hi (W_hi + W_lo)
  forward_tile_pre_lo<FP>(L.lo, wf, a0, a1);  // + x_lo W_hi
  store_partial_logits(L.red, a0, a1);
  __syncthreads();
}

}  // namespace

// ---------------------------------------------------------------------------
template <int FP, bool kCenter = false>
__global__ __launch_bounds__(256) void fit_lossgrad_f32_kernel(FitDev dv, F32Dev fd) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const F32Lds<FP> L(lds);
  constexpr int NT = FP / 64;
  const int g = blockIdx.x, G = gridDim.x, K = dv.K, N = dv.N;
  const int ntiles = dv.Npad >> 5;
  if (g >= ntiles) return;  // no tile: no partial (the reduction sums min(G, tiles) of them)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int sr = tid >> 3, sc0 = (tid & 7) * 2;
  const bool v0 = sc0 < K, v1 = sc0 + 1 < K;
  WFrag<FP> wf;  // the trial weights do not depend on the tile: their latency overlaps the first staging
  load_wfrag<FP>(wf, dv.whi, dv.wlo, K);
  const Center<FP, kCenter> cen(fd.center);
  const float bz0 = dv.b_eff[sc0], bz1 = dv.b_eff[sc0 + 1];
  f32x4 acc[NT];
#pragma unroll
  for (int n = 0; n < NT; ++n) acc[n] = f32x4{0, 0, 0, 0};
  float loss = 0.f, rs0 = 0.f, rs1 = 0.f;
  for (int tile = g; tile < ntiles; tile += G) {
    const int64_t row0 = (int64_t)tile * 32;
    stage_and_forward<FP, kCenter>(L, fd.X, dv.y, row0, wf, cen);
    {  // softmax + cross entropy: 8 threads per row, 2 classes each
      const float z0 = v0 ? load_logit(L.red, sr, sc0) + bz0 : -INFINITY;
      const float z1 = v1 ? load_logit(L.red, sr, sc0 + 1) + bz1 : -INFINITY;
      float mx = fmaxf(z0, z1);
      mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 4, 64));
      const float e0 = v0 ? __expf(z0 - mx) : 0.f, e1 = v1 ? __expf(z1 - mx) : 0.f;
      float se = e0 + e1;
      se += __shfl_xor(se, 1, 64);
      se += __shfl_xor(se, 2, 64);
      se += __shfl_xor(se, 4, 64);
      const bool valid = row0 + sr < N;
      const int yl = L.ylab[sr];
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
      unsigned short h, l;
      split_bf16(r0, h, l);
      L.rt[sc0 * 32 + sr] = h;
      L.rt[512 + sc0 * 32 + sr] = l;
      split_bf16(r1, h, l);
      L.rt[(sc0 + 1) * 32 + sr] = h;
      L.rt[512 + (sc0 + 1) * 32 + sr] = l;
    }
    __syncthreads();
    bwd_tile_acc<FP>(L.hi, L.rt, acc);        // (R_hi + R_lo)^T x_hi
    bwd_tile_acc<FP, true>(L.lo, L.rt, acc);  // + R_hi^T x_lo
    __syncthreads();                          // the next tile's staging overwrites the images and rt
  }
  // fixed order: a butterfly over the lanes of one class pair, then the waves in order
#pragma unroll
  for (int o = 8; o < 64; o <<= 1) {
    rs0 += __shfl_xor(rs0, o, 64);
    rs1 += __shfl_xor(rs1, o, 64);
  }
  if (lane < 8) {
    L.rsum[w * 16 + sc0] = rs0;
    L.rsum[w * 16 + sc0 + 1] = rs1;
  }
  loss = wave_sum(loss);
  if (lane == 0) L.lred[w] = loss;
  __syncthreads();
  float pv = 0.f;
  if (tid < 16) pv = ((L.rsum[tid] + L.rsum[16 + tid]) + L.rsum[32 + tid]) + L.rsum[48 + tid];
  if (tid == 16) pv = L.lred[0] + L.lred[1] + L.lred[2] + L.lred[3];
  if (tid < 17) dv.part[(size_t)g * kPartStride + tid] = pv;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    const int f = (w * NT + n) * 16 + (lane & 15);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = (lane >> 4) * 4 + i;
      if (c < K) dv.gpart[((size_t)g * K + c) * FP + f] = acc[n][i];
    }
  }
}

// ---------------------------------------------------------------------------
// Column statistics.  Thread t: 16-B chunk t % C (4 floats) of the rows t / C, + L, ... of
// every tile of its workgroup, as fit_stats_kernel splits them; each element becomes a
// double before it is added or squared (the square of an fp32 value is exact in fp64).
// Per workgroup the row lanes are combined in order through LDS.
template <int FP>
__global__ __launch_bounds__(256) void fit_stats_f32_kernel(FitDev dv, F32Dev fd) {
  constexpr int C = FP / 4;   // 16-B chunks per row
  constexpr int L = 256 / C;  // row lanes
  static_assert(C * L == 256, "FP in {128..1024}");
  constexpr int RPL = 32 / L;              // rows of a tile per lane
  constexpr int B = RPL < 8 ? RPL : 8;     // loads in flight
  __shared__ double red[256 * 8];          // [L][C][sum 4 | square 4]
  __shared__ float mm[256 * 8];            // [L][C][min 4 | max 4]
  const int t = threadIdx.x, ch = t % C, rl = t / C;
  const int ntiles = dv.Npad >> 5, N = dv.N;
  double s[4], q[4];
  float mn[4], mx[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    s[e] = q[e] = 0.0;
    mn[e] = INFINITY;
    mx[e] = -INFINITY;
  }
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * 32 + rl;
#pragma unroll
    for (int j0 = 0; j0 < RPL; j0 += B) {
      f32x4 v[B];
#pragma unroll
      for (int j = 0; j < B; ++j) v[j] = *(const f32x4*)(fd.X + (row0 + (int64_t)L * (j0 + j)) * FP + ch * 4);
#pragma unroll
      for (int j = 0; j < B; ++j) {
        if (row0 + L * (j0 + j) >= N) continue;  // padding rows enter neither the sums nor min / max
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float xf = v[j][e];
          const double x = (double)xf;
          s[e] += x;
          q[e] += x * x;
          mn[e] = fminf(mn[e], xf);
          mx[e] = fmaxf(mx[e], xf);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    red[t * 8 + e] = s[e];  // t = rl * C + ch
    red[t * 8 + 4 + e] = q[e];
    mm[t * 8 + e] = mn[e];
    mm[t * 8 + 4 + e] = mx[e];
  }
  __syncthreads();
  for (int k = t; k < C * 8; k += 256) {  // k = chunk * 8 + {sum e | square e}
    const int j = k & 7, f = (k >> 3) * 4 + (j & 3);
    double a = 0.0;
    float m = j < 4 ? INFINITY : -INFINITY;
    for (int r = 0; r < L; ++r) {  // row lanes in order
      a += red[r * C * 8 + k];
      const float o = mm[r * C * 8 + k];
      m = j < 4 ? fminf(m, o) : fmaxf(m, o);
    }
    const size_t at = ((size_t)blockIdx.x * 2 + (j >> 2)) * FP + f;
    dv.spart[at] = a;
    fd.mmpart[at] = m;
  }
}

// fit_stats_fin_kernel's rule (sample std, n - 1, padding features 0) on the G partials in
// workgroup order; sigma is 0 exactly when the column's maximum equals its minimum.
__global__ __launch_bounds__(256) void fit_stats_f32_fin_kernel(FitDev dv, F32Dev fd, int G) {
  const int f = blockIdx.x * 256 + threadIdx.x, FP = dv.FP;
  if (f >= FP) return;
  double a = 0.0, b = 0.0;
  float mn = INFINITY, mx = -INFINITY;
  for (int g = 0; g < G; ++g) {
    a += dv.spart[((size_t)g * 2) * FP + f];
    b += dv.spart[((size_t)g * 2 + 1) * FP + f];
    mn = fminf(mn, fd.mmpart[((size_t)g * 2) * FP + f]);
    mx = fmaxf(mx, fd.mmpart[((size_t)g * 2 + 1) * FP + f]);
  }
  const double n = (double)dv.N;
  double sd = 0.0;
  if (f < dv.F && n > 1.0 && mx > mn) {
    const double mean = a / n;
    const double var = (b - n * mean * mean) / (n - 1.0);
    sd = var > 0.0 ? sqrt(var) : 0.0;
  }
  dv.std_[f] = (float)sd;
  dv.inv_std[f] = sd > 0.0 ? (float)(1.0 / sd) : 0.f;
  // the centre: the mean; a constant column's own value, so that it stages to exactly 0 (one
  // row makes every column constant); 0 for padding features
  fd.center[f] = f < dv.F ? (mx > mn ? (float)(a / n) : mn) : 0.f;
}

// ---------------------------------------------------------------------------
// The centred mode's vector kernels.  Centring by any constant c is a reparametrisation,
// z = (x - c) w + b' with b' = b + sum_f c_f w_f: the optimiser runs in (beta, b') and these
// map the intercepts and the gradient between the two.  One workgroup, fp64, and a fixed
// order: thread t sums the features t, t + 256, ... in order, then a tree over the threads.
__device__ __forceinline__ double center_block_sum(double v, double* red) {
  const int t = threadIdx.x;
  __syncthreads();  // the previous sum's readers are done
  red[t] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  return red[0];
}

// w_eff is the raw coefficient fit_begin_kernel / fit_write_trial wrote the fragments from.
__global__ __launch_bounds__(256) void fit_center_begin_kernel(FitDev dv, F32Dev fd, const float* w0, int raw) {
  __shared__ double red[256];
  const int t = threadIdx.x, FP = dv.FP, KF = dv.K * dv.FP;
  for (int k = 0; k < dv.K; ++k) {
    double a = 0.0;
    for (int f = t; f < dv.F; f += 256) {
      const int e = k * FP + f;
      float we;
      if (raw) {
        we = w0 ? w0[e] : 0.f;
      } else {
        const float iv = dv.inv_std[f];
        we = iv > 0.f ? dv.x[e] * iv : dv.wfix[e];
      }
      a += (double)fd.center[f] * (double)we;
    }
    a = center_block_sum(a, red);
    if (t == 0) {
      const float bp = (float)((double)(raw ? (w0 ? w0[KF + k] : 0.f) : dv.x[KF + k]) + a);
      dv.b_eff[k] = bp;
      if (!raw) {
        dv.x[KF + k] = bp;
        dv.beta_t[KF + k] = bp;
      }
    }
  }
}

__global__ __launch_bounds__(256) void fit_center_finalize_kernel(FitDev dv, F32Dev fd, float* __restrict__ w_out) {
  __shared__ double red[256];
  __shared__ double b[16];
  const int t = threadIdx.x, FP = dv.FP, K = dv.K, KF = dv.K * dv.FP;
  for (int k = 0; k < K; ++k) {
    double a = 0.0;  // over the fp32 coefficients as exported: their rounding is compensated, not doubled
    for (int f = t; f < dv.F; f += 256) a += (double)fd.center[f] * (double)w_out[k * FP + f];
    a = center_block_sum(a, red);
    if (t == 0) b[k] = (double)dv.x[KF + k] - a;
  }
  if (t == 0) {
    double bm = 0.0;
    for (int k = 0; k < K; ++k) bm += b[k];
    bm /= (double)K;
    for (int k = 0; k < K; ++k) w_out[KF + k] = (float)(b[k] - bm);
  }
}

__global__ __launch_bounds__(256) void fit_center_grad_kernel(FitDev dv, F32Dev fd, float* __restrict__ grad) {
  const int e = blockIdx.x * 256 + threadIdx.x, FP = dv.FP, KF = dv.K * dv.FP;
  if (e >= dv.n) return;
  float g = dv.g_t[e];
  if (e < KF) {
    const int k = e / FP, f = e - k * FP;
    g = (float)((double)g + (double)fd.center[f] * (double)dv.g_t[KF + k]);
  }
  grad[e] = g;
}

// ---------------------------------------------------------------------------
// Rows < N only are written; a row's outputs come from its own MFMA rows and its own 8
// threads, so they do not depend on the rows beside it.
template <int FP, bool kCenter = false>
__global__ __launch_bounds__(256) void score_f32_kernel(FitDev dv, F32Dev fd, ScoreOut o) {
  extern __shared__ __attribute__((aligned(16))) char lds[];
  const F32Lds<FP> L(lds);
  __shared__ int cl[256];  // [16][16]
  __shared__ int noor;
  const int tid = threadIdx.x, K = dv.K, N = dv.N;
  const int sr = tid >> 3, sc0 = (tid & 7) * 2;
  const bool v0 = sc0 < K, v1 = sc0 + 1 < K;
  cl[tid] = 0;
  if (tid == 0) noor = 0;  // (published by the barriers of the first tile)
  WFrag<FP> wf;
  load_wfrag<FP>(wf, dv.whi, dv.wlo, K);
  const Center<FP, kCenter> cen(fd.center);
  const float bz0 = dv.b_eff[sc0], bz1 = dv.b_eff[sc0 + 1];
  const int ntiles = (N + 31) >> 5;  // <= Npad / 32: every staged row is readable
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row0 = (int64_t)tile * 32, row = row0 + sr;
    stage_and_forward<FP, kCenter>(L, fd.X, dv.y, row0, wf, cen);
    const int yl = L.ylab[sr];
    const float z0 = load_logit(L.red, sr, sc0) + bz0, z1 = load_logit(L.red, sr, sc0 + 1) + bz1;
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
    if (row < N) {
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
    __syncthreads();  // the next tile's staging overwrites the logits and the labels
  }
  __syncthreads();
  const int v = cl[tid];
  if (v) atomicAdd(o.conf + tid, v);
  if (tid == 0 && noor) atomicAdd(o.oor, noor);
}

// ---------------------------------------------------------------------------
void prepare_fit_f32_kernels() {
  static bool done = false;
  if (done) return;
  constexpr hipFuncAttribute kDyn = hipFuncAttributeMaxDynamicSharedMemorySize;
  for_each_int<128, 256, 512, 1024>([&](auto fp) {
    (void)hipFuncSetAttribute((const void*)fit_lossgrad_f32_kernel<fp()>, kDyn, (int)fit_f32_lds_bytes(fp()));
    (void)hipFuncSetAttribute((const void*)score_f32_kernel<fp()>, kDyn, (int)fit_f32_lds_bytes(fp()));
    (void)hipFuncSetAttribute((const void*)fit_lossgrad_f32_kernel<fp(), true>, kDyn, (int)fit_f32_lds_bytes(fp()));
    (void)hipFuncSetAttribute((const void*)score_f32_kernel<fp(), true>, kDyn, (int)fit_f32_lds_bytes(fp()));
  });
  done = true;
}

void launch_fit_stats_f32(const FitDev& dv, const F32Dev& fd, int G, hipStream_t s) {
  dispatch_f32_fp(dv.FP, [&](auto fp) { fit_stats_f32_kernel<fp()><<<G, 256, 0, s>>>(dv, fd); });
  fit_stats_f32_fin_kernel<<<(dv.FP + 255) / 256, 256, 0, s>>>(dv, fd, G);
}

void launch_fit_lossgrad_f32(const FitDev& dv, const F32Dev& fd, int G, bool centred, hipStream_t s) {
  dispatch_f32_fp(dv.FP, [&](auto fp) {
    if (centred)
      fit_lossgrad_f32_kernel<fp(), true><<<G, 256, fit_f32_lds_bytes(fp()), s>>>(dv, fd);
    else
      fit_lossgrad_f32_kernel<fp()><<<G, 256, fit_f32_lds_bytes(fp()), s>>>(dv, fd);
  });
}

void launch_score_f32(const FitDev& dv, const F32Dev& fd, int G, bool centred, const ScoreOut& o, hipStream_t s) {
  dispatch_f32_fp(dv.FP, [&](auto fp) {
    if (centred)
      score_f32_kernel<fp(), true><<<G, 256, fit_f32_lds_bytes(fp()), s>>>(dv, fd, o);
    else
      score_f32_kernel<fp()><<<G, 256, fit_f32_lds_bytes(fp()), s>>>(dv, fd, o);
  });
}

void launch_fit_center_begin(const FitDev& dv, const F32Dev& fd, const float* w0, int raw, hipStream_t s) {
  fit_center_begin_kernel<<<1, 256, 0, s>>>(dv, fd, w0, raw);
}

void launch_fit_center_finalize(const FitDev& dv, const F32Dev& fd, float* w_out, hipStream_t s) {
  fit_center_finalize_kernel<<<1, 256, 0, s>>>(dv, fd, w_out);
}

void launch_fit_center_grad(const FitDev& dv, const F32Dev& fd, float* grad, hipStream_t s) {
  fit_center_grad_kernel<<<(dv.n + 255) / 256, 256, 0, s>>>(dv, fd, grad);
}

}  // namespace psx
