// fp32-row kernels (see fit_f32.hip): the full-batch fit's evaluation, statistics and
// scoring for dense rows kept in fp32, float [Npad][FP] with FP in {128, 256, 512, 1024}.
// A tile is staged as two bf16 images (hi and lo, tile.h's stage_tile_f32) from one read
// of the rows, so the products reach near-fp32 accuracy on the bf16 MFMA.  Plain streaming
// launches: no cross-workgroup waits, no float atomics, every sum in a fixed order.  The
// vector side (fit_begin / fit_reduce / fit_dots / fit_update / fit_finalize of
// fit_kernels.h) is launched unchanged on the same FitDev, whose bf16 row pointer stays null.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_kernels.h"
#include "lr_kernels.h"
#include "score_kernels.h"

namespace psx {

// LDS of one workgroup: the hi and the lo image of a 32-row tile, then the tail of
// eval_lds_bytes (logits 8 KB, residual tile 2 KB, labels and the per-wave sums).
constexpr size_t fit_f32_lds_bytes(int FP) { return eval_lds_bytes(FP) + (size_t)kTileRows * FP * 2; }
constexpr int kFitF32MaxFP = 1024;
static_assert(fit_f32_lds_bytes(kFitF32MaxFP) == 142848 && fit_f32_lds_bytes(kFitF32MaxFP) <= kLdsPerWorkgroup,
              "two tile images of the widest fp32 rows fit the 160 KB LDS of gfx950");
static_assert(fit_f32_lds_bytes(2 * kFitF32MaxFP) > kLdsPerWorkgroup, "nothing wider does");

inline bool fit_f32_fp_supported(int FP) { return FP == 128 || FP == 256 || FP == 512 || FP == 1024; }
// Workgroups of 4 waves a compute unit holds at once: what its LDS allows (1 at 1,024,
// 2 at 512, 3 at 256, 5 at 128), at most the 4 the narrowest kernel's registers allow
// (81 VGPRs + 16 AGPRs: 4 waves per SIMD, profiles/r23/README.md).
constexpr int fit_f32_wg_per_cu(int FP) {
  const size_t n = kLdsPerWorkgroup / fit_f32_lds_bytes(FP);
  return n < 1 ? 1 : (n > 4 ? 4 : (int)n);
}

// What the fp32 family keeps beside FitDev (per dataset).
struct F32Dev {
  const float* X;  // [Npad][FP] fp32, rows >= N and columns >= F zero
  float* mmpart;   // [G][2][FP] per-workgroup column minimum / maximum over the rows < N
  float* center;   // [FP] c_f: the column's mean, a constant column's value itself, 0 for padding features
};

void prepare_fit_f32_kernels();
// sigma / 1/sigma and the centre c of every feature over the N rows, every element widened
// to double (G workgroups, then one fixed-order pass); a column is constant iff its max == min
void launch_fit_stats_f32(const FitDev& dv, const F32Dev& fd, int G, hipStream_t s);
// loss partials, residual sums and the [G][K][FP] gradient partials at the trial fragments
// (one launch); launch_fit_reduce follows unchanged.  centred: on the rows x - c
void launch_fit_lossgrad_f32(const FitDev& dv, const F32Dev& fd, int G, bool centred, hipStream_t s);
// the row outputs of score_kernels.h at the trial fragments (labels required, no histogram)
void launch_score_f32(const FitDev& dv, const F32Dev& fd, int G, bool centred, const ScoreOut& o, hipStream_t s);

// The centred mode's three vector kernels: fp64, one workgroup, a fixed summation order.
// After launch_fit_begin (same w0 and raw): b'_k = b_k + sum_f c_f w_eff[k][f] -> b_eff, and,
// in a fit (raw == 0), the optimiser's intercept entries of x and beta_t.
void launch_fit_center_begin(const FitDev& dv, const F32Dev& fd, const float* w0, int raw, hipStream_t s);
// After launch_fit_finalize: w_out's intercepts = b'_k - sum_f c_f w_out[k][f], centred over the classes.
void launch_fit_center_finalize(const FitDev& dv, const F32Dev& fd, float* w_out, hipStream_t s);
// The last evaluation's gradient in raw coordinates: grad[k][f] = g_t[k][f] + c_f g_t[b_k], intercepts copied.
void launch_fit_center_grad(const FitDev& dv, const F32Dev& fd, float* grad, hipStream_t s);

}  // namespace psx
