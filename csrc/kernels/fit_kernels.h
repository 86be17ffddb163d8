// Full-batch fit kernels (see fit_kernels.hip): statistics, one loss + gradient
// evaluation over a resident dataset, its fixed-order reduction with the L2 term
// and the controller's dots, the vector update of one controller action, and the
// finalisation.  Plain streaming launches: no cross-workgroup waits, no float
// atomics, every reduction in a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_step.h"  // FitStep, the result block's layout

namespace psx {

// Vectors of the fit: n = K*FP + K elements in the model's device layout
// ([K][FP] coefficients, then K intercepts); the curvature pairs have stride nv.
struct FitDev {
  const uint16_t* X;  // [Npad][FP] bf16, rows >= N zero
  const int32_t* y;   // [Npad]
  int N, Npad;
  int K, F, FP, H;
  int n, nv;
  float *x, *d, *g_c, *g_t, *beta_t;  // [nv] iterate, direction, gradient at x, gradient / point of the trial
  float *S, *Y;                       // [H][nv]
  float* wfix;                        // [nv] frozen coefficients of constant features (zero_const off)
  float *std_, *inv_std;              // [FP]
  float* b_eff;                       // [16] trial intercepts
  uint16_t *whi, *wlo;                // [16*FP] trial weight fragments (classes >= K stay zero)
  float* gpart;                       // [G][K][FP] per-workgroup sums of R^T X
  float* part;                        // [G][32] per-workgroup residual sums [16], loss
  double* spart;                      // [G][2][FP] per-workgroup column sums / sums of squares
  double* dpart;                      // [reduce workgroups][kFitDotStride]
  double* out;                        // [kFitOutWords]
};

void prepare_fit_kernels();
int fit_reduce_grid(int n);
// sigma / 1/sigma of every feature over the N rows (G workgroups, then one fixed-order pass)
void launch_fit_stats(const FitDev& dv, int G, hipStream_t s);
// x = w0 * sigma (zeros without w0), trial point = x; raw: the weights themselves, no standardisation
void launch_fit_begin(const FitDev& dv, const float* w0, int zero_const, int raw, hipStream_t s);
void launch_fit_lossgrad(const FitDev& dv, int G, hipStream_t s);
// raw: gradient in the original feature space, no L2 term, no dots with the solver's vectors
void launch_fit_reduce(const FitDev& dv, int G, double reg, int raw, hipStream_t s);
void launch_fit_update(const FitDev& dv, const FitStep& st, hipStream_t s);
void launch_fit_finalize(const FitDev& dv, int center, float* w_out, hipStream_t s);

}  // namespace psx
