// Weighted full-batch fit kernels of the wide (CSR) model (see wide_fit_weighted.hip):
// the objective of fit_weighted.h in the subspace of the touched features.
//
//   v_i = sample_weight_i * class_weight[y_i]  (the fp32 product)
//   train = {i : fold_i != holdout},  u_i = v_i on train, 0 elsewhere,  h_i = v_i on the held-out rows
//   W = sum u,  f = (1/W) sum u_i loss_i + 0.5 reg sum beta^2,  f_ho = (1/W_ho) sum h_i loss_i
//
// sigma is the weighted sample std over all training rows, absent entries counting as
// zeros.  Unlike the dense kernels, which form a row's weight per tile from its three
// streams, these keep ONE fp32 per row, ueff[r] = +v on a training row and -v on a
// held-out one: the statistics pass meets a row once per ENTRY (through crow[e]) and
// would otherwise pay three dependent gathers there.  Another held-out fold is the
// weights kernel plus the statistics kernel; U, uniq and the inverted index stay
// those of the whole dataset.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wide_fit_kernels.h"

namespace psx {

constexpr int kWideWeightsMaxWG = 1024;  // workgroups of the weights kernel = rows of wpart

struct WideFitWeightsDev {
  const float* sw;      // [N] sample weights; null: 1
  const uint8_t* fold;  // [N] fold ids; null: no row is held out
  int holdout;          // fold whose rows are held out; < 0: none
  float cw[16];         // class weights (1 without a table); K == 1: entries 0 and 1
  float* ueff;          // [N] +v training row, -v held-out row (the sign BIT decides: -0.f is held out)
  double* wpart;        // [workgroups][3] sum u, sum h, rows with u > 0
  double* wsum;         // [3] W, W_ho, L (live training rows)
  double* ho;           // [1] held-out mean loss of the last evaluation
};

inline int wide_fit_weights_grid(int64_t N) {
  const int64_t b = (N + 255) / 256;
  return (int)(b < 1 ? 1 : b > kWideWeightsMaxWG ? kWideWeightsMaxWG : b);
}

// ueff and wsum from the three streams
void launch_wide_fit_weights(const WideFitDev& dv, const WideFitWeightsDev& wd, hipStream_t s);
// weighted sigma / 1/sigma of the touched features (needs ueff and wsum)
void launch_wide_fit_stats_w(const WideFitDev& dv, const WideFitWeightsDev& wd, hipStream_t s);
// the row pass: R[r] = u * residual (0 on held-out rows); part[w][16] the weighted training
// loss, part[w][17] the weighted held-out loss.  The column pass that follows is the plain one.
void launch_wide_fit_rows_w(const WideFitDev& dv, const WideFitWeightsDev& wd, int G, hipStream_t s);
// launch_wide_fit_reduce with 1/W for 1/N; the held-out mean -> wd.ho
void launch_wide_fit_reduce_w(const WideFitDev& dv, const WideFitWeightsDev& wd, double reg, int raw, hipStream_t s);

}  // namespace psx
