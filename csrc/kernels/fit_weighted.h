// Weighted full-batch fit kernels (see fit_weighted.hip): the dense fit of
// fit_kernels.hip with a weight per row and a held-out fold.
//
//   train = {i : fold_i != holdout},  u_i = sample_weight_i * class_weight[y_i]
//   W = sum_train u_i,  f = (1/W) sum_train u_i CE_i + 0.5 reg sum beta^2
//   f_ho = (1/W_ho) sum_{fold_i == holdout} u_i CE_i
//
// sigma is the weighted sample std over the training rows.  A row's weight is formed
// per tile from the three streams below: no [N] buffer of effective weights exists,
// and another held-out fold is another kernel argument.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_kernels.h"

namespace psx {

struct FitWeightsDev {
  const float* sw;      // [Npad] sample weights; null: 1
  const uint8_t* fold;  // [Npad] fold ids; null: no row is held out
  int holdout;          // fold whose rows are held out; < 0: none
  float cw[16];         // class weights (1 without a table)
  double* wpart;        // [G][2] per-workgroup sum u over the training / held-out rows
  float* mmpart;        // [G][2][FP] per-workgroup feature min / max over the rows of positive training weight
  double* wsum;         // [2] W, W_ho
  double* ho;           // [1] held-out mean loss of the last evaluation
};

void prepare_fit_weighted_kernels();
// weighted sigma / 1/sigma over the training rows, W and W_ho -> wd.wsum
void launch_fit_stats_w(const FitDev& dv, const FitWeightsDev& wd, int G, hipStream_t s);
// part[g][16] gets the weighted training loss, part[g][17] the weighted held-out loss
void launch_fit_lossgrad_w(const FitDev& dv, const FitWeightsDev& wd, int G, hipStream_t s);
// launch_fit_reduce with 1/W for 1/N; the held-out mean -> wd.ho
void launch_fit_reduce_w(const FitDev& dv, const FitWeightsDev& wd, int G, double reg, int raw, hipStream_t s);

}  // namespace psx
