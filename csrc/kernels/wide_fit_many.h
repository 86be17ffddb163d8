// Many wide (CSR) fits per read of the rows (see wide_fit_many.hip): the weighted
// evaluation of wide_fit_weighted.hip for M models that share the rows, the labels, the
// sample and class weights, the fold stream, the inverted index and the work items, and
// differ in the held-out fold, the penalty and the iterate -- the fits of a
// cross-validation grid.
//
// The wide evaluation is bound by gathers: an entry of a row costs one gather of KP
// floats from the trial weights and another from R in the column pass, 4 * KP useful
// bytes of a 128-byte line.  Here the models lie side by side per feature:
//
//   line   the 32 fp32 of one feature (or one residual row, or one work item): 128 bytes
//   slot   KP adjacent columns of a line; 32 / KP slots (32 / 16 / 8 / 4 / 2 at KP 1 .. 16)
//   pass   one row pass + column pass + reduction that serves up to 32 / KP models
//
// Model m sits in pass m / slots, slot m % slots, for the whole call.  The geometry is a
// function of KP alone: an empty or finished slot computes on zeros or is skipped, so a
// model's numbers depend neither on its slot nor on the models beside it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "wide_fit_kernels.h"

namespace psx {

constexpr int kWideLine = 32;                       // fp32 of one line
constexpr int kWideManyPart = 3 * kWideLine;        // a wave's partial: 32 residual sums, 32 training, 32 held-out losses
constexpr int kWideManyOutWords = kFitOutWords + 1;  // a model's result block, then its held-out mean loss
constexpr int wide_many_slots(int KP) { return kWideLine / KP; }

// One model as the batched vector kernels see it (a device array, model on blockIdx.y).
struct WideManyModel {
  // the dataset and geometry; the model's OWN compact vectors x .. wfix, S, Y, dpart and
  // out (its result block); std_ / inv_std of its held-out fold; gitem / part / bsum the
  // pass buffers.  weff and R are unused (null).
  WideFitDev dv;
  const double* wsum;  // [3] W, W_ho, L of its held-out fold
  const float* w0;     // full layout [F*KP + KP]: start (begin) / weights (raw); null: zeros
  float* wm;           // its pass's interleaved trial weights [U + 1][32], the intercept row last
  double reg;
  int col0;  // first column of its slot
};

// One pass of the evaluation.
struct WideManyPass {
  WideFitDev dv;        // the dataset, W; R [N][32], gitem [I][32], part [W][96], bsum [32] of the pass buffers
  const float* v;       // [N] sample_weight * class_weight[y]
  const uint8_t* fold;  // [N] or null
  const float* wm;      // [U + 1][32]
  int hold[kWideLine];  // held-out fold of every slot; < 0: none
  unsigned live;        // slots with an unfinished model; the others are skipped (R = 0)
};

// v[r] = sample_weight[r] * class_weight[y[r]] (sw null: 1; the fp32 product of wide_fit_weights_kernel)
void launch_wide_many_weights(const WideFitDev& dv, const float* sw, const float (&cw)[16], float* v, hipStream_t s);
// x = w0 * sigma gathered through uniq, trial point = x -> the model's slot; raw: the weights themselves
void launch_wide_many_begin(const WideManyModel* mm, int M, int n, int zero_const, int raw, hipStream_t s);
// row pass and column pass of one pass, then the W residual-sum partials -> bsum
void launch_wide_many_eval(const WideManyPass& ps, int G, hipStream_t s);
// models [m0, m0 + cnt) of that pass, before the next pass overwrites its buffers: g_t and the
// partial dots, then f_t, the mean loss, the dots and the held-out mean -> the model's result
// block; a model that is not live is skipped
void launch_wide_many_reduce(const WideManyModel* mm, const int* live, int m0, int cnt, int n, int raw,
                             hipStream_t s);
void launch_wide_many_update(const WideManyModel* mm, const FitStep* steps, int M, int n, hipStream_t s);
// model m's touched features and intercepts -> w_all + m * (F*KP + KP) (as launch_wide_fit_finalize,
// centred over the classes when its penalty is 0)
void launch_wide_many_finalize(const WideManyModel* mm, int M, int64_t U, float* w_all, hipStream_t s);
// model m's g_t -> grads + m * (F*KP + KP) through uniq (zeroed by the caller)
void launch_wide_many_scatter(const WideManyModel* mm, int M, int n, float* grads, hipStream_t s);

}  // namespace psx
