// Full-batch trainer of the wide (CSR) model: the objective and the optimiser of
// fit.h, in the subspace of the U distinct features the dataset touches (the others
// have sigma 0 by definition and are excluded).  All solver vectors have
// n = U*KP + KP elements in the device layout of a WideSpec(U, K).
//
// The dataset's one-time structures (sorted feature ids, compact columns, inverted
// index, work items of the column pass) are built by the caller on the device and
// handed over as pointers; set_data computes the statistics and sizes the workspace.
// Per evaluation the host launches the row pass, the column pass and the reduction
// (wide_fit_kernels.hip); the lifecycle and the loop are FitDriver's (fit_driver.h),
// as for the dense fitter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "../kernels/wide_fit_kernels.h"
#include "../kernels/wide_fit_weighted.h"
#include "fit_driver.h"

namespace psx {

class WideFitMany;

class WideBatchFitter : public FitDriver {
 public:
  // max_wg <= 0: eight workgroups (32 row waves) per compute unit
  WideBatchFitter(int K, int KP, int hist, int max_wg);
  ~WideBatchFitter() override;

  void set_data(const WideFitData& d, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);  // [U]
  // Row weights u_i = sample_weight_i * class_weight[y_i] and a held-out fold (the
  // objective is stated in csrc/kernels/wide_fit_weighted.h), with BatchFitter's
  // contract: sample_weight [N] fp32 and fold [N] uint8 are device buffers, caller-owned
  // as the rows are; class_weight is K host floats (two, for labels 0 and 1, when
  // K == 1); each may be null.  holdout < 0: no row is held out.  Valid after set_data;
  // ends a fit in progress and runs the weights and statistics kernels -- the inverted
  // index and the work items are untouched.  All null and holdout < 0: back to the plain
  // kernels and statistics.  A new set_data clears the weights.
  void set_weights(const float* sample_weight, const float* class_weight, const uint8_t* fold, int holdout,
                   hipStream_t s);
  bool weighted() const { return weighted_; }
  int class_weights() const { return dv_.K == 1 ? 2 : dv_.K; }  // entries of the class table
  // The held-out rows' weighted mean loss at the last evaluation (0 without held-out weight).
  double holdout_loss(hipStream_t s);
  // Device-event milliseconds of one evaluation at the current trial point, by stage:
  // row pass, column pass, reduction (tools/bench_wide_fit.py).  raw = 1: the reduction
  // of loss_grad (gradient only); raw = 0: the reduction of a fit's evaluation, which
  // also reads the solver's vectors for the 4 + 2 hist fp64 dots.
  std::vector<float> stage_ms(int raw, hipStream_t s);
  // Many fits per read of the rows (wide_fit_many.h) on the resident dataset; its workspace
  // is its own, made on first use and dropped by the next set_data.  It keeps its own row
  // weights and statistics: set_weights and a fit in progress here are not disturbed.
  WideFitMany& many();
  int padded_classes() const { return dv_.KP; }
  size_t full_size() const { return ((size_t)dv_.F + 1) * dv_.KP; }  // F*KP + KP of the loaded dataset's model

 protected:
  // the weights are the full layout [F*KP + KP]: begin gathers w0 through uniq, finalize
  // writes only the touched features and the intercepts, the gradient of an untouched
  // feature is 0.  The vectors exist after set_data (n == 0 before it).
  int64_t rows() const override { return ws_ ? dv_.N : 0; }
  FitVectors vectors() const override;
  void launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) override;
  void launch_eval(double reg, int raw, hipStream_t s) override;
  void launch_update(const FitStep& st, hipStream_t s) override;
  void launch_finalize(int center, float* w_out, hipStream_t s) override;
  void export_grad(float* grad, hipStream_t s) override;

 private:
  void launch_rows(hipStream_t s);                         // the plain or the weighted row pass
  void launch_reduce(double reg, int raw, hipStream_t s);  // ... and reduction
  WideFitDev dv_{};
  WideFitWeightsDev wd_{};
  bool weighted_ = false;
  void* ws_ = nullptr;  // per-dataset workspace (every size depends on U, N or the items)
  std::unique_ptr<WideFitMany> many_;
};

}  // namespace psx
