// Full-batch trainer: fits the dense model to a dataset resident in HBM until the
// optimiser converges (Spark's LogisticRegression.fit with standardization=true,
// elasticNetParam=0; the objective is stated in csrc/kernels/fit_kernels.hip).
//
// Per evaluation the host launches fit_lossgrad and fit_reduce, reads (f_t, dots)
// from a pinned block after one stream wait, runs the HOST build of the streaming
// solver's controller (ctrl_step of solver_ctrl.h: the same line search and compact
// L-BFGS, with no slot budget) and launches fit_update with the resulting action,
// whose scalars travel as kernel arguments.  No ring, no slot limit, no graph.
// The loop itself is FitLoop (fit_loop.h) and the lifecycle around it FitDriver
// (fit_driver.h), both shared with the wide fitter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>

#include "../kernels/fit_kernels.h"
#include "../kernels/fit_weighted.h"
#include "fit_driver.h"

namespace psx {

class FitMany;

class BatchFitter : public FitDriver {
 public:
  // max_wg <= 0: two workgroups per compute unit
  BatchFitter(int K, int F, int FP, int hist, int max_wg);
  ~BatchFitter() override;

  // X [Npad][FP] bf16 with Npad = N rounded up to 32 (padding rows zero), y [Npad];
  // caller-owned, must outlive every later call.  Computes the feature statistics.
  void set_data(const uint16_t* X, const int32_t* y, int64_t N, int64_t Npad, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);  // [FP]
  // Row weights u_i = sample_weight_i * class_weight[y_i] and a held-out fold (the
  // objective is stated in csrc/kernels/fit_weighted.h).  sample_weight [Npad] fp32 and
  // fold [Npad] uint8 are device buffers, caller-owned as the rows are; class_weight is
  // K host floats; each may be null.  holdout < 0: no row is held out.  Valid after
  // set_data; ends a fit in progress and computes the weighted statistics.  All null
  // and holdout < 0: back to the plain kernels and statistics.  A new set_data clears
  // the weights.
  void set_weights(const float* sample_weight, const float* class_weight, const uint8_t* fold, int holdout,
                   hipStream_t s);
  bool weighted() const { return weighted_; }
  int classes() const { return dv_.K; }
  int width() const { return dv_.FP; }
  // The held-out rows' weighted mean loss at the last evaluation (0 without held-out weight).
  double holdout_loss(hipStream_t s);
  // Many fits per read of the rows (fit_many.h) on the resident rows; its workspace is
  // built on first use and dropped by set_data.  It keeps vectors of its own: a fit in
  // progress and the weights set here are left as they are.
  FitMany& many();

 protected:
  // the weights are [K*FP + K]; the vectors exist from construction
  int64_t rows() const override { return dv_.X ? dv_.N : 0; }
  FitVectors vectors() const override;
  void launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) override;
  void launch_eval(double reg, int raw, hipStream_t s) override;
  void launch_update(const FitStep& st, hipStream_t s) override;
  void launch_finalize(int center, float* w_out, hipStream_t s) override;
  void export_grad(float* grad, hipStream_t s) override;

 private:
  FitDev dv_{};
  FitWeightsDev wd_{};
  bool weighted_ = false;
  void* ws_ = nullptr;
  void* data_ws_ = nullptr;  // per-dataset partials (sized by the grid)
  std::unique_ptr<FitMany> many_;
};

}  // namespace psx
