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

#include "../kernels/fit_kernels.h"
#include "fit_driver.h"

namespace psx {

class BatchFitter : public FitDriver {
 public:
  // max_wg <= 0: two workgroups per compute unit
  BatchFitter(int K, int F, int FP, int hist, int max_wg);
  ~BatchFitter() override;

  // X [Npad][FP] bf16 with Npad = N rounded up to 32 (padding rows zero), y [Npad];
  // caller-owned, must outlive every later call.  Computes the feature statistics.
  void set_data(const uint16_t* X, const int32_t* y, int64_t N, int64_t Npad, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);  // [FP]

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
  void* ws_ = nullptr;
  void* data_ws_ = nullptr;  // per-dataset partials (sized by the grid)
};

}  // namespace psx
