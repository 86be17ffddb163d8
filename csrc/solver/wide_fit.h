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

#include <vector>

#include "../kernels/wide_fit_kernels.h"
#include "fit_driver.h"

namespace psx {

class WideBatchFitter : public FitDriver {
 public:
  // max_wg <= 0: eight workgroups (32 row waves) per compute unit
  WideBatchFitter(int K, int KP, int hist, int max_wg);
  ~WideBatchFitter() override;

  void set_data(const WideFitData& d, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);  // [U]
  // Device-event milliseconds of one evaluation at the current trial point, by stage:
  // row pass, column pass, reduction (tools/bench_wide_fit.py).  raw = 1: the reduction
  // of loss_grad (gradient only); raw = 0: the reduction of a fit's evaluation, which
  // also reads the solver's vectors for the 4 + 2 hist fp64 dots.
  std::vector<float> stage_ms(int raw, hipStream_t s);

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
  WideFitDev dv_{};
  void* ws_ = nullptr;  // per-dataset workspace (every size depends on U, N or the items)
};

}  // namespace psx
