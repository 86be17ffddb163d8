// Full-batch trainer and scorer of the panel family: dense bf16 rows of 2,048 < F <=
// 16,384 features (padded to FP in {4096, 8192, 16384}), evaluated by the panel kernels
// of csrc/kernels/panel_fit.hip.  The objective, the optimiser and the lifecycle are the
// dense fitter's (fit.h): FitDriver and FitLoop drive it, and the vector kernels of
// fit_kernels.hip run unchanged on the same FitDev.  No row weights and no batched fits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kernels/panel_fit.h"
#include "fit_driver.h"

namespace psx {

class PanelBatchFitter : public FitDriver {
 public:
  // max_wg: row blocks of one launch (each block has one workgroup per live panel).
  // max_wg <= 0: eight workgroups per compute unit over all panels.
  PanelBatchFitter(int K, int F, int FP, int hist, int max_wg);
  ~PanelBatchFitter() override;

  // X [Npad][FP] bf16 with Npad = N rounded up to 32 (padding rows zero), y [Npad];
  // caller-owned, must outlive every later call.  stats: compute the feature statistics
  // (a fit needs them; loss_grad and score do not).
  void set_data(const uint16_t* X, const int32_t* y, int64_t N, int64_t Npad, bool stats, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);  // [FP]
  // Score the resident rows with the weights w ([K*FP + K], the model's device layout):
  // o's row outputs are [N]; labels are required, o.hist must be null.  Ends a fit in
  // progress (its trial point is overwritten).
  void score(const float* w, const ScoreOut& o, hipStream_t s);
  // Mean milliseconds over `reps` evaluations at the weights w of the forward, the residual
  // and the backward launch and of the reduction (tools/bench_panel_fit.py).  Ends a fit in progress.
  std::vector<float> time_launches(const float* w, int reps, hipStream_t s);

 protected:
  int64_t rows() const override { return dv_.X ? dv_.N : 0; }
  FitVectors vectors() const override;
  void launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) override;
  void launch_eval(double reg, int raw, hipStream_t s) override;
  void launch_update(const FitStep& st, hipStream_t s) override;
  void launch_finalize(int center, float* w_out, hipStream_t s) override;
  void export_grad(float* grad, hipStream_t s) override;

 private:
  FitDev dv_{};
  PanelDev pd_{};
  bool auto_grid_ = false, have_stats_ = false;
  void* ws_ = nullptr;
  void* data_ws_ = nullptr;  // per-dataset partials (sized by the grid and the rows)
};

}  // namespace psx
