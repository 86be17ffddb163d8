// Full-batch trainer and scorer of the fp32-row family: dense rows kept in fp32, padded to
// FP in {128, 256, 512, 1024}, evaluated by the two-image kernels of
// csrc/kernels/fit_f32.hip.  The objective, the optimiser and the lifecycle are the dense
// fitter's (fit.h): FitDriver and FitLoop drive it, and the vector kernels of
// fit_kernels.hip run unchanged on the same FitDev.  No row weights and no batched fits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../kernels/fit_f32.h"
#include "fit_driver.h"

namespace psx {

class F32BatchFitter : public FitDriver {
 public:
  // max_wg: workgroups of one launch.  max_wg <= 0: as many per compute unit as the two
  // tile images leave room for in its LDS (fit_f32_wg_per_cu: 1 at 1,024 .. 4 at 128).
  // centred: every kernel multiplies x - c_f, c the columns' means (the statistics pass writes
  // them, or set_center); the optimiser runs in (beta, b' = b + sum_f c_f w_f), and what goes
  // in and comes out -- w0, the fitted weights, loss_grad's gradient, score's weights -- stays
  // in raw coordinates.  Off: exactly the uncentred launches.
  F32BatchFitter(int K, int F, int FP, int hist, int max_wg, bool centred = false);
  ~F32BatchFitter() override;

  // X [Npad][FP] fp32 with Npad = N rounded up to 32 (padding rows and columns zero),
  // y [Npad]; caller-owned, must outlive every later call.  stats: compute the feature
  // statistics (a fit needs them; loss_grad and score do not).
  void set_data(const float* X, const int32_t* y, int64_t N, int64_t Npad, bool stats, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);  // [FP]
  // The centre of a dataset loaded without statistics (a scorer's: the training set's), c [FP]
  // on the device with zeros in the padding; copied.  set_data forgets it.
  void set_center(const float* c, hipStream_t s);
  void read_center(float* c_out, hipStream_t s);  // [FP]
  bool centred() const { return centred_; }
  // loss_grad with the gradient left in centred coordinates, with respect to (w, b').
  double loss_grad_centred(const float* w, float* grad, hipStream_t s);
  // Score the resident rows with the weights w ([K*FP + K], the model's device layout):
  // o's row outputs are [N]; labels are required, o.hist must be null.  Ends a fit in
  // progress (its trial point is overwritten).
  void score(const float* w, const ScoreOut& o, hipStream_t s);
  // Mean milliseconds over `reps` evaluations at the weights w of the loss + gradient launch
  // and of the reduction (tools/bench_fit_f32.py).  Ends a fit in progress.
  std::vector<float> time_launches(const float* w, int reps, hipStream_t s);

 protected:
  int64_t rows() const override { return fd_.X ? dv_.N : 0; }
  FitVectors vectors() const override;
  void launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) override;
  void launch_eval(double reg, int raw, hipStream_t s) override;
  void launch_update(const FitStep& st, hipStream_t s) override;
  void launch_finalize(int center, float* w_out, hipStream_t s) override;
  void export_grad(float* grad, hipStream_t s) override;

 private:
  FitDev dv_{};  // (its bf16 row pointer stays null)
  F32Dev fd_{};
  void need_center(const char* what) const;
  bool have_stats_ = false;
  const bool centred_;
  bool have_center_ = false;
  bool export_raw_ = true;  // export_grad maps a centred gradient back (off inside loss_grad_centred)
  void* ws_ = nullptr;
  void* data_ws_ = nullptr;  // per-dataset partials (sized by the grid)
};

}  // namespace psx
