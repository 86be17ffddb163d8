// Full-batch trainer: fits the dense model to a dataset resident in HBM until the
// optimiser converges (Spark's LogisticRegression.fit with standardization=true,
// elasticNetParam=0; the objective is stated in csrc/kernels/fit_kernels.hip).
//
// Per evaluation the host launches fit_lossgrad and fit_reduce, reads (f_t, dots)
// from a pinned block after one stream wait, runs the HOST build of the streaming
// solver's controller (ctrl_step of solver_ctrl.h: the same line search and compact
// L-BFGS, with no slot budget) and launches fit_update with the resulting action,
// whose scalars travel as kernel arguments.  No ring, no slot limit, no graph.
// The loop itself is FitLoop (fit_loop.h), shared with the wide fitter.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../kernels/fit_kernels.h"
#include "fit_loop.h"

namespace psx {

class BatchFitter {
 public:
  // max_wg <= 0: two workgroups per compute unit
  BatchFitter(int K, int F, int FP, int hist, int max_wg);
  ~BatchFitter();
  BatchFitter(const BatchFitter&) = delete;
  BatchFitter& operator=(const BatchFitter&) = delete;

  // X [Npad][FP] bf16 with Npad = N rounded up to 32 (padding rows zero), y [Npad];
  // caller-owned, must outlive every later call.  Computes the feature statistics.
  void set_data(const uint16_t* X, const int32_t* y, int64_t N, int64_t Npad, hipStream_t s);
  // Mean cross entropy at w (device layout) and its gradient -> grad [K*FP + K]:
  // no standardisation, no L2 term.
  double loss_grad(const float* w, float* grad, hipStream_t s);
  // Start a fit at w0 (nullptr: zeros).
  void begin(const float* w0, const FitOpts& o, hipStream_t s);
  // Evaluate until the fit ends or `max_accept` more steps were accepted; true: ended.
  bool run(int max_accept, hipStream_t s);
  // The current iterate, finalised, -> w_out [K*FP + K] (synchronous).
  void current(float* w_out, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);
  // Copies of the optimiser's vectors into caller-owned device buffers (nullptr: skip):
  // x, d, g_c, g_t, beta_t, wfix are [nv], S and Y [hist][nv].  Synchronous, read-only.
  void read_state(float* x, float* d, float* g_c, float* g_t, float* beta_t, float* wfix, float* S, float* Y,
                  hipStream_t s);
  int n() const { return dv_.n; }
  int nv() const { return dv_.nv; }

  bool done() const { return loop_.done(); }
  const std::string& reason() const { return loop_.reason(); }
  int evals() const { return loop_.ctrl().evals; }
  int accepted() const { return loop_.ctrl().nacc; }
  int ls_fail() const { return loop_.ctrl().ls_fail; }
  int dir_reset() const { return loop_.ctrl().dir_reset; }
  double objective() const { return loop_.ctrl().f_c; }
  double log_loss() const { return loop_.log_loss(); }
  const std::vector<double>& history() const { return loop_.history(); }
  const std::vector<double>& eval_seconds() const { return eval_s_; }
  int grid() const { return G_; }

 private:
  void evaluate(double reg, int raw, hipStream_t s);
  FitDev dv_{};
  int max_wg_ = 0, G_ = 1;
  void* ws_ = nullptr;
  void* data_ws_ = nullptr;  // per-dataset partials (sized by the grid)
  double* pin_ = nullptr;
  FitLoop loop_;
  std::vector<double> eval_s_;
};

}  // namespace psx
