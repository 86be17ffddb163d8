// Full-batch trainer of the wide (CSR) model: the objective and the optimiser of
// fit.h, in the subspace of the U distinct features the dataset touches (the others
// have sigma 0 by definition and are excluded).  All solver vectors have
// n = U*KP + KP elements in the device layout of a WideSpec(U, K).
//
// The dataset's one-time structures (sorted feature ids, compact columns, inverted
// index, work items of the column pass) are built by the caller on the device and
// handed over as pointers; set_data computes the statistics and sizes the workspace.
// Per evaluation the host launches the row pass, the column pass and the reduction
// (wide_fit_kernels.hip), then runs FitLoop (fit_loop.h), the loop the dense fitter runs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../kernels/wide_fit_kernels.h"
#include "fit_loop.h"

namespace psx {

class WideBatchFitter {
 public:
  // max_wg <= 0: eight workgroups (32 row waves) per compute unit
  WideBatchFitter(int K, int KP, int hist, int max_wg);
  ~WideBatchFitter();
  WideBatchFitter(const WideBatchFitter&) = delete;
  WideBatchFitter& operator=(const WideBatchFitter&) = delete;

  void set_data(const WideFitData& d, hipStream_t s);
  // Mean loss at w (full device layout [F*KP + KP]) and its gradient -> grad (same
  // layout; untouched features get 0): no standardisation, no L2 term.
  double loss_grad(const float* w, float* grad, hipStream_t s);
  // Start a fit at w0 (full layout; nullptr: zeros).
  void begin(const float* w0, const FitOpts& o, hipStream_t s);
  bool run(int max_accept, hipStream_t s);
  // The current iterate, finalised, scattered into w_out [F*KP + KP]; only the touched
  // features and the intercepts are written (synchronous).
  void current(float* w_out, hipStream_t s);
  void read_std(float* std_out, hipStream_t s);  // [U]
  // Copies of the optimiser's vectors into caller-owned device buffers (nullptr: skip):
  // x, d, g_c, g_t, beta_t, wfix are [nv], S and Y [hist][nv].  Synchronous, read-only.
  void read_state(float* x, float* d, float* g_c, float* g_t, float* beta_t, float* wfix, float* S, float* Y,
                  hipStream_t s);
  int n() const { return dv_.n; }  // 0 before set_data
  int nv() const { return dv_.nv; }
  // Device-event milliseconds of one evaluation at the current trial point, by stage:
  // row pass, column pass, reduction (tools/bench_wide_fit.py).  raw = 1: the reduction
  // of loss_grad (gradient only); raw = 0: the reduction of a fit's evaluation, which
  // also reads the solver's vectors for the 4 + 2 hist fp64 dots.
  std::vector<float> stage_ms(int raw, hipStream_t s);

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
  WideFitDev dv_{};
  int max_wg_ = 0, G_ = 1;
  void* ws_ = nullptr;  // per-dataset workspace (every size depends on U, N or the items)
  double* pin_ = nullptr;
  FitLoop loop_;
  std::vector<double> eval_s_;
};

}  // namespace psx
