// Many dense fits advanced in lockstep on one read of the rows per evaluation round
// (the kernels and their vocabulary: csrc/kernels/fit_many.h).
//
// The jobs share the fitter's resident rows and labels and the sample-weight, class-
// weight and fold streams; each has its own penalty, held-out fold and start.  One
// FitLoop per job: a round evaluates every unfinished job at its own trial point (one
// launch per pass of many_capacity jobs, the pass buffers reduced before the next pass),
// copies all result blocks to pinned memory behind ONE stream wait, runs every job's
// ctrl_step on its own block and applies all actions with one batched update.  A
// finished job's slot goes inactive (no update, result ignored) and a pass without a
// live slot is not launched; jobs keep their slots, so a job's numbers do not depend on
// which other jobs run beside it.  sigma, W and W_ho are computed once per distinct
// held-out fold by the weighted statistics kernel and shared by the jobs that hold it out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../kernels/fit_many.h"
#include "../kernels/fit_weighted.h"
#include "fit_loop.h"

namespace psx {

struct FitManyJob {
  double reg_param = 0.0;
  int holdout = -1;           // < 0: no row is held out
  const float* w0 = nullptr;  // device [n]: the start of a fit / the weights of an evaluation; null: zeros
};

struct FitManyResult {
  double objective, log_loss;
  int accepted, evals, ls_fail;
  std::string reason;
  std::vector<double> history;
};

class FitMany {
 public:
  // dv: the fitter's geometry, rows and statistics partials; wd: its weight partials; G: its grid
  FitMany(const FitDev& dv, const FitWeightsDev& wd, int G);
  ~FitMany();
  FitMany(const FitMany&) = delete;
  FitMany& operator=(const FitMany&) = delete;

  int capacity() const { return many_capacity(dv_.FP, dv_.K); }
  // Fit every job; job m's finalised weights -> w_out + m * n, its sigma -> std_out + m * FP
  // (device buffers).  o.reg_param is ignored: the jobs carry their own.
  std::vector<FitManyResult> fit(const float* sample_weight, const float* class_weight, const uint8_t* fold,
                                 const std::vector<FitManyJob>& jobs, const FitOpts& o, float* w_out, float* std_out,
                                 hipStream_t s);
  // One raw evaluation of every job's w0 (no standardisation, no penalty): the weighted
  // mean loss of the training rows, its gradient -> grads + m * n, the held-out mean loss.
  void loss_grad(const float* sample_weight, const float* class_weight, const uint8_t* fold,
                 const std::vector<FitManyJob>& jobs, float* grads, std::vector<double>& losses,
                 std::vector<double>& holdout_losses, hipStream_t s);
  // seconds of every evaluation round of the last call (all passes, the reductions, the wait)
  const std::vector<double>& round_seconds() const { return round_s_; }

 private:
  void place(const float* sw, const float* cw, const uint8_t* fold, const std::vector<FitManyJob>& jobs, hipStream_t s);
  void reserve(int M, int D);
  void release();
  void round(int raw, hipStream_t s);

  FitDev dv_{};         // geometry, rows, spart
  FitWeightsDev wd_{};  // streams of the call, wpart / mmpart
  int G_ = 1, M_ = 0, D_ = 0, NP_ = 0;
  void* ws_ = nullptr;
  // [M][nv] vectors (S, Y [M][H][nv]), per model dpart and result block
  float *x_ = nullptr, *d_ = nullptr, *g_c_ = nullptr, *g_t_ = nullptr, *beta_t_ = nullptr, *wfix_ = nullptr;
  float *S_ = nullptr, *Y_ = nullptr;
  double *dpart_ = nullptr, *out_ = nullptr;
  float *std_ = nullptr, *inv_std_ = nullptr;  // [D][FP], one set per distinct held-out fold
  double* wsum_ = nullptr;                     // [D][2]
  uint16_t *whi_ = nullptr, *wlo_ = nullptr;   // [passes * GP][16 * FP]
  float* b_eff_ = nullptr;                     // [passes * GP][16]
  int* hold_ = nullptr;                        // [passes * capacity]
  FitManyModel* mm_ = nullptr;                 // [M]
  float *gpart_ = nullptr, *part_ = nullptr;   // one pass
  // pinned: the jobs' actions, live flags and result blocks
  void* pin_ = nullptr;
  FitStep* steps_ = nullptr;
  int* live_ = nullptr;
  double* pout_ = nullptr;
  const FitStep* steps_dev_ = nullptr;  // the kernels' addresses of steps_ / live_
  const int* live_dev_ = nullptr;
  std::vector<int> sigma_of_;  // job -> its sigma set
  std::vector<FitLoop> loops_;
  std::vector<double> round_s_;
};

}  // namespace psx
