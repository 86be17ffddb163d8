// Many wide (CSR) fits advanced in lockstep on one read of the rows, of the inverted
// index and of the work items per evaluation round (the kernels and their vocabulary:
// csrc/kernels/wide_fit_many.h) -- FitMany's contract (fit_many.h) for the wide fitter.
//
// The jobs share the fitter's resident dataset and the sample-weight, class-weight and
// fold streams; each has its own penalty, held-out fold and start.  One FitLoop per job:
// a round evaluates every unfinished job at its own trial point (per pass of
// many-capacity jobs the row pass, the column pass and the reduction, the pass buffers
// reduced before the next pass), copies all result blocks to pinned memory behind ONE
// stream wait, runs every job's ctrl_step on its own block and applies all actions with
// one batched update.  A finished job's slot goes inactive and a pass without a live
// slot is not launched; jobs keep their slots for the whole call.  sigma, W, W_ho and
// the live-row count come once per distinct held-out fold from the weighted fitter's own
// weights and statistics kernels, run unchanged on scratch of this object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../kernels/wide_fit_many.h"
#include "../kernels/wide_fit_weighted.h"
#include "fit_loop.h"
#include "fit_many.h"  // FitManyJob, FitManyResult

namespace psx {

class WideFitMany {
 public:
  // dv: the fitter's dataset and geometry (after set_data); G: its row-pass grid
  WideFitMany(const WideFitDev& dv, int G);
  ~WideFitMany();
  WideFitMany(const WideFitMany&) = delete;
  WideFitMany& operator=(const WideFitMany&) = delete;

  int capacity() const { return wide_many_slots(dv_.KP); }
  // Fit every job.  w_out [M][F*KP + KP] already holds every job's untouched features (as
  // WideBatchFitter::current's buffer does): job m's touched features and intercepts are
  // written into w_out + m * (F*KP + KP), its sigma -> std_out + m * U (device buffers).
  // Starts (FitManyJob::w0) are in the full layout.  o.reg_param is ignored.
  std::vector<FitManyResult> fit(const float* sample_weight, const float* class_weight, const uint8_t* fold,
                                 const std::vector<FitManyJob>& jobs, const FitOpts& o, float* w_out, float* std_out,
                                 hipStream_t s);
  // One raw evaluation of every job's w0 (full layout; no standardisation, no penalty): the
  // weighted mean loss of the training rows, its gradient -> grads + m * (F*KP + KP) (zero
  // on untouched features), the held-out mean loss.
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

  WideFitDev dv_{};  // the dataset and geometry; R, gitem, part, bsum -> this object's pass buffers
  const uint8_t* fold_ = nullptr;
  int G_ = 1, M_ = 0, D_ = 0, NP_ = 0;
  size_t full_ = 0;  // F*KP + KP
  void* ws_ = nullptr;
  // [M][nv] vectors (S, Y [M][H][nv]), per model dpart and result block
  float *x_ = nullptr, *d_ = nullptr, *g_c_ = nullptr, *g_t_ = nullptr, *beta_t_ = nullptr, *wfix_ = nullptr;
  float *S_ = nullptr, *Y_ = nullptr;
  double *dpart_ = nullptr, *out_ = nullptr;
  float *std_ = nullptr, *inv_std_ = nullptr;  // [D][U + 1], one set per distinct held-out fold
  double* wsum_ = nullptr;                     // [D][3]
  float* wm_ = nullptr;                        // [passes][U + 1][32] interleaved trial weights
  WideManyModel* mm_ = nullptr;                // [M]
  float *v_ = nullptr, *ueff_ = nullptr;       // [N] row weights; the statistics passes' scratch
  double *wpart_ = nullptr, *ho_ = nullptr;    // (the weights kernel's partials)
  // pinned: the jobs' actions, live flags and result blocks
  void* pin_ = nullptr;
  FitStep* steps_ = nullptr;
  int* live_ = nullptr;
  double* pout_ = nullptr;
  const FitStep* steps_dev_ = nullptr;  // the kernels' addresses of steps_ / live_
  const int* live_dev_ = nullptr;
  std::vector<int> sigma_of_, hold_;  // job -> its sigma set; job -> its held-out fold
  std::vector<FitLoop> loops_;
  std::vector<double> round_s_;
};

}  // namespace psx
