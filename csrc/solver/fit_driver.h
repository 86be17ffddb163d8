// The host driver of a full-batch fit, written once for the dense fitter (fit.h) and
// the wide one (wide_fit.h): the lifecycle loss_grad / begin / run / current around
// FitLoop (fit_loop.h), the pinned result block of one evaluation, the evaluation
// timing and the read-only view of the optimiser's vectors.  A fitter supplies its
// kernels through the launch_* hooks and says what it holds (rows, vectors).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../kernels/fit_step.h"
#include "fit_loop.h"

namespace psx {

// The optimiser's vectors as either fitter keeps them: x, d, g_c, g_t, beta_t, wfix
// are [nv] (n used), S and Y [H][nv]; out is the device copy of the result block.
// Null pointers and n == 0: the fitter has no vectors yet.
struct FitVectors {
  int n, nv, H;
  float *x, *d, *g_c, *g_t, *beta_t, *S, *Y, *wfix;
  double* out;
};

// Carves one allocation into 256-byte aligned pieces.  A layout is run twice: without
// a base to size the allocation (`off` ends as its bytes), then with it to set the pointers.
struct Carver {
  char* base = nullptr;
  size_t off = 0;
  template <class T>
  void take(T*& p, size_t count) {
    if (base) p = reinterpret_cast<T*>(base + off);
    off = (off + count * sizeof(T) + 255) / 256 * 256;
  }
};

// The pieces both fitters have (dv.nv and dv.H set): the eight optimiser vectors, the
// reduce workgroups' partial dots and the result block.
template <class Dev>
void carve_fit_vectors(Carver& c, Dev& dv, int reduce_grid) {
  const size_t nv = dv.nv, H = dv.H;
  c.take(dv.x, nv), c.take(dv.d, nv), c.take(dv.g_c, nv), c.take(dv.g_t, nv), c.take(dv.beta_t, nv);
  c.take(dv.S, H * nv), c.take(dv.Y, H * nv), c.take(dv.wfix, nv);
  c.take(dv.dpart, (size_t)reduce_grid * kFitDotStride), c.take(dv.out, kFitOutWords);
}

class FitDriver {
 public:
  virtual ~FitDriver();
  FitDriver(const FitDriver&) = delete;
  FitDriver& operator=(const FitDriver&) = delete;

  // Mean loss at w (the model's device layout) and its gradient -> grad (same layout):
  // no standardisation, no L2 term.  Ends a fit in progress (its trial point is overwritten).
  double loss_grad(const float* w, float* grad, hipStream_t s);
  // Start a fit at w0 (nullptr: zeros).
  void begin(const float* w0, const FitOpts& o, hipStream_t s);
  // Evaluate until the fit ends or `max_accept` more steps were accepted; true: ended.
  bool run(int max_accept, hipStream_t s);
  // The current iterate, finalised, -> w_out in the model's device layout (synchronous).
  void current(float* w_out, hipStream_t s);
  // Copies of the optimiser's vectors into caller-owned device buffers (nullptr: skip):
  // x, d, g_c, g_t, beta_t, wfix are [nv], S and Y [hist][nv].  Synchronous, read-only.
  void read_state(float* x, float* d, float* g_c, float* g_t, float* beta_t, float* wfix, float* S, float* Y,
                  hipStream_t s);
  int n() const { return vectors().n; }
  int nv() const { return vectors().nv; }

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

 protected:
  // max_wg <= 0: per_cu workgroups per compute unit
  FitDriver(int max_wg, int per_cu);
  void end_fit() { loop_.stop(); }  // a new dataset: no fit in progress

  virtual int64_t rows() const = 0;  // of the loaded dataset; 0: none
  virtual FitVectors vectors() const = 0;
  // x = w0 in the solver's space (zeros without w0), trial point = x; raw: the weights themselves
  virtual void launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) = 0;
  // loss, gradient, f_t and the dots at the trial point -> the device result block
  virtual void launch_eval(double reg, int raw, hipStream_t s) = 0;
  virtual void launch_update(const FitStep& st, hipStream_t s) = 0;
  virtual void launch_finalize(int center, float* w_out, hipStream_t s) = 0;
  // the raw gradient of the last evaluation -> grad in the model's device layout
  virtual void export_grad(float* grad, hipStream_t s) = 0;

  int max_wg_ = 0, G_ = 1;

 private:
  void evaluate(double reg, int raw, hipStream_t s);
  double* pin_ = nullptr;
  FitLoop loop_;
  std::vector<double> eval_s_;
};

}  // namespace psx
