#include "fit_driver.h"

#include <chrono>
#include <stdexcept>

#include "solver.h"

namespace psx {

FitDriver::FitDriver(int max_wg, int per_cu) : max_wg_(max_wg) {
  if (max_wg_ <= 0) {
    int dev = 0;
    hipDeviceProp_t p;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    hip_check(hipGetDeviceProperties(&p, dev), "hipGetDeviceProperties");
    max_wg_ = per_cu * p.multiProcessorCount;
  }
  hip_check(hipHostMalloc(reinterpret_cast<void**>(&pin_), kFitOutWords * sizeof(double), hipHostMallocDefault),
            "hipHostMalloc(fit result block)");
}

FitDriver::~FitDriver() {
  if (pin_) (void)hipHostFree(pin_);
}

void FitDriver::evaluate(double reg, int raw, hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  launch_eval(reg, raw, s);
  hip_check(hipGetLastError(), "fit evaluation launch");
  hip_check(hipMemcpyAsync(pin_, vectors().out, kFitOutWords * sizeof(double), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(fit result block)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit evaluation)");
  eval_s_.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

double FitDriver::loss_grad(const float* w, float* grad, hipStream_t s) {
  if (rows() < 1) throw std::runtime_error("loss_grad: no dataset (set_data first)");
  if (!w || !grad) throw std::invalid_argument("loss_grad: null weights or gradient buffer");
  loop_.stop();  // the trial point is overwritten
  launch_begin(w, 1, /*raw=*/1, s);
  evaluate(0.0, /*raw=*/1, s);
  eval_s_.pop_back();
  export_grad(grad, s);
  hip_check(hipGetLastError(), "gradient export");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(loss_grad)");
  return pin_[kFitOutLoss];
}

void FitDriver::begin(const float* w0, const FitOpts& o, hipStream_t s) {
  if (rows() < 1) throw std::runtime_error("fit: no dataset (set_data first)");
  if (rows() < 2) throw std::invalid_argument("fit: at least 2 rows are needed");
  loop_.start(o, vectors().H);
  eval_s_.clear();
  launch_begin(w0, o.zero_const, /*raw=*/0, s);
  hip_check(hipGetLastError(), "fit_begin launch");
}

bool FitDriver::run(int max_accept, hipStream_t s) {
  return loop_.run(
      max_accept, pin_, [&](double reg) { evaluate(reg, 0, s); },
      [&](const FitStep& st) {
        launch_update(st, s);
        hip_check(hipGetLastError(), "fit_update launch");
      });
}

void FitDriver::current(float* w_out, hipStream_t s) {
  if (!loop_.begun()) throw std::runtime_error("fit: begin() first");
  if (!w_out) throw std::invalid_argument("fit: null output buffer");
  launch_finalize(loop_.opts().reg_param == 0.0, w_out, s);
  hip_check(hipGetLastError(), "fit_finalize launch");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_finalize)");
}

void FitDriver::read_state(float* x, float* d, float* g_c, float* g_t, float* beta_t, float* wfix, float* S, float* Y,
                           hipStream_t s) {
  const FitVectors v = vectors();
  if (!v.x) throw std::runtime_error("read_state: no dataset (set_data first)");
  const size_t nv = (size_t)v.nv, H = (size_t)v.H;
  const struct {
    float* dst;
    const float* src;
    size_t words;
  } parts[] = {{x, v.x, nv},           {d, v.d, nv},       {g_c, v.g_c, nv}, {g_t, v.g_t, nv},
               {beta_t, v.beta_t, nv}, {wfix, v.wfix, nv}, {S, v.S, H * nv}, {Y, v.Y, H * nv}};
  for (const auto& p : parts)
    if (p.dst)
      hip_check(hipMemcpyAsync(p.dst, p.src, p.words * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(fit state)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit state)");
}

}  // namespace psx
