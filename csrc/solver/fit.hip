#include "fit.h"

#include <climits>
#include <stdexcept>

#include "solver.h"

namespace psx {

// two 32-row tiles of up to 76 KB LDS in flight per CU
BatchFitter::BatchFitter(int K, int F, int FP, int hist, int max_wg) : FitDriver(max_wg, 2) {
  if (!fp_supported(FP)) throw std::invalid_argument("unsupported padded feature width " + std::to_string(FP));
  if (K < 2 || K > 16) throw std::invalid_argument("num classes must be in [2,16]");
  if (F < 1 || F > FP) throw std::invalid_argument("feature count must be in [1, padded width]");
  if (hist < 1 || hist > kMaxHist) throw std::invalid_argument("history must be in [1,16]");
  dv_.K = K;
  dv_.F = F;
  dv_.FP = FP;
  dv_.H = hist;
  dv_.n = K * FP + K;
  dv_.nv = (dv_.n + 63) / 64 * 64;
  auto layout = [&](Carver& c) {
    carve_fit_vectors(c, dv_, fit_reduce_grid(dv_.n));
    c.take(dv_.std_, FP), c.take(dv_.inv_std, FP), c.take(dv_.b_eff, 16);
    c.take(dv_.whi, (size_t)16 * FP), c.take(dv_.wlo, (size_t)16 * FP);
  };
  Carver size;
  layout(size);
  hip_check(hipMalloc(&ws_, size.off), "hipMalloc(fit workspace)");
  hip_check(hipMemset(ws_, 0, size.off), "hipMemset(fit workspace)");
  Carver place{static_cast<char*>(ws_)};
  layout(place);
  prepare_fit_kernels();
}

BatchFitter::~BatchFitter() {
  if (ws_) (void)hipFree(ws_);
  if (data_ws_) (void)hipFree(data_ws_);
}

void BatchFitter::set_data(const uint16_t* X, const int32_t* y, int64_t N, int64_t Npad, hipStream_t s) {
  if (N < 1 || N >= INT_MAX - 64) throw std::invalid_argument("row count must be in [1, 2^31 - 64)");
  if (Npad != (N + 31) / 32 * 32) throw std::invalid_argument("the rows must be padded to a multiple of 32");
  if (!X || !y) throw std::invalid_argument("null rows or labels");
  end_fit();
  dv_.X = X;
  dv_.y = y;
  dv_.N = (int)N;
  dv_.Npad = (int)Npad;
  const int ntiles = dv_.Npad / 32;
  G_ = ntiles < max_wg_ ? ntiles : max_wg_;
  if (data_ws_) {
    hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    hip_check(hipFree(data_ws_), "hipFree(fit partials)");
    data_ws_ = nullptr;
  }
  const size_t G = G_;
  auto layout = [&](Carver& c) {
    c.take(dv_.gpart, G * dv_.K * dv_.FP), c.take(dv_.part, G * 32), c.take(dv_.spart, G * 2 * dv_.FP);
  };
  Carver size;
  layout(size);
  hip_check(hipMalloc(&data_ws_, size.off), "hipMalloc(fit partials)");
  Carver place{static_cast<char*>(data_ws_)};
  layout(place);
  launch_fit_stats(dv_, G_, s);
  hip_check(hipGetLastError(), "fit_stats launch");
}

FitVectors BatchFitter::vectors() const {
  return {dv_.n, dv_.nv, dv_.H, dv_.x, dv_.d, dv_.g_c, dv_.g_t, dv_.beta_t, dv_.S, dv_.Y, dv_.wfix, dv_.out};
}

void BatchFitter::launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) {
  launch_fit_begin(dv_, w0, zero_const, raw, s);
}

void BatchFitter::launch_eval(double reg, int raw, hipStream_t s) {
  launch_fit_lossgrad(dv_, G_, s);
  launch_fit_reduce(dv_, G_, reg, raw, s);
}

void BatchFitter::launch_update(const FitStep& st, hipStream_t s) { launch_fit_update(dv_, st, s); }

void BatchFitter::launch_finalize(int center, float* w_out, hipStream_t s) {
  launch_fit_finalize(dv_, center, w_out, s);
}

void BatchFitter::export_grad(float* grad, hipStream_t s) {
  hip_check(hipMemcpyAsync(grad, dv_.g_t, (size_t)dv_.n * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(gradient)");
}

void BatchFitter::read_std(float* std_out, hipStream_t s) {
  hip_check(hipMemcpyAsync(std_out, dv_.std_, (size_t)dv_.FP * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(std)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(std)");
}

}  // namespace psx
