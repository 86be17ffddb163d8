#include "fit.h"

#include <chrono>
#include <climits>
#include <cmath>
#include <stdexcept>

#include "solver.h"

namespace psx {

static size_t fit_align(size_t v) { return (v + 255) / 256 * 256; }

BatchFitter::BatchFitter(int K, int F, int FP, int hist, int max_wg) : max_wg_(max_wg) {
  if (!fp_supported(FP)) throw std::invalid_argument("unsupported padded feature width " + std::to_string(FP));
  if (K < 2 || K > 16) throw std::invalid_argument("num classes must be in [2,16]");
  if (F < 1 || F > FP) throw std::invalid_argument("feature count must be in [1, padded width]");
  if (hist < 1 || hist > kMaxHist) throw std::invalid_argument("history must be in [1,16]");
  if (max_wg_ <= 0) {
    int dev = 0;
    hipDeviceProp_t p;
    hip_check(hipGetDevice(&dev), "hipGetDevice");
    hip_check(hipGetDeviceProperties(&p, dev), "hipGetDeviceProperties");
    max_wg_ = 2 * p.multiProcessorCount;  // two 32-row tiles of up to 76 KB LDS in flight per CU
  }
  dv_.K = K;
  dv_.F = F;
  dv_.FP = FP;
  dv_.H = hist;
  dv_.n = K * FP + K;
  dv_.nv = (dv_.n + 63) / 64 * 64;
  const size_t nv = dv_.nv, H = hist;
  size_t off = 0;
  auto take = [&](size_t bytes) {
    const size_t o = off;
    off = fit_align(off + bytes);
    return o;
  };
  const size_t o_x = take(nv * 4), o_d = take(nv * 4), o_gc = take(nv * 4), o_gt = take(nv * 4), o_bt = take(nv * 4);
  const size_t o_S = take(H * nv * 4), o_Y = take(H * nv * 4), o_wfix = take(nv * 4);
  const size_t o_std = take((size_t)FP * 4), o_istd = take((size_t)FP * 4), o_beff = take(16 * 4);
  const size_t o_whi = take((size_t)16 * FP * 2), o_wlo = take((size_t)16 * FP * 2);
  const size_t o_dpart = take((size_t)fit_reduce_grid(dv_.n) * kFitDotStride * 8);
  const size_t o_out = take((size_t)kFitOutWords * 8);
  hip_check(hipMalloc(&ws_, off), "hipMalloc(fit workspace)");
  hip_check(hipMemset(ws_, 0, off), "hipMemset(fit workspace)");
  char* b = static_cast<char*>(ws_);
  dv_.x = reinterpret_cast<float*>(b + o_x);
  dv_.d = reinterpret_cast<float*>(b + o_d);
  dv_.g_c = reinterpret_cast<float*>(b + o_gc);
  dv_.g_t = reinterpret_cast<float*>(b + o_gt);
  dv_.beta_t = reinterpret_cast<float*>(b + o_bt);
  dv_.S = reinterpret_cast<float*>(b + o_S);
  dv_.Y = reinterpret_cast<float*>(b + o_Y);
  dv_.wfix = reinterpret_cast<float*>(b + o_wfix);
  dv_.std_ = reinterpret_cast<float*>(b + o_std);
  dv_.inv_std = reinterpret_cast<float*>(b + o_istd);
  dv_.b_eff = reinterpret_cast<float*>(b + o_beff);
  dv_.whi = reinterpret_cast<uint16_t*>(b + o_whi);
  dv_.wlo = reinterpret_cast<uint16_t*>(b + o_wlo);
  dv_.dpart = reinterpret_cast<double*>(b + o_dpart);
  dv_.out = reinterpret_cast<double*>(b + o_out);
  hip_check(hipHostMalloc(reinterpret_cast<void**>(&pin_), kFitOutWords * sizeof(double), hipHostMallocDefault),
            "hipHostMalloc(fit result block)");
  prepare_fit_kernels();
}

BatchFitter::~BatchFitter() {
  if (ws_) (void)hipFree(ws_);
  if (data_ws_) (void)hipFree(data_ws_);
  if (pin_) (void)hipHostFree(pin_);
}

void BatchFitter::set_data(const uint16_t* X, const int32_t* y, int64_t N, int64_t Npad, hipStream_t s) {
  if (N < 1 || N >= INT_MAX - 64) throw std::invalid_argument("row count must be in [1, 2^31 - 64)");
  if (Npad != (N + 31) / 32 * 32) throw std::invalid_argument("the rows must be padded to a multiple of 32");
  if (!X || !y) throw std::invalid_argument("null rows or labels");
  loop_.stop();
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
  const size_t G = G_, KF = (size_t)dv_.K * dv_.FP;
  const size_t b_gpart = fit_align(G * KF * 4), b_part = fit_align(G * 32 * 4), b_spart = fit_align(G * 2 * dv_.FP * 8);
  hip_check(hipMalloc(&data_ws_, b_gpart + b_part + b_spart), "hipMalloc(fit partials)");
  char* b = static_cast<char*>(data_ws_);
  dv_.gpart = reinterpret_cast<float*>(b);
  dv_.part = reinterpret_cast<float*>(b + b_gpart);
  dv_.spart = reinterpret_cast<double*>(b + b_gpart + b_part);
  launch_fit_stats(dv_, G_, s);
  hip_check(hipGetLastError(), "fit_stats launch");
}

void BatchFitter::evaluate(double reg, int raw, hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  launch_fit_lossgrad(dv_, G_, s);
  launch_fit_reduce(dv_, G_, reg, raw, s);
  hip_check(hipGetLastError(), "fit evaluation launch");
  hip_check(hipMemcpyAsync(pin_, dv_.out, kFitOutWords * sizeof(double), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(fit result block)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit evaluation)");
  eval_s_.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

double BatchFitter::loss_grad(const float* w, float* grad, hipStream_t s) {
  if (!dv_.X) throw std::runtime_error("loss_grad: no dataset (set_data first)");
  if (!w || !grad) throw std::invalid_argument("loss_grad: null weights or gradient buffer");
  loop_.stop();  // the trial fragments are overwritten
  launch_fit_begin(dv_, w, 1, /*raw=*/1, s);
  evaluate(0.0, /*raw=*/1, s);
  eval_s_.pop_back();
  hip_check(hipMemcpyAsync(grad, dv_.g_t, (size_t)dv_.n * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(gradient)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(loss_grad)");
  return pin_[kFitOutLoss];
}

void BatchFitter::begin(const float* w0, const FitOpts& o, hipStream_t s) {
  if (!dv_.X) throw std::runtime_error("fit: no dataset (set_data first)");
  if (dv_.N < 2) throw std::invalid_argument("fit: at least 2 rows are needed");
  loop_.start(o, dv_.H);
  eval_s_.clear();
  launch_fit_begin(dv_, w0, o.zero_const, /*raw=*/0, s);
  hip_check(hipGetLastError(), "fit_begin launch");
}

bool BatchFitter::run(int max_accept, hipStream_t s) {
  return loop_.run(
      max_accept, pin_, [&](double reg) { evaluate(reg, 0, s); },
      [&](const FitStep& st) {
        launch_fit_update(dv_, st, s);
        hip_check(hipGetLastError(), "fit_update launch");
      });
}

void BatchFitter::current(float* w_out, hipStream_t s) {
  if (!loop_.begun()) throw std::runtime_error("fit: begin() first");
  if (!w_out) throw std::invalid_argument("fit: null output buffer");
  launch_fit_finalize(dv_, loop_.opts().reg_param == 0.0, w_out, s);
  hip_check(hipGetLastError(), "fit_finalize launch");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_finalize)");
}

void BatchFitter::read_std(float* std_out, hipStream_t s) {
  hip_check(hipMemcpyAsync(std_out, dv_.std_, (size_t)dv_.FP * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(std)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(std)");
}

void BatchFitter::read_state(float* x, float* d, float* g_c, float* g_t, float* beta_t, float* wfix, float* S, float* Y,
                             hipStream_t s) {
  const size_t nv = (size_t)dv_.nv, H = (size_t)dv_.H;
  const struct {
    float* dst;
    const float* src;
    size_t words;
  } parts[] = {{x, dv_.x, nv},           {d, dv_.d, nv},       {g_c, dv_.g_c, nv}, {g_t, dv_.g_t, nv},
               {beta_t, dv_.beta_t, nv}, {wfix, dv_.wfix, nv}, {S, dv_.S, H * nv}, {Y, dv_.Y, H * nv}};
  for (const auto& p : parts)
    if (p.dst)
      hip_check(hipMemcpyAsync(p.dst, p.src, p.words * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(fit state)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit state)");
}

}  // namespace psx
