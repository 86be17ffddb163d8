#include "fit_f32.h"

#include <climits>
#include <stdexcept>
#include <string>

#include "solver.h"

namespace psx {

F32BatchFitter::F32BatchFitter(int K, int F, int FP, int hist, int max_wg, bool centred)
    : FitDriver(max_wg, fit_f32_wg_per_cu(fit_f32_fp_supported(FP) ? FP : kFitF32MaxFP)), centred_(centred) {
  if (!fit_f32_fp_supported(FP))
    throw std::invalid_argument("fp32 rows: padded width " + std::to_string(FP) +
                                " is not 128, 256, 512 or 1024 (two tile images of wider rows do not fit the LDS)");
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
    c.take(fd_.center, FP);
  };
  Carver size;
  layout(size);
  hip_check(hipMalloc(&ws_, size.off), "hipMalloc(fp32 fit workspace)");
  hip_check(hipMemset(ws_, 0, size.off), "hipMemset(fp32 fit workspace)");
  Carver place{static_cast<char*>(ws_)};
  layout(place);
  prepare_fit_f32_kernels();
}

F32BatchFitter::~F32BatchFitter() {
  if (ws_) (void)hipFree(ws_);
  if (data_ws_) (void)hipFree(data_ws_);
}

void F32BatchFitter::set_data(const float* X, const int32_t* y, int64_t N, int64_t Npad, bool stats, hipStream_t s) {
  if (N < 1 || N >= INT_MAX - 64) throw std::invalid_argument("row count must be in [1, 2^31 - 64)");
  if (Npad != (N + 31) / 32 * 32) throw std::invalid_argument("the rows must be padded to a multiple of 32");
  if (!X || !y) throw std::invalid_argument("null rows or labels");
  end_fit();
  fd_.X = X;
  dv_.y = y;
  dv_.N = (int)N;
  dv_.Npad = (int)Npad;
  const int ntiles = dv_.Npad / 32;
  G_ = ntiles < max_wg_ ? ntiles : max_wg_;
  if (data_ws_) {
    hip_check(hipStreamSynchronize(s), "hipStreamSynchronize");
    hip_check(hipFree(data_ws_), "hipFree(fp32 fit partials)");
    data_ws_ = nullptr;
  }
  const size_t Gs = G_;
  auto layout = [&](Carver& c) {  // every workgroup writes its whole slice of each: no clearing
    c.take(dv_.gpart, Gs * dv_.K * dv_.FP), c.take(dv_.part, Gs * 32);
    c.take(dv_.spart, Gs * 2 * dv_.FP), c.take(fd_.mmpart, Gs * 2 * dv_.FP);
  };
  Carver size;
  layout(size);
  hip_check(hipMalloc(&data_ws_, size.off), "hipMalloc(fp32 fit partials)");
  Carver place{static_cast<char*>(data_ws_)};
  layout(place);
  have_stats_ = have_center_ = stats;
  if (stats) {
    launch_fit_stats_f32(dv_, fd_, G_, s);
    hip_check(hipGetLastError(), "fit_stats_f32 launch");
  }
}

void F32BatchFitter::score(const float* w, const ScoreOut& o, hipStream_t s) {
  if (!fd_.X) throw std::runtime_error("score: no dataset (set_data first)");
  if (!w || !o.pred || !o.conf || !o.oor) throw std::invalid_argument("score: null weights or output buffers");
  if (o.hist) throw std::invalid_argument("score: the fp32-row scorer has no score histogram");
  need_center("score");
  end_fit();
  launch_begin(w, 1, /*raw=*/1, s);  // the weights' fragments and intercepts
  launch_score_f32(dv_, fd_, G_, centred_, o, s);
  hip_check(hipGetLastError(), "score_f32 launch");
}

void F32BatchFitter::need_center(const char* what) const {
  if (centred_ && !have_center_)
    throw std::runtime_error(std::string(what) + ": the centred mode needs the dataset's statistics or set_center");
}

void F32BatchFitter::set_center(const float* c, hipStream_t s) {
  if (!fd_.X) throw std::runtime_error("set_center: no dataset (set_data first)");
  if (!c) throw std::invalid_argument("set_center: null centre");
  end_fit();
  hip_check(hipMemcpyAsync(fd_.center, c, (size_t)dv_.FP * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(centre)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(centre)");  // the caller's buffer may go
  have_center_ = true;
}

void F32BatchFitter::read_center(float* c_out, hipStream_t s) {
  if (!have_center_) throw std::runtime_error("read_center: no statistics and no set_center");
  hip_check(hipMemcpyAsync(c_out, fd_.center, (size_t)dv_.FP * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(centre)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(centre)");
}

double F32BatchFitter::loss_grad_centred(const float* w, float* grad, hipStream_t s) {
  if (!centred_) throw std::runtime_error("loss_grad_centred: the fitter was built without the centred mode");
  struct Restore {
    bool& v;
    ~Restore() { v = true; }
  } restore{export_raw_};
  export_raw_ = false;
  return loss_grad(w, grad, s);
}

std::vector<float> F32BatchFitter::time_launches(const float* w, int reps, hipStream_t s) {
  if (!fd_.X || !w || reps < 1) throw std::invalid_argument("time_launches: a dataset, weights and reps >= 1");
  need_center("time_launches");
  end_fit();
  launch_begin(w, 1, /*raw=*/1, s);
  hipEvent_t ev[3];
  for (auto& e : ev) hip_check(hipEventCreate(&e), "hipEventCreate");
  std::vector<float> ms(2, 0.f);
  for (int r = 0; r < reps; ++r) {
    hip_check(hipEventRecord(ev[0], s), "hipEventRecord");
    launch_fit_lossgrad_f32(dv_, fd_, G_, centred_, s);
    hip_check(hipEventRecord(ev[1], s), "hipEventRecord");
    launch_fit_reduce(dv_, G_, 0.0, /*raw=*/1, s);
    hip_check(hipEventRecord(ev[2], s), "hipEventRecord");
    hip_check(hipEventSynchronize(ev[2]), "hipEventSynchronize");
    for (int k = 0; k < 2; ++k) {
      float t = 0.f;
      hip_check(hipEventElapsedTime(&t, ev[k], ev[k + 1]), "hipEventElapsedTime");
      ms[k] += t / (float)reps;
    }
  }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return ms;
}

FitVectors F32BatchFitter::vectors() const {
  return {dv_.n, dv_.nv, dv_.H, dv_.x, dv_.d, dv_.g_c, dv_.g_t, dv_.beta_t, dv_.S, dv_.Y, dv_.wfix, dv_.out};
}

void F32BatchFitter::launch_begin(const float* w0, int zero_const, int raw, hipStream_t s) {
  if (!raw && !have_stats_) throw std::runtime_error("fit: the dataset was loaded without statistics");
  need_center("evaluation");
  launch_fit_begin(dv_, w0, zero_const, raw, s);
  if (centred_) launch_fit_center_begin(dv_, fd_, w0, raw, s);  // the intercepts become b'
}

void F32BatchFitter::launch_eval(double reg, int raw, hipStream_t s) {
  launch_fit_lossgrad_f32(dv_, fd_, G_, centred_, s);
  launch_fit_reduce(dv_, G_, reg, raw, s);
}

void F32BatchFitter::launch_update(const FitStep& st, hipStream_t s) { launch_fit_update(dv_, st, s); }

void F32BatchFitter::launch_finalize(int center, float* w_out, hipStream_t s) {
  launch_fit_finalize(dv_, center, w_out, s);
  if (centred_) launch_fit_center_finalize(dv_, fd_, w_out, s);  // b' -> the raw intercepts
}

void F32BatchFitter::export_grad(float* grad, hipStream_t s) {
  if (centred_ && export_raw_) return launch_fit_center_grad(dv_, fd_, grad, s);
  hip_check(hipMemcpyAsync(grad, dv_.g_t, (size_t)dv_.n * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(gradient)");
}

void F32BatchFitter::read_std(float* std_out, hipStream_t s) {
  if (!have_stats_) throw std::runtime_error("read_std: the dataset was loaded without statistics");
  hip_check(hipMemcpyAsync(std_out, dv_.std_, (size_t)dv_.FP * 4, hipMemcpyDeviceToDevice, s), "hipMemcpyAsync(std)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(std)");
}

}  // namespace psx
