#include "wide_fit_many.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

#include "fit_driver.h"  // Carver
#include "solver.h"

namespace psx {

WideFitMany::WideFitMany(const WideFitDev& dv, int G) : dv_(dv), G_(G) {
  dv_.W = 4 * G;
  dv_.weff = dv_.R = dv_.gitem = dv_.part = dv_.bsum = nullptr;
  full_ = ((size_t)dv_.F + 1) * dv_.KP;
}

WideFitMany::~WideFitMany() { release(); }

void WideFitMany::release() {
  if (ws_) (void)hipFree(ws_);
  if (pin_) (void)hipHostFree(pin_);
  ws_ = pin_ = nullptr;
  M_ = D_ = NP_ = 0;
}

// Device and pinned memory for M jobs with D distinct held-out folds.
void WideFitMany::reserve(int M, int D) {
  if (M == M_ && D == D_) return;
  release();
  const int cap = capacity(), NP = (M + cap - 1) / cap;
  const size_t nv = dv_.nv, H = dv_.H, m = M, NB = wide_fit_reduce_grid(dv_.n), U1 = (size_t)dv_.U + 1, N = dv_.N;
  auto layout = [&](Carver& c) {
    c.take(x_, m * nv), c.take(d_, m * nv), c.take(g_c_, m * nv), c.take(g_t_, m * nv), c.take(beta_t_, m * nv);
    c.take(wfix_, m * nv), c.take(S_, m * H * nv), c.take(Y_, m * H * nv);
    c.take(dpart_, m * NB * kFitDotStride), c.take(out_, m * kWideManyOutWords);
    c.take(std_, D * U1), c.take(inv_std_, D * U1), c.take(wsum_, (size_t)D * 3);
    c.take(wm_, (size_t)NP * U1 * kWideLine), c.take(mm_, m);
    c.take(v_, N), c.take(ueff_, N), c.take(wpart_, (size_t)wide_fit_weights_grid(dv_.N) * 3), c.take(ho_, 1);
    c.take(dv_.R, N * kWideLine), c.take(dv_.gitem, ((size_t)dv_.n_items + 1) * kWideLine);
    c.take(dv_.part, (size_t)dv_.W * kWideManyPart), c.take(dv_.bsum, kWideLine);
  };
  Carver size;
  layout(size);
  hip_check(hipMalloc(&ws_, size.off), "hipMalloc(wide fit_many workspace)");
  Carver place{static_cast<char*>(ws_)};
  layout(place);
  Carver pin;
  auto pinned = [&](Carver& c) { c.take(steps_, m), c.take(live_, m), c.take(pout_, m * kWideManyOutWords); };
  pinned(pin);
  hip_check(hipHostMalloc(&pin_, pin.off, hipHostMallocDefault), "hipHostMalloc(wide fit_many steps and result blocks)");
  Carver pplace{static_cast<char*>(pin_)};
  pinned(pplace);
  void *sd = nullptr, *ld = nullptr;
  hip_check(hipHostGetDevicePointer(&sd, steps_, 0), "hipHostGetDevicePointer");
  hip_check(hipHostGetDevicePointer(&ld, live_, 0), "hipHostGetDevicePointer");
  steps_dev_ = static_cast<const FitStep*>(sd);
  live_dev_ = static_cast<const int*>(ld);
  M_ = M;
  D_ = D;
  NP_ = NP;
}

// Slots, descriptors, the row weights and the statistics of every distinct held-out fold.
void WideFitMany::place(const float* sw, const float* cw, const uint8_t* fold, const std::vector<FitManyJob>& jobs,
                        hipStream_t s) {
  const int M = (int)jobs.size();
  if (M < 1) throw std::invalid_argument("fit_many: no jobs");
  std::vector<int> holds;  // distinct, in order of first use
  sigma_of_.assign(M, 0);
  hold_.assign(M, -1);
  for (int m = 0; m < M; ++m) {
    const int h = jobs[m].holdout < 0 ? -1 : jobs[m].holdout;
    if (h > 255) throw std::invalid_argument("fit_many: fold ids are 0..255");
    if (h >= 0 && !fold) throw std::invalid_argument("fit_many: a held-out fold needs fold ids");
    if (jobs[m].reg_param < 0.0 || !(jobs[m].reg_param == jobs[m].reg_param))
      throw std::invalid_argument("fit_many: reg_param must be >= 0");
    auto it = std::find(holds.begin(), holds.end(), h);
    sigma_of_[m] = (int)(it - holds.begin());
    if (it == holds.end()) holds.push_back(h);
    hold_[m] = h;
  }
  reserve(M, (int)holds.size());
  fold_ = fold;
  const int KP = dv_.KP, cap = capacity(), nc = dv_.K == 1 ? 2 : dv_.K;
  const size_t nv = dv_.nv, H = dv_.H, NB = wide_fit_reduce_grid(dv_.n), U1 = (size_t)dv_.U + 1;
  std::vector<WideManyModel> mm(M);
  for (int m = 0; m < M; ++m) {
    const int pass = m / cap, slot = m % cap, sg = sigma_of_[m];
    WideManyModel& md = mm[m];
    md.dv = dv_;
    md.dv.x = x_ + m * nv, md.dv.d = d_ + m * nv, md.dv.g_c = g_c_ + m * nv, md.dv.g_t = g_t_ + m * nv;
    md.dv.beta_t = beta_t_ + m * nv, md.dv.wfix = wfix_ + m * nv;
    md.dv.S = S_ + m * H * nv, md.dv.Y = Y_ + m * H * nv;
    md.dv.dpart = dpart_ + m * NB * kFitDotStride;
    md.dv.out = out_ + (size_t)m * kWideManyOutWords;
    md.dv.std_ = std_ + (size_t)sg * U1, md.dv.inv_std = inv_std_ + (size_t)sg * U1;
    md.wsum = wsum_ + (size_t)sg * 3;
    md.w0 = jobs[m].w0;
    md.wm = wm_ + (size_t)pass * U1 * kWideLine;
    md.reg = jobs[m].reg_param;
    md.col0 = slot * KP;
  }
  // empty slots and the classes >= K of a slot gather zeros
  hip_check(hipMemsetAsync(wm_, 0, (size_t)NP_ * U1 * kWideLine * 4, s), "hipMemsetAsync(fit_many trial weights)");
  hip_check(hipMemcpyAsync(mm_, mm.data(), mm.size() * sizeof(WideManyModel), hipMemcpyHostToDevice, s),
            "hipMemcpyAsync(fit_many models)");
  WideFitWeightsDev wd{};
  wd.sw = sw, wd.fold = fold, wd.ueff = ueff_, wd.wpart = wpart_, wd.ho = ho_;
  for (int c = 0; c < 16; ++c) wd.cw[c] = c < nc ? (cw ? cw[c] : 1.f) : 0.f;
  launch_wide_many_weights(dv_, sw, wd.cw, v_, s);
  for (size_t i = 0; i < holds.size(); ++i) {  // the weighted fitter's kernels, unchanged; ueff_ is their scratch
    WideFitDev sdv = dv_;
    sdv.std_ = std_ + i * U1, sdv.inv_std = inv_std_ + i * U1;
    wd.holdout = holds[i];
    wd.wsum = wsum_ + i * 3;
    launch_wide_fit_weights(sdv, wd, s);
    launch_wide_fit_stats_w(sdv, wd, s);
  }
  hip_check(hipGetLastError(), "wide fit_many statistics launch");
  // the host vectors end here; the statistics passes stay out of the first round's time
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_many models)");
  for (int m = 0; m < M; ++m) {
    live_[m] = 1;
    steps_[m] = FitStep{};
  }
  round_s_.clear();
}

// One evaluation of every live job: per pass the row pass, the column pass, the
// reduction and its jobs' dots, then one copy of all result blocks and one wait.
void WideFitMany::round(int raw, hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  const int cap = capacity();
  const size_t U1 = (size_t)dv_.U + 1;
  for (int p = 0; p < NP_; ++p) {
    const int m0 = p * cap, cnt = std::min(cap, M_ - m0);
    WideManyPass ps{};
    for (int i = 0; i < kWideLine; ++i) ps.hold[i] = -1;
    for (int i = 0; i < cnt; ++i) {
      ps.hold[i] = hold_[m0 + i];
      if (live_[m0 + i]) ps.live |= 1u << i;
    }
    if (!ps.live) continue;
    ps.dv = dv_;
    ps.v = v_, ps.fold = fold_;
    ps.wm = wm_ + (size_t)p * U1 * kWideLine;
    launch_wide_many_eval(ps, G_, s);
    launch_wide_many_reduce(mm_, live_dev_, m0, cnt, dv_.n, raw, s);
  }
  hip_check(hipGetLastError(), "wide fit_many evaluation launch");
  hip_check(hipMemcpyAsync(pout_, out_, (size_t)M_ * kWideManyOutWords * sizeof(double), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(fit_many result blocks)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_many evaluation)");
  round_s_.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

std::vector<FitManyResult> WideFitMany::fit(const float* sample_weight, const float* class_weight,
                                            const uint8_t* fold, const std::vector<FitManyJob>& jobs, const FitOpts& o,
                                            float* w_out, float* std_out, hipStream_t s) {
  if (dv_.N < 2) throw std::invalid_argument("fit: at least 2 rows are needed");
  if (!w_out || !std_out) throw std::invalid_argument("fit_many: null output buffer");
  const int M = (int)jobs.size();
  loops_.assign(M, FitLoop{});
  for (int m = 0; m < M; ++m) {  // (validates the options before any launch)
    FitOpts om = o;
    om.reg_param = jobs[m].reg_param;
    loops_[m].start(om, dv_.H);
  }
  place(sample_weight, class_weight, fold, jobs, s);
  launch_wide_many_begin(mm_, M, dv_.n, o.zero_const, /*raw=*/0, s);
  hip_check(hipGetLastError(), "wide fit_many begin launch");
  for (;;) {
    bool any = false;
    for (int m = 0; m < M; ++m) any |= (live_[m] = loops_[m].wants_eval() ? 1 : 0) != 0;
    if (!any) break;
    round(0, s);
    bool act = false;
    for (int m = 0; m < M; ++m) {
      steps_[m].action = kActNone;
      if (!live_[m]) continue;
      loops_[m].step(pout_ + (size_t)m * kWideManyOutWords, [&](const FitStep& st) {
        steps_[m] = st;
        act = true;
      });
    }
    if (act) {
      launch_wide_many_update(mm_, steps_dev_, M, dv_.n, s);
      hip_check(hipGetLastError(), "wide fit_many update launch");
    }
  }
  launch_wide_many_finalize(mm_, M, dv_.U, w_out, s);
  hip_check(hipGetLastError(), "wide fit_many finalize launch");
  const size_t U1 = (size_t)dv_.U + 1;
  for (int m = 0; m < M && dv_.U > 0; ++m)
    hip_check(hipMemcpyAsync(std_out + (size_t)m * dv_.U, std_ + (size_t)sigma_of_[m] * U1, (size_t)dv_.U * 4,
                             hipMemcpyDeviceToDevice, s),
              "hipMemcpyAsync(std)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_many finalize)");
  std::vector<FitManyResult> res(M);
  for (int m = 0; m < M; ++m) {
    const FitLoop& l = loops_[m];
    res[m] = {l.ctrl().f_c, l.log_loss(), l.ctrl().nacc, l.ctrl().evals, l.ctrl().ls_fail, l.reason(), l.history()};
  }
  return res;
}

void WideFitMany::loss_grad(const float* sample_weight, const float* class_weight, const uint8_t* fold,
                            const std::vector<FitManyJob>& jobs, float* grads, std::vector<double>& losses,
                            std::vector<double>& holdout_losses, hipStream_t s) {
  if (!grads) throw std::invalid_argument("loss_grad_many: null gradient buffer");
  for (const auto& j : jobs)
    if (!j.w0) throw std::invalid_argument("loss_grad_many: null weights");
  place(sample_weight, class_weight, fold, jobs, s);
  const int M = (int)jobs.size();
  launch_wide_many_begin(mm_, M, dv_.n, 1, /*raw=*/1, s);
  hip_check(hipGetLastError(), "wide fit_many begin launch");
  round(1, s);
  hip_check(hipMemsetAsync(grads, 0, (size_t)M * full_ * 4, s), "hipMemsetAsync(gradients)");
  launch_wide_many_scatter(mm_, M, dv_.n, grads, s);
  hip_check(hipGetLastError(), "wide fit_many scatter launch");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(loss_grad_many)");
  losses.resize(M);
  holdout_losses.resize(M);
  for (int m = 0; m < M; ++m) {
    losses[m] = pout_[(size_t)m * kWideManyOutWords + kFitOutLoss];
    holdout_losses[m] = pout_[(size_t)m * kWideManyOutWords + kFitOutWords];
  }
}

}  // namespace psx
