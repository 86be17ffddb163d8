#include "fit_many.h"

#include <algorithm>
#include <chrono>
#include <stdexcept>

#include "fit_driver.h"  // Carver
#include "solver.h"

namespace psx {

FitMany::FitMany(const FitDev& dv, const FitWeightsDev& wd, int G) : dv_(dv), wd_(wd), G_(G) {
  prepare_fit_many_kernels();
  prepare_fit_weighted_kernels();
}

FitMany::~FitMany() { release(); }

void FitMany::release() {
  if (ws_) (void)hipFree(ws_);
  if (pin_) (void)hipHostFree(pin_);
  ws_ = pin_ = nullptr;
  M_ = D_ = NP_ = 0;
}

// Device and pinned memory for M jobs with D distinct held-out folds.
void FitMany::reserve(int M, int D) {
  if (M == M_ && D == D_) return;
  release();
  const int cap = capacity(), GP = many_groups(dv_.FP, many_kp(dv_.K));
  const int NP = (M + cap - 1) / cap;
  const size_t nv = dv_.nv, H = dv_.H, FP = dv_.FP, m = M, NB = fit_reduce_grid(dv_.n), ng = (size_t)NP * GP;
  auto layout = [&](Carver& c) {
    c.take(x_, m * nv), c.take(d_, m * nv), c.take(g_c_, m * nv), c.take(g_t_, m * nv), c.take(beta_t_, m * nv);
    c.take(wfix_, m * nv), c.take(S_, m * H * nv), c.take(Y_, m * H * nv);
    c.take(dpart_, m * NB * kFitDotStride), c.take(out_, m * kManyOutWords);
    c.take(std_, D * FP), c.take(inv_std_, D * FP), c.take(wsum_, (size_t)D * 2);
    c.take(whi_, ng * 16 * FP), c.take(wlo_, ng * 16 * FP), c.take(b_eff_, ng * 16), c.take(hold_, (size_t)NP * cap);
    c.take(mm_, m);
    c.take(gpart_, (size_t)G_ * cap * dv_.K * FP), c.take(part_, (size_t)G_ * cap * 32);
  };
  Carver size;
  layout(size);
  hip_check(hipMalloc(&ws_, size.off), "hipMalloc(fit_many workspace)");
  Carver place{static_cast<char*>(ws_)};
  layout(place);
  Carver pin;
  auto pinned = [&](Carver& c) { c.take(steps_, m), c.take(live_, m), c.take(pout_, m * kManyOutWords); };
  pinned(pin);
  hip_check(hipHostMalloc(&pin_, pin.off, hipHostMallocDefault), "hipHostMalloc(fit_many steps and result blocks)");
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

// Slots, descriptors and the statistics of every distinct held-out fold.
void FitMany::place(const float* sw, const float* cw, const uint8_t* fold, const std::vector<FitManyJob>& jobs,
                    hipStream_t s) {
  if (!dv_.X) throw std::runtime_error("fit_many: no dataset (set_data first)");
  const int M = (int)jobs.size();
  if (M < 1) throw std::invalid_argument("fit_many: no jobs");
  std::vector<int> holds;  // distinct, in order of first use
  sigma_of_.assign(M, 0);
  for (int m = 0; m < M; ++m) {
    const int h = jobs[m].holdout < 0 ? -1 : jobs[m].holdout;
    if (h > 255) throw std::invalid_argument("fit_many: fold ids are 0..255");
    if (h >= 0 && !fold) throw std::invalid_argument("fit_many: a held-out fold needs fold ids");
    if (jobs[m].reg_param < 0.0 || !(jobs[m].reg_param == jobs[m].reg_param))
      throw std::invalid_argument("fit_many: reg_param must be >= 0");
    auto it = std::find(holds.begin(), holds.end(), h);
    sigma_of_[m] = (int)(it - holds.begin());
    if (it == holds.end()) holds.push_back(h);
  }
  reserve(M, (int)holds.size());
  wd_.sw = sw;
  wd_.fold = fold;
  for (int c = 0; c < 16; ++c) wd_.cw[c] = c < dv_.K ? (cw ? cw[c] : 1.f) : 0.f;

  const int K = dv_.K, FP = dv_.FP, KP = many_kp(K), SPG = 16 / KP, cap = capacity();
  const size_t nv = dv_.nv, H = dv_.H, NB = fit_reduce_grid(dv_.n);
  std::vector<FitManyModel> mm(M);
  std::vector<int> hold((size_t)NP_ * cap, -1);
  for (int m = 0; m < M; ++m) {
    const int pass = m / cap, slot = m % cap, group = pass * (cap / SPG) + slot / SPG, sg = sigma_of_[m];
    FitManyModel& md = mm[m];
    md.dv = dv_;
    md.dv.x = x_ + m * nv, md.dv.d = d_ + m * nv, md.dv.g_c = g_c_ + m * nv, md.dv.g_t = g_t_ + m * nv;
    md.dv.beta_t = beta_t_ + m * nv, md.dv.wfix = wfix_ + m * nv;
    md.dv.S = S_ + m * H * nv, md.dv.Y = Y_ + m * H * nv;
    md.dv.dpart = dpart_ + m * NB * kFitDotStride;
    md.dv.out = out_ + (size_t)m * kManyOutWords;
    md.dv.std_ = std_ + (size_t)sg * FP, md.dv.inv_std = inv_std_ + (size_t)sg * FP;
    md.dv.whi = whi_ + (size_t)group * 16 * FP, md.dv.wlo = wlo_ + (size_t)group * 16 * FP;
    md.dv.b_eff = b_eff_ + (size_t)group * 16;
    md.dv.gpart = gpart_ + (size_t)slot * K * FP;
    md.dv.part = part_ + (size_t)slot * 32;
    md.wsum = wsum_ + (size_t)sg * 2;
    md.w0 = jobs[m].w0;
    md.reg = jobs[m].reg_param;
    md.col0 = (slot % SPG) * KP;
    md.gstride = cap * K * FP;
    md.pstride = cap * 32;
    hold[m] = holds[sg];
  }
  // empty slots and the classes >= K of a slot multiply zero fragments
  const size_t ng = (size_t)NP_ * (cap / SPG);
  hip_check(hipMemsetAsync(whi_, 0, ng * 16 * FP * 2, s), "hipMemsetAsync(fit_many fragments)");
  hip_check(hipMemsetAsync(wlo_, 0, ng * 16 * FP * 2, s), "hipMemsetAsync(fit_many fragments)");
  hip_check(hipMemsetAsync(b_eff_, 0, ng * 16 * 4, s), "hipMemsetAsync(fit_many intercepts)");
  hip_check(hipMemcpyAsync(mm_, mm.data(), mm.size() * sizeof(FitManyModel), hipMemcpyHostToDevice, s),
            "hipMemcpyAsync(fit_many models)");
  hip_check(hipMemcpyAsync(hold_, hold.data(), hold.size() * sizeof(int), hipMemcpyHostToDevice, s),
            "hipMemcpyAsync(fit_many held-out folds)");
  for (size_t i = 0; i < holds.size(); ++i) {
    FitDev sdv = dv_;
    sdv.std_ = std_ + i * FP, sdv.inv_std = inv_std_ + i * FP;
    FitWeightsDev swd = wd_;
    swd.holdout = holds[i];
    swd.wsum = wsum_ + i * 2;
    launch_fit_stats_w(sdv, swd, G_, s);
    hip_check(hipGetLastError(), "fit_stats_w launch");
  }
  // the host vectors end here; the statistics passes stay out of the first round's time
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_many models)");
  for (int m = 0; m < M; ++m) {
    live_[m] = 1;
    steps_[m] = FitStep{};
  }
  round_s_.clear();
}

// One evaluation of every live job: per pass the tile walk, its reduction and its jobs'
// dots, then one copy of all result blocks and one wait.
void FitMany::round(int raw, hipStream_t s) {
  const auto t0 = std::chrono::steady_clock::now();
  const int KP = many_kp(dv_.K), SPG = 16 / KP, cap = capacity(), GP = cap / SPG;
  const int ntiles = dv_.Npad >> 5, nfw = ntiles < G_ ? ntiles : G_;
  for (int p = 0; p < NP_; ++p) {
    const int m0 = p * cap, cnt = std::min(cap, M_ - m0);
    unsigned gmask = 0;
    for (int i = 0; i < cnt; ++i)
      if (live_[m0 + i]) gmask |= 1u << (i / SPG);
    if (!gmask) continue;
    FitManyPass ps{};
    ps.X = dv_.X, ps.y = dv_.y, ps.N = dv_.N, ps.Npad = dv_.Npad, ps.K = dv_.K;
    ps.sw = wd_.sw, ps.fold = wd_.fold;
    for (int c = 0; c < 16; ++c) ps.cw[c] = wd_.cw[c];
    ps.whi = whi_ + (size_t)p * GP * 16 * dv_.FP, ps.wlo = wlo_ + (size_t)p * GP * 16 * dv_.FP;
    ps.b_eff = b_eff_ + (size_t)p * GP * 16;
    ps.hold = hold_ + (size_t)p * cap;
    ps.gpart = gpart_, ps.part = part_;
    ps.gmask = gmask;
    launch_fit_many_lossgrad(ps, dv_.FP, G_, s);
    launch_fit_many_reduce(mm_, live_dev_, m0, cnt, dv_.n, nfw, raw, s);
  }
  hip_check(hipGetLastError(), "fit_many evaluation launch");
  hip_check(hipMemcpyAsync(pout_, out_, (size_t)M_ * kManyOutWords * sizeof(double), hipMemcpyDeviceToHost, s),
            "hipMemcpyAsync(fit_many result blocks)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_many evaluation)");
  round_s_.push_back(std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

std::vector<FitManyResult> FitMany::fit(const float* sample_weight, const float* class_weight, const uint8_t* fold,
                                        const std::vector<FitManyJob>& jobs, const FitOpts& o, float* w_out,
                                        float* std_out, hipStream_t s) {
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
  launch_fit_many_begin(mm_, M, dv_.n, o.zero_const, /*raw=*/0, s);
  hip_check(hipGetLastError(), "fit_many_begin launch");
  for (;;) {
    bool any = false;
    for (int m = 0; m < M; ++m) any |= (live_[m] = loops_[m].wants_eval() ? 1 : 0) != 0;
    if (!any) break;
    round(0, s);
    bool act = false;
    for (int m = 0; m < M; ++m) {
      steps_[m].action = kActNone;
      if (!live_[m]) continue;
      loops_[m].step(pout_ + (size_t)m * kManyOutWords, [&](const FitStep& st) {
        steps_[m] = st;
        act = true;
      });
    }
    if (act) {
      launch_fit_many_update(mm_, steps_dev_, M, dv_.n, s);
      hip_check(hipGetLastError(), "fit_many_update launch");
    }
  }
  launch_fit_many_finalize(mm_, M, dv_.FP, w_out, s);
  hip_check(hipGetLastError(), "fit_many_finalize launch");
  for (int m = 0; m < M; ++m)
    hip_check(hipMemcpyAsync(std_out + (size_t)m * dv_.FP, std_ + (size_t)sigma_of_[m] * dv_.FP, (size_t)dv_.FP * 4,
                             hipMemcpyDeviceToDevice, s),
              "hipMemcpyAsync(std)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(fit_many_finalize)");
  std::vector<FitManyResult> res(M);
  for (int m = 0; m < M; ++m) {
    const FitLoop& l = loops_[m];
    res[m] = {l.ctrl().f_c, l.log_loss(), l.ctrl().nacc, l.ctrl().evals, l.ctrl().ls_fail, l.reason(), l.history()};
  }
  return res;
}

void FitMany::loss_grad(const float* sample_weight, const float* class_weight, const uint8_t* fold,
                        const std::vector<FitManyJob>& jobs, float* grads, std::vector<double>& losses,
                        std::vector<double>& holdout_losses, hipStream_t s) {
  if (!grads) throw std::invalid_argument("loss_grad_many: null gradient buffer");
  for (const auto& j : jobs)
    if (!j.w0) throw std::invalid_argument("loss_grad_many: null weights");
  place(sample_weight, class_weight, fold, jobs, s);
  const int M = (int)jobs.size();
  launch_fit_many_begin(mm_, M, dv_.n, 1, /*raw=*/1, s);
  hip_check(hipGetLastError(), "fit_many_begin launch");
  round(1, s);
  hip_check(hipMemcpy2DAsync(grads, (size_t)dv_.n * 4, g_t_, (size_t)dv_.nv * 4, (size_t)dv_.n * 4, M,
                             hipMemcpyDeviceToDevice, s),
            "hipMemcpy2DAsync(gradients)");
  hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(loss_grad_many)");
  losses.resize(M);
  holdout_losses.resize(M);
  for (int m = 0; m < M; ++m) {
    losses[m] = pout_[(size_t)m * kManyOutWords + kFitOutLoss];
    holdout_losses[m] = pout_[(size_t)m * kManyOutWords + kFitOutWords];
  }
}

}  // namespace psx
