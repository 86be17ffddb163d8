// The controller loop of a full-batch fit, written once for the dense fitter
// (fit.hip) and the wide one (wide_fit.hip): evaluate, run the HOST build of
// solver_ctrl.h's ctrl_step on (f_t, dots), keep the objective history, hand the
// resulting action to the fitter and name the termination reason.  It launches
// nothing itself and includes nothing of HIP (csrc/tests/host_selftest.cc runs it on
// the CPU): the caller supplies "evaluate" (fills the result block of fit_step.h) and
// "apply step" (FitDriver of fit_driver.h launches the fitter's update kernel).
#pragma once
#include <climits>
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

#include "../kernels/fit_step.h"

namespace psx {

struct FitOpts {
  int max_iter = 100;
  double tol = 1e-6;
  double reg_param = 0.0;
  int ls_max = 20;
  int zero_const = 1;
};

class FitLoop {
 public:
  // Validate the options and reset every piece of state of the previous fit.
  void start(const FitOpts& o, int hist) {
    if (o.reg_param < 0.0 || !(o.reg_param == o.reg_param)) throw std::invalid_argument("fit: reg_param must be >= 0");
    if (o.max_iter < 0 || o.ls_max < 1 || o.tol < 0.0) throw std::invalid_argument("fit: bad max_iter / ls_max / tol");
    opts_ = o;
    cfg_ = SolverCfg{};
    cfg_.iters = o.max_iter;
    cfg_.hist = hist;
    cfg_.ls_max = o.ls_max;
    cfg_.mode = kModeLBFGS;
    cfg_.center = o.reg_param == 0.0;
    cfg_.zero_const = o.zero_const;
    cfg_.nslots = INT_MAX;  // the slot budget never fires
    cfg_.tol = (float)o.tol;
    ctrl_init(ctrl_);
    slot_ = 0;
    max_evals_ = (long long)o.max_iter * o.ls_max + 1;
    history_.clear();
    reason_.clear();
    log_loss_ = 0.0;
    begun_ = true;
    done_ = false;
  }
  // No fit in progress (a new dataset, or a single evaluation overwrote the trial point).
  void stop() {
    begun_ = false;
    done_ = true;
  }

  // Evaluate until the fit ends or `max_accept` more steps were accepted; true: ended.
  // evaluate(reg_param) leaves the result block in `pin`; apply(step) applies one action.
  template <class Eval, class Apply>
  bool run(int max_accept, const double* pin, Eval&& evaluate, Apply&& apply) {
    if (!begun_) throw std::runtime_error("fit: begin() first");
    const int nacc0 = ctrl_.nacc;
    while (!done_) {
      if (ctrl_.evals >= max_evals_) {  // never expected: every line search ends within ls_max evaluations
        reason_ = "max_iter";
        done_ = true;
        break;
      }
      evaluate(opts_.reg_param);
      const double f_t = pin[kFitOutF];
      const int phase0 = ctrl_.phase, nacc_prev = ctrl_.nacc;
      ctrl_step(ctrl_, cfg_, f_t, pin + kFitOutDots, slot_, scratch_);
      if (slot_ < INT_MAX - 2) ++slot_;
      if (phase0 == kPhInit) {
        history_.push_back(f_t);
        log_loss_ = pin[kFitOutLoss];
      } else if (ctrl_.nacc > nacc_prev) {
        history_.push_back(ctrl_.f_c);
        log_loss_ = pin[kFitOutLoss];
      }
      if (ctrl_.action != kActDone && ctrl_.action != kActNone) {
        FitStep st{};
        st.action = ctrl_.action;
        st.push_slot = ctrl_.push_slot;
        st.t = ctrl_.t;
        st.t_acc = ctrl_.t_acc;
        st.cg = ctrl_.cg;
        for (int i = 0; i < kMaxHist; ++i) {
          st.cs[i] = ctrl_.cs[i];
          st.cy[i] = ctrl_.cy[i];
        }
        apply(st);
      }
      if (ctrl_.phase == kPhDone) {
        done_ = true;
        const bool finite = std::isfinite(f_t);
        if (ctrl_.action == kActAcceptDone)
          reason_ = ctrl_.iter >= cfg_.iters ? "max_iter" : "tol";
        else if (phase0 == kPhInit)  // ended at the starting point
          reason_ = !finite ? "no_descent" : (cfg_.iters <= 0 ? "max_iter" : "tol");
        else  // a line search spent its budget without sufficient decrease (or met a non-finite objective)
          reason_ = finite ? "line_search" : "no_descent";
        break;
      }
      if (ctrl_.nacc - nacc0 >= max_accept) break;
    }
    return done_;
  }

  bool begun() const { return begun_; }
  bool done() const { return done_; }
  const FitOpts& opts() const { return opts_; }
  const Ctrl& ctrl() const { return ctrl_; }
  const std::string& reason() const { return reason_; }
  double log_loss() const { return log_loss_; }
  const std::vector<double>& history() const { return history_; }

 private:
  FitOpts opts_{};
  SolverCfg cfg_{};
  Ctrl ctrl_{};
  CtrlScratch scratch_{};
  bool begun_ = false, done_ = true;
  int slot_ = 0;
  long long max_evals_ = 0;
  double log_loss_ = 0.0;
  std::string reason_;
  std::vector<double> history_;
};

}  // namespace psx
