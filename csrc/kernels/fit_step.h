// What the host loop of a full-batch fit (csrc/solver/fit_loop.h) shares with the
// fit kernels, without any HIP include: the layout of the pinned result block, the
// controller action as it travels to the update kernel, and the update of one vector
// element.  The loop's CPU self-test builds this with a plain C++ compiler.
#pragma once
#include <cstddef>

#include "solver_ctrl.h"

namespace psx {

constexpr int kFitDotStride = 40;  // per-workgroup partial dots: num_dots(kMaxHist) + ||beta||^2, padded
// host block of one evaluation: f_t, mean cross entropy, then the dots in num_dots(hist) layout
constexpr int kFitOutF = 0, kFitOutLoss = 1, kFitOutDots = 2;
constexpr int kFitOutWords = kFitOutDots + 3 + 2 * kMaxHist + 1;

// One controller action for fit_update (Action of solver_ctrl.h).
struct FitStep {
  int action, push_slot;
  double t, t_acc, cg;
  double cs[kMaxHist], cy[kMaxHist];
};

// One controller action on element e.  x + t d is formed in fp64 and rounded once,
// identically for the trial point and for the accepted iterate, so the accepted x is
// exactly the point that was evaluated.
template <class Dev, class WriteTrial>
PSX_HD inline __attribute__((always_inline)) void fit_update_body(const Dev& dv, const FitStep& st, int e,
                                                                  WriteTrial&& write_trial) {
  float x = dv.x[e], d = dv.d[e];
  if (st.action == kActInit) {
    const float gc = dv.g_t[e];
    dv.g_c[e] = gc;
    d = (float)(st.cg * (double)gc);
    dv.d[e] = d;
  } else if (st.action == kActAccept || st.action == kActAcceptDone) {
    x = (float)((double)x + st.t_acc * (double)d);
    dv.x[e] = x;
    if (st.action == kActAccept) {
      const float gt = dv.g_t[e], gc = dv.g_c[e];
      if (st.push_slot >= 0) {
        dv.S[(size_t)st.push_slot * dv.nv + e] = (float)(st.t_acc * (double)d);
        dv.Y[(size_t)st.push_slot * dv.nv + e] = gt - gc;
      }
      dv.g_c[e] = gt;
      double nd = st.cg * (double)gt;
      for (int i = 0; i < dv.H; ++i)  // (this thread alone wrote element e of the pushed pair)
        nd += st.cs[i] * (double)dv.S[(size_t)i * dv.nv + e] + st.cy[i] * (double)dv.Y[(size_t)i * dv.nv + e];
      d = (float)nd;
      dv.d[e] = d;
    }
  }
  if (st.action == kActInit || st.action == kActTrial || st.action == kActAccept)
    write_trial(e, (float)((double)x + st.t * (double)d));
}

}  // namespace psx
