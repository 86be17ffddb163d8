// Panel kernels (see panel_fit.hip): the full-batch fit's evaluation, statistics and
// scoring for dense bf16 rows of 2,048 < F <= 16,384 features, padded to FP in
// {4096, 8192, 16384} and processed in feature panels of 1,024 columns.  Plain
// streaming launches: no cross-workgroup waits, no float atomics, every sum in a
// fixed order.  The vector side (fit_begin / fit_reduce / fit_dots / fit_update /
// fit_finalize of fit_kernels.h) is launched unchanged on the same FitDev.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_kernels.h"
#include "score_kernels.h"

namespace psx {

constexpr int kPanelCols = 1024;
constexpr int kPanelFragWords = 16 * kPanelCols;  // one panel's slice of whi / wlo (write_frag's chunk-major order)

inline bool panel_fp_supported(int FP) { return FP == 4096 || FP == 8192 || FP == 16384; }
// Panels that hold a real feature; the others are all padding and are never read:
// their partial logits are not summed and their gradient partials stay zero.
inline int panel_live(int F) { return (F + kPanelCols - 1) / kPanelCols; }

// What the panel evaluation keeps beside FitDev (per dataset).
struct PanelDev {
  float* zpart;  // [live panels][Npad][16] partial logits of the trial weights
  uint16_t* rt;  // [Npad / 32][2][16][32] residual tiles, bf16 hi | lo, transposed (bwd_tile_acc's A operand)
  int PL;        // live panels
};

void prepare_panel_kernels();
// sigma / 1/sigma of every feature over the N rows: (G, PL) workgroups, then one fixed-order pass
void launch_panel_stats(const FitDev& dv, const PanelDev& pd, int G, hipStream_t s);
// loss partials, residual sums and the [G][K][FP] gradient partials at the trial fragments
// (three launches); launch_fit_reduce follows unchanged
void launch_panel_lossgrad(const FitDev& dv, const PanelDev& pd, int G, hipStream_t s);
// its three launches one by one (step 0: forward, 1: residuals, 2: backward), for timing
void launch_panel_step(const FitDev& dv, const PanelDev& pd, int G, int step, hipStream_t s);
// the forward at the trial fragments, then the row outputs of score_kernels.h (labels required, no histogram)
void launch_panel_score(const FitDev& dv, const PanelDev& pd, int G, const ScoreOut& o, hipStream_t s);

}  // namespace psx
