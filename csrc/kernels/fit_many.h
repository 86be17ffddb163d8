// Many dense fits per read of the rows (see fit_many.hip): the weighted evaluation of
// fit_weighted.hip for M models that share the rows, the labels, the sample and class
// weights and the fold stream, and differ in the held-out fold, the penalty and the
// iterate -- the fits of a cross-validation grid.
//
//   slot   KP adjacent MFMA columns, KP the smallest of 2, 4, 8, 16 that is >= K
//   group  the 16 columns of one v_mfma_f32_16x16x32_bf16 product: 16 / KP slots
//   pass   one launch that serves GP groups (many_groups(FP, KP), a template parameter)
//
// Model m sits in slot m of the row of slots: pass m / capacity, slot m % capacity.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_kernels.h"

namespace psx {

constexpr int many_kp(int K) { return K <= 2 ? 2 : K <= 4 ? 4 : K <= 8 ? 8 : 16; }
// Groups of one pass: the largest of 4, 3, 2, 1 that compiles with 0 bytes of scratch.  A
// group's accumulators take FP / 16 registers per thread next to the staging loads: 4
// groups up to FP 512, 3 at FP 1024 (4 spills), 1 at FP 2048 (2 spills), the same for
// every KP (the compiler's resource report: profiles/r20/README.md).
constexpr int many_groups(int FP, int /*KP*/) { return FP <= 512 ? 4 : FP == 1024 ? 3 : 1; }
constexpr int many_capacity(int FP, int K) { return many_groups(FP, many_kp(K)) * (16 / many_kp(K)); }

constexpr int kManyOutWords = kFitOutWords + 1;  // a model's result block, then its held-out mean loss

// One model as the batched vector kernels see it (a device array, model on blockIdx.y).
struct FitManyModel {
  // the model's own vectors, std_ / inv_std of its held-out fold, out = its result block;
  // whi / wlo / b_eff are its GROUP's fragments and intercepts, gpart / part its slot's
  // partials of workgroup 0 in the pass buffers
  FitDev dv;
  const double* wsum;  // [2] W, W_ho of its held-out fold
  const float* w0;     // start (begin) / weights (raw); null: zeros
  double reg;
  int col0;              // first MFMA column of its slot within the group
  int gstride, pstride;  // floats between two workgroups' partials
};

// One pass of the evaluation: GP groups against the same staged tiles.
struct FitManyPass {
  const uint16_t* X;
  const int32_t* y;
  int N, Npad, K;
  const float* sw;      // [Npad] or null
  const uint8_t* fold;  // [Npad] or null
  float cw[16];
  const uint16_t *whi, *wlo;  // [GP][16 * FP]
  const float* b_eff;         // [GP][16]
  const int* hold;            // [GP * 16 / KP] held-out fold of every slot; < 0: none
  float* gpart;               // [G][slots][K][FP]
  float* part;                // [G][slots][32]: K residual sums, [16] training loss, [17] held-out loss
  unsigned gmask;             // groups with a live slot; the others are skipped
};

void prepare_fit_many_kernels();
void launch_fit_many_lossgrad(const FitManyPass& ps, int FP, int G, hipStream_t s);
// x = w0 * sigma, trial point = x; raw: the weights themselves (as launch_fit_begin)
void launch_fit_many_begin(const FitManyModel* mm, int M, int n, int zero_const, int raw, hipStream_t s);
// models [m0, m0 + cnt) of one pass, before the next pass overwrites its partials: g_t and the
// partial dots, then f_t, the mean loss, the dots and the held-out mean -> the model's result
// block (as launch_fit_reduce_w); a model that is not live is skipped
void launch_fit_many_reduce(const FitManyModel* mm, const int* live, int m0, int cnt, int n, int nfw, int raw,
                            hipStream_t s);
void launch_fit_many_update(const FitManyModel* mm, const FitStep* steps, int M, int n, hipStream_t s);
// model m's iterate -> w_out + m * n (centred over the classes when its penalty is 0)
void launch_fit_many_finalize(const FitManyModel* mm, int M, int FP, float* w_out, hipStream_t s);

}  // namespace psx
