// Scoring a dataset with a trained model (gfx950): per-row prediction, class
// probabilities and loss plus the confusion counts, one pass over the rows and
// one launch per call.  One kernel per model family:
//   * dense: bf16 rows [T][FP] against the hi/lo MFMA fragments of
//     make_fragments (model columns at coff = 0), 32-row tiles (tile.h);
//     multinomial only, 2 <= K <= 16 (the one-logit model is the wide family's);
//   * wide: CSR rows against the dense weight vector [F][KP] + KP intercepts,
//     one wavefront per row (wide_row.h).
//
// Per row r with margins z[c], c < K:
//   pred[r]  argmax with the evaluation kernels' rule (strict >, lowest class
//            wins a tie; K == 1, the binary model: z > 0 ? 1 : 0)
//   proba    (optional) [T][C] fp32, C = K (binary: 2): softmax over the K real
//            classes with the row maximum subtracted; binary: (1 - s(z), s(z))
//   nll[r]   (optional, needs y) logsumexp(z) - z[y]; binary: softplus(z) - y z
//            with y = label > 0.  A multinomial label outside [0, K) gives NaN
//            and is counted in *oor
//   conf     (needs y) [16][16] int32 counts [label][pred], labels clamped as the
//            evaluation kernels clamp them; accumulated (the caller zeroes it)
//   hist     (optional, needs y) [Ch][2][512] int32, Ch = K: the distribution of the
//            one-vs-rest log-odds per class and label side, accumulated (the caller
//            zeroes it).  l_c = z_c - logsumexp_{j != c}(z_j) = log(p_c / (1 - p_c)),
//            the sum over the other classes taken directly from exp(z_j - max)
//            (+inf when they all underflow); binary: l_0 = z_0.  Bin
//            256 + clamp(round_to_nearest(16 l_c), -256, 255): width 1/16 in
//            log-odds, l = 0 in the middle of bin 256.  The clamp runs in float, so
//            +inf lands in bin 511, -inf and NaN in bin 0.  Side 1: rows labelled c
//            (binary: y > 0), side 0: every other row; a multinomial row whose
//            label is outside [0, K) enters no cell (it is counted in *oor).
// Plain streaming launches: integer atomics only, no cross-workgroup waits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psx {

struct ScoreOut {
  int32_t* pred;  // [T]
  float* proba;   // [T][C] or null
  float* nll;     // [T] or null (needs labels)
  int* conf;      // [256], accumulated; null without labels
  int* oor;       // [1] rows whose label is outside [0, K), accumulated; null without labels
  int* hist;      // [K][2][512] score histogram, accumulated; null: off (needs labels)
};

constexpr int kHistBins = 512;             // per class and side
constexpr int kHistCells = 2 * kHistBins;  // per class
// Forms of the dense kernel's histogram (launch_score's hist_form picks between the last two).
constexpr int kHistOff = 0, kHistLds = 1, kHistGlobal = 2;
constexpr size_t kLdsPerWorkgroup = 160 * 1024;  // gfx950
// kHistLds when the K * 4 KB table fits beside the tile, else kHistGlobal.
int score_hist_form(int FP, int K);

void prepare_score_kernels();  // dynamic-LDS limits (dense; the wide kernel's histogram table)
// y == nullptr: no labels (nll / conf / oor / hist are ignored).  hist_form (only with
// o.hist): 0 = score_hist_form(FP, K), or kHistLds / kHistGlobal; returns false when
// kHistLds is asked for and its table does not fit (nothing is launched).
bool launch_score(int FP, int K, const uint16_t* X, const int32_t* y, int T, const uint16_t* wf_hi,
                  const uint16_t* wf_lo, const float* b, const ScoreOut& o, hipStream_t s, int hist_form = 0);
void launch_wide_score(int K, int KP, int64_t F, const int64_t* indptr, const int32_t* idx, const uint16_t* val,
                       const int32_t* y, int T, const float* w, const ScoreOut& o, hipStream_t s);

}  // namespace psx
