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
};

void prepare_score_kernels();  // dynamic-LDS limits of the dense kernel
// y == nullptr: no labels (nll / conf / oor are ignored).
void launch_score(int FP, int K, const uint16_t* X, const int32_t* y, int T, const uint16_t* wf_hi,
                  const uint16_t* wf_lo, const float* b, const ScoreOut& o, hipStream_t s);
void launch_wide_score(int K, int KP, int64_t F, const int64_t* indptr, const int32_t* idx, const uint16_t* val,
                       const int32_t* y, int T, const float* w, const ScoreOut& o, hipStream_t s);

}  // namespace psx
