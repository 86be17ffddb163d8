// Full-batch fit of the wide (CSR) model (see wide_fit_kernels.hip): the fit runs in
// the subspace of the U distinct features the dataset touches, in the device layout
// of a WideSpec(U, K): [U][KP] coefficients feature-major, then KP intercepts.  One
// evaluation is a pass over the rows (margins, softmax / sigmoid, residual rows R), a
// pass over the inverted index (R^T X per work item) and the fixed-order reduction.
// Plain streaming launches: no cross-workgroup waits, no atomics, every sum in an
// order that depends on the data and the options alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fit_kernels.h"

namespace psx {

constexpr int kWideFitShort = 32;  // items of up to this many entries take the KP-lane mapping of the column pass
constexpr int kWideReduceMaxWG = 1024;  // workgroups of the reduction (256 elements each per trip, then grid-stride)

// Device pointers and sizes of one resident dataset (caller-owned, alive until the next
// set_data): the rows as CSR over the compact columns, the inverted index ordered by
// (column, row), and the work items of the column pass.
struct WideFitData {
  const int64_t* indptr;  // [N+1]
  const int32_t* col;     // [nnz] compact column of every entry (index into uniq)
  const uint16_t* val;    // [nnz] bf16
  const int32_t* y;       // [N]
  const int32_t* uniq;    // [U] sorted distinct feature ids
  const int64_t* colptr;  // [U+1]
  const int32_t* crow;    // [nnz]
  const uint16_t* cval;   // [nnz] bf16
  // entries [begin, end) of one column; column u owns the items [col_item0[u], col_item0[u+1]), in chunk order
  const int64_t* item_begin;   // [n_items]
  const int64_t* item_end;     // [n_items]
  const int32_t* col_item0;    // [U+1] first item of every column
  const int32_t* short_items;  // [n_short] items of <= kWideFitShort entries
  const int32_t* long_items;   // [n_long] the others
  int64_t N, U, F;             // rows, touched features, features of the full model
  int64_t n_items, n_short, n_long;
};

// The dataset plus the fit's vectors and scratch (set_data checks N, n and n_items < 2^31).
struct WideFitDev : WideFitData {
  int K, KP, H;
  int n, nv;     // n = U*KP + KP
  int W;         // waves of the row pass (one partial each)
  float *x, *d, *g_c, *g_t, *beta_t;  // [nv]
  float *S, *Y;                       // [H][nv]
  float* wfix;                        // [nv]
  float* weff;                        // [nv] trial weights in the original feature space + intercepts
  float *std_, *inv_std;              // [U]
  float* R;                           // [N][KP] residual rows
  float* gitem;                       // [I][KP]
  float* part;                        // [W][32] per-wave residual sums [16], loss at [16]
  float* bsum;                        // [16] the W residual-sum partials, summed in a fixed order
  double* dpart;                      // [reduce workgroups][kFitDotStride]
  double* out;                        // [kFitOutWords]
};

// sigma / 1/sigma of the touched features from the inverted index (fp64, two-pass)
void launch_wide_fit_stats(const WideFitDev& dv, hipStream_t s);
// x = w0 * sigma gathered through uniq (w0: full layout or nullptr), trial point = x; raw: weff = w0 itself
void launch_wide_fit_begin(const WideFitDev& dv, const float* w0, int zero_const, int raw, hipStream_t s);
void launch_wide_fit_rows(const WideFitDev& dv, int G, hipStream_t s);
void launch_wide_fit_cols(const WideFitDev& dv, hipStream_t s);
int wide_fit_reduce_grid(int n);  // workgroups of the reduction = rows of dpart
void launch_wide_fit_reduce(const WideFitDev& dv, double reg, int raw, hipStream_t s);
void launch_wide_fit_update(const WideFitDev& dv, const FitStep& st, hipStream_t s);
// w_out [F*KP + KP] (already holding the untouched features' values) gets the touched
// features' coefficients and the intercepts; centring over the classes as the dense fit
void launch_wide_fit_finalize(const WideFitDev& dv, int center, float* w_out, hipStream_t s);
// dst [F*KP + KP] (zeroed by the caller) <- compact src [n] through uniq
void launch_wide_fit_scatter(const WideFitDev& dv, const float* src, float* dst, hipStream_t s);

}  // namespace psx
