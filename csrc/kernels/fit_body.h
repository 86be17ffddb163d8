// Device bodies shared by the dense fit kernels (fit_kernels.hip) and the wide ones
// (wide_fit_kernels.hip): what does not depend on the weight layout.  fit_dots_body
// turns the reduce workgroups' partial dots and the evaluation's loss partials into
// the pinned result block; fit_update_body (fit_step.h, also built for the host)
// applies one controller action to element e of the solver vectors and hands the new
// trial value to the layout's writer.
#pragma once
#include <hip/hip_runtime.h>

#include "fit_kernels.h"

namespace psx {

// One workgroup of 256 threads: the NB partial dots (4 strided lanes per value,
// combined in order), the nfw loss partials (part[g * 32 + 16]), f_t.
__device__ __forceinline__ void fit_dots_body(const double* __restrict__ dpart, const float* __restrict__ part,
                                              double* __restrict__ out, int H, int N, int NB, int nfw, double reg,
                                              int raw) {
  __shared__ double red[4][64];
  __shared__ double lred[256];
  const int t = threadIdx.x, k = t & 63, q = t >> 6;
  const int nd = raw ? 0 : 3 + 2 * H + 1;
  double a = 0.0;
  if (k < nd)
    for (int b = q; b < NB; b += 4) a += dpart[(size_t)b * kFitDotStride + k];
  red[q][k] = a;
  double ls = 0.0;
  for (int g = t; g < nfw; g += 256) ls += (double)part[(size_t)g * 32 + 16];
  lred[t] = ls;
  __syncthreads();
  if (t < nd - 1) out[kFitOutDots + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (t == 0) {
    double loss = 0.0;
    for (int i = 0; i < 256; ++i) loss += lred[i];
    loss /= (double)N;
    double bb = 0.0;
    if (nd > 0) bb = ((red[0][nd - 1] + red[1][nd - 1]) + red[2][nd - 1]) + red[3][nd - 1];
    out[kFitOutF] = loss + 0.5 * reg * bb;
    out[kFitOutLoss] = loss;
  }
}

}  // namespace psx
